"""CPU (ctypes, no device): mi355_guided_candidates and mi355_merge_pair_results against their numpy twins in tests/guided_ref.py, byte for byte."""
import numpy as np
import pytest

from tests import guided_ref as gr

W, H = 1000, 750


def _shift(tx, ty, s=1.0, rot=0.0, p6=0.0, p7=0.0, m8=1.0):
    c, sn = s * np.cos(rot), s * np.sin(rot)
    return np.array([c, -sn, tx, sn, c, ty, p6, p7, m8], np.float32)


def block_layout():
    """a 4 x 4 block of frames, 60 % overlap along x and 40 % along y, each with a little rotation, scale and perspective of its own"""
    rng = np.random.default_rng(5)
    return np.stack([_shift(0.4 * W * c + rng.normal(0, 3), 0.6 * H * r + rng.normal(0, 3), 1 + rng.normal(0, 0.01), rng.normal(0, 0.02), rng.normal(0, 1e-6), rng.normal(0, 1e-6))
                     for r in range(4) for c in range(4)])


def strip_layout(n=12):
    """a strip: every frame a third of a frame further along x, the canvas scale drifting (m[8] != 1 here and there)"""
    t = np.stack([_shift(W / 3.0 * k, 4.0 * np.sin(k), 1 + 0.002 * k, 0.01 * k) for k in range(n)])
    t[3] *= np.float32(2.0)                                 # the same map, another scale of the matrix
    t[n - 1] *= np.float32(-0.5)
    return t


def _same(lib, w, h, t, have=None, min_points=0):
    pairs, guides = lib.guided_candidates(w, h, t, have, min_points)
    rp, rg = gr.guided_candidates(w, h, t, have, min_points)
    assert pairs.dtype == np.int32 and guides.dtype == np.float32
    assert np.array_equal(pairs, rp), (pairs.tolist(), rp.tolist())
    assert guides.tobytes() == rg.tobytes()
    assert lib.guided_candidates_count(w, h, t, have, min_points) == len(rp)
    assert [tuple(p) for p in pairs] == sorted(tuple(p) for p in pairs)
    return pairs, guides


@pytest.mark.parametrize("layout", [block_layout, strip_layout])
def test_pairs_and_guides_equal_the_numpy_twin(lib, layout):
    t = layout()
    pairs, guides = _same(lib, W, H, t)
    assert 0 < len(pairs) < len(t) * (len(t) - 1) // 2      # neighbours overlap, far frames do not
    assert np.allclose(guides[:, 8], 1.0)
    have = pairs[::2]
    rest, _ = _same(lib, W, H, t, have)
    assert len(rest) == len(pairs) - len(have) and not {tuple(p) for p in rest} & {tuple(p) for p in have}
    _same(lib, W, H, t, have[:, ::-1])                      # a covered pair may be written (j, i)
    for mp in (-3, 1, 2, 5, 9, 18, 19):
        n = len(_same(lib, W, H, t, None, mp)[0])
        assert mp != 19 or n == 0                           # there are 18 control points
    assert len(_same(lib, W, H, t, None, -3)[0]) == len(pairs) == len(_same(lib, W, H, t, None, 2)[0])
    _same(lib, 1, 1, t)
    _same(lib, 4001, 2999, t)


def test_unplaced_frames_and_singular_transforms(lib):
    t = strip_layout(8)
    t[2, 8] = 0.0                                           # not placed
    t[4] = _shift(W / 3.0 * 4, 0.0)
    t[4, 3:6] = t[4, 0:3]                                   # rank 2: det == 0
    t[5] = np.array([1, 0, 0, 0, 1, 0, 0, 0, np.inf], np.float32)
    t[6, 0] = np.nan
    pairs, _ = _same(lib, W, H, t)
    assert len(pairs) > 0 and not {2, 4, 5, 6} & set(pairs.ravel().tolist())
    u = strip_layout(4)
    u[1] = np.array([0, 0, 1, 0, 0, 1, 1, 0, 1e-30], np.float32)      # finite, placed, det == 0
    _same(lib, W, H, u)
    assert len(_same(lib, W, H, np.zeros((5, 9), np.float32))[0]) == 0
    assert len(_same(lib, W, H, np.zeros((0, 9), np.float32))[0]) == 0


def test_count_only_and_short_buffer(lib):
    import imagemosaicing_amd as im
    t = block_layout()
    n = lib.guided_candidates_count(W, H, t)
    full, guides = lib.guided_candidates(W, H, t, max_pairs=n)
    assert len(full) == n
    bigger, _ = lib.guided_candidates(W, H, t, max_pairs=n + 7)
    assert np.array_equal(bigger, full)
    with pytest.raises(im.Mi355Error, match="max_pairs=%d .*%d pairs" % (n - 1, n)):
        lib.guided_candidates(W, H, t, max_pairs=n - 1)
    with pytest.raises(im.Mi355Error, match="frame size"):
        lib.guided_candidates(0, H, t)
    # the raw call: a short buffer reports the count and writes nothing
    import ctypes as C
    L = im.load_library()
    pairs = np.full((n, 2), -7, np.int32)
    cnt = C.c_int(-1)
    rc = L.mi355_guided_candidates(W, H, len(t), t.ctypes.data_as(C.c_void_p), None, 0, 0, pairs.ctypes.data_as(C.c_void_p), None, n - 1, C.byref(cnt))
    assert rc < 0 and cnt.value == n and (pairs == -7).all()
    rc = L.mi355_guided_candidates(W, H, len(t), t.ctypes.data_as(C.c_void_p), None, 0, 0, pairs.ctypes.data_as(C.c_void_p), None, n, C.byref(cnt))
    assert rc == 0 and np.array_equal(pairs, full)          # guides may be NULL


def _records(lib, spec, salt):
    """records (i, j, n_in) with recognisable contents"""
    r = np.zeros(len(spec), lib.PAIR_RESULT)
    for k, (i, j, n_in) in enumerate(spec):
        r[k]["i"], r[k]["j"], r[k]["n_in"], r[k]["n_selected"], r[k]["accepted"] = i, j, n_in, n_in + 1, int(n_in > 30)
        r[k]["H"] = np.arange(9) + salt + k
        r[k]["a"]["x"][:max(n_in, 0)] = salt + k
    return r


def test_merge_pair_results(lib):
    base = _records(lib, [(0, 1, 40), (1, 2, 10), (2, 3, 50), (3, 4, 31)], 100)
    extra = _records(lib, [(1, 2, 45), (2, 3, 50), (3, 4, 12), (0, 2, 33), (5, 6, 0), (0, 2, 60), (0, 2, 60), (1, 0, 99)], 200)
    got = lib.merge_pair_results(base, extra)
    want = gr.merge_pair_results(base, extra)
    assert got.tobytes() == want.tobytes()
    assert [(int(r["i"]), int(r["j"]), int(r["n_in"])) for r in got] == [(0, 1, 40), (1, 2, 45), (2, 3, 50), (3, 4, 31), (0, 2, 60), (5, 6, 0), (1, 0, 99)]
    assert got[1].tobytes() == extra[0].tobytes()           # larger n_in: the extra record, whole
    assert got[2].tobytes() == base[2].tobytes()            # equal n_in: base wins
    assert got[3].tobytes() == base[3].tobytes()            # smaller n_in: base stays
    assert got[4].tobytes() == extra[5].tobytes()           # of two equal extra records the earlier
    # disjoint sets, empty sets
    a, b = _records(lib, [(0, 1, 40)], 1), _records(lib, [(4, 5, 2), (2, 3, 9)], 2)
    assert lib.merge_pair_results(a, b).tobytes() == a.tobytes() + b.tobytes() == gr.merge_pair_results(a, b).tobytes()
    assert lib.merge_pair_results(a, b[:0]).tobytes() == a.tobytes() and lib.merge_pair_results(a[:0], b).tobytes() == b.tobytes()
    assert len(lib.merge_pair_results(a[:0], b[:0])) == 0
    # out may be base when it has room
    import ctypes as C
    import imagemosaicing_amd as im
    L = im.load_library()
    buf = np.zeros(len(base) + len(extra), lib.PAIR_RESULT)
    buf[:len(base)] = base
    n = C.c_int(0)
    assert L.mi355_merge_pair_results(buf.ctypes.data_as(C.c_void_p), len(base), extra.ctypes.data_as(C.c_void_p), len(extra), buf.ctypes.data_as(C.c_void_p), C.byref(n)) == 0
    assert buf[:n.value].tobytes() == want.tobytes()
    assert L.mi355_merge_pair_results(None, 1, None, 0, buf.ctypes.data_as(C.c_void_p), C.byref(n)) < 0


def test_default_params(lib):
    p = lib.default_guided_params()
    assert (p.radius, p.max_dist2, p.reserved) == (4.0, 90000, 0) and p.ratio == np.float32(0.8)
    q = lib.default_guided_params(radius=2.5, max_dist2=7, ratio=0.0)
    assert (q.radius, q.max_dist2, q.ratio) == (2.5, 7, 0.0)
