"""GPU: SURF detect+describe and its pair stage (HIP, csrc/surf.hip) vs oracle/oracle_surf.c, bit for bit, at the size limits and on
adversarial content.  tests/test_surf_patterns_oracle.py shows on the oracle alone that these inputs hold what they are for: tie groups and a
max_kp cut inside one, keypoints past row / column 8191, a gray sum above 2^32, every step of the layer mask, orientation discs and descriptor
windows cut by the frame edge, bit-equal train descriptors, a threshold walk that runs to zero, more than 2^21 Hessian maxima.

One context serves every extraction test, in file order: large frames, the small-size matrix, large frames again."""
import ctypes as C

import numpy as np
import pytest

from tests import oracle_lib as ol
from tests import sift_patterns as sp
from tests import surf_patterns as su
from tests.synth_frames import terrain

pytestmark = pytest.mark.gpu
FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")


@pytest.fixture(scope="module")
def orc():
    return ol.load_oracle_fast()


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _same(got, want, tag):
    (kp, d), (okp, od) = got, want
    assert len(kp) == len(okp), f"{tag}: {len(kp)} vs {len(okp)} keypoints"
    for f in FIELDS:
        a, b = kp[f], okp[f]
        same = a.view(np.uint32) == b.view(np.uint32) if a.dtype.kind == "f" else a == b
        assert same.all(), (tag, f, np.where(~same)[0][:5], a[~same][:3], b[~same][:3])
    assert np.array_equal(d.view(np.uint32), od.view(np.uint32)), (tag, "descriptors", int((d.view(np.uint32) != od.view(np.uint32)).any(1).sum()))


def _get(ctx, img_id, max_kp):
    """mi355_surf_get_features: the resident features of img_id"""
    import imagemosaicing_amd as im
    n = C.c_int(0)
    ctx._chk(ctx.L.mi355_surf_get_features(ctx._h, int(img_id), None, None, 0, C.byref(n)))
    m = min(n.value, max_kp)
    kp, desc = np.zeros(max(m, 1), im.KEYPOINT), np.zeros((max(m, 1), 128), np.float32)
    ctx._chk(ctx.L.mi355_surf_get_features(ctx._h, int(img_id), _vp(kp), _vp(desc), m, C.byref(n)))
    return kp[:m].copy(), desc[:m].copy()


def _extract_dev(ctx, img_id, img, thr, max_kp):
    """mi355_surf_extract_dev on a device copy of the frame, then the features back"""
    import torch
    img = np.ascontiguousarray(img)
    d = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    n = C.c_int(0)
    ctx._chk(ctx.L.mi355_surf_extract_dev(ctx._h, int(img_id), C.c_void_p(d.data_ptr()), img.shape[1], img.shape[0], img.strides[0],
                                          C.c_float(thr), int(max_kp), C.byref(n)))
    got = _get(ctx, img_id, max_kp)
    assert len(got[0]) == n.value
    del d
    return got


def _run(ctx, orc, items, dev_every=0):
    """items: [(tag, frame, threshold, max_kp)] -> SurfExtract (and every dev_every-th through the device form) against the oracle"""
    want = ol.parallel_map(lambda it: orc.surf(it[1], it[2], it[3]), items)
    out = []
    for k, ((tag, img, thr, mk), o) in enumerate(zip(items, want)):
        got = ctx.SurfExtract(7, img, thr, mk)
        _same(got, o, tag)
        _same(_get(ctx, 7, mk), o, tag + " get_features")
        if dev_every and k % dev_every == 0:
            _same(_extract_dev(ctx, 8, img, thr, mk), o, tag + " dev")
        out.append(got)
    return out


FIRST = ("terrain 1100x780", (1100, 780, 7), 20.0, su.KEEP_ALL)


def _first():
    tag, (w, h, seed), thr, mk = FIRST
    return (tag, terrain(w, h, seed=seed), thr, mk)


# ---- large ------------------------------------------------------------------------------------------------------------------------
def test_large_first_tie_cut_and_limit_shapes(ctx, orc):
    """the first case (run again at the end of the file), the tiled frame whole and cut inside its tie group, the 16383-wide / -high frames
    (14-bit row and column fields of the sort key)"""
    items = [_first()]
    w, h, seed, P, mk = su.TIE_CUT
    items += [("tiled48 640x480 keep-all", su.tie_cut_frame(), su.THR, su.KEEP_ALL), ("tiled48 640x480 cut in tie group", su.tie_cut_frame(), su.THR, mk)]
    items += [(f"{c} {w}x{h}", su.limit_frame(w, h, c), thr, mk) for (w, h, c, thr, mk) in su.LIMIT_SHAPES]
    got = _run(ctx, orc, items, dev_every=2)
    assert len(got[0][0]) > 2000 and len(got[1][0]) == 3120 and len(got[2][0]) == mk
    assert got[3][0]["x"].max() > 16350 and got[4][0]["y"].max() > 16350 and len(got[5][0]) == 20000
    assert len(got[6][0]) == 0 and len(got[7][0]) == 0


def test_bright_frame_integral_wraps(ctx, orc):
    """gray sum 5.03e9 > 2^32: the integral image wraps near row 3757, keypoints below it"""
    got = _run(ctx, orc, [("bright", su.bright(), su.THR, su.KEEP_ALL)], dev_every=1)
    assert (got[0][0]["y"] > 3800).sum() >= 300


@pytest.mark.parametrize("size", [(320, 240), (333, 257)])
def test_content_matrix(ctx, orc, size):
    w, h = size
    m = su.content_matrix(w, h)
    got = _run(ctx, orc, [(f"{n} {w}x{h}", img, su.THR, su.KEEP_ALL) for n, img in m.items()], dev_every=5)
    for n, (kp, _) in zip(m, got):
        assert (len(kp) == 0) == (n in su.ZERO_KEYPOINT_PATTERNS), n
    # cuts inside tie groups: every tied pattern at a max_kp in the middle of its largest group
    items = []
    for n, (kp, _) in zip(m, got):
        if n in su.TIE_PATTERNS:
            r = kp["response"].view(np.uint32)
            u, first, cnt = np.unique(r, return_index=True, return_counts=True)
            g = int(np.argmax(cnt))
            assert cnt[g] >= 8
            items.append((f"{n} {w}x{h} cut", m[n], su.THR, int(first[g] + cnt[g] // 2)))
    _run(ctx, orc, items)


# ---- small ------------------------------------------------------------------------------------------------------------------------
def test_shape_matrix(ctx, orc):
    """every size of the small-size matrix (layers and octaves that do not fit, frames below one 64 x 16 tile, tile edges +- 1), terrain and
    binary noise; zero keypoints only where surf_patterns allows it"""
    items = [(f"{c} {w}x{h}", img, su.THR_SHAPE, su.KEEP_ALL) for (w, h) in su.SHAPES for c, img in su.shape_frames(w, h).items()]
    got = _run(ctx, orc, items, dev_every=7)
    k = 0
    for (w, h) in su.SHAPES:
        for c in su.shape_frames(16, 16):
            allowed = not su.octaves_possible(w, h) or (c, w, h) in su.ZERO_BY_CONTENT
            assert (len(got[k][0]) == 0) == allowed, (c, w, h, len(got[k][0]))
            k += 1


def test_one_image_id_grows_and_shrinks(ctx, orc):
    """one img_id extracted three times: 333x257 keep-all, 1100x780 keep-all (more keypoints, larger planes), 200x160 with max_kp = 5"""
    seq = [("a", terrain(333, 257, seed=5), 20.0, su.KEEP_ALL), ("b", terrain(1100, 780, seed=8), 5.0, su.KEEP_ALL), ("c", terrain(200, 160, seed=6), 20.0, 5)]
    want = ol.parallel_map(lambda it: orc.surf(it[1], it[2], it[3]), seq)
    assert len(want[0][0]) < len(want[1][0]) and len(want[2][0]) == 5
    for (tag, img, thr, mk), o in zip(seq, want):
        _same(ctx.SurfExtract(31, img, thr, mk), o, "grow/shrink " + tag)
        _same(_get(ctx, 31, su.KEEP_ALL), o, "grow/shrink get_features " + tag)
    _same(_extract_dev(ctx, 31, seq[0][1], seq[0][2], seq[0][3]), want[0], "grow/shrink dev")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_working(ctx, orc):
    import imagemosaicing_amd as im
    normal = terrain(200, 160, seed=31)
    want = orc.surf(normal, 20.0, 4096)
    assert len(want[0]) > 50

    def ok_after(tag):
        _same(ctx.SurfExtract(7, normal, 20.0, 4096), want, "after " + tag)

    ok_after("nothing")
    for (w, h) in [(15, 16), (16, 15), (16384, 16), (16, 16384)]:
        with pytest.raises(im.Mi355Error):
            ctx.SurfExtract(7, np.full((h, w, 3), 90, np.uint8))
        with pytest.raises(im.Mi355Error):
            _extract_dev(ctx, 7, np.full((h, w, 3), 90, np.uint8), su.THR, 100)
        ok_after(f"{w}x{h}")
    kp, desc, n = np.zeros(64, im.KEYPOINT), np.zeros((64, 128), np.float32), C.c_int(0)
    with pytest.raises(im.Mi355Error):                             # width_step < 3 w
        ctx._chk(ctx.L.mi355_surf_extract(ctx._h, 7, _vp(normal), 200, 160, 599, C.c_float(20.0), 64, _vp(kp), _vp(desc), C.byref(n)))
    ok_after("width_step")
    for mk in (0, (1 << 21) + 1):
        with pytest.raises(im.Mi355Error):
            ctx._chk(ctx.L.mi355_surf_extract(ctx._h, 7, _vp(normal), 200, 160, 600, C.c_float(20.0), mk, None, None, C.byref(n)))
        ok_after(f"max_kp {mk}")
    ctx.SurfExtract(40, normal, 20.0, 4096); ctx.SurfExtract(41, terrain(200, 160, seed=32), 20.0, 4096)
    good = ctx.SurfMatchPairs([(40, 41)], 2.5, 1)
    for kw in (dict(match_dist=float("nan")), dict(match_dist=100.5), dict(match_dist=float("inf")), dict(max_features=0), dict(max_features=401)):
        with pytest.raises(im.Mi355Error):
            ctx.SurfMatchPairs([(40, 41)], 2.5, 1, **kw)
        assert ctx.SurfMatchPairs([(40, 41)], 2.5, 1).tobytes() == good.tobytes()
        ok_after(str(kw))
    with pytest.raises(im.Mi355Error):
        ctx.SurfMatchPairs([(40, 9999)], 2.5, 1)
    with pytest.raises(im.Mi355Error):
        _get(ctx, 9999, 16)
    ok_after("unknown id")


def test_more_than_2_21_maxima_is_refused(ctx, orc):
    """the 0 / 255 lattice at 6000 x 6000 and threshold 0: 2 229 049 accepted maxima on the oracle (tests/test_surf_patterns_oracle.py)"""
    import imagemosaicing_amd as im
    with pytest.raises(im.Mi355Error, match="Hessian maxima"):
        ctx.SurfExtract(7, su.lattice(), 0.0, 16)
    normal = terrain(200, 160, seed=31)
    _same(ctx.SurfExtract(7, normal, 20.0, 4096), orc.surf(normal, 20.0, 4096), "after the 2^21 refusal")


# ---- pair stage ---------------------------------------------------------------------------------------------------------------------
def _check_record(r, i, j, want, tag, min_inliers=18):
    nin, i1, i2, Ho, ns = want
    assert (int(r["i"]), int(r["j"])) == (i, j), tag
    assert int(r["n_selected"]) == ns, (tag, int(r["n_selected"]), ns)
    assert int(r["accepted"]) == int(nin > min_inliers), (tag, int(r["accepted"]), nin)
    if nin > min_inliers:
        assert int(r["n_in"]) == nin, (tag, int(r["n_in"]), nin)
        assert np.array_equal(r["a"][:nin], i1[:nin]) and np.array_equal(r["b"][:nin], i2[:nin]), tag
        assert np.array_equal(r["H"].view(np.uint32), Ho.view(np.uint32)), tag
    else:
        assert int(r["n_in"]) <= min_inliers, tag


def test_pairs_with_tied_descriptors_and_the_full_walk(ctx, orc):
    """dup pair (bit-equal train rows), self pair and tiled pair (the walk ends at distT <= 0), pairs with a flat frame on either side;
    match_dist / max_features at their limits and two seeds against bf_match_f32 + select_by_distance + ransac2d"""
    fi, fj = su.dup_pair()
    seed, P, dx, dy = su.TILED_PAIR
    frames = [fi, fj, sp.tiled(320, 240, seed, P), sp.tiled_shifted(320, 240, seed, P, dx, dy), su.flat(320, 240)]
    F = [g for g in _run(ctx, orc, [(f"pair frame {k}", f, su.THR, su.KEEP_ALL) for k, f in enumerate(frames)])]
    for k, f in enumerate(frames):
        ctx.SurfExtract(200 + k, f, su.THR, su.KEEP_ALL)
    pairs = [(0, 1), (1, 0), (0, 0), (2, 3), (2, 2), (4, 0), (0, 4), (4, 4)]
    for s in (1, 4):
        res = ctx.SurfMatchPairs([(200 + i, 200 + j) for (i, j) in pairs], 2.5, s)
        want = ol.parallel_map(lambda p: orc.surf_match_pair(F[p[0]], F[p[1]], 2.5, s), pairs)
        for r, (i, j), o in zip(res, pairs, want):
            _check_record(r, 200 + i, 200 + j, o, (i, j, s))
        assert int(res[0]["accepted"]) == 1 and [int(r["n_selected"]) for r in res[2:]] == [0] * 6
    (k1, d1), (k2, d2) = F[0], F[1]
    idx, dist = orc.bf_match_f32(d1, d2)
    xy1, xy2 = np.stack([k1["x"], k1["y"]], 1), np.stack([k2["x"], k2["y"]], 1)
    seen = []
    for md, mf, s in [(0.5, 1, 1), (0.5, 400, 1), (100.0, 400, 1), (100.0, 1, 4), (-1.0, 200, 1), (0.05, 400, 4), (0.5, 200, 4)] + [(md, mf, 1) for md, mf in su.FEW_SELECTED + su.WALK_TO_EPS]:
        r = ctx.SurfMatchPairs([(200, 201)], 2.5, s, match_dist=md, max_features=mf)[0]
        s1, s2 = orc.select_by_distance(idx, dist, xy1, xy2, md, mf)
        ok, i1, i2, Ho = orc.ransac2d(s1, s2, 2.5, 1000, s)
        _check_record(r, 200, 201, (len(i1), i1, i2, Ho, len(s1)), (md, mf, s))
        seen.append(len(s1))
    assert max(seen) > 300 and 0 in seen and any(1 <= n <= 3 for n in seen) and seen[-2:] == [2, 2], seen


def test_pairs_at_ragged_feature_counts(ctx, orc):
    """1, 63, 64, 65, 255, 256 and 257 features on each side: the 64-row train tile and the 256-query workgroup of the matcher"""
    a, b = su.count_frames()
    A = [orc.surf(a, su.THR, n) for n in su.FEATURE_COUNTS]
    B = [orc.surf(b, su.THR, n) for n in su.FEATURE_COUNTS]
    for k, n in enumerate(su.FEATURE_COUNTS):
        _same(ctx.SurfExtract(300 + k, a, su.THR, n), A[k], f"count {n} a")
        _same(ctx.SurfExtract(320 + k, b, su.THR, n), B[k], f"count {n} b")
        assert len(A[k][0]) == len(B[k][0]) == n
    K = range(len(su.FEATURE_COUNTS))
    pairs = [(i, j) for i in K for j in K]
    res = ctx.SurfMatchPairs([(300 + i, 320 + j) for (i, j) in pairs], 2.5, 1)
    want = ol.parallel_map(lambda p: orc.surf_match_pair(A[p[0]], B[p[1]], 2.5, 1), pairs)
    for r, (i, j), o in zip(res, pairs, want):
        _check_record(r, 300 + i, 320 + j, o, ("counts", su.FEATURE_COUNTS[i], su.FEATURE_COUNTS[j]))
    assert int(res["accepted"].sum()) >= 4 and int((res["n_selected"] > 0).sum()) >= 30


def test_600_pairs_in_one_call_and_split_calls(ctx, orc):
    """the ring schedule of 40 small frames with 0 .. 100+ features: 600 pairs, two batches of the pair stage (512 + 88) whose largest
    query counts differ; the same pairs in two calls split at 300 and in three split at 511 / 513 give the same bytes"""
    import imagemosaicing_amd as im
    R = su.ring_frames()
    F = ol.parallel_map(lambda it: orc.surf(*it), R)
    for k, (img, thr, mk) in enumerate(R):
        _same(ctx.SurfExtract(400 + k, img, thr, mk), F[k], f"ring frame {k}")
    sched = im.surf_pair_schedule(su.RING_N)
    assert len(sched) == 600
    pairs = sched + 400
    res = ctx.SurfMatchPairs(pairs, 2.5, 4)
    want = ol.parallel_map(lambda p: orc.surf_match_pair(F[p[0]], F[p[1]], 2.5, 4), [tuple(int(v) for v in p) for p in sched])
    for r, (i, j), o in zip(res, sched, want):
        _check_record(r, 400 + int(i), 400 + int(j), o, ("ring", int(i), int(j)))
    assert 100 < int(res["accepted"].sum()) < 500
    for cuts in ([300], [511, 513]):
        parts = np.split(pairs, cuts)
        again = np.concatenate([ctx.SurfMatchPairs(p, 2.5, 4) for p in parts])
        assert again.tobytes() == res.tobytes(), cuts


# ---- large again --------------------------------------------------------------------------------------------------------------------
def test_large_again_after_everything(ctx, orc):
    """the first case once more on the same context, after the small frames, the refusals and the pair calls"""
    got = _run(ctx, orc, [_first(), ("terrain 2000x1500", terrain(2000, 1500, seed=9), 2.0, su.KEEP_ALL)], dev_every=1)
    assert len(got[1][0]) > 20000
