"""CPU: mi355_solve_gains (host only) against the numpy restatement (tests/gain_ref.py): random and restated statistics, channels 1 and 3,
gains of 1 for frames without an equation, bit-identical repeats, and every argument error of the solve."""
import numpy as np
import pytest

from tests import gain_ref as gr

ROWS = [dict(), dict(channels=1), dict(sigma_g=10.0), dict(sigma_n=3.0, sigma_g=0.5, channels=1)]


def random_stats(n, n_pairs, seed, skip=()):
    import imagemosaicing_amd as im
    rng = np.random.default_rng(seed)
    gain = rng.uniform(0.8, 1.2, n)
    pairs = set()
    for k in range(n - 1):
        pairs.add((k, k + 1))
    while len(pairs) < n_pairs:
        a, b = sorted(rng.choice(n, 2, replace=False))
        pairs.add((int(a), int(b)))
    pairs = sorted(p for p in pairs if p[0] not in skip and p[1] not in skip)
    st = np.zeros(len(pairs), im.GAIN_PAIR_STATS)
    cover = rng.integers(1000, 5000, n).astype(np.int64)
    for k in skip:
        cover[k] = 0
    for i, (a, b) in enumerate(pairs):
        nn = int(rng.integers(0, 800)) if i % 7 else 0                      # some listed pairs without overlap
        base = rng.uniform(60, 180, 3)
        st[i]["a"], st[i]["b"], st[i]["n"] = a, b, nn
        st[i]["sum_a"] = np.round(base * gain[a] * nn).astype(np.int64)
        st[i]["sum_b"] = np.round(base * gain[b] * nn).astype(np.int64)
    return st, cover


def rel_err(g, ref):
    return float(np.max(np.abs(g.astype(np.float64) - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("kw", ROWS)
@pytest.mark.parametrize("seed", [1, 2])
def test_solve_random_matches_numpy(lib, kw, seed):
    st, cover = random_stats(60, 150, seed)
    g = lib.solve_gains(st, cover, **kw)
    ref = gr.solve_ref(st, cover, **kw)
    assert g.dtype == np.float32 and g.shape == (60, 3)
    # the float32 result is the double solution rounded once: within half an ulp of float plus the solve's own error
    assert np.array_equal(g, ref.astype(np.float32)) or rel_err(g, ref) < 1e-7
    # the double solve itself, seen through a channel whose float rounding is exact enough: the normal-equation residual
    for c, (A, rhs) in enumerate(gr.normal_equations(st, cover, **kw)):
        x = ref[:, c]
        act = np.diag(A) > 0
        assert np.max(np.abs(A[np.ix_(act, act)] @ x[act] - rhs[act])) <= 1e-9 * np.max(np.abs(rhs))


def test_solve_double_accuracy(lib):
    """the solve is accurate to 1e-9 of the exact solution: with gains that are representable the float result is exact"""
    st, cover = random_stats(200, 600, 5)
    for kw in ROWS:
        g = lib.solve_gains(st, cover, **kw)
        ref = gr.solve_ref(st, cover, **kw)
        # float32 rounding bounds what the output can show: 2^-24 relative; nothing beyond one float ulp of the exact value
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(g.astype(np.float64) - ref) <= ulp), kw


def test_isolated_and_skipped_frames_get_one(lib):
    st, cover = random_stats(30, 60, 3, skip=(4, 17))
    cover[29] = 0                                       # frame 29 without cover: its pairs have n = 0 too
    keep = [(s["a"] != 29 and s["b"] != 29) for s in st]
    st = st[np.array(keep)]
    g = lib.solve_gains(st, cover)
    for k in (4, 17, 29):
        assert np.all(g[k] == 1.0), (k, g[k])
    # a frame that covers points but has no listed pair: A[k][k] = beta N_k = rhs[k]
    st2 = st[(st["a"] != 10) & (st["b"] != 10)]
    g2 = lib.solve_gains(st2, cover)
    assert np.all(g2[10] == 1.0)
    ref = gr.solve_ref(st2, cover)
    assert rel_err(g2, ref) < 1e-7


def test_restated_stats_solve(lib, oracle):
    """statistics restated from the oracle's refined render of a small overlapping set, solved by the library and by numpy"""
    from tests.synth import texture, warp_cases
    imgs = [(texture(160, 120, s).astype(np.float64) * (0.9 + 0.05 * s)).clip(0, 255).astype(np.uint8) for s in range(4)]
    Hs = warp_cases()
    h9s = np.stack([Hs[0], Hs[1], Hs[3], Hs[2]]).astype(np.float32)
    h9s[1, 2] += 60
    h9s[2, 5] += 50
    h9s[3, 2] -= 40
    maps = gr.frame_sample_maps(oracle, imgs, h9s)
    pairs = [(0, 1), (1, 2), (0, 2), (2, 3), (0, 3)]
    recs, cover = gr.stats_ref(maps, pairs, 2)
    st = gr.to_records(recs, pairs)
    assert all(r[0] > 0 for r in recs)
    for kw in ROWS:
        g = lib.solve_gains(st, cover, **kw)
        assert rel_err(g, gr.solve_ref(st, cover, **kw)) < 1e-7, kw


def test_solve_bit_identical_repeats(lib):
    st, cover = random_stats(300, 1200, 9)
    a = lib.solve_gains(st, cover)
    for _ in range(3):
        assert np.array_equal(lib.solve_gains(st, cover).view(np.uint32), a.view(np.uint32))
    # the record order of the input is part of the input; the same records give the same bits in a fresh copy
    assert np.array_equal(lib.solve_gains(st.copy(), cover.copy()).view(np.uint32), a.view(np.uint32))


def _err(lib, st, cover, match, **kw):
    with pytest.raises(lib.Mi355Error) as e:
        lib.solve_gains(st, cover, **kw)
    assert e.value.code == -1 and match in str(e.value), str(e.value)


def test_solve_argument_errors(lib):
    st, cover = random_stats(10, 15, 4)
    bad = st.copy(); bad[3]["b"] = bad[3]["a"]
    _err(lib, bad, cover, "pair 3 (%d, %d): a == b" % (bad[3]["a"], bad[3]["a"]))
    bad = st.copy(); bad[2]["b"] = 10
    _err(lib, bad, cover, "pair 2 (%d, 10): position outside [0, 10)" % bad[2]["a"])
    bad = st.copy(); bad[1]["a"] = -1
    _err(lib, bad, cover, "pair 1 (-1, ")
    bad = st.copy(); bad[5]["a"], bad[5]["b"] = st[0]["b"], st[0]["a"]         # the unordered pair of record 0 again
    _err(lib, bad, cover, "pair 5 (%d, %d) repeats pair 0" % (st[0]["b"], st[0]["a"]))
    _err(lib, st, cover, "channels=2", channels=2)
    _err(lib, st, cover, "sigma_n=", sigma_n=0.0)
    _err(lib, st, cover, "sigma_g=", sigma_g=-1.0)
    _err(lib, st[:0], np.zeros(65536, np.int64), "n=65536")
    _err(lib, st[:0], np.zeros(0, np.int64), "n=0")


def test_default_params(lib):
    p = lib.gain_params()
    assert (p.sigma_n, p.channels, p.step) == (10.0, 3, 8) and p.sigma_g == np.float32(0.1)
    assert lib.GAIN_PAIR_STATS.itemsize == 64
