"""CPU: the local registration (include/mi355_mosaic.h, "local registration").  The host twin of the statistics kernel
(mi355_tie_residual_stats_host) against the numpy restatement of tests/local_warp_ref.py bit for bit, the host solve
(mi355_solve_local_warps) against its dense solve, properties of the definition on the restatement, and what the step is for: on synthetic
surveys (tests/local_warp_cases.py) the ties' canvas disagreement falls, a planar survey is left alone, and two frames agree better
photometrically.  The GPU tests (tests/test_gpu_local_warp.py) ask the kernels for the restatement's bytes.

Measured with the restatement at the defaults (grid 8 x 6, min_ties 8, max_residual 8, max_shift 8, smooth 2, prior 0.25; six frames of
160 x 120, 15 pairs, about 4400 ties; survey seeds 1..5; printed by the tests, the sweep is scratch/local_warp_sweep.py):
  fields of 2 px : ratio after / before of the ties' rms canvas disagreement 0.323 0.306 0.314 0.304 0.337 (about 2.0 px -> 0.63 px)
  planar, 0.5 px tie noise : largest |D| 0.204 0.221 0.245 0.248 0.222 px
The assertions allow a quarter over the largest of each: 0.421 and 0.310 px."""
import os
import subprocess
import sys

import numpy as np
import pytest

import imagemosaicing_amd as im
from tests import local_warp_cases as lc
from tests import local_warp_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (1, 2, 3, 4, 5)
RATIO_BOUND = 0.337 * 1.25
HARM_BOUND = 0.248 * 1.25


@pytest.fixture(scope="module")
def surveys():
    return {seed: lc.survey(seed=seed) for seed in SEEDS}


@pytest.fixture(scope="module")
def edge():
    e = lc.edge_case()
    e["stats"] = lr.stats(e["rec"], e["w"], e["h"], e["h9s"], **e["params"])
    return e


# ---- the host twin and the host solve against the restatement ----------------------------------------------------------------------------
def test_host_statistics_equal_the_restatement_bit_for_bit(surveys, edge):
    got = im.tie_residual_stats_host(edge["rec"], edge["w"], edge["h"], edge["h9s"], **edge["params"])
    assert np.array_equal(got, edge["stats"])
    assert got[-8] == edge["n_skipped"] and not got[-7:].any()
    NN, sd = 63, lr.stride(8, 6)
    tails = got[:-8].reshape(edge["n"], sd)[:, 7 * NN:]
    assert (tails[:, 2:5] > 0).any(0).all() and tails[0, 0] > 400           # every reject kind occurs, and ties are kept
    assert not got[4 * sd:5 * sd].any()                                       # the frame that takes no part
    # frame 5 holds the threshold ties alone: of twelve, two lie one step above max_residual, four sides are kept (|d| at and one step below
    # max_shift), six are lost to max_shift
    assert tails[5, 0] == 4 and tails[5, 2:5].tolist() == [0, 2, 6]
    for grid in ((8, 6), (1, 1), (16, 16), (3, 2)):
        s = surveys[1]
        p = dict(grid_x=grid[0], grid_y=grid[1])
        assert np.array_equal(im.tie_residual_stats_host(s["rec"], s["w"], s["h"], s["h9s"], **p), lr.stats(s["rec"], s["w"], s["h"], s["h9s"], **p)), grid
    assert np.array_equal(im.tie_residual_stats_host(s["rec"][:0], s["w"], s["h"], s["h9s"]), np.zeros(im.local_warp_stats_len(s["n"], 8, 6), np.int64))


def check_solve(st, n, **p):
    grids, rep = im.solve_local_warps(st, n, **p)
    _, sols, reps = lr.solve(st, n, **dict(lr.DEFAULTS, **p))
    ms = dict(lr.DEFAULTS, **p)["max_shift"]
    for k in range(n):
        sol = np.clip(sols[k], -ms, ms).reshape(grids[k].shape)
        # 1e-9 relative in the infinity norm, and the rounding of the cast to float
        tol = 1e-9 * max(np.abs(sols[k]).max(), 1e-300) + np.abs(sol) * 2.0 ** -24
        assert (np.abs(grids[k].astype(np.float64) - sol) <= tol).all(), k
        for name in ("n_ties", "rej_den", "rej_residual", "rej_side", "solved"):
            assert rep[name][k] == reps[k][name], (k, name)
        # the report's doubles come from the sums and the unclamped solution: 1e-9 relative to rms_before (rms_after is a difference of
        # terms of that size); max_shift is read off the float grid
        for name in ("rms_before", "rms_after"):
            assert abs(rep[name][k] - reps[k][name]) <= 1e-9 * reps[k]["rms_before"], (k, name, rep[name][k], reps[k][name])
        assert abs(rep["max_shift"][k] - reps[k]["max_shift"]) <= 2.0 ** -23 * reps[k]["max_shift"], (k, rep["max_shift"][k], reps[k]["max_shift"])
    return grids, rep


def test_host_solve_equals_the_restatement(surveys, edge):
    s = surveys[2]
    st = lr.stats(s["rec"], s["w"], s["h"], s["h9s"])
    grids, rep = check_solve(st, s["n"])
    assert rep["solved"].all() and (rep["rms_after"] < rep["rms_before"]).all()
    check_solve(st, s["n"], smooth=0.0, prior=1e-3)
    check_solve(st, s["n"], smooth=50.0, prior=4.0, max_shift=0.5)            # the clamp takes hold
    g, rep = check_solve(edge["stats"], edge["n"], **edge["params"])
    assert rep["solved"][3] == 0 and not g[3].any() and not g[4].any()        # 4 kept sides < min_ties, and the frame that takes no part
    for grid in ((1, 1), (16, 16)):
        p = dict(grid_x=grid[0], grid_y=grid[1])
        check_solve(lr.stats(s["rec"], s["w"], s["h"], s["h9s"], **p), s["n"], **p)
    # two calls, the same bits
    again, _ = im.solve_local_warps(st, s["n"])
    assert np.array_equal(again.view(np.uint32), grids.view(np.uint32))


def test_host_solve_gives_the_same_bits_for_every_thread_count(tmp_path):
    code = ("import hashlib, sys, numpy as np\n"
            "sys.path.insert(0, %r)\n"
            "import imagemosaicing_amd as im\n"
            "from tests import local_warp_cases as lc, local_warp_ref as lr\n"
            "s = lc.survey(seed=3)\n"
            "st = im.tie_residual_stats_host(s['rec'], s['w'], s['h'], s['h9s'])\n"
            "g, rep = im.solve_local_warps(st, s['n'])\n"
            "print(hashlib.sha256(g.tobytes() + rep.tobytes()).hexdigest())\n" % ROOT)
    out = []
    for threads in ("1", "3", "8"):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, MI355_HOST_THREADS=threads), timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out.append(r.stdout.strip())
    assert len(out[0]) == 64 and out[0] == out[1] == out[2]


def test_host_refusals_name_the_value(surveys):
    s = surveys[1]
    st = lr.stats(s["rec"], s["w"], s["h"], s["h9s"])
    bad = [("grid_x", dict(grid_x=0)), ("grid_x", dict(grid_x=17)), ("grid_y", dict(grid_y=0)), ("grid_y", dict(grid_y=17)),
           ("max_residual", dict(max_residual=float("nan"))), ("max_residual", dict(max_residual=0.0)), ("max_shift", dict(max_shift=float("inf"))),
           ("max_shift", dict(max_shift=0.0)), ("max_shift", dict(max_shift=64.5)), ("smooth", dict(smooth=-1.0)), ("smooth", dict(smooth=float("nan"))),
           ("prior", dict(prior=0.0)), ("prior", dict(prior=float("inf"))), ("min_ties", dict(min_ties=-1))]
    for word, kw in bad:
        for call in (lambda: im.tie_residual_stats_host(s["rec"], s["w"], s["h"], s["h9s"], **kw), lambda: im.solve_local_warps(st, s["n"], **kw)):
            with pytest.raises(im.Mi355Error) as e:
                call()
            assert e.value.code == -1 and word in str(e.value), (word, str(e.value))
    p = im.local_warp_params()
    p.reserved = 1
    with pytest.raises(im.Mi355Error, match="reserved"):
        im.solve_local_warps(st, s["n"], params=p)
    for w, h, word in (([160] * 5 + [8], s["h"], "grid_x"), (s["w"], [120] * 5 + [6], "grid_y"), ([160] * 5 + [1], s["h"], "w="), (s["w"], [120] * 5 + [(1 << 20) + 1], "h=")):
        with pytest.raises(im.Mi355Error) as e:
            im.tie_residual_stats_host(s["rec"], w, h, s["h9s"])
        assert word in str(e.value) and "frame 5" in str(e.value)
    neg = st.copy()
    neg[3] = -1
    with pytest.raises(im.Mi355Error, match="negative"):
        im.solve_local_warps(neg, s["n"])
    # a frame that takes no part may have any size
    h9s = s["h9s"].copy()
    h9s[5, 8] = 0.0
    im.tie_residual_stats_host(s["rec"], [160] * 5 + [1], s["h"], h9s)


# ---- properties of the definition ----------------------------------------------------------------------------------------------------------
def test_shuffled_records_and_ties_give_the_same_sums(surveys, edge):
    rng = np.random.default_rng(0)
    for s, p in ((surveys[1], {}), (edge, edge["params"])):
        rec = s["rec"].copy()
        rng.shuffle(rec)
        for r in rec:
            m = int(r["n_in"])
            if 1 <= m <= 400:
                o = rng.permutation(m)
                r["a"][:m], r["b"][:m] = r["a"][:m][o], r["b"][:m][o]
        assert np.array_equal(lr.stats(rec, s["w"], s["h"], s["h9s"], **p), lr.stats(s["rec"], s["w"], s["h"], s["h9s"], **p))


def test_a_tie_on_a_node_touches_one_node():
    w, h = lc.EDGE_W, lc.EDGE_H
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    NN, sd = 63, lr.stride(8, 6)
    for u, v in ((0, 0), (8, 6), (3, 2), (8, 0), (0, 6)):
        p = np.array([[12.0 * u, 12.0 * v]], np.float32)
        st = lr.stats(lc.records([(0, 1, p, p)]), [w] * 2, [h] * 2, h9s)
        for k in range(2):
            blk = st[k * sd:(k + 1) * sd]
            assert np.flatnonzero(blk[:7 * NN]).tolist() == [v * 9 + u] and blk[v * 9 + u] == 65536 ** 2      # residual 0: the b sums stay zero
            assert blk[7 * NN:7 * NN + 5].tolist() == [1, 0, 0, 0, 0]
    # with a displacement, the same node's right-hand sides and nothing else: r = (2, -1), m = (36, 24) is node (3, 2) of both frames
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    a, b = np.array([[35.0, 24.5]], np.float32), np.array([[37.0, 23.5]], np.float32)
    st = lr.stats(lc.records([(0, 1, a, b)]), [w] * 2, [h] * 2, h9s)
    q = 2 * 9 + 3
    for k, (dx, dy) in enumerate(((-1.0, 0.5), (1.0, -0.5))):
        blk = st[k * sd:(k + 1) * sd]
        assert np.flatnonzero(blk[:7 * NN]).tolist() == [q, 5 * NN + q, 6 * NN + q]
        assert blk[5 * NN + q] == 65536 * int(256 * dx) and blk[6 * NN + q] == 65536 * int(256 * dy) and blk[7 * NN + 1] == 256 * 256 + 128 * 128


def test_the_zero_grid_is_the_identity():
    rng = np.random.default_rng(3)
    for (w, h), (gx, gy) in (((2, 2), (1, 1)), ((3, 2), (2, 1)), ((33, 29), (8, 6)), ((97, 73), (16, 16)), ((40, 31), (39, 30))):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out, n = lr.apply(img, np.zeros((gy + 1, gx + 1, 2), np.float32))
        assert np.array_equal(out, img) and n == 0
        # a grid too small to reach the Q8 nodes is the zero grid
        out, n = lr.apply(img, np.full((gy + 1, gx + 1, 2), 0.0019, np.float32))
        assert np.array_equal(out, img) and n == 0


def test_ties_in_one_corner_stay_bounded_and_decay():
    w, h = 160, 120
    rng = np.random.default_rng(4)
    a = np.stack([rng.uniform(2, 30, 300), rng.uniform(2, 25, 300)], -1)
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    for shift, ms in ((3.0, 8.0), (7.0, 2.0)):
        b = a + [shift, 0.0]                                                  # r = (shift, 0): frame 0 wants D = -shift / 2 in that corner, frame 1 +
        st = lr.stats(lc.records([(0, 1, a.astype(np.float32), b.astype(np.float32))]), [w] * 2, [h] * 2, h9s, max_shift=8.0)
        grids, _, reps = lr.solve(st, 2, **dict(lr.DEFAULTS, max_shift=ms))
        assert reps[0]["solved"] and reps[0]["n_ties"] == 300
        g = grids[0][..., 0]
        assert np.abs(grids).max() <= ms
        assert g[0, 0] < 0 and abs(g[0, 0]) >= min(ms, 0.4 * shift)
        # where there are no ties the solution obeys smooth * Laplacian = prior * D: it falls by exp(-sqrt(prior / smooth)) = 0.70 per node,
        # to 0.12 over the six nodes between the ties and the far columns; twice that is allowed
        assert abs(g[-1, -1]) < 0.25 * abs(g[0, 0]) and abs(g[0, -1]) < 0.25 * abs(g[0, 0])
        m = np.abs(g)
        assert (np.diff(m[0, 1:]) <= 1e-6).all() and (np.diff(m[1:, 0]) <= 1e-6).all()      # away from the ties the field only falls
        assert np.abs(grids[0][..., 1]).max() < 0.02 * abs(g[0, 0]) + 1e-3
        assert np.allclose(grids[1], -grids[0], atol=2e-2 * shift)


# ---- quality ---------------------------------------------------------------------------------------------------------------------------------
def test_the_ties_disagreement_falls(surveys):
    for seed in SEEDS:
        s = surveys[seed]
        _, grids, reps = lc.register(s)
        before, after = lc.disagreement(s), lc.disagreement(s, grids)
        print("seed %d: %d ties, rms disagreement %.3f -> %.3f px, ratio %.3f" % (seed, s["rec"]["n_in"].sum(), before, after, after / before))
        assert all(r["solved"] for r in reps) and before > 1.0
        assert after / before <= RATIO_BOUND


def test_a_planar_survey_with_exact_ties_is_left_alone():
    s = lc.survey(seed=1, amp=0.0)
    st, grids, reps = lc.register(s)
    assert all(r["solved"] and r["rej_residual"] == 0 and r["rej_side"] == 0 for r in reps)
    assert not lr.node_q8(grids).any()
    rng = np.random.default_rng(1)
    for k in range(s["n"]):
        img = rng.integers(0, 256, (s["h"][k], s["w"][k], 3), dtype=np.uint8)
        out, n = lr.apply(img, grids[k])
        assert np.array_equal(out, img) and n == 0
    g, rep = im.solve_local_warps(im.tie_residual_stats_host(s["rec"], s["w"], s["h"], s["h9s"]), s["n"])
    assert not lr.node_q8(g).any()


def test_tie_noise_on_a_planar_survey_moves_little():
    for seed in SEEDS:
        s = lc.survey(seed=seed, amp=0.0, noise=0.5)
        _, grids, _ = lc.register(s)
        print("seed %d: largest |D| %.3f px" % (seed, np.abs(grids).max()))
        assert np.abs(grids).max() <= HARM_BOUND


def test_two_frames_agree_better_after_the_apply():
    s = lc.survey(n=2, seed=6, amp=2.5)
    assert len(s["rec"]) == 1 and s["rec"]["n_in"][0] > 100
    imgs = [lc.render(s, k) for k in range(2)]
    _, grids, _ = lc.register(s)
    before = lc.photometric_difference(s, imgs, 0, 1)
    after = lc.photometric_difference(s, [lr.apply(imgs[k], grids[k])[0] for k in range(2)], 0, 1)
    print("mean absolute gray difference %.2f -> %.2f" % (before, after))
    assert after < before
