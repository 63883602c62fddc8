"""CPU: the projective refinement's host side (mi355_pair_normal_blocks_host, mi355_global_projective_refine*) against tests/projective_ref.py.

Measured on the cases below (tests/projective_cases.py, seed 1 unless stated):
  * loop against the ref: the largest corner difference between the ref solving by Cholesky and by numpy.linalg.lstsq is 1.1e-12 px (grid16)
    to 1.4e-9 px (strip12, noisy, prior 0); 100 times that stays below one float32 ulp of the largest canvas coordinate (1.2e-4 px at 1613 on
    grid16, 2.4e-4 px at 3814 on strip12), so the float32 ulp is the bound on every case: the library's corners differ from the ref's by
    4.1e-5 .. 1.3e-4 px, the rounding of its float32 output.
  * strip12 / exact / prior 0 runs on seed 2: with seed 1 the exact ties converge to the float32 rounding floor of the tie points (cost 9e-8)
    where `c' < c` is decided by the last bit, and the library takes one more (rejected) trial than the ref.
  * ground truth, grid16 exact, prior 0: the ref ends 1.5e-4 px from the truth (the prototype: 1e-4), the library 1.7e-4; the bound is 1.5e-3.
  * grid16 with 0.5 px noise at the default prior: data rms 1.105 -> 0.977 px; the largest distance of a corner from the affine start is
    3.2 px (the prototype: 4.3 px).  Recorded, not asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest

import imagemosaicing_amd as im
from tests import projective_cases as pc
from tests import projective_ref as pr

_CACHE = {}


def _survey(name, noise, seed=1):
    key = (name, noise, seed)
    if key not in _CACHE:
        _CACHE[key] = pc.survey(name, noise, seed)
    return _CACHE[key]


def _edge():
    if "edge" not in _CACHE:
        recs, h8, part = pc.edge_records()
        _CACHE["edge"] = (recs, h8, part, pr.blocks(recs, h8, part))
    return _CACHE["edge"]


def _same_blocks(got, want):
    for p, (g, w) in enumerate(zip(got, want)):
        assert (int(g["i"]), int(g["j"]), int(g["n_in"])) == (w["i"], w["j"], w["n_in"]), p
        assert g["N"].tobytes() == w["N"].tobytes() and g["g"].tobytes() == w["g"].tobytes(), p
        assert np.float64(g["cost"]).tobytes() == np.float64(w["cost"]).tobytes(), p


def _refine(s, **kw):
    fixed, label = kw.pop("fixed", None), kw.pop("label", None)
    return im.global_projective_refine_results(s["recs"], s["w"], s["h"], kw.pop("start", s["start"]), fixed=fixed, label=label, params=im.projective_params(**kw))


@pytest.mark.parametrize("count", pc.EDGE_COUNTS)
def test_host_blocks_equal_ref_bits_on_edge_records(count):
    recs, h8, part, want = _edge()
    _same_blocks(im.pair_normal_blocks_host(recs[:count], h8, part), want[:count])
    if count == 257:
        kept = [(w["n_in"], float(w["cost"])) for w in want]
        assert kept[9] == (401, 0.0) and kept[10][0] == recs["n_in"][10] and kept[10][1] == 0.0       # malformed: zero block, n_in kept
        assert kept[3] == (0, 0.0) and kept[4] == (0, 0.0) and kept[6] == (0, 0.0) and kept[12] == (0, 0.0)
        assert kept[1][1] > 0 and kept[2][1] > 0 and kept[8][1] > 0
        assert sum(1 for p in range(20, 60) if kept[p][1] > 0) == 40


@pytest.mark.parametrize("name", ["grid16", "strip12"])
def test_host_blocks_equal_ref_bits_on_surveys(name):
    s = _survey(name, 0.5)
    part, h8 = pr.start_state(s["start"], None, None)
    _same_blocks(im.pair_normal_blocks_host(s["recs"], h8, part), pr.blocks(s["recs"], h8, part))


def test_ref_gradient_is_minus_half_the_cost_gradient():
    """the ref's g of a pair = -1/2 of the central-difference gradient of its cost, steps 1e-6 * max(|h_j|, scale_j), within 1e-6 of the largest
    entry (truncation plus rounding of such a difference is of order eps^(2/3) = 4e-11: four decades of room)"""
    s = _survey("grid16", 0.5)
    part, h8 = pr.start_state(s["start"], None, None)
    part[:] = 1
    scale = np.array([1.0, 1.0, 640.0, 1.0, 1.0, 640.0, 1e-3, 1e-3])
    for p in (0, 7, 20):
        rec = s["recs"][p]
        b = pr.block(rec, h8, part)
        num = np.zeros(16)
        for side_, img in ((0, b["i"]), (1, b["j"])):
            for j in range(8):
                d = 1e-6 * max(abs(h8[img, j]), scale[j])
                hp, hm = h8.copy(), h8.copy()
                hp[img, j] += d
                hm[img, j] -= d
                num[8 * side_ + j] = (pr.block(rec, hp, part)["cost"] - pr.block(rec, hm, part)["cost"]) / (hp[img, j] - hm[img, j])
        want = -0.5 * num
        print("gradient check pair", p, "largest entry %.4g" % np.abs(b["g"]).max(), "largest difference %.3g" % np.abs(b["g"] - want).max())
        assert np.abs(b["g"] - want).max() <= 1e-6 * np.abs(b["g"]).max()


LOOP_CASES = [(name, noise, prior) for name in ("grid16", "strip12") for noise in (0.0, 0.5) for prior in (0.0, 0.01)]


@pytest.mark.parametrize("name,noise,prior", LOOP_CASES)
def test_loop_against_ref(name, noise, prior):
    seed = 2 if (name, noise, prior) == ("strip12", 0.0, 0.0) else 1            # see the header
    s = _survey(name, noise, seed)
    out, rep = _refine(s, prior=prior)
    h_chol, free, r_chol = pr.refine(s["recs"], s["w"], s["h"], s["start"], prior=prior)
    h_lsq, _, r_lsq = pr.refine(s["recs"], s["w"], s["h"], s["start"], prior=prior, solver="lstsq")
    assert (rep["trials"], rep["accepted"]) == (r_chol["trials"], r_chol["accepted"])
    assert (rep["n_free"], rep["n_pairs_used"], rep["n_points"]) == (r_chol["n_free"], r_chol["n_pairs_used"], r_chol["n_points"])
    assert rep["cost0"] == r_chol["cost0"]                    # the start's system is the same bits: blocks, order of assembly
    c_lib, c_chol, c_lsq = (pr.corners(x, s["w"], s["h"]) for x in (pr.transforms_h8(out), h_chol, h_lsq))
    own = np.abs(c_chol - c_lsq).max() if (r_chol["trials"], r_chol["accepted"]) == (r_lsq["trials"], r_lsq["accepted"]) else 0.0
    bound = max(100.0 * own, float(np.spacing(np.float32(np.abs(c_chol).max()))))
    diff = np.abs(c_lib - c_chol).max()
    print(name, noise, prior, "trials", rep["trials"], "accepted", rep["accepted"], "ref cholesky-lstsq %.3g px" % own, "bound %.3g px" % bound, "library-ref %.3g px" % diff)
    assert diff <= bound


@pytest.mark.parametrize("name", ["grid16", "strip12"])
def test_exact_properties(name):
    s = _survey(name, 0.5)
    out, rep = _refine(s)
    assert rep["cost0"] < 1e7
    assert rep["cost_data"] + rep["cost_prior"] <= rep["cost0"] and rep["cost_data"] <= rep["cost0"]
    assert rep["accepted"] >= 1 and rep["cost_data"] < rep["cost0"]
    # fixed images, label-0 images and images that take no part come back bit for bit
    start = s["start"].copy()
    start["m"][5] *= 2.0                                       # m8 = 2: the same transform, normalised on the way out if the image is free
    start["m"][8][8] = 0.0                                     # takes no part
    fixed = np.zeros(s["n"], np.int32)
    fixed[[0, 3]] = 1
    label = np.ones(s["n"], np.int32)
    label[7] = 0
    out2, rep2 = _refine(s, start=start, fixed=fixed, label=label)
    for k in (0, 3, 7, 8):
        assert out2[k].tobytes() == start[k].tobytes(), k
    assert rep2["n_free"] == s["n"] - 4 and out2["m"][5][8] == 1.0 and (out2["fixed"][[1, 2, 5]] == 0).all()
    # max_iters = 0 returns the input
    out0, rep0 = _refine(s, max_iters=0)
    assert out0.tobytes() == s["start"].tobytes() and rep0["trials"] == 0 and rep0["cost_data"] == rep0["cost0"]
    # prior = 1e9: the prior outweighs the data 1e9 to 1 (and no rejected trial contributes): no corner leaves the start by 0.01 px
    outp, repp = _refine(s, prior=1e9)
    move = np.abs(pr.corners(pr.transforms_h8(outp), s["w"], s["h"]) - pr.corners(pr.transforms_h8(s["start"]), s["w"], s["h"])).max()
    print(name, "prior 1e9: largest corner move %.3g px" % move)
    assert move <= 0.01
    # the three forms give equal bits; two calls give equal bits
    flat = im.results_to_match_pairs(s["recs"])
    outf, repf = im.global_projective_refine(flat, s["w"], s["h"], s["start"])
    assert outf.tobytes() == out.tobytes() and repf == rep
    again, rep_again = _refine(s)
    assert again.tobytes() == out.tobytes() and rep_again == rep


def test_flat_list_cuts_runs_of_more_than_400():
    """a run of 500 equal (ptA_i, ptB_i) is two pairs of 400 and 100: the same bits as two records"""
    rng = np.random.default_rng(3)
    n = 500
    xy = rng.uniform(0, 600, (n, 2)).astype(np.float32)
    flat = np.zeros(n, im.MATCHPAIR)
    flat["ai"], flat["bi"] = 0, 1
    flat["ax"], flat["ay"] = xy[:, 0] + 100, xy[:, 1]
    flat["bx"], flat["by"] = xy[:, 0] + rng.normal(0, 0.3, n).astype(np.float32), xy[:, 1] + rng.normal(0, 0.3, n).astype(np.float32)
    recs = np.zeros(2, im.PAIR_RESULT)
    for p, (lo, hi) in enumerate(((0, 400), (400, 500))):
        recs["i"][p], recs["j"][p], recs["n_in"][p], recs["accepted"][p] = 0, 1, hi - lo, 1
        for f, g in (("a", "a"), ("b", "b")):
            recs[f]["x"][p, :hi - lo], recs[f]["y"][p, :hi - lo] = flat[g + "x"][lo:hi], flat[g + "y"][lo:hi]
    start = im.global_affine_align_results(recs, 2)
    w, h = np.full(2, 640, np.int32), np.full(2, 480, np.int32)
    a, ra = im.global_projective_refine(flat, w, h, start)
    b, rb = im.global_projective_refine_results(recs, w, h, start)
    assert a.tobytes() == b.tobytes() and ra == rb and ra["n_pairs_used"] == 2 and ra["n_points"] == 500


def test_no_free_image_or_no_used_pair_returns_the_input():
    s = _survey("strip12", 0.5)
    out, rep = _refine(s, fixed=np.ones(s["n"], np.int32))
    assert out.tobytes() == s["start"].tobytes() and all(v == 0 for v in rep.values())
    out, rep = im.global_projective_refine_results(np.zeros(0, im.PAIR_RESULT), s["w"], s["h"], s["start"])
    assert out.tobytes() == s["start"].tobytes() and all(v == 0 for v in rep.values())


def test_thread_counts_give_equal_bits(tmp_path):
    """a strip of 300 frames 10 px apart, every frame tied to its neighbour and to the frame 40 further on: 2392 unknowns with an envelope of
    320 columns, 8 x 299 x 320^2 = 2.4e8 multiply-subtracts per factorisation -- a team of 9 with 16 host threads, of 4 with 4, none with 1"""
    script = tmp_path / "projective_threads.py"
    script.write_text(
        "import sys, hashlib, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import imagemosaicing_amd as im\n"
        "from tests import projective_cases as pc\n"
        "n = 300\n"
        "G = [np.array([[1.0, 0, 10.0 * k], [0, 1.0, 0], [1e-6 * (k %% 3), 0, 1.0]]) for k in range(n)]\n"
        "G = [np.linalg.inv(G[0]) @ g for g in G]\n"
        "pairs = [(k, k + d) for k in range(n) for d in (1, 40) if k + d < n]\n"
        "recs = pc.records_from_truth(G, pairs, 11, noise=0.3, per_pair=40, min_keep=4)\n"
        "assert len(recs) == len(pairs)\n"
        "w, h = np.full(n, pc.W, np.int32), np.full(n, pc.H, np.int32)\n"
        "start = im.global_affine_align_results(recs, n)\n"
        "out, rep = im.global_projective_refine_results(recs, w, h, start, params=im.projective_params(max_iters=3))\n"
        "assert rep['n_free'] == n - 1 and rep['accepted'] >= 1 and np.isfinite(out['m']).all()\n"
        "print(hashlib.sha1(out.tobytes()).hexdigest(), rep['trials'], rep['accepted'], repr(rep['cost_data']), repr(rep['cost_prior']))\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    seen = set()
    for th in ("1", "4", "16"):
        r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, MI355_HOST_THREADS=th), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        seen.add(r.stdout.strip().splitlines()[-1])
    assert len(seen) == 1, seen


def test_ground_truth():
    s = _survey("grid16", 0.0)
    out, rep = _refine(s, prior=0.0)
    h_ref, _, _ = pr.refine(s["recs"], s["w"], s["h"], s["start"], prior=0.0)
    truth = pr.corners(pc.truth_h8(s["G"]), s["w"], s["h"])
    e_ref = np.abs(pr.corners(h_ref, s["w"], s["h"]) - truth).max()
    e_lib = np.abs(pr.corners(pr.transforms_h8(out), s["w"], s["h"]) - truth).max()
    e_start = np.abs(pr.corners(pr.transforms_h8(s["start"]), s["w"], s["h"]) - truth).max()
    print("grid16 exact, prior 0: corners from the truth: start %.3g px, ref %.3g px, library %.3g px" % (e_start, e_ref, e_lib))
    assert e_lib <= 10.0 * e_ref
    s = _survey("grid16", 0.5)
    out, rep = _refine(s)
    rms0, rms = np.sqrt(rep["cost0"] / rep["n_points"]), np.sqrt(rep["cost_data"] / rep["n_points"])
    move = np.abs(pr.corners(pr.transforms_h8(out), s["w"], s["h"]) - pr.corners(pr.transforms_h8(s["start"]), s["w"], s["h"])).max()
    print("grid16 noisy, default prior: data rms %.4g -> %.4g px, largest corner move from the start %.3g px (prototype: 4.3)" % (rms0, rms, move))
    assert rms < rms0


def test_argument_errors():
    s = _survey("strip12", 0.5)
    L = im.load_library()

    def err(match, code=-1, recs=None, w=None, h=None, **kw):
        with pytest.raises(im.Mi355Error, match=match) as e:
            im.global_projective_refine_results(s["recs"] if recs is None else recs, s["w"] if w is None else w, s["h"] if h is None else h, s["start"],
                                                params=im.projective_params(**kw))
        assert e.value.code == code
    err("max_iters = -1", max_iters=-1)
    err("prior = -", prior=-0.5)
    err("lambda0 = -", lambda0=-1.0)
    err("lambda_up = 1.0", lambda_up=1.0)
    err("lambda_down = 0.5", lambda_down=0.5)
    err("min_rel_decrease = -", min_rel_decrease=-1e-3)
    for name in ("prior", "lambda0", "lambda_up", "lambda_down", "min_rel_decrease"):
        err(name + " = (nan|inf)", **{name: float("nan")})
        err(name + " = (nan|inf)", **{name: float("inf")})
    err("image 3 is 1 x 480", w=np.where(np.arange(s["n"]) == 3, 1, s["w"]).astype(np.int32))
    err("image 4 is 640 x 0", h=np.where(np.arange(s["n"]) == 4, 0, s["h"]).astype(np.int32))
    bad = s["recs"].copy()
    bad["n_in"][2] = 401
    err("n_in = 401", recs=bad)
    bad = s["recs"].copy()
    bad["j"][1] = s["n"]
    err("outside", recs=bad)
    bad = s["recs"].copy()
    bad["a"]["x"][0, 0] = np.inf
    err("not finite", code=-2, recs=bad)
    # NULL pointers and n_images < 1, straight through the C ABI
    st, out = s["start"], np.zeros(s["n"], im.IMAGE_TRANSFORM)
    p = lambda a: a.ctypes.data
    import ctypes as C
    args = lambda **o: [C.c_void_p(o.get("r", p(s["recs"]))), len(s["recs"]), o.get("n", s["n"]), C.c_void_p(o.get("w", p(s["w"]))), C.c_void_p(o.get("h", p(s["h"]))), None, None,
                        C.c_void_p(o.get("start", p(st))), None, C.c_void_p(o.get("out", p(out))), None]
    for o, text in ((dict(n=0), "n_images = 0"), (dict(w=None), "NULL w"), (dict(h=None), "NULL h"), (dict(start=None), "NULL start"), (dict(out=None), "NULL out"), (dict(r=None), "NULL records")):
        assert L.mi355_global_projective_refine_results(*args(**o)) == -1
        assert text in L.mi355_last_error(None).decode(), (text, L.mi355_last_error(None))
    assert L.mi355_global_projective_refine_results(*args()) == 0            # report and params may be NULL
    assert L.mi355_pair_normal_blocks_host(None, 3, None, None, 4, None) == -1
