"""CPU: the lens self-calibration's host side (mi355_pair_calib_blocks_host, mi355_calibrate_lens*, mi355_match_pairs_to_results) against
tests/calib_ref.py on the cases of tests/calib_cases.py.

Bounds and where they come from:
  * blocks: bit for bit.
  * theta columns against central differences of the residual (step 1e-6, at the true camera where the fixed point settles to the last bit):
    truncation is of order step^2 times the third derivative and rounding 1e-16 * 520 / 1e-6 = 5e-8 px against columns of 10 .. 100 px, so 1e-6
    of a column's largest entry ("Lens self-calibration", Checks) leaves a decade.  The library's block of the same record
    at the same theta is held to the rows that are differentiated, bit for bit, so the check is of the library's columns.
  * loop against the ref loop (dense damped system, numpy): the same accepted-trial count and every free coefficient within 1e-9 of the
    reference's value, with noise and without, whatever the mask (measured: at most 6e-11, the largest for p2 of the tangential camera on
    exact ties).  The one exception is a coefficient whose truth is zero on EXACT ties (p1, p2 of the radial camera under mask 15): it ends
    at the rounding floor, 1.6e-8 and 1.7e-10 where both loops differ by 1e-16, a value that no relative bound describes; those two are
    compared absolutely, to 1e-9 of k1's size.
  * the step count and the tolerance of the fixed point (MI355_CALIB_STEPS, MI355_CALIB_TOL): test_fixed_point_constants_cover_the_stated_
    cameras states the cameras of the header's claim and holds reference and library to it.
  * the homography that the flat form fits to a run: against numpy's SVD solution of the header's shifted and scaled system on the same ties,
    kept in double, the two images of every tie within 1e-3 px
    (the library hands H over as floats: 6e-8 of entries that move a point by up to 640 px, 2e-4 px for the sum of the terms).
  * noisy runs (0.5 px, mask k1 | k2, seeds 1..3): the reference's own largest distort-map error per layout, times 1.25 (the project's quarter
    over a swept figure), bounds the library's; the library's error also lies within 10 % of the reference's on every case, and its rms within
    1.1 x the reference's.  Measured, reference = library to the digits shown (map error in px, rms in px):
        grid16   seed 1  0.0742  0.940 | seed 2  0.2506  0.963 | seed 3  0.6083  0.943      bound 0.760
        strip12  seed 1  0.6390  0.961 | seed 2  0.4636  0.985 | seed 3  0.3369  0.968      bound 0.799
    (the rms of a tie's two residual components under 0.5 px of noise on both coordinates of both sides is 1.0 px before any fit)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import imagemosaicing_amd as im
from tests import calib_cases as cc
from tests import calib_ref as cr

_CACHE = {}
TH0 = cc.CAM_START[4:]
THETAS = {"zero": TH0, "truth": cc.THETA_TRUE, "bad": cc.THETA_BAD}


def cam_of(theta, base=cc.CAM_TRUE):
    return tuple(base[:4]) + tuple(theta)


def same_blocks(got, want):
    for p, (g, w) in enumerate(zip(got, want)):
        assert (int(g["i"]), int(g["j"]), int(g["n_in"]), int(g["n_bad"])) == (w["i"], w["j"], w["n_in"], w["n_bad"]), p
        assert g["N"].tobytes() == w["N"].tobytes() and g["g"].tobytes() == w["g"].tobytes(), p
        assert np.float64(g["cost"]).tobytes() == np.float64(w["cost"]).tobytes(), p


def edge(which):
    """the edge records, their states and the reference's blocks at one theta (computed once)"""
    if "edge" not in _CACHE:
        _CACHE["edge"] = cc.edge_records()
    recs, h8 = _CACHE["edge"]
    if ("edge", which) not in _CACHE:
        _CACHE[("edge", which)] = cr.blocks(recs, h8, cam_of(THETAS[which]), THETAS[which])
    return recs, h8, _CACHE[("edge", which)]


def ref_run(name, noise, seed, mask, cam=cc.CAM_TRUE):
    key = ("run", name, noise, seed, mask, cam)
    if key not in _CACHE:
        _CACHE[key] = cr.calibrate(cc.survey(name, noise, seed, cam), cc.CAM_START, mask=mask)
    return _CACHE[key]


def lib_run(name, noise, seed, mask, cam=cc.CAM_TRUE):
    out, rep = im.calibrate_lens_results(cc.survey(name, noise, seed, cam), im.Camera(*cc.CAM_START), mask=mask)
    return cr.cam_tuple(out), rep


@pytest.mark.parametrize("which", ["zero", "truth", "bad"])
@pytest.mark.parametrize("count", cc.EDGE_COUNTS + (23,))
def test_host_blocks_equal_ref_bits_on_edge_records(count, which):
    recs, h8, want = edge(which)
    got = im.pair_calib_blocks_host(recs[:count], h8[:count], im.Camera(*cam_of(THETAS[which])))
    same_blocks(got, want[:count])
    if count == 23:
        assert [int(v) for v in got["n_in"][5:15]] == [0] + list(cc.EDGE_N_IN[1:])                 # min_ties - 1 is not used
        assert [int(got["n_in"][p]) for p in (15, 16, 17, 18, 20, 21)] == [0] * 6 and not got["cost"][[15, 16, 17, 18, 20, 21]].any()
        assert (got["cost"][[0, 1, 2, 3, 4, 19, 22]] > 0).all()
        if which == "bad":
            assert (got["n_bad"][got["n_in"] > 0] > 0).all() and (got["n_bad"] < got["n_in"])[[0, 4]].all()
        else:
            assert not got["n_bad"].any()


@pytest.mark.parametrize("which", ["zero", "truth"])
@pytest.mark.parametrize("name", ["grid16", "strip12"])
def test_host_blocks_equal_ref_bits_on_surveys(name, which):
    recs = cc.survey(name, 0.5)
    h8 = np.array([cr.start_state(r["H"], cc.CAM_START) for r in recs])
    cam = cam_of(THETAS[which])
    got = im.pair_calib_blocks_host(recs, h8, im.Camera(*cam))
    same_blocks(got, cr.blocks(recs, h8, cam, THETAS[which]))
    assert (got["n_in"] == recs["n_in"]).all()


def test_theta_columns_equal_central_differences():
    recs = cc.survey("grid16", 0.5, cam=cc.CAM_TANGENTIAL)
    theta = np.array(cc.CAM_TANGENTIAL[4:]) + np.array([0, 0, 0, 0, 0.01])
    for p in (0, 5, 17):
        r = recs[p]
        n = int(r["n_in"])
        h = cr.start_state(r["H"], cc.CAM_START)
        pts = [r[s][f][:n].astype(np.float64) for s, f in (("a", "x"), ("a", "y"), ("b", "x"), ("b", "y"))]
        X, Y, good = cr.tie_rows(cc.CAM_TRUE, theta, h, *pts)
        assert good.all()
        # the library's block of this record at this theta is made of exactly these rows: what holds for their columns holds for its own
        got = im.pair_calib_blocks_host(recs[p:p + 1], h.reshape(1, 8), im.Camera(*cam_of(theta)))
        terms = np.empty((2 * n, 14, 14))
        terms[0::2], terms[1::2] = X[:, :, None] * X[:, None, :], Y[:, :, None] * Y[:, None, :]
        S = cr._ordered_sum(terms)
        assert int(got["n_in"][0]) == n and int(got["n_bad"][0]) == 0
        assert got["N"][0].tobytes() == S[np.tril_indices(13)].tobytes() and got["g"][0].tobytes() == S[13, :13].tobytes()
        for m in range(5):
            tp, tm = theta.copy(), theta.copy()
            tp[m] += 1e-6
            tm[m] -= 1e-6
            fd = (cr.residuals(cc.CAM_TRUE, tp, h, *pts) - cr.residuals(cc.CAM_TRUE, tm, h, *pts)) / (tp[m] - tm[m])
            for J, col in ((X, 0), (Y, 1)):
                err, size = np.abs(J[:, 8 + m] - fd[:, col]).max(), np.abs(J[:, 8 + m]).max()
                print("record", p, "theta", m, "xy"[col], "largest entry %.4g largest difference %.3g" % (size, err))
                assert err <= 1e-6 * size


def _corner_shift(theta):
    """how far the distort map of (CAM_TRUE's intrinsics, theta) moves the frame's corners, the largest of the four, in pixels"""
    x, y = np.array([0.0, cc.W - 1, 0.0, cc.W - 1]), np.array([0.0, 0.0, cc.H - 1, cc.H - 1])
    xs, ys = cc.distort_pixels(cc.CAM_TRUE[:4] + tuple(theta), x, y)
    return float(np.hypot(xs - x, ys - y).max())


def _scaled(direction, frac):
    """the multiple of `direction` (five coefficients) that moves a corner by frac of the half-diagonal (bisection from below)"""
    d, lo, hi = np.array(direction, np.float64), 0.0, 10.0
    want = frac * np.hypot(cc.CAM_TRUE[2], cc.CAM_TRUE[3])
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _corner_shift(d * mid) < want else (lo, mid)
    return d * lo


# direction in (k1, k2, p1, p2, k3), share of the half-diagonal, good at every pixel of the frame with the header's constants
FIXED_POINT_CAMERAS = [((1, 0, 0, 0, 0), 0.1, True), ((-1, 0, 0, 0, 0), 0.1, True), ((0, 1, 0, 0, 0), 0.1, True), ((0, 0, 0, 0, 1), 0.1, True),
                       ((0, 0, 1, 0, 0), 0.1, True), ((0, 0, -1, 0, 0), 0.1, True), ((0, 0, 0, 1, 0), 0.1, True), ((0, 0, 0, -1, 0), 0.1, True),
                       ((-1, 0.25, 0.02, -0.02, 0), 0.1, True), ((1, 1, 0.05, 0.05, 1), 0.1, True), ((-1, 0.5, -0.03, 0.03, 0.5), 0.1, True),
                       ((0, -1, 0, 0, 0), 0.06, True), ((0, 0, 0, 0, -1), 0.04, True),
                       ((0, -1, 0, 0, 0), 0.1, False), ((0, 0, 0, 0, -1), 0.06, False), ((0, 0, 0, 0, -1), 0.1, False)]


def test_fixed_point_constants_cover_the_stated_cameras():
    """MI355_CALIB_STEPS and MI355_CALIB_TOL against the header's claim, on every pixel of the 640 x 480 frame with the reference and on a
    20 x 20 grid of ties that holds the four corners with the library (h = identity, both sides the same points)."""
    assert (cr.STEPS, cr.TOL) == (16, 1e-7)
    u, v = np.meshgrid(np.arange(cc.W, dtype=np.float64), np.arange(cc.H, dtype=np.float64))
    gx, gy = np.meshgrid(np.linspace(0, cc.W - 1, 20), np.linspace(0, cc.H - 1, 20))
    rec = cc.make_record(0, 1, gx.ravel(), gy.ravel(), gx.ravel(), gy.ravel(), 1, np.eye(3, dtype=np.float32).reshape(9))
    h = np.array([[1.0, 0, 0, 0, 1.0, 0, 0, 0]])
    for direction, frac, everywhere in FIXED_POINT_CAMERAS:
        theta = _scaled(direction, frac)
        assert abs(_corner_shift(theta) - frac * 399.3) < 0.01
        good = cr.undistort_points(cc.CAM_TRUE, theta, u, v)[3]
        lib = im.pair_calib_blocks_host(rec, h, im.Camera(*cam_of(theta)))
        print(direction, frac, ["%.4g" % t for t in theta], "pixels not good", int((~good).sum()), "library n_bad", int(lib["n_bad"][0]))
        assert bool(good.all()) == everywhere
        assert int(lib["n_in"][0]) == 400 and int(lib["n_bad"][0]) == cr.block(rec[0], h[0], cam_of(theta), theta)["n_bad"]
        assert (int(lib["n_bad"][0]) == 0) == everywhere          # where the frame is not good everywhere, its corners are not
    # the slowest of the stated cameras, k3 alone, is what the step count is for: 14 steps leave its corners unsettled, 15 settle them
    theta = _scaled((0, 0, 0, 0, 1), 0.1)
    assert not cr.undistort_points(cc.CAM_TRUE, theta, u, v, steps=14)[3].all()
    assert cr.undistort_points(cc.CAM_TRUE, theta, u, v, steps=15)[3].all()


def test_gradient_part_is_minus_half_the_cost_gradient():
    """the library's g of a record = -1/2 of the central-difference gradient of the library's cost over the 8 state values and theta, within
    1e-6 of the largest entry (steps 1e-6 of the entry's scale)"""
    recs = cc.survey("grid16", 0.5)
    theta0 = np.array([-0.1, 0.02, 0.001, -0.001, 0.01])
    for p in (0, 11):
        rec = recs[p:p + 1]
        h0 = cr.start_state(rec[0]["H"], cc.CAM_START)
        cost = lambda h, t: float(im.pair_calib_blocks_host(rec, h.reshape(1, 8), im.Camera(*cam_of(t)))["cost"][0])
        g = im.pair_calib_blocks_host(rec, h0.reshape(1, 8), im.Camera(*cam_of(theta0)))["g"][0]
        num = np.zeros(13)
        for k in range(13):
            hp, hm, tp, tm = h0.copy(), h0.copy(), theta0.copy(), theta0.copy()
            if k < 8:
                d = 1e-6 * max(abs(h0[k]), 1e-2)
                hp[k] += d
                hm[k] -= d
                num[k] = (cost(hp, tp) - cost(hm, tm)) / (hp[k] - hm[k])
            else:
                tp[k - 8] += 1e-7
                tm[k - 8] -= 1e-7
                num[k] = (cost(hp, tp) - cost(hm, tm)) / (tp[k - 8] - tm[k - 8])
        print("gradient check record", p, "largest entry %.4g largest difference %.3g" % (np.abs(g).max(), np.abs(g + 0.5 * num).max()))
        assert np.abs(g + 0.5 * num).max() <= 1e-6 * np.abs(g).max()


LOOP_CASES = [("grid16", 0.0, 3, cc.CAM_TRUE), ("strip12", 0.0, 3, cc.CAM_TRUE), ("grid16", 0.5, 3, cc.CAM_TRUE), ("strip12", 0.5, 3, cc.CAM_TRUE),
              ("grid16", 0.0, 15, cc.CAM_TANGENTIAL), ("strip12", 0.5, 15, cc.CAM_TANGENTIAL), ("grid16", 0.0, 15, cc.CAM_TRUE), ("grid16", 0.5, 31, cc.CAM_TRUE)]


@pytest.mark.parametrize("name,noise,mask,cam", LOOP_CASES)
def test_loop_against_ref(name, noise, mask, cam):
    want, wrep = ref_run(name, noise, 1, mask, cam)
    got, rep = lib_run(name, noise, 1, mask, cam)
    print(name, noise, mask, "ref", want[4:], wrep, "lib", got[4:], rep)
    assert rep["accepted"] == wrep["accepted"] >= 3
    assert (rep["n_pairs_used"], rep["n_points"], rep["n_unused_records"]) == (wrep["n_pairs_used"], wrep["n_points"], wrep["n_unused_records"])
    assert rep["cost0"] == wrep["cost0"]
    assert got[:4] == want[:4] == cc.CAM_START[:4]
    for m in range(5):
        if not mask >> m & 1:
            assert got[4 + m] == 0.0
        elif cam[4 + m] == 0.0 and noise == 0.0:            # zero up to rounding: see the module docstring
            assert abs(got[4 + m] - want[4 + m]) <= 1e-9 * abs(cam[4]), m
        else:
            print("coefficient", m, "relative difference %.3g" % (abs(got[4 + m] - want[4 + m]) / abs(want[4 + m])))
            assert abs(got[4 + m] - want[4 + m]) <= 1e-9 * abs(want[4 + m]), m


@pytest.mark.parametrize("name", ["grid16", "strip12"])
@pytest.mark.parametrize("mask,cam", [(3, cc.CAM_TRUE), (15, cc.CAM_TRUE), (15, cc.CAM_TANGENTIAL)])
def test_exact_ties_recover_the_camera(name, mask, cam):
    got, rep = lib_run(name, 0.0, 1, mask, cam)
    err = cc.map_error(got, cam)
    print(name, mask, got[4:], "map error %.3g px, rms %.3g -> %.3g px" % (err, np.sqrt(rep["cost0"] / rep["n_points"]), np.sqrt(rep["cost"] / rep["n_points"])))
    assert err <= 1e-3
    assert cc.map_error(cc.CAM_START, cam) > 20            # what the start camera is off by


@pytest.mark.parametrize("name", ["grid16", "strip12"])
def test_noisy_ties(name):
    ref_err, rows = [], []
    for seed in (1, 2, 3):
        want, wrep = ref_run(name, 0.5, seed, 3)
        got, rep = lib_run(name, 0.5, seed, 3)
        e_ref, e_lib = cc.map_error(want, cc.CAM_TRUE), cc.map_error(got, cc.CAM_TRUE)
        rms_ref, rms_lib = np.sqrt(wrep["cost"] / wrep["n_points"]), np.sqrt(rep["cost"] / rep["n_points"])
        print(name, "seed", seed, "map error ref %.4f lib %.4f px, rms ref %.4f lib %.4f px (start %.3f)" % (e_ref, e_lib, rms_ref, rms_lib, np.sqrt(rep["cost0"] / rep["n_points"])))
        ref_err.append(e_ref)
        rows.append((e_ref, e_lib, rms_ref, rms_lib))
    bound = 1.25 * max(ref_err)
    for e_ref, e_lib, rms_ref, rms_lib in rows:
        assert e_lib <= bound and abs(e_lib - e_ref) <= 0.1 * e_ref
        assert rms_lib <= 1.1 * rms_ref and rms_lib < 1.1


def test_thread_counts_give_equal_bits(tmp_path):
    script = tmp_path / "calib_threads.py"
    script.write_text(
        "import sys, hashlib\nsys.path.insert(0, %r)\nimport numpy as np\nimport imagemosaicing_amd as im\nfrom tests import calib_cases as cc\n"
        "recs = np.concatenate([cc.survey('grid16', 0.5, seed) for seed in range(1, 11)])\n"
        "assert len(recs) >= 256 and recs['n_in'].sum() > 4000\n"
        "out, rep = im.calibrate_lens_results(recs, im.Camera(*cc.CAM_START), mask=15)\n"
        "assert rep['accepted'] >= 3 and rep['n_pairs_used'] == len(recs)\n"
        "print(hashlib.sha1(bytes(out)).hexdigest(), rep['trials'], rep['accepted'], repr(rep['cost']), repr(rep['lambda']))\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    seen = set()
    for th in ("1", "4", "16"):
        r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, MI355_HOST_THREADS=th), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        seen.add(r.stdout.strip().splitlines()[-1])
    assert len(seen) == 1, seen


def test_flat_list_equals_results_form_and_cuts_runs_at_400():
    flat = cc.flat_survey("strip12", 0.5, per_pair=1100)
    recs = im.match_pairs_to_results(flat)
    runs = np.flatnonzero(np.r_[True, (flat["ai"][1:] != flat["ai"][:-1]) | (flat["bi"][1:] != flat["bi"][:-1])])
    lengths = np.diff(np.r_[runs, len(flat)])
    assert lengths.max() > 400 and len(recs) == sum(-(-int(v) // 400) for v in lengths) > len(lengths)
    assert int(recs["n_in"].sum()) == len(flat) and recs["n_in"].max() == 400 and recs["accepted"].all() and (recs["H"][:, 8] == 1).all()
    k, same, worst_fit = 0, None, 0.0
    for r in recs:                                  # the ties in order, untouched
        n = int(r["n_in"])
        assert (r["i"], r["j"]) == (flat["ai"][k], flat["bi"][k])
        assert r["a"]["x"][:n].tobytes() == flat["ax"][k:k + n].tobytes() and r["b"]["y"][:n].tobytes() == flat["by"][k:k + n].tobytes()
        x, y = r["b"]["x"][:n].astype(np.float64), r["b"]["y"][:n].astype(np.float64)
        Hm = r["H"].astype(np.float64).reshape(3, 3)
        d = Hm[2, 0] * x + Hm[2, 1] * y + 1
        fit = np.hypot((Hm[0, 0] * x + Hm[0, 1] * y + Hm[0, 2]) / d - r["a"]["x"][:n], (Hm[1, 0] * x + Hm[1, 1] * y + Hm[1, 2]) / d - r["a"]["y"][:n])
        assert np.sqrt((fit ** 2).mean()) < 4.0        # the fitted H explains its ties to the lens error (2 px rms) and the noise
        # ... and is the header's least-squares homography of the run (shifted and scaled sides): numpy's solution of the same system by SVD,
        # kept in double, maps every tie to the same place
        xa, ya = r["a"]["x"][:n].astype(np.float64), r["a"]["y"][:n].astype(np.float64)
        ma, mb = np.array([xa.mean(), ya.mean()]), np.array([x.mean(), y.mean()])
        sa = 1 / np.sqrt(((xa - ma[0]) ** 2 + (ya - ma[1]) ** 2).mean())
        sb = 1 / np.sqrt(((x - mb[0]) ** 2 + (y - mb[1]) ** 2).mean())
        xan, yan, xn, yn = (xa - ma[0]) * sa, (ya - ma[1]) * sa, (x - mb[0]) * sb, (y - mb[1]) * sb
        z, o = np.zeros(n), np.ones(n)
        A = np.concatenate([np.stack([xn, yn, o, z, z, z, -xan * xn, -xan * yn], 1), np.stack([z, z, z, xn, yn, o, -yan * xn, -yan * yn], 1)])
        g = np.append(np.linalg.lstsq(A, np.concatenate([xan, yan]), rcond=None)[0], 1.0).reshape(3, 3)
        un, vn, dn = g[0, 0] * xn + g[0, 1] * yn + g[0, 2], g[1, 0] * xn + g[1, 1] * yn + g[1, 2], g[2, 0] * xn + g[2, 1] * yn + 1
        apart = np.hypot((Hm[0, 0] * x + Hm[0, 1] * y + Hm[0, 2]) / d - (un / dn / sa + ma[0]),
                         (Hm[1, 0] * x + Hm[1, 1] * y + Hm[1, 2]) / d - (vn / dn / sa + ma[1])).max()
        worst_fit = max(worst_fit, apart)
        assert apart <= 1e-3, (k, apart)
        k += n
    print("fitted H against numpy's least squares: images of a tie at most %.3g px apart" % worst_fit)
    for mask in (3, 15):
        a, arep = im.calibrate_lens(flat, im.Camera(*cc.CAM_START), mask=mask)
        b, brep = im.calibrate_lens_results(recs, im.Camera(*cc.CAM_START), mask=mask)
        same = (a, b) if mask == 3 else same
        assert bytes(a) == bytes(b) and arep == brep and arep["n_pairs_used"] == len(recs) and arep["accepted"] >= 3
    # another H for the same ties is another start, not another answer
    other = recs.copy()
    other["H"][:, 2] += 1.0
    c, _ = im.calibrate_lens_results(other, im.Camera(*cc.CAM_START), mask=3)
    b = same[1]
    assert abs(c.k1 - b.k1) < 1e-5 * abs(b.k1) and bytes(c) != bytes(b)


def test_no_used_record_returns_the_start_camera():
    start = im.Camera(520.0, 520.0, 256.0, 240.0, 0.01, -0.02, 0.001, 0.002, 0.003)
    recs, _ = cc.edge_records()
    sets = [recs[:0], recs[[5, 15, 16, 17, 18, 21]], cc.bad_scale_records()]
    for s in sets:
        out, rep = im.calibrate_lens_results(s, start)
        assert bytes(out) == bytes(start)
        assert rep == dict(trials=0, accepted=0, n_pairs_used=0, n_unused_records=0, n_points=0, cost0=0.0, cost=0.0) | {"lambda": 0.0}
    h8 = np.array([cr.start_state(r["H"], cr.cam_tuple(start)) for r in sets[2]])
    assert (~np.isfinite(h8)).any(axis=1).all()
    # beside used records the unused accepted ones are counted
    mixed = np.concatenate([cc.survey("strip12", 0.5), cc.bad_scale_records(), recs[[15]]])
    out, rep = im.calibrate_lens_results(mixed, im.Camera(*cc.CAM_START[:2], 256.0, 240.0, 0, 0, 0, 0, 0))
    assert rep["n_pairs_used"] == 11 and rep["n_unused_records"] == 3 and rep["accepted"] >= 3


def test_bad_ties_at_the_start_camera_fail_naming_record_and_tie():
    recs = cc.survey("strip12", 0.5)
    with pytest.raises(im.Mi355Error) as e:
        im.calibrate_lens_results(recs, im.Camera(*cam_of(cc.THETA_BAD)))
    assert e.value.code == -2 and "record 0 (0, 1)" in str(e.value) and "tie " in str(e.value)
    h8 = np.array([cr.start_state(r["H"], cc.CAM_START) for r in recs])
    X, Y, good = cr.tie_rows(cc.CAM_TRUE, cc.THETA_BAD, h8[0], *[recs[0][s][f][:recs[0]["n_in"]].astype(np.float64) for s, f in (("a", "x"), ("a", "y"), ("b", "x"), ("b", "y"))])
    assert "the first is tie %d " % int(np.flatnonzero(~good)[0]) in str(e.value)


def test_argument_errors():
    L = im.load_library()
    recs = np.ascontiguousarray(cc.survey("strip12", 0.5))
    flat = im.results_to_match_pairs(recs)
    good = cc.CAM_START

    def refused(text, cam=good, fn=im.calibrate_lens_results, data=recs, **kw):
        with pytest.raises(im.Mi355Error) as e:
            fn(data, im.Camera(*cam), **kw)
        assert e.value.code == -1 and text in str(e.value), (text, str(e.value))
        assert text in L.mi355_last_error(None).decode()

    for k, name in enumerate(cr.CAM_FIELDS):
        for v in (np.nan, np.inf):
            cam = list(good)
            cam[k] = v
            refused("camera %s = " % name, cam)
    refused("camera fx = 0.0", (0.0,) + good[1:])
    refused("camera fy = -520.0", (520.0, -520.0) + good[2:], fn=im.calibrate_lens, data=flat)
    for mask in (0, 32, 64, -1):
        refused("mask = %d" % mask, mask=mask)
    for mt in (7, 401, -3):
        refused("min_ties = %d" % mt, min_ties=mt)
    refused("max_iters = -1", max_iters=-1)
    for name, vals in (("lambda0", (-1e-3, np.nan, np.inf)), ("lambda_up", (1.0, -2.0, np.nan)), ("lambda_down", (1.0, np.inf)), ("min_rel_decrease", (-1e-9, np.nan))):
        for v in vals:
            refused(name + " = ", **{name: v})
            refused(name + " = ", fn=im.calibrate_lens, data=flat, **{name: v})
    # NULLs and counts straight through the C ABI
    cam, out, rep, par = im.Camera(*good), im.Camera(), im.CalibReport(), im.calib_params()
    rp, fp = recs.ctypes.data_as(C.c_void_p), flat.ctypes.data_as(C.c_void_p)
    for fn, args, text in (
            (L.mi355_calibrate_lens_results, (None, 3, C.byref(cam), None, C.byref(out), None), "n_pairs = 3 with NULL records"),
            (L.mi355_calibrate_lens_results, (rp, -1, C.byref(cam), None, C.byref(out), None), "n_pairs = -1"),
            (L.mi355_calibrate_lens_results, (rp, len(recs), None, None, C.byref(out), None), "NULL camera"),
            (L.mi355_calibrate_lens_results, (rp, len(recs), C.byref(cam), None, None, None), "NULL out"),
            (L.mi355_calibrate_lens, (None, 5, C.byref(cam), None, C.byref(out), None), "n = 5 with a NULL list"),
            (L.mi355_calibrate_lens, (fp, -2, C.byref(cam), None, C.byref(out), None), "n = -2"),
            (L.mi355_calibrate_lens, (fp, len(flat), None, C.byref(par), C.byref(out), C.byref(rep)), "NULL camera"),
            (L.mi355_calibrate_lens, (fp, len(flat), C.byref(cam), None, None, None), "NULL out"),
            (L.mi355_pair_calib_blocks_host, (None, 3, None, C.byref(cam), 16, None), "NULL records"),
            (L.mi355_pair_calib_blocks_host, (rp, 3, None, C.byref(cam), 16, None), "NULL h8"),
            (L.mi355_pair_calib_blocks_host, (rp, 3, rp, C.byref(cam), 16, None), "NULL out"),
            (L.mi355_pair_calib_blocks_host, (rp, 3, rp, None, 16, rp), "NULL camera"),
            (L.mi355_pair_calib_blocks_host, (rp, -1, rp, C.byref(cam), 16, rp), "n = -1"),
            (L.mi355_pair_calib_blocks_host, (rp, 3, rp, C.byref(cam), 5, rp), "min_ties = 5"),
            (L.mi355_match_pairs_to_results, (None, 2, None, 0, C.byref(C.c_int())), "n = 2 with a NULL list"),
            (L.mi355_match_pairs_to_results, (fp, len(flat), None, 0, None), "NULL n_out"),
            (L.mi355_match_pairs_to_results, (fp, len(flat), rp, 2, C.byref(C.c_int())), "cap = 2")):
        assert fn(*args) == -1, text
        assert text in L.mi355_last_error(None).decode(), (text, L.mi355_last_error(None))
    assert L.mi355_calibrate_lens_results(rp, len(recs), C.byref(cam), None, C.byref(out), None) == 0            # params and report may be NULL
    assert out.k1 != 0 and L.mi355_pair_calib_blocks_host(None, 0, None, C.byref(cam), 16, None) == 0
    L.mi355_default_calib_params(None)
    p = im.calib_params()
    assert (p.max_iters, p.mask, p.min_ties, p.lambda0, p.lambda_up, p.lambda_down, p.min_rel_decrease) == (20, 3, 16, 1e-3, 10.0, 10.0, 1e-6)
