"""Pair records for the lens self-calibration's tests, built from planar ground truth as tests/projective_cases.py builds its own: frames of
640 x 480 of one camera looking at one plane.  Ideal pinhole points are drawn from a box 40 px larger than the frame, mapped through the truth
homographies, and both sides are pushed through the true camera's distortion; a tie is kept where both observed sides lie in the frame.
Positions are rounded to float32, with optional Gaussian noise.  A record's H is the least-squares homography of its own observed ties (what
the pair stage would hand over), with H[8] replaced by a residual as Ransac2D leaves it.  Also the record edge cases of the block kernel."""
import numpy as np

import imagemosaicing_amd as im

W, H = 640, 480
MARGIN = 40.0
CAM_TRUE = (520.0, 520.0, 319.5, 239.5, -0.12, 0.03, 0.0, 0.0, 0.0)
CAM_TANGENTIAL = (520.0, 520.0, 319.5, 239.5, -0.12, 0.03, 0.002, -0.002, 0.0)
CAM_START = CAM_TRUE[:4] + (0.0,) * 5


def _apply(G, x, y):
    d = G[2, 0] * x + G[2, 1] * y + G[2, 2]
    return (G[0, 0] * x + G[0, 1] * y + G[0, 2]) / d, (G[1, 0] * x + G[1, 1] * y + G[1, 2]) / d


def truth_transforms(centres, seed, persp=2e-5, yaw_deg=8.0):
    """frame -> canvas homographies between the PINHOLE frames (projective_cases' construction with a wider yaw)"""
    rng = np.random.default_rng(seed)
    G = []
    for k, (cx, cy) in enumerate(centres):
        if k == 0:
            G.append(np.array([[1.0, 0, cx - W / 2.0], [0, 1.0, cy - H / 2.0], [0, 0, 1.0]]))
            continue
        yaw = np.deg2rad(rng.uniform(-yaw_deg, yaw_deg))
        s = 1 + rng.uniform(-0.02, 0.02)
        R = s * np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
        t = np.array([cx, cy]) - R @ np.array([W / 2.0, H / 2.0])
        A = np.array([[R[0, 0], R[0, 1], t[0]], [R[1, 0], R[1, 1], t[1]], [0, 0, 1.0]])
        Pm = np.array([[1.0, 0, 0], [0, 1.0, 0], [rng.uniform(-persp, persp), rng.uniform(-persp, persp), 1.0]])
        G.append(A @ Pm)
    G0inv = np.linalg.inv(G[0])
    return [G0inv @ g for g in G]


def distort_pixels(cam, x, y):
    """pinhole pixel -> observed pixel of the camera (double)"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam
    xn, yn = (x - cx) / fx, (y - cy) / fy
    r2 = xn * xn + yn * yn
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    tx = 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)
    ty = p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn
    return fx * (xn * rad + tx) + cx, fy * (yn * rad + ty) + cy


def fit_homography(xb, yb, xa, ya):
    """least-squares H (9 floats, H[8] = 1) with (xa, ya) ~ H (xb, yb)"""
    z, o = np.zeros_like(xb), np.ones_like(xb)
    A = np.concatenate([np.stack([xb, yb, o, z, z, z, -xa * xb, -xa * yb], 1), np.stack([z, z, z, xb, yb, o, -ya * xb, -ya * yb], 1)])
    h = np.linalg.lstsq(A, np.concatenate([xa, ya]), rcond=None)[0]
    return np.concatenate([h, [1.0]]).astype(np.float32)


def make_record(i, j, xa, ya, xb, yb, accepted=1, Hm=None):
    r = np.zeros(1, im.PAIR_RESULT)
    n = len(xa)
    r["i"], r["j"], r["n_in"], r["n_selected"], r["ok"], r["accepted"] = i, j, n, n, accepted, accepted
    m = min(n, 400)
    r["a"]["x"][0, :m], r["a"]["y"][0, :m] = np.asarray(xa, np.float32)[:m], np.asarray(ya, np.float32)[:m]
    r["b"]["x"][0, :m], r["b"]["y"][0, :m] = np.asarray(xb, np.float32)[:m], np.asarray(yb, np.float32)[:m]
    if Hm is None:
        Hm = fit_homography(r["b"]["x"][0, :m].astype(np.float64), r["b"]["y"][0, :m].astype(np.float64),
                            r["a"]["x"][0, :m].astype(np.float64), r["a"]["y"][0, :m].astype(np.float64))
    r["H"][0] = Hm
    r["H"][0, 8] = 0.75          # Ransac2D's residual lives here: the start state must not read it as m8
    return r


def ties_from_truth(G, pairs, seed, cam, noise=0.0, per_pair=60, min_keep=16):
    """yields (i, j, xa, ya, xb, yb) of every pair that keeps at least min_keep ties"""
    rng = np.random.default_rng(seed)
    Ginv = [np.linalg.inv(g) for g in G]
    for (i, j) in pairs:
        x, y = rng.uniform(-MARGIN, W - 1 + MARGIN, per_pair), rng.uniform(-MARGIN, H - 1 + MARGIN, per_pair)
        xj, yj = _apply(Ginv[j], *_apply(G[i], x, y))
        xa, ya = distort_pixels(cam, x, y)
        xb, yb = distort_pixels(cam, xj, yj)
        keep = (xa >= 0) & (xa <= W - 1) & (ya >= 0) & (ya <= H - 1) & (xb >= 0) & (xb <= W - 1) & (yb >= 0) & (yb <= H - 1)
        if keep.sum() < min_keep:
            continue
        xa, ya, xb, yb = xa[keep], ya[keep], xb[keep], yb[keep]
        if noise > 0:
            xa, ya = xa + rng.normal(0, noise, len(xa)), ya + rng.normal(0, noise, len(xa))
            xb, yb = xb + rng.normal(0, noise, len(xa)), yb + rng.normal(0, noise, len(xa))
        yield i, j, xa, ya, xb, yb


def layout(name, seed):
    if name == "grid16":
        centres = [(W / 2 + c * 0.5 * W, H / 2 + r * 0.5 * H) for r in range(4) for c in range(4)]
        pairs = [(i, j) for i in range(16) for j in range(i + 1, 16)]          # all pairs: the ones without overlap drop out
    elif name == "strip12":
        centres = [(W / 2 + k * 0.45 * W, H / 2) for k in range(12)]
        pairs = [(k, k + 1) for k in range(11)]
    else:
        raise KeyError(name)
    return truth_transforms(centres, seed), pairs


def flat_survey(name, noise=0.0, seed=1, cam=CAM_TRUE, per_pair=60):
    """the layout's ties as the flat MATCHPAIR list: a run per pair, of any length"""
    G, pairs = layout(name, seed)
    out = []
    for i, j, xa, ya, xb, yb in ties_from_truth(G, pairs, seed + 100, cam, noise, per_pair):
        v = np.zeros(len(xa), im.MATCHPAIR)
        v["ai"], v["bi"], v["ax"], v["ay"], v["bx"], v["by"] = i, j, xa, ya, xb, yb
        out.append(v)
    return np.concatenate(out)


_CACHE = {}


def survey(name, noise=0.0, seed=1, cam=CAM_TRUE, per_pair=60):
    """-> PAIR_RESULT records of the layout (cached: treat as read-only)"""
    key = (name, noise, seed, cam, per_pair)
    if key not in _CACHE:
        G, pairs = layout(name, seed)
        recs = np.concatenate([make_record(*t) for t in ties_from_truth(G, pairs, seed + 100, cam, noise, per_pair)])
        recs.setflags(write=False)
        _CACHE[key] = recs
    return _CACHE[key]


MIN_TIES = 16
EDGE_N_IN = (MIN_TIES - 1, MIN_TIES, 31, 32, 33, 63, 64, 65, 399, 400)
EDGE_COUNTS = (1, 3, 4, 5)                     # record counts: both sides of the four-per-workgroup step, unequal tie counts inside one
THETA_TRUE = CAM_TRUE[4:]
THETA_BAD = (-1.6, 0.0, 0.0, 0.0, 0.0)         # rad reaches zero inside the frame: the fixed point does not settle there


def edge_records(seed=11):
    """-> (recs, h8 [n, 8]): the block entry points' record cases under the true camera's intrinsics, with states near the identity
    (normalised coordinates).  The records' own H are not read by the block entry points."""
    rng = np.random.default_rng(seed)
    recs = []

    def rec(n_in, i=None, j=None, accepted=1, Hm=None):
        i = int(rng.integers(0, 30)) if i is None else i
        j = i + 1 + int(rng.integers(0, 5)) if j is None else j
        xa, ya, xb, yb = rng.uniform(0, W - 1, n_in), rng.uniform(0, H - 1, n_in), rng.uniform(0, W - 1, n_in), rng.uniform(0, H - 1, n_in)
        return make_record(i, j, xa, ya, xb, yb, accepted, np.eye(3, dtype=np.float32).reshape(9) if Hm is None else Hm)

    recs.append(rec(400))                       # 0..4: one workgroup and a wave of the next, unequal counts
    recs.append(rec(MIN_TIES))
    recs.append(rec(65))
    recs.append(rec(33))
    recs.append(rec(399))
    for n_in in EDGE_N_IN:                      # 5..14
        recs.append(rec(n_in))
    recs.append(rec(100, accepted=0))           # 15: not accepted
    recs.append(rec(100, i=7, j=7))             # 16: i == j
    recs.append(rec(100, i=-1, j=3))            # 17: negative index
    recs.append(rec(100, i=3, j=-2))            # 18
    r = rec(64)                                 # 19: ties on the principal point, either side
    r["a"]["x"][0, 0], r["a"]["y"][0, 0] = CAM_TRUE[2], CAM_TRUE[3]
    r["b"]["x"][0, 1], r["b"]["y"][0, 1] = CAM_TRUE[2], CAM_TRUE[3]
    r["a"]["x"][0, 2], r["a"]["y"][0, 2], r["b"]["x"][0, 2], r["b"]["y"][0, 2] = CAM_TRUE[2], CAM_TRUE[3], CAM_TRUE[2], CAM_TRUE[3]
    recs.append(r)
    recs.append(rec(120))                       # 20: its state below is not finite -> unused
    recs.append(rec(401))                       # 21: more ties than a record holds -> unused
    recs.append(rec(48))                        # 22
    recs = np.concatenate(recs)
    h8 = np.zeros((len(recs), 8))
    for p in range(len(recs)):
        h8[p] = [1 + rng.uniform(-0.05, 0.05), rng.uniform(-0.1, 0.1), rng.uniform(-0.5, 0.5), rng.uniform(-0.1, 0.1), 1 + rng.uniform(-0.05, 0.05),
                 rng.uniform(-0.5, 0.5), rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)]
    h8[20, 3] = np.inf
    return recs, h8


def bad_scale_records():
    """three accepted records of 40 ties whose start state is not finite under CAM_START: a NaN in H, an infinite H[6], and (with cx = 256,
    cy = 240) an H whose K^-1 M K has a zero last entry"""
    rng = np.random.default_rng(5)
    out = []
    for k in range(3):
        Hm = np.eye(3, dtype=np.float32).reshape(9)
        if k == 0:
            Hm[1] = np.nan
        elif k == 1:
            Hm[6] = np.inf
        else:
            Hm[6] = -1.0 / 256.0
        out.append(make_record(k, k + 1, rng.uniform(0, W - 1, 40), rng.uniform(0, H - 1, 40), rng.uniform(0, W - 1, 40), rng.uniform(0, H - 1, 40), 1, Hm))
    return np.concatenate(out)


def map_error(cam_a, cam_b):
    """largest difference of the two cameras' distort maps (mi355_undistort_map, own intrinsics) over the frame, in pixels"""
    xa, ya = im.undistort_map(im.Camera(*cam_a), W, H)
    xb, yb = im.undistort_map(im.Camera(*cam_b), W, H)
    return float(np.sqrt((xa.astype(np.float64) - xb) ** 2 + (ya.astype(np.float64) - yb) ** 2).max())
