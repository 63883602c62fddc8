"""Pair records for the projective refinement's tests, built from planar ground truth: frames of 640 x 480 looking at one plane, frame 0 the
canvas (identity), every other frame a mild homography of it; tie points are exact images of one ground point in both frames, rounded to
float32, with optional Gaussian noise.  Also the record edge cases the block kernel is checked on."""
import numpy as np

import imagemosaicing_amd as im

W, H = 640, 480


def _apply(G, x, y):
    d = G[2, 0] * x + G[2, 1] * y + G[2, 2]
    return (G[0, 0] * x + G[0, 1] * y + G[0, 2]) / d, (G[1, 0] * x + G[1, 1] * y + G[1, 2]) / d


def truth_transforms(centres, seed, persp=2e-5):
    """frame -> canvas homographies (m8 = 1); frame 0 is the identity placed at its centre"""
    rng = np.random.default_rng(seed)
    G = []
    for k, (cx, cy) in enumerate(centres):
        if k == 0:
            G.append(np.array([[1.0, 0, cx - W / 2.0], [0, 1.0, cy - H / 2.0], [0, 0, 1.0]]))
            continue
        yaw = np.deg2rad(rng.uniform(-3, 3))
        s = 1 + rng.uniform(-0.02, 0.02)
        R = s * np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
        t = np.array([cx, cy]) - R @ np.array([W / 2.0, H / 2.0])
        A = np.array([[R[0, 0], R[0, 1], t[0]], [R[1, 0], R[1, 1], t[1]], [0, 0, 1.0]])
        Pm = np.array([[1.0, 0, 0], [0, 1.0, 0], [rng.uniform(-persp, persp), rng.uniform(-persp, persp), 1.0]])
        G.append(A @ Pm)
    # the canvas is frame 0's own pixel grid: the fixed frame's start (identity) is then its truth
    G0inv = np.linalg.inv(G[0])
    return [G0inv @ g for g in G]


def records_from_truth(G, pairs, seed, noise=0.0, per_pair=60, min_keep=8):
    rng = np.random.default_rng(seed)
    Ginv = [np.linalg.inv(g) for g in G]
    out = []
    for (i, j) in pairs:
        x, y = rng.uniform(0, W - 1, per_pair), rng.uniform(0, H - 1, per_pair)
        cx, cy = _apply(G[i], x, y)
        xj, yj = _apply(Ginv[j], cx, cy)
        keep = (xj >= 0) & (xj <= W - 1) & (yj >= 0) & (yj <= H - 1)
        if keep.sum() < min_keep:
            continue
        xa, ya, xb, yb = x[keep], y[keep], xj[keep], yj[keep]
        if noise > 0:
            xa, ya = xa + rng.normal(0, noise, len(xa)), ya + rng.normal(0, noise, len(xa))
            xb, yb = xb + rng.normal(0, noise, len(xa)), yb + rng.normal(0, noise, len(xa))
        r = np.zeros(1, im.PAIR_RESULT)
        n = len(xa)
        r["i"], r["j"], r["n_in"], r["n_selected"], r["ok"], r["accepted"] = i, j, n, n, 1, 1
        r["a"]["x"][0, :n], r["a"]["y"][0, :n] = xa.astype(np.float32), ya.astype(np.float32)
        r["b"]["x"][0, :n], r["b"]["y"][0, :n] = xb.astype(np.float32), yb.astype(np.float32)
        out.append(r)
    return np.concatenate(out)


def survey(name, noise=0.0, seed=1):
    """-> dict(recs, n, w, h, G (truth, frame -> canvas), start (the affine alignment of the records))"""
    if name == "grid16":
        centres = [(W / 2 + c * 0.5 * W, H / 2 + r * 0.5 * H) for r in range(4) for c in range(4)]
        n = 16
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]          # all pairs: the ones without overlap drop out below
    elif name == "strip12":
        centres = [(W / 2 + k * 0.45 * W, H / 2) for k in range(12)]
        n = 12
        pairs = [(k, k + 1) for k in range(n - 1)]
    else:
        raise KeyError(name)
    G = truth_transforms(centres, seed)
    recs = records_from_truth(G, pairs, seed + 100, noise)
    start = im.global_affine_align_results(recs, n)
    return dict(recs=recs, n=n, w=np.full(n, W, np.int32), h=np.full(n, H, np.int32), G=G, start=start)


def truth_h8(G):
    return np.array([(g / g[2, 2]).reshape(9)[:8] for g in G])


EDGE_IMAGES = 48
EDGE_COUNTS = (1, 3, 4, 5, 257)           # record counts: both sides of the four-per-workgroup step


def edge_records(seed=7):
    """257 records that walk the block entry points' cases, with parameters and flags for 48 images:
    -> (recs, h8 [48, 8], part [48]).  part: images 0 and 5 fixed (2), image 7 label 0 / image 9 m8 = 0 (both 0), the rest 1."""
    rng = np.random.default_rng(seed)
    n_img = EDGE_IMAGES
    h8 = np.zeros((n_img, 8))
    for k in range(n_img):
        h8[k] = [1 + rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(-3000, 3000),
                 rng.uniform(-0.05, 0.05), 1 + rng.uniform(-0.05, 0.05), rng.uniform(-3000, 3000), rng.uniform(-1e-4, 1e-4), rng.uniform(-1e-4, 1e-4)]
    h8[3, 6:] = [1e-4, -1e-4]
    part = np.ones(n_img, np.uint8)
    part[[0, 5]] = 2
    part[[7, 9]] = 0
    n_ins = [1, 31, 63, 64, 65, 399, 400]
    recs = np.zeros(257, im.PAIR_RESULT)
    for p in range(257):
        r = recs[p:p + 1]
        n_in = n_ins[p % 7]
        i, j = int(rng.integers(0, n_img)), int(rng.integers(0, n_img))
        if i == j:
            j = (i + 1) % n_img
        acc = 1
        if p == 1:   i, j = 0, 11                     # i fixed
        elif p == 2: i, j = 12, 5                     # j fixed
        elif p == 3: i, j = 0, 5                      # both fixed: not used
        elif p == 4: i, j = 7, 13                     # label 0
        elif p == 6: i, j = 14, 9                     # m8 = 0
        elif p == 8: i, j = 30, 2                     # i > j
        elif p == 9: n_in = 401                       # malformed: zero block, n_in kept
        elif p == 10: j = n_img                       # index outside: zero block, n_in kept
        elif p == 12: i, j = 20, 20                   # i == j: not used
        elif p == 13: n_in = 0
        elif 20 <= p < 60: i, j = 21, 22 + (p % 20)   # one image in 40 pairs
        elif p % 5 == 0: acc = 0                      # accepted and non-accepted interleaved
        m = min(n_in, 400)
        r["i"], r["j"], r["n_in"], r["accepted"], r["ok"] = i, j, n_in, acc, acc
        for f in ("a", "b"):
            r[f]["x"][0, :m] = rng.uniform(0, 4000, m).astype(np.float32)
            r[f]["y"][0, :m] = rng.uniform(0, 3000, m).astype(np.float32)
        if m >= 2:
            r["a"]["x"][0, 0], r["a"]["y"][0, 0] = 0.0, 0.0
            r["b"]["x"][0, 1], r["b"]["y"][0, 1] = 3999.5, 0.0
    return recs, h8, part
