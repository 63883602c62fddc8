"""Surveys for pair verification's tests: projective_cases' planar truth (frames of 640 x 480, 0.5 px of tie noise, 200 candidate ties per
pair, a pair kept iff more than 30 fall in both frames), every record with a homography fitted to its own ties, plus wrong pairs of two
kinds, alternating: FAR (two frames without a true pair, 60 ties that agree with a random similarity) and SHIFTED (a true pair whose b
list moved by one period).  Also the records and graphs the kernels' edge cases are checked on."""
import numpy as np

import imagemosaicing_amd as im
from tests import projective_cases as pc

W, H = pc.W, pc.H
PER_PAIR, MIN_KEEP, NOISE = 200, 31, 0.5


def fit_h(ax, ay, bx, by):
    """normalised DLT, float64: the homography b -> a (frame j -> frame i), scaled to m8 = 1"""
    def norm(x, y):
        mx, my = x.mean(), y.mean()
        s = np.sqrt(2.0) / max(np.sqrt(((x - mx) ** 2 + (y - my) ** 2).mean()), 1e-12)
        return np.array([[s, 0, -s * mx], [0, s, -s * my], [0, 0, 1.0]])
    Ta, Tb = norm(ax, ay), norm(bx, by)
    xa, ya = Ta[0, 0] * ax + Ta[0, 2], Ta[1, 1] * ay + Ta[1, 2]
    xb, yb = Tb[0, 0] * bx + Tb[0, 2], Tb[1, 1] * by + Tb[1, 2]
    z, o = np.zeros_like(xa), np.ones_like(xa)
    A = np.concatenate([np.stack([xb, yb, o, z, z, z, -xa * xb, -xa * yb, -xa], 1), np.stack([z, z, z, xb, yb, o, -ya * xb, -ya * yb, -ya], 1)])
    h = np.linalg.svd(A)[2][-1].reshape(3, 3)
    M = np.linalg.inv(Ta) @ h @ Tb
    return M / M[2, 2]


def set_h(r):
    """fits r's H to its ties (r: a one-record array); H[8] = the largest residual of the fit, as Ransac2D leaves it"""
    n = int(r["n_in"][0])
    ax, ay = r["a"]["x"][0, :n].astype(np.float64), r["a"]["y"][0, :n].astype(np.float64)
    bx, by = r["b"]["x"][0, :n].astype(np.float64), r["b"]["y"][0, :n].astype(np.float64)
    M = fit_h(ax, ay, bx, by)
    X, Y = pc._apply(M, bx, by)
    h = M.reshape(9).astype(np.float32)
    h[8] = np.float32(max(np.sqrt(((X - ax) ** 2 + (Y - ay) ** 2).max()), 1e-3))
    r["H"][0] = h


def layout(name):
    if name == "grid36":
        centres = [(W / 2 + c * 0.4 * W, H / 2 + r * 0.4 * H) for r in range(6) for c in range(6)]
        return centres, [(i, j) for i in range(36) for j in range(i + 1, 36)]
    if name == "strip40d":
        return [(W / 2 + k * 0.2 * W, H / 2) for k in range(40)], [(i, j) for i in range(40) for j in range(i + 1, 40)]
    if name == "strip_adjacent":
        return [(W / 2 + k * 0.45 * W, H / 2) for k in range(12)], [(k, k + 1) for k in range(11)]
    if name == "strip30s":          # the sparse strip of the limits: every frame meets its +-2 neighbours only
        return [(W / 2 + k * 0.4 * W, H / 2) for k in range(30)], [(i, j) for i in range(30) for j in range(i + 1, min(i + 3, 30))]
    raise KeyError(name)


def survey(name, seed=1, wrong_pct=0):
    """-> dict(recs, n, G (truth, frame -> canvas), wrong (bool per record), kind (0 right, 1 far, 2 shifted))"""
    centres, pairs = layout(name)
    n = len(centres)
    G = pc.truth_transforms(centres, seed)
    recs = pc.records_from_truth(G, pairs, seed + 100, NOISE, per_pair=PER_PAIR, min_keep=MIN_KEEP)
    kind = np.zeros(len(recs), np.int32)
    rng = np.random.default_rng(seed + 1000)
    n_wrong = int(round(len(recs) * wrong_pct / 100.0))
    true_pairs = {(int(r["i"]), int(r["j"])) for r in recs}
    free = [(i, j) for i in range(n) for j in range(i + 1, n) if (i, j) not in true_pairs]
    far = []
    shifted = rng.permutation(len(recs))
    n_shift = 0
    for t in range(n_wrong):
        if t % 2 == 0 and free:
            i, j = free.pop(int(rng.integers(0, len(free))))
            m = 60
            ax, ay = rng.uniform(0, W - 1, m), rng.uniform(0, H - 1, m)
            yaw = np.deg2rad(rng.uniform(-5, 5))
            c, s = np.cos(yaw), np.sin(yaw)
            tx, ty = rng.uniform(-200, 200), rng.uniform(-150, 150)
            bx = c * (ax - W / 2) - s * (ay - H / 2) + W / 2 + tx + rng.normal(0, NOISE, m)
            by = s * (ax - W / 2) + c * (ay - H / 2) + H / 2 + ty + rng.normal(0, NOISE, m)
            r = np.zeros(1, im.PAIR_RESULT)
            r["i"], r["j"], r["n_in"], r["n_selected"], r["ok"], r["accepted"] = i, j, m, m, 1, 1
            r["a"]["x"][0, :m], r["a"]["y"][0, :m] = ax.astype(np.float32), ay.astype(np.float32)
            r["b"]["x"][0, :m], r["b"]["y"][0, :m] = bx.astype(np.float32), by.astype(np.float32)
            far.append(r)
        else:
            q = int(shifted[n_shift])
            n_shift += 1
            m = int(recs["n_in"][q])
            dx = float(rng.choice([-1, 1]) * rng.uniform(12, 60))
            dy = float(rng.choice([-5.0, 5.0]))
            recs["b"]["x"][q, :m] = (recs["b"]["x"][q, :m].astype(np.float64) + dx).astype(np.float32)
            recs["b"]["y"][q, :m] = (recs["b"]["y"][q, :m].astype(np.float64) + dy).astype(np.float32)
            kind[q] = 2
    if far:
        recs = np.concatenate([recs] + far)
        kind = np.concatenate([kind, np.ones(len(far), np.int32)])
        order = rng.permutation(len(recs))          # the wrong pairs anywhere in the list
        recs, kind = recs[order], kind[order]
    for q in range(len(recs)):
        set_h(recs[q:q + 1])
    return dict(recs=recs, n=n, G=G, kind=kind, wrong=kind != 0, name=name, seed=seed, wrong_pct=wrong_pct)


def corner_error(tr, G):
    """the largest distance of a frame corner under tr (IMAGE_TRANSFORM) from its place under the truth G"""
    worst = 0.0
    for k, g in enumerate(G):
        M = tr["m"][k].astype(np.float64).reshape(3, 3)
        for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
            X, Y = pc._apply(M, x, y)
            tx, ty = pc._apply(g, x, y)
            worst = max(worst, float(np.hypot(X - tx, Y - ty)))
    return worst


# ---- records for the edge and residual kernels --------------------------------------------------------------------------------------------
EDGE_IMAGES = pc.EDGE_IMAGES
EDGE_COUNTS = pc.EDGE_COUNTS


def edge_records(seed=11):
    """257 records in the style of projective_cases.edge_records, each with an H: n_in in {1, 31, 63, 64, 65, 399, 400}, accepted and
    non-accepted interleaved, n_in = 0 and 401, an index outside the images, i == j, a singular H, an H with a NaN, an H whose inverse
    overflows, a tie on a frame's horizon.  Frame pairs repeat: these records feed the edge and residual entry points, not the adjacency.
    (A double inverse of float32 entries cannot overflow short of det == 0 -- every numerator is below 2^257 and a non-zero determinant
    above 2^-500 -- so "overflows" is walked as: the smallest determinant float32 entries give, an infinite entry, and det == 0.)"""
    rng = np.random.default_rng(seed)
    n_img = EDGE_IMAGES
    n_ins = [1, 31, 63, 64, 65, 399, 400]
    recs = np.zeros(257, im.PAIR_RESULT)
    for p in range(257):
        r = recs[p:p + 1]
        n_in = n_ins[p % 7]
        i, j = int(rng.integers(0, n_img)), int(rng.integers(0, n_img))
        if i == j:
            j = (i + 1) % n_img
        acc = 1
        H = np.array([1 + rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(-300, 300), rng.uniform(-0.05, 0.05),
                      1 + rng.uniform(-0.05, 0.05), rng.uniform(-300, 300), rng.uniform(-1e-5, 1e-5), rng.uniform(-1e-5, 1e-5), rng.uniform(0.1, 3)], np.float32)
        if p == 9: n_in = 401
        elif p == 10: j = n_img
        elif p == 11: i = -1
        elif p == 12: i, j = 20, 20
        elif p == 13: n_in = 0
        elif p == 14: H[:8] = [1, 2, 3, 2, 4, 6, 0, 0]                         # singular: B is not finite
        elif p == 15: H[4] = np.nan
        elif p == 16: H[:8] = [1e-45, 0, 3e38, 0, 1e-45, 3e38, 0, 0]           # det = 2e-90, inverse entries up to 2e128: finite (see below)
        elif p == 17: H[2] = np.inf                                           # the inverse "overflows": F itself is not finite
        elif p == 18: H[:8] = [0, 0, 3e38, 0, 0, 3e38, 3e38, 3e38]             # det = 0 with numerators of 9e76: inf and NaN in B
        elif p == 19: i, j = 7, 9                                             # the residual tests give frame 7 label 0, frame 9 m8 = 0
        elif p == 23: i, j = 3, 30                                            # frame 3 has a horizon inside the ties' range
        elif p % 5 == 0: acc = 0
        m = min(n_in, 400)
        r["i"], r["j"], r["n_in"], r["accepted"], r["ok"] = i, j, n_in, acc, acc
        r["H"][0] = H
        for f in ("a", "b"):
            r[f]["x"][0, :m] = rng.uniform(0, 4000, m).astype(np.float32)
            r[f]["y"][0, :m] = rng.uniform(0, 3000, m).astype(np.float32)
        if m >= 2:
            r["a"]["x"][0, 0], r["a"]["y"][0, 0] = 0.0, 0.0
            r["b"]["x"][0, 1], r["b"]["y"][0, 1] = 3999.5, -0.0
    return recs


def edge_transforms(seed=12):
    """48 random transforms for the residual tests (float32 [48, 9]) and labels: frame 7 has label 0, frame 9 m8 = 0, frame 3 a horizon that
    crosses the ties' range (den <= 0 for some ties)"""
    rng = np.random.default_rng(seed)
    h9 = np.zeros((EDGE_IMAGES, 9), np.float32)
    for k in range(EDGE_IMAGES):
        h9[k] = [1 + rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(-3000, 3000), rng.uniform(-0.05, 0.05), 1 + rng.uniform(-0.05, 0.05),
                 rng.uniform(-3000, 3000), rng.uniform(-1e-5, 1e-5), rng.uniform(-1e-5, 1e-5), 1.0]
    h9[3, 6:] = [-5e-4, 0, 1.0]                  # den = 1 - x / 2000: zero at x = 2000
    h9[9, 8] = 0.0
    label = np.ones(EDGE_IMAGES, np.int32)
    label[7] = 0
    return h9, label


# ---- crafted graphs for the cycle kernel ----------------------------------------------------------------------------------------------------
def _edge(i, j, F, box=(0.0, 0.0, 100.0, 80.0), n_in=50, testable=True):
    e = np.zeros(1, im.PAIR_EDGE)
    F = np.asarray(F, np.float64).reshape(9)
    e["i"], e["j"], e["n_in"], e["flags"] = i, j, n_in, 3 if testable else 1
    e["box"], e["F"] = np.asarray(box, np.float32), F
    with np.errstate(all="ignore"):
        e["B"] = np.linalg.inv(F.reshape(3, 3)).reshape(9) / np.linalg.inv(F.reshape(3, 3))[2, 2] if testable else np.nan
    return e


def _shift(tx, ty):
    return [1, 0, tx, 0, 1, ty, 0, 0, 1]


def translation_graph(n_common, err=(0.0, 0.0), seed=0, flip=True):
    """frames 0 and 1 joined by one edge and by n_common frames 2 .. adjacent to both; every map is an integer translation by the frames'
    positions, the edge (0, 1) itself is off by `err`: all its triangles have the cycle error |err| exactly.  With flip every other edge is
    stored in the opposite orientation (F and B exchanged).  -> (edges, n_images)"""
    rng = np.random.default_rng(seed)
    n = n_common + 2
    pos = rng.integers(-500, 500, (n, 2)).astype(np.float64)

    def edge(i, j, extra=(0.0, 0.0)):                 # F maps frame j to frame i: x_i = x_j + pos_j - pos_i
        d = pos[j] - pos[i]
        e = _edge(i, j, _shift(d[0] + extra[0], d[1] + extra[1]))
        e["B"][0] = _shift(-(d[0] + extra[0]), -(d[1] + extra[1]))
        return e
    out = [edge(0, 1, err)]
    for k in range(2, n):
        out.append(edge(k, 0) if (flip and k % 2) else edge(0, k))
        out.append(edge(1, k) if (flip and k % 3 == 0) else edge(k, 1))
    return np.concatenate(out), n


def star_graph(big=400, small=2):
    """frame 0 with `big` neighbours opposite frame 1 with `small`: the edge (0, 1) walks frame 1's list and searches frame 0's.  The common
    neighbours are the last `small - 1` frames."""
    n = big + 1
    out = [_edge(0, 1, _shift(3, 4))]
    for k in range(2, n):
        out.append(_edge(0, k, _shift(k, -k)))
    for k in range(n - (small - 1), n):
        out.append(_edge(k, 1, _shift(3 - k, 4 + k)))          # k <- 1, consistent with 0 <- k <- 1
    return np.concatenate(out), n


def special_graph():
    """a triangle 0-1-2 stored in mixed orientations plus: an edge whose control point lies on a neighbour's horizon, a zero-area box, an edge
    that is not testable, and an edge without any common neighbour.  -> (edges, n_images)"""
    out = [_edge(0, 1, _shift(10, 0)), _edge(2, 1, _shift(-5, 7)), _edge(0, 2, _shift(15, -7))]          # consistent: (0<-1) = (0<-2)(2<-1)
    # frame 3: its map from frame 1 has a horizon at x = 50 of the (0, 1) box -> den <= 0 at x1 = 100
    out.append(_edge(3, 1, [1, 0, 0, 0, 1, 0, -0.02, 0, 1]))
    out.append(_edge(0, 3, _shift(10, 0)))
    # frames 4, 5: the edge (4, 5) has a zero-area box (n_in = 1)
    out.append(_edge(4, 5, _shift(1, 1), box=(7.5, 9.25, 7.5, 9.25), n_in=1))
    out.append(_edge(4, 0, _shift(2, 2)))
    out.append(_edge(5, 0, _shift(1, 1)))
    # frame 6: an edge that is usable but not testable (no part of the adjacency), and one without a common neighbour
    out.append(_edge(6, 0, _shift(0, 0), testable=False))
    out.append(_edge(6, 7, _shift(1, 2)))
    return np.concatenate(out), 8
