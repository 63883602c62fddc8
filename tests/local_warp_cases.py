"""Inputs of the local registration's tests (tests/test_local_warp_ref.py, tests/test_gpu_local_warp.py): small synthetic surveys in
tests/synth_survey.py's layout whose ties are exact under the homography plus a smooth low-frequency displacement per frame, the measures
taken on them, and pair records built to meet every branch of the statistics."""
import numpy as np

import imagemosaicing_amd as im
from tests import local_warp_ref as lr
from tests.synth_survey import affine3, frame_layout

F = np.float32


# ---- smooth per-frame displacement fields -------------------------------------------------------------------------------------------------
def field(seed, w, h, amp):
    """a smooth field of about `amp` pixels over a w x h frame, at most three quarters of a wave across it: f(x, y) -> [m, 2]; amp 0: none"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (2, 3))
    ph = rng.uniform(0.0, 2.0 * np.pi, (2, 3, 2))
    fr = rng.uniform(0.5, 1.5, (2, 3, 2))

    def f(x, y):
        out = np.zeros((len(x), 2))
        for a in range(2):
            for t in range(3):
                out[:, a] += c[a, t] * np.sin(np.pi * fr[a, t, 0] * x / w + ph[a, t, 0]) * np.sin(np.pi * fr[a, t, 1] * y / h + ph[a, t, 1])
        return amp * out
    return f


def records(pairs):
    """PAIR_RESULT records from [(i, j, a [m, 2], b [m, 2])]; accepted, at most 400 ties each"""
    rec = np.zeros(len(pairs), im.PAIR_RESULT)
    for r, (i, j, a, b) in zip(rec, pairs):
        m = len(a)
        assert m <= 400
        r["i"], r["j"], r["n_in"], r["n_selected"], r["ok"], r["accepted"] = i, j, m, m, 1, 1
        r["a"]["x"][:m], r["a"]["y"][:m] = a[:, 0], a[:, 1]
        r["b"]["x"][:m], r["b"]["y"][:m] = b[:, 0], b[:, 1]
        r["H"][:] = np.eye(3, dtype=F).reshape(9)
    return rec


def survey(n=6, w=160, h=120, per_row=3, seed=1, amp=2.0, noise=0.0, ties=396, min_ties=24):
    """dict(rec, w, h, h9s, A, fields): frame k sees the ground point A_k p0 at pixel p0 + field_k(p0) (+ noise); h9s are the exact A_k,
    so what the ties disagree by on the canvas is the fields alone"""
    A, _ = frame_layout(n, w, h, seed=seed, per_row=per_row)
    M = [affine3(a) for a in A]
    Mi = [np.linalg.inv(m) for m in M]
    fields = [field(1000 * seed + k, w, h, amp) for k in range(n)]
    rng = np.random.default_rng(77 + seed)
    pairs = []
    for i in range(n):
        for j in range(i + 1, n):
            p = np.stack([rng.uniform(2, w - 3, 4 * ties), rng.uniform(2, h - 3, 4 * ties)], -1)
            g = p @ M[i][:2, :2].T + M[i][:2, 2]
            q = g @ Mi[j][:2, :2].T + Mi[j][:2, 2]
            a = p + fields[i](p[:, 0], p[:, 1]) + rng.normal(0, 1, p.shape) * noise
            b = q + fields[j](q[:, 0], q[:, 1]) + rng.normal(0, 1, p.shape) * noise
            ok = (q[:, 0] >= 2) & (q[:, 0] <= w - 3) & (q[:, 1] >= 2) & (q[:, 1] <= h - 3)
            for pts in (a, b):
                ok &= (pts[:, 0] >= 0) & (pts[:, 0] <= w - 1) & (pts[:, 1] >= 0) & (pts[:, 1] <= h - 1)
            if ok.sum() >= min_ties:
                pairs.append((i, j, a[ok][:ties].astype(F), b[ok][:ties].astype(F)))
    h9s = np.stack([m.reshape(9) for m in M]).astype(F)
    return dict(rec=records(pairs), w=[w] * n, h=[h] * n, h9s=h9s, A=A, fields=fields, n=n)


# ---- measures ------------------------------------------------------------------------------------------------------------------------------
def move(grid, w, h, p, iters=8):
    """where the source pixels p [m, 2] land in the frame corrected by `grid`: the q with q + D(q) = p"""
    p = np.asarray(p, np.float64)
    q = p.copy()
    for _ in range(iters):
        q = p - lr.grid_at(grid, w, h, np.clip(q[:, 0], 0, w - 1), np.clip(q[:, 1], 0, h - 1))
    return q


def disagreement(s, grids=None):
    """rms canvas distance of the two sides of every tie, with the ties moved into the corrected frames where grids are given"""
    tot, cnt = 0.0, 0
    for r in s["rec"]:
        m, i, j = int(r["n_in"]), int(r["i"]), int(r["j"])
        a = np.stack([r["a"]["x"][:m], r["a"]["y"][:m]], -1).astype(np.float64)
        b = np.stack([r["b"]["x"][:m], r["b"]["y"][:m]], -1).astype(np.float64)
        if grids is not None:
            a, b = move(grids[i], s["w"][i], s["h"][i], a), move(grids[j], s["w"][j], s["h"][j], b)
        ci = lr.pmap(s["h9s"][i].astype(np.float64), a[:, 0], a[:, 1])
        cj = lr.pmap(s["h9s"][j].astype(np.float64), b[:, 0], b[:, 1])
        tot += float(((ci[0] - cj[0]) ** 2 + (ci[1] - cj[1]) ** 2).sum())
        cnt += m
    return np.sqrt(tot / cnt)


def register(s, **params):
    """reference statistics and solve at the defaults with `params` replaced: (stats, grids, reports)"""
    p = dict(lr.DEFAULTS, **params)
    st = lr.stats(s["rec"], s["w"], s["h"], s["h9s"], **p)
    grids, _, reports = lr.solve(st, s["n"], **p)
    return st, grids, reports


# ---- the photometric case ------------------------------------------------------------------------------------------------------------------
def scene(X, Y):
    return 127.5 + 60.0 * np.sin(0.21 * X + 0.5) * np.sin(0.17 * Y + 1.0) + 50.0 * np.sin(0.09 * X - 0.13 * Y)


def render(s, k):
    """frame k of the survey as a BGR image: pixel p shows the ground point of the p0 with p0 + field(p0) = p"""
    w, h = s["w"][k], s["h"][k]
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    p = np.stack([u.ravel(), v.ravel()], -1)
    p0 = p.copy()
    for _ in range(12):
        p0 = p - s["fields"][k](p0[:, 0], p0[:, 1])
    M = affine3(s["A"][k])
    g = p0 @ M[:2, :2].T + M[:2, 2]
    a = np.clip(np.floor(scene(g[:, 0], g[:, 1]) + 0.5), 0, 255).astype(np.uint8).reshape(h, w)
    return np.repeat(a[..., None], 3, -1)


def gray_at(img, x, y):
    """bilinear gray (double) of a BGR image whose channels are equal, at positions inside [0, w-1] x [0, h-1]"""
    g = img[..., 0].astype(np.float64)
    h, w = g.shape
    xi, yi = np.minimum(x.astype(np.int64), w - 2), np.minimum(y.astype(np.int64), h - 2)
    q, p = x - xi, y - yi
    return (1 - p) * ((1 - q) * g[yi, xi] + q * g[yi, xi + 1]) + p * ((1 - q) * g[yi + 1, xi] + q * g[yi + 1, xi + 1])


def photometric_difference(s, imgs, i, j, step=2, margin=4):
    """mean absolute gray difference of frames i and j at the canvas lattice points (step apart) both cover, `margin` pixels inside"""
    Mi, Mj = np.linalg.inv(affine3(s["A"][i])), np.linalg.inv(affine3(s["A"][j]))
    corners = np.array([[0, 0], [s["w"][i], 0], [0, s["h"][i]], [s["w"][i], s["h"][i]]], np.float64) @ affine3(s["A"][i])[:2, :2].T + affine3(s["A"][i])[:2, 2]
    X, Y = np.meshgrid(np.arange(np.floor(corners[:, 0].min()), corners[:, 0].max(), step), np.arange(np.floor(corners[:, 1].min()), corners[:, 1].max(), step))
    c = np.stack([X.ravel(), Y.ravel()], -1)
    pi, pj = c @ Mi[:2, :2].T + Mi[:2, 2], c @ Mj[:2, :2].T + Mj[:2, 2]
    ok = np.ones(len(c), bool)
    for p, k in ((pi, i), (pj, j)):
        ok &= (p[:, 0] >= margin) & (p[:, 0] <= s["w"][k] - 1 - margin) & (p[:, 1] >= margin) & (p[:, 1] <= s["h"][k] - 1 - margin)
    assert ok.sum() > 500
    return float(np.abs(gray_at(imgs[0], pi[ok, 0], pi[ok, 1]) - gray_at(imgs[1], pj[ok, 0], pj[ok, 1])).mean())


# ---- records for every branch of the statistics ----------------------------------------------------------------------------------------
EDGE_W, EDGE_H = 97, 73            # (w-1) / 8 = 12 and (h-1) / 6 = 12: the nodes of the 8 x 6 grid lie on whole pixels
EDGE_PARAMS = dict(grid_x=8, grid_y=6, max_residual=8.0, max_shift=3.0)


def up32(v):
    return np.nextafter(F(v), F(np.inf))


def down32(v):
    return np.nextafter(F(v), F(-np.inf))


THRESHOLD_STEPS = ("at", "above", "below")


def threshold_ties():
    """(0, 5, a, b): twelve ties between the two identity frames, so that r = b - a and |d| = |r| / 2 on either side: per axis (x with
    a.x = 0 and b.x = r, y downwards with a.y = 8 and b.y = 8 - r) r exactly at, one float32 step above and one below max_residual = 8, then
    the same around 2 max_shift = 6.  The small coordinate carries the step, so every float32 holds its value exactly (asserted), and the
    restatement must put each tie on its side of its threshold (asserted)."""
    rs = [F(8.0), up32(8.0), down32(8.0), F(6.0), up32(6.0), down32(6.0)]
    a64 = np.array([[0.0, 30.0]] * 6 + [[30.0, 8.0]] * 6)
    b64 = np.array([[float(r), 30.0] for r in rs] + [[30.0, 8.0 - float(r)] for r in rs])
    a, b = a64.astype(F), b64.astype(F)
    assert np.array_equal(a.astype(np.float64), a64) and np.array_equal(b.astype(np.float64), b64)
    geo = (np.eye(3).reshape(9), np.eye(3).reshape(9), EDGE_W, EDGE_H)
    bad, far, sides = lr.tie_sides(geo, geo, a64, b64, EDGE_PARAMS["max_residual"], EDGE_PARAMS["max_shift"])
    r = np.abs(b64 - a64).sum(1)
    assert not bad.any() and len(set(r[:6])) == 6 and np.array_equal(r[:6], r[6:])
    assert far.tolist() == [False, True, False, False, False, False] * 2                  # r * r > 64 one step above 8 only
    for kept, qx, qy, dx, dy, lost in sides:
        d = np.maximum(np.abs(dx), np.abs(dy))
        assert (d[[0, 2, 4, 6, 8, 10]] > 3.0).all() and (d[[3, 9]] == 3.0).all() and (d[[5, 11]] < 3.0).all() and (d[[5, 11]] > 2.999999).all()
        assert kept.tolist() == [False, False, False, True, False, True] * 2             # |d| <= 3 at and one step below 6 only
        assert lost.tolist() == [True, False, True, False, True, False] * 2
    return 0, 5, a, b


def edge_case():
    """dict(rec, w, h, h9s, params): six frames -- 0 and 5 the identity, 1 and 2 whole-pixel translations (every double of a tie is exact),
    3 projective with a denominator that changes sign at x = 50, 4 not taking part (h9[8] = 0) -- and records that are not accepted, have
    bad indices, i == j or a frame not taking part, n_in of 1 and of 400, ties one float32 step on either side of both thresholds, q
    exactly on w - 1, h - 1 and on nodes, and one frame in 65 records"""
    w, h = EDGE_W, EDGE_H
    n = 6
    h9s = np.tile(np.eye(3, dtype=F).reshape(9), (n, 1))
    h9s[1, 2], h9s[1, 5] = 40.0, 10.0
    h9s[2, 2], h9s[2, 5] = -30.0, 20.0
    h9s[3, 6] = -1.0 / 50.0
    h9s[4, 8] = 0.0
    rng = np.random.default_rng(5)

    def rand_pair(i, j, m, spread=1.5):
        """m ties between translated frames i and j with residuals of about `spread` pixels"""
        ti, tj = h9s[i, [2, 5]].astype(np.float64), h9s[j, [2, 5]].astype(np.float64)
        lo = np.maximum(ti, tj) + 4.0
        hi = np.minimum(ti + [w - 1, h - 1], tj + [w - 1, h - 1]) - 4.0
        c = rng.uniform(lo, hi, (m, 2))
        return i, j, (c - ti + rng.normal(0, spread, (m, 2))).astype(F), (c - tj + rng.normal(0, spread, (m, 2))).astype(F)

    pairs = [rand_pair(0, 1, 400), rand_pair(0, 2, 1), rand_pair(1, 2, 200, 4.0)]
    pairs.append(threshold_ties())
    # q exactly on w - 1 / h - 1, on the origin and on nodes: residual 0 between frame 0 and frame 2 (-30, +20)
    nodes = np.array([[w - 1, h - 1], [w - 1, 36], [48, h - 1], [30, 20], [36, 24], [48, 36], [96, 24], [36, 72], [42.5, 30.25]], np.float64)
    pa = nodes.astype(F)
    pb = (nodes - h9s[2, [2, 5]]).astype(F)                                     # frame 2's side may leave its frame: REJ_SIDE there
    pairs.append((0, 2, pa, pb))
    # the projective frame: ties at columns on both sides of its pole
    xs = np.array([10, 30, 45, 49, 50, 51, 55, 80], np.float64)
    pb = np.stack([xs, np.full(len(xs), 20.0)], -1)
    den = 1.0 + float(h9s[3, 6]) * xs
    with np.errstate(divide="ignore", invalid="ignore"):
        pa = np.stack([np.clip(xs / den, 0, w - 1), np.clip(20.0 / den, 0, h - 1)], -1)
    pairs.append((0, 3, np.nan_to_num(pa, posinf=0, neginf=0).astype(F), pb.astype(F)))
    pairs.append((3, 1, pb.astype(F), (pa - [40, 10]).astype(F)))
    # frame 1 in 65 records
    for r in range(65):
        pairs.append(rand_pair(r % 2 * 2, 1, 7))
    rec = records(pairs)
    extra = np.zeros(7, im.PAIR_RESULT)
    extra[:] = rec[0]
    extra[0]["accepted"] = 0
    extra[1]["i"] = -1
    extra[2]["j"] = n
    extra[3]["j"] = extra[3]["i"]
    extra[4]["j"] = 4                      # takes no part
    extra[5]["n_in"] = 0
    extra[6]["n_in"] = 401
    return dict(rec=np.concatenate([rec[:3], extra, rec[3:]]), w=[w] * n, h=[h] * n, h9s=h9s, n=n, params=dict(EDGE_PARAMS), n_skipped=7)
