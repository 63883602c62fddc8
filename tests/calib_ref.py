"""The lens self-calibration of include/mi355_mosaic.h ("lens self-calibration") restated op by op in numpy (double, every product, sum and
quotient rounded on its own: numpy's elementwise operations do exactly that): the blocks bit for bit, the loop with one DENSE damped system over
all unknowns in place of the library's per-record elimination.  Test reference only."""
import numpy as np

MAX_SELECTED = 400
STEPS = 16                  # MI355_CALIB_STEPS
TOL = 1e-7                  # MI355_CALIB_TOL, normalised units
K1, K2, P1, P2, K3 = 1, 2, 4, 8, 16
CAM_FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")


def cam_tuple(cam):
    """a camera as nine python floats, from a dict, a sequence, or anything with the nine attributes (capi.Camera)"""
    if isinstance(cam, dict):
        return tuple(float(cam[f]) for f in CAM_FIELDS)
    if hasattr(cam, "fx"):
        return tuple(float(getattr(cam, f)) for f in CAM_FIELDS)
    return tuple(float(v) for v in cam)


def _terms(x, y, k1, k2, p1, p2, k3):
    xx, yy, xy = x * x, y * y, x * y
    r2, a1 = xx + yy, xy + xy
    t = r2 * k3
    t = k2 + t
    t = r2 * t
    t = k1 + t
    t = r2 * t
    rad = 1.0 + t
    tx = (p1 * a1) + (p2 * (r2 + (xx + xx)))
    ty = (p1 * (r2 + (yy + yy))) + (p2 * a1)
    return xx, yy, xy, r2, a1, rad, tx, ty


def undistort_points(cam, theta, xo, yo, steps=STEPS, tol=TOL):
    """U_theta of observed pixels -> (x, y normalised, G [.., 2, 5] = dU/dtheta, good)"""
    fx, fy, cx, cy = cam_tuple(cam)[:4]
    k1, k2, p1, p2, k3 = (np.float64(v) for v in theta)
    xo, yo = np.asarray(xo, np.float64), np.asarray(yo, np.float64)
    with np.errstate(all="ignore"):
        xd, yd = (xo - cx) / fx, (yo - cy) / fy
        x, y = xd.copy(), yd.copy()
        dx = dy = np.zeros_like(x)
        for _ in range(steps):
            _, _, _, _, _, rad, tx, ty = _terms(x, y, k1, k2, p1, p2, k3)
            inv = 1.0 / rad
            xn, yn = (xd - tx) * inv, (yd - ty) * inv
            dx, dy = xn - x, yn - y
            x, y = xn, yn
        xx, yy, xy, r2, a1, rad, tx, ty = _terms(x, y, k1, k2, p1, p2, k3)
        dr = r2 * k3
        dr = 3.0 * dr
        dr = (k2 + k2) + dr
        dr = r2 * dr
        dr = k1 + dr
        d2 = dr + dr
        x2, y2 = x + x, y + y
        a11 = (rad + d2 * xx) + ((p1 * y2) + (p2 * (6.0 * x)))
        a12 = (d2 * xy) + ((p1 * x2) + (p2 * y2))
        a22 = (rad + d2 * yy) + ((p1 * (6.0 * y)) + (p2 * x2))
        det = a11 * a22 - a12 * a12
        idet = 1.0 / det
        r4 = r2 * r2
        r6 = r4 * r2
        ex = [x * r2, x * r4, a1, r2 + (xx + xx), x * r6]
        ey = [y * r2, y * r4, r2 + (yy + yy), a1, y * r6]
        G = np.zeros(x.shape + (2, 5))
        for m in range(5):
            G[..., 0, m] = -((a22 * ex[m] - a12 * ey[m]) * idet)
            G[..., 1, m] = -((a11 * ey[m] - a12 * ex[m]) * idet)
        good = np.isfinite(x) & np.isfinite(y) & np.isfinite(idet) & (np.abs(dx) <= tol) & (np.abs(dy) <= tol)
    return x, y, G, good


def tie_rows(cam, theta, h, ax, ay, bx, by):
    """-> (X [n, 14], Y [n, 14], good [n]): the rows [d r / d (h, theta) | -r] of ties under state h (8 doubles)"""
    fx, fy = cam_tuple(cam)[:2]
    ua, va, Ga, ga = undistort_points(cam, theta, ax, ay)
    ub, vb, Gb, gb = undistort_points(cam, theta, bx, by)
    n = len(ua)
    X, Y = np.zeros((n, 14)), np.zeros((n, 14))
    with np.errstate(all="ignore"):
        w = (h[6] * ub + h[7] * vb) + 1.0
        u = (h[0] * ub + h[1] * vb) + h[2]
        v = (h[3] * ub + h[4] * vb) + h[5]
        q1 = 1.0 / w
        qx, qy, px, py = ub * q1, vb * q1, u * q1, v * q1
        X[:, 0], X[:, 1], X[:, 2], X[:, 6], X[:, 7] = -(fx * qx), -(fx * qy), -(fx * q1), fx * (px * qx), fx * (px * qy)
        Y[:, 3], Y[:, 4], Y[:, 5], Y[:, 6], Y[:, 7] = -(fy * qx), -(fy * qy), -(fy * q1), fy * (py * qx), fy * (py * qy)
        dxu, dxv = (h[0] - px * h[6]) * q1, (h[1] - px * h[7]) * q1
        dyu, dyv = (h[3] - py * h[6]) * q1, (h[4] - py * h[7]) * q1
        for m in range(5):
            cxm = dxu * Gb[:, 0, m] + dxv * Gb[:, 1, m]
            cym = dyu * Gb[:, 0, m] + dyv * Gb[:, 1, m]
            X[:, 8 + m] = fx * (Ga[:, 0, m] - cxm)
            Y[:, 8 + m] = fy * (Ga[:, 1, m] - cym)
        X[:, 13] = fx * (px - ua)
        Y[:, 13] = fy * (py - va)
        good = ga & gb & np.isfinite(px) & np.isfinite(py)
    return X, Y, good


def residuals(cam, theta, h, ax, ay, bx, by):
    """r = (fx (ua - px), fy (va - py)) per tie: [n, 2]"""
    X, Y, _ = tie_rows(cam, theta, h, ax, ay, bx, by)
    return np.stack([-X[:, 13], -Y[:, 13]], axis=1)


def used(rec, h, min_ties=16):
    n_in, i, j = int(rec["n_in"]), int(rec["i"]), int(rec["j"])
    return bool(rec["accepted"]) and min_ties <= n_in <= MAX_SELECTED and i != j and i >= 0 and j >= 0 and bool(np.isfinite(h).all())


def _ordered_sum(terms):
    z = np.zeros((1,) + terms.shape[1:])
    return np.cumsum(np.concatenate([z, terms], axis=0), axis=0)[-1]


def block(rec, h, cam, theta, min_ties=16):
    """-> dict(i, j, n_in, n_bad, cost, g [13], N [91]) of one PAIR_RESULT record under its state h"""
    out = dict(i=int(rec["i"]), j=int(rec["j"]), n_in=0, n_bad=0, cost=0.0, g=np.zeros(13), N=np.zeros(91))
    if not used(rec, h, min_ties):
        return out
    n = int(rec["n_in"])
    a, b = rec["a"][:n], rec["b"][:n]
    X, Y, good = tie_rows(cam, theta, h, a["x"], a["y"], b["x"], b["y"])
    X[~good] = 0.0
    Y[~good] = 0.0
    terms = np.empty((2 * n, 14, 14))
    terms[0::2] = X[:, :, None] * X[:, None, :]
    terms[1::2] = Y[:, :, None] * Y[:, None, :]
    S = _ordered_sum(terms)
    r, c = np.tril_indices(13)
    out.update(n_in=n, n_bad=int((~good).sum()), N=S[r, c].copy(), g=S[13, :13].copy(), cost=float(S[13, 13]))
    return out


def blocks(recs, h8, cam, theta, min_ties=16):
    return [block(r, h8[p], cam, theta, min_ties) for p, r in enumerate(recs)]


def start_state(H9, cam):
    """K^-1 M K scaled to h8 = 1 for one record's float H (M[8] = 1): 8 doubles, possibly not finite"""
    fx, fy, cx, cy = (np.float64(v) for v in cam_tuple(cam)[:4])
    m = np.asarray(H9, np.float32).astype(np.float64).copy()
    m[8] = 1.0
    T = np.zeros((3, 3))
    with np.errstate(all="ignore"):
        for r in range(3):
            T[r, 0] = m[3 * r] * fx
            T[r, 1] = m[3 * r + 1] * fy
            T[r, 2] = (m[3 * r] * cx + m[3 * r + 1] * cy) + m[3 * r + 2]
        G = np.zeros(9)
        for c in range(3):
            G[c] = (T[0, c] - cx * T[2, c]) / fx
            G[3 + c] = (T[1, c] - cy * T[2, c]) / fy
            G[6 + c] = T[2, c]
        return G[:8] / G[8]


DEFAULTS = dict(max_iters=20, mask=K1 | K2, min_ties=16, lambda0=1e-3, lambda_up=10.0, lambda_down=10.0, min_rel_decrease=1e-6)


def calibrate(recs, cam, **kw):
    """the loop on PAIR_RESULT records -> (camera tuple, report dict).  One dense damped system over theta's free entries and every used
    record's eight: N + lambda diag(N), solved by numpy."""
    P = dict(DEFAULTS, **kw)
    cam = cam_tuple(cam)
    theta = np.array(cam[4:], np.float64)
    free = [m for m in range(5) if P["mask"] >> m & 1]
    recs = recs[recs["accepted"] != 0]
    h8 = np.array([start_state(r["H"], cam) for r in recs]).reshape(len(recs), 8)
    B = blocks(recs, h8, cam, theta, P["min_ties"])
    use = [p for p, b in enumerate(B) if b["n_in"] > 0]
    rep = dict(trials=0, accepted=0, n_pairs_used=0, n_unused_records=0, n_points=0, cost0=0.0, cost=0.0)
    rep["lambda"] = 0.0
    if not use:
        return cam, rep
    bad = [(p, B[p]["n_bad"]) for p in use if B[p]["n_bad"]]
    assert not bad, bad
    npar = len(free)
    D = npar + 8 * len(use)
    tri = np.tril_indices(13)
    cols = [8 + m for m in free]

    def assemble(BB):
        N, g, c = np.zeros((D, D)), np.zeros(D), np.float64(0.0)
        for o, p in enumerate(use):
            full = np.zeros((13, 13))
            full[tri] = BB[p]["N"]
            full = full + np.tril(full, -1).T
            s = npar + 8 * o
            N[s:s + 8, s:s + 8] = full[:8, :8]
            N[s:s + 8, :npar] = full[:8][:, cols]
            N[:npar, s:s + 8] = full[:8][:, cols].T
            N[:npar, :npar] += full[cols][:, cols]
            g[s:s + 8] = BB[p]["g"][:8]
            g[:npar] += BB[p]["g"][cols]
            c = c + BB[p]["cost"]
        return N, g, float(c)

    N, g, c = assemble(B)
    assert np.isfinite(c)
    rep.update(n_pairs_used=len(use), n_unused_records=len(recs) - len(use), n_points=int(sum(B[p]["n_in"] for p in use)), cost0=c)
    lam = P["lambda0"]
    while rep["trials"] < P["max_iters"] and c != 0.0 and lam <= 1e16:
        rep["trials"] += 1
        M = N + lam * np.diag(np.diag(N))
        ok = True
        try:
            np.linalg.cholesky(M)
            d = np.linalg.solve(M, g)
        except np.linalg.LinAlgError:
            ok = False
        if ok:
            tt, ht = theta.copy(), h8.copy()
            tt[free] = theta[free] + d[:npar]
            for o, p in enumerate(use):
                ht[p] = h8[p] + d[npar + 8 * o:npar + 8 * o + 8]
            Bt = blocks(recs, ht, cam, tt, P["min_ties"])
            N2, g2, c2 = assemble(Bt)
            ok = bool(np.isfinite(c2) and c2 < c and not any(Bt[p]["n_bad"] for p in use))
        if ok:
            rep["accepted"] += 1
            theta, h8, N, g = tt, ht, N2, g2
            lam = lam / P["lambda_down"]
            rel = (c - c2) / c
            c = c2
            if rel < P["min_rel_decrease"]:
                break
        else:
            lam = lam * P["lambda_up"]
    rep["cost"] = c
    rep["lambda"] = lam
    return cam[:4] + tuple(float(v) for v in theta), rep


def distort_map(cam, w, h):
    """the double-precision distort map of a camera over the pixel grid (own intrinsics out): (xs, ys) [h, w]"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam_tuple(cam)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    x, y = (u - cx) / fx, (v - cy) / fy
    _, _, _, _, _, rad, tx, ty = _terms(x, y, k1, k2, p1, p2, k3)
    return fx * (x * rad + tx) + cx, fy * (y * rad + ty) + cy
