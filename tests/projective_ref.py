"""The projective refinement of include/mi355_mosaic.h restated op by op in numpy (double, every product, sum and quotient rounded on its own:
numpy's elementwise operations do exactly that): the blocks bit for bit, the loop with a DENSE scaled Cholesky (or least squares) in place of the
library's envelope factorisation.  Test reference only."""
import numpy as np

MAX_SELECTED = 400


def side(h, x, y):
    """h: 8 doubles; x, y: arrays (or scalars) of doubles -> (Jx [.., 8], Jy [.., 8], U, V)"""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    w = (h[6] * x + h[7] * y) + 1.0
    u = (h[0] * x + h[1] * y) + h[2]
    v = (h[3] * x + h[4] * y) + h[5]
    with np.errstate(all="ignore"):
        qx, qy, q1 = x / w, y / w, 1.0 / w
        U, V = u / w, v / w
    z = np.zeros_like(qx)
    Jx = np.stack([qx, qy, q1, z, z, z, -(U * qx), -(U * qy)], axis=-1)
    Jy = np.stack([z, z, z, qx, qy, q1, -(V * qx), -(V * qy)], axis=-1)
    return Jx, Jy, U, V


def used(rec, part, n_images):
    """(is the record used, the n_in its block carries) as a block entry point sees it (part: 0 no part, 1 takes part, 2 fixed)"""
    n_in, i, j = int(rec["n_in"]), int(rec["i"]), int(rec["j"])
    if not rec["accepted"] or n_in < 1:
        return False, 0
    if n_in > MAX_SELECTED or not (0 <= i < n_images) or not (0 <= j < n_images):
        return False, n_in
    if i == j or not part[i] or not part[j] or (part[i] == 2 and part[j] == 2):
        return False, 0
    return True, n_in


def _ordered_sum(terms):
    """terms [m, ...] added one by one from +0.0 in index order"""
    z = np.zeros((1,) + terms.shape[1:])
    return np.cumsum(np.concatenate([z, terms], axis=0), axis=0)[-1]


def block(rec, h8, part):
    """-> dict(i, j, n_in, cost, g [16], N [136]) of one PAIR_RESULT record"""
    n_images = len(part)
    ok, keep = used(rec, part, n_images)
    out = dict(i=int(rec["i"]), j=int(rec["j"]), n_in=keep, cost=0.0, g=np.zeros(16), N=np.zeros(136))
    if not ok:
        return out
    n = keep
    a, b = rec["a"][:n], rec["b"][:n]
    Jxa, Jya, Ua, Va = side(h8[out["i"]], a["x"].astype(np.float64), a["y"].astype(np.float64))
    Jxb, Jyb, Ub, Vb = side(h8[out["j"]], b["x"].astype(np.float64), b["y"].astype(np.float64))
    X = np.concatenate([Jxa, -Jxb, (Ub - Ua)[:, None]], axis=1)          # [n, 17]: Rx | rx
    Y = np.concatenate([Jya, -Jyb, (Vb - Va)[:, None]], axis=1)
    with np.errstate(all="ignore"):
        terms = np.empty((2 * n, 17, 17))
        terms[0::2] = X[:, :, None] * X[:, None, :]
        terms[1::2] = Y[:, :, None] * Y[:, None, :]
        S = _ordered_sum(terms)
    r, c = np.tril_indices(16)
    out["N"] = S[r, c].copy()             # tril_indices walks rows, then columns: r(r+1)/2 + c
    out["g"] = S[16, :16].copy()
    out["cost"] = float(S[16, 16])
    return out


def blocks(recs, h8, part):
    return [block(r, h8, part) for r in recs]


def start_state(start, fixed, label):
    """-> (part [n] uint8, h8 [n, 8])"""
    n = len(start)
    part = np.zeros(n, np.uint8)
    h8 = np.zeros((n, 8))
    for k in range(n):
        m8 = start["m"][k][8]
        if not np.isfinite(m8) or m8 == 0 or (label is not None and label[k] == 0):
            continue
        fx = (fixed[k] != 0) if fixed is not None else (k == 0)
        part[k] = 2 if fx else 1
        h8[k] = start["m"][k][:8].astype(np.float64) / np.float64(m8)
    return part, h8


DEFAULTS = dict(max_iters=20, prior=0.01, lambda0=1e-3, lambda_up=10.0, lambda_down=10.0, min_rel_decrease=1e-6)


def refine(recs, w, h, start, fixed=None, label=None, solver="cholesky", **kw):
    """the loop; recs: PAIR_RESULT array.  -> (h8 final [n, 8] doubles, free image list, report dict)"""
    P = dict(DEFAULTS, **kw)
    n_images = len(start)
    part, h8 = start_state(start, fixed, label)
    recs = recs[recs["accepted"] != 0]
    B = blocks(recs, h8, part)
    use = [p for p, b in enumerate(B) if b["n_in"] > 0]
    for p in use:
        assert B[p]["n_in"] <= MAX_SELECTED and 0 <= B[p]["i"] < n_images and 0 <= B[p]["j"] < n_images
    nk = np.zeros(n_images, np.int64)
    for p in use:
        nk[B[p]["i"]] += B[p]["n_in"]
        nk[B[p]["j"]] += B[p]["n_in"]
    free = [k for k in range(n_images) if part[k] == 1 and nk[k] > 0]
    rep = dict(trials=0, accepted=0, n_free=0, n_pairs_used=0, n_points=0, cost0=0.0, cost_data=0.0, cost_prior=0.0)
    rep["lambda"] = 0.0
    if not free or not use:
        return h8, [], rep
    col = {k: o for o, k in enumerate(free)}
    D = 8 * len(free)
    ctl, tgt, omega = {}, {}, {}
    for k in free:
        omega[k] = (P["prior"] * np.float64(nk[k])) / 9.0
        pts = [((np.float64(p) * np.float64(w[k] - 1)) / 2.0, (np.float64(q) * np.float64(h[k] - 1)) / 2.0) for q in range(3) for p in range(3)]
        ctl[k] = np.array(pts)
        _, _, U, V = side(h8[k], ctl[k][:, 0], ctl[k][:, 1])
        tgt[k] = np.stack([U, V], axis=1)
    tri = np.tril_indices(16)

    def assemble(hh, BB):
        N = np.zeros((D, D))
        g = np.zeros(D)
        cd = np.float64(0.0)
        for p in use:
            b = BB[p]
            full = np.zeros((16, 16))
            full[tri] = b["N"]
            for (img, o0) in ((b["i"], 0), (b["j"], 8)):
                if img in col:
                    o = 8 * col[img]
                    N[o:o + 8, o:o + 8] += np.tril(full[o0:o0 + 8, o0:o0 + 8])
                    g[o:o + 8] += b["g"][o0:o0 + 8]
            if b["i"] in col and b["j"] in col:
                oi, oj = 8 * col[b["i"]], 8 * col[b["j"]]
                if oj > oi:
                    N[oj:oj + 8, oi:oi + 8] += full[8:, :8]
                else:
                    N[oi:oi + 8, oj:oj + 8] += full[8:, :8].T
            cd = cd + b["cost"]
        cp = np.float64(0.0)
        for k in free:
            Jx, Jy, U, V = side(hh[k], ctl[k][:, 0], ctl[k][:, 1])
            rx, ry = tgt[k][:, 0] - U, tgt[k][:, 1] - V
            X = np.concatenate([Jx, rx[:, None]], axis=1)
            Y = np.concatenate([Jy, ry[:, None]], axis=1)
            terms = np.empty((18, 9, 9))
            terms[0::2] = X[:, :, None] * X[:, None, :]
            terms[1::2] = Y[:, :, None] * Y[:, None, :]
            S = _ordered_sum(terms)
            o = 8 * col[k]
            N[o:o + 8, o:o + 8] += np.tril(omega[k] * S[:8, :8])
            g[o:o + 8] += omega[k] * S[8, :8]
            cp = cp + omega[k] * S[8, 8]
        return N, g, float(cd), float(cp)

    N, g, cd, cp = assemble(h8, B)
    c = cd + cp
    assert np.isfinite(c)
    rep.update(n_free=len(free), n_pairs_used=len(use), n_points=int(sum(B[p]["n_in"] for p in use)), cost0=c)
    lam = P["lambda0"]
    while rep["trials"] < P["max_iters"] and c != 0.0 and lam <= 1e16:
        rep["trials"] += 1
        d = np.diag(N)
        s = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 1.0)
        Nf = N + np.tril(N, -1).T
        M = (s[:, None] * Nf) * s[None, :] + lam * np.eye(D)
        rhs = s * g
        ok = True
        try:
            L = np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            ok = False
        if ok:
            if solver == "cholesky":
                y = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
            else:
                y = np.linalg.lstsq(M, rhs, rcond=None)[0]
            ht = h8.copy()
            for k in free:
                o = 8 * col[k]
                ht[k] = h8[k] + s[o:o + 8] * y[o:o + 8]
            Bt = blocks(recs, ht, part)
            N2, g2, cd2, cp2 = assemble(ht, Bt)
            c2 = cd2 + cp2
            ok = bool(np.isfinite(c2) and c2 < c)
        if ok:
            rep["accepted"] += 1
            h8, N, g, cd, cp = ht, N2, g2, cd2, cp2
            lam = lam / P["lambda_down"]
            rel = (c - c2) / c
            c = c2
            if rel < P["min_rel_decrease"]:
                break
        else:
            lam = lam * P["lambda_up"]
    rep.update(cost_data=cd, cost_prior=cp)
    rep["lambda"] = lam
    return h8, free, rep


def corners(h8, w, h):
    """canvas positions of the four corners of every frame under 8-parameter transforms: [n, 4, 2]"""
    out = np.zeros((len(h8), 4, 2))
    for k in range(len(h8)):
        xs = np.array([0.0, w[k] - 1.0, 0.0, w[k] - 1.0])
        ys = np.array([0.0, 0.0, h[k] - 1.0, h[k] - 1.0])
        with np.errstate(all="ignore"):
            _, _, U, V = side(h8[k], xs, ys)
        out[k, :, 0], out[k, :, 1] = U, V
    return out


def transforms_h8(tr):
    """IMAGE_TRANSFORM array -> [n, 8] doubles (m / m8; zeros where m8 is 0)"""
    m = tr["m"].astype(np.float64)
    with np.errstate(all="ignore"):
        return np.where(m[:, 8:9] != 0, m[:, :8] / m[:, 8:9], 0.0)
