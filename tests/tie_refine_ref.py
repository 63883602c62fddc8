"""numpy restatement of the tie-point refinement defined in include/mi355_mosaic.h ("tie-point refinement by patch correlation"), written from
the header: float32 arrays where the header says float, float64 where it says double, int64 for the correlation sums, one numpy operation per
rounding.  refine_ties() gives the records, status, ncc2 and report the library must give byte for byte."""
import numpy as np

SFPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("id", "<i4")])
PAIR_RESULT = np.dtype([("i", "<i4"), ("j", "<i4"), ("n_in", "<i4"), ("n_selected", "<i4"), ("ok", "<i4"), ("accepted", "<i4"), ("H", "<f4", (9,)),
                        ("_pad", "<i4"), ("a", SFPOINT, (400,)), ("b", SFPOINT, (400,))])
TIE_REPORT = np.dtype([("i", "<i4"), ("j", "<i4"), ("n_in", "<i4"), ("n_out", "<i4"), ("flags", "<i4"), ("count", "<i4", (8,)), ("_pad", "<i4"),
                       ("ncc_q_sum", "<i8")])
NONE, REFINED, EDGE, FLAT, LOW, BORDER = range(6)
F_NOT_ACCEPTED, F_NO_FRAME, F_BAD, F_DEMOTED = 1, 2, 4, 8
DEFAULTS = dict(radius=7, search=3, drop_mask=0, min_ncc=0.7)
f32 = np.float32


def gray(img):
    """int64 [h, w]: (1868 B + 9617 G + 4899 R + 8192) >> 14 of a BGR uint8 image"""
    v = img.astype(np.int64)
    return (1868 * v[..., 0] + 9617 * v[..., 1] + 4899 * v[..., 2] + 8192) >> 14


def apply_div9(M, x, y):
    """hm::apply_div9 on float32 arrays (or scalars): two true divisions, sums left to right"""
    den = (M[6] * x + M[7] * y) + M[8]
    return ((M[0] * x + M[1] * y) + M[2]) / den, ((M[3] * x + M[4] * y) + M[5]) / den


def inside(x, y, w, h):
    return (x >= f32(0)) & (x < f32(w - 1)) & (y >= f32(0)) & (y < f32(h - 1))


def sample(g, x, y):
    """the gray sample (hm::bilin of the four texel grays) at float32 positions that are inside; int64"""
    xi, yi = x.astype(np.int32), y.astype(np.int32)
    q, p = x - xi.astype(f32), y - yi.astype(f32)
    s00, s01, s10, s11 = (g[yi + dy, xi + dx].astype(f32) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)))
    omp, omq = f32(1) - p, f32(1) - q
    t0, t1, t2, t3 = (s00 * omp) * omq, (s01 * omp) * q, (s10 * p) * omq, (s11 * p) * q
    v = ((t0 + t1) + t2) + t3
    return v.astype(np.int32).astype(np.uint8).astype(np.int64)


def tie_one(M, ax, ay, bx, by, gi, gj, R, S, min_ncc):
    """one tie: (status, peak as float64, a'.x, a'.y) -- steps 1 to 8 of the header"""
    hi, wi = gi.shape
    hj, wj = gj.shape
    fR = f32(R)
    with np.errstate(all="ignore"):
        if not (inside(bx - fR, by - fR, wj, hj) and inside(bx + fR, by + fR, wj, hj)):
            return EDGE, 0.0, ax, ay
        ut = np.arange(-R, R + 1).astype(f32)
        tx, ty = np.meshgrid(bx + ut, by + ut)
        assert inside(tx, ty, wj, hj).all()
        T = sample(gj, tx, ty)
        X0, Y0 = apply_div9(M, bx, by)
        uw = np.arange(-(R + S), R + S + 1).astype(f32)
        gx, gy = np.meshgrid(bx + uw, by + uw)
        X, Y = apply_div9(M, gx, gy)
        xs, ys = (X - X0) + ax, (Y - Y0) + ay
        if not inside(xs, ys, wi, hi).all():
            return EDGE, 0.0, ax, ay
        W = sample(gi, xs, ys)
        n = np.int64((2 * R + 1) ** 2)
        St, Stt = T.sum(), (T * T).sum()
        vt = n * Stt - St * St
        if vt == 0:
            return FLAT, 0.0, ax, ay
        win = np.lib.stride_tricks.sliding_window_view(W, T.shape)              # [dy + S, dx + S, v, u]
        Sw, Sww, Stw = win.sum((2, 3)), (win * win).sum((2, 3)), (win * T).sum((2, 3))
        vw, num = n * Sww - Sw * Sw, n * Stw - St * Sw
        numd = num.astype(np.float64)
        sq = (numd * numd) / (np.float64(vt) * vw.astype(np.float64))
        score = np.where((num > 0) & (vw > 0), sq, 0.0)
        idx = int(np.argmax(score))                                             # the first of equal maxima: the smallest index
        iy, ix = divmod(idx, 2 * S + 1)
        dx, dy = ix - S, iy - S
        peak = np.float64(score[iy, ix])
        if peak == 0.0 or peak < np.float64(f32(min_ncc)) * np.float64(f32(min_ncc)):
            return LOW, peak, ax, ay
        if abs(dx) == S or abs(dy) == S:
            return BORDER, peak, ax, ay

        def offset(sm, sp):
            den = (sm - peak) + (sp - peak)
            return (np.float64(0.5) * (sm - sp)) / den if den < 0 else np.float64(0.0)

        ex = f32(np.float64(dx) + offset(score[iy, ix - 1], score[iy, ix + 1]))
        ey = f32(np.float64(dy) + offset(score[iy - 1, ix], score[iy + 1, ix]))
        X1, Y1 = apply_div9(M, bx + ex, by + ey)
        return REFINED, peak, ax + (X1 - X0), ay + (Y1 - Y0)


def refine_ties(records, imgs, min_inliers=30, **params):
    """records: PAIR_RESULT array; imgs: list of [h, w, 3] uint8 arrays or None.  Returns (records, status [n, 400], ncc2 [n, 400], report)."""
    p = dict(DEFAULTS, **params)
    R, S, mask = int(p["radius"]), int(p["search"]), int(p["drop_mask"])
    rec = np.ascontiguousarray(records, PAIR_RESULT)
    n, n_images = len(rec), len(imgs)
    out = rec.copy()
    status, ncc2, report = np.zeros((n, 400), np.uint8), np.zeros((n, 400), f32), np.zeros(n, TIE_REPORT)
    grays = {}
    for r in range(n):
        e = rec[r]
        i, j, nin = int(e["i"]), int(e["j"]), int(e["n_in"])
        rep = report[r]
        rep["i"], rep["j"], rep["n_in"], rep["n_out"] = i, j, nin, nin
        if e["accepted"] == 0:
            rep["flags"] = F_NOT_ACCEPTED
        elif nin < 1 or nin > 400 or not (0 <= i < n_images) or not (0 <= j < n_images) or i == j:
            rep["flags"] = F_BAD
        elif imgs[i] is None or imgs[j] is None:
            rep["flags"] = F_NO_FRAME
        if rep["flags"]:
            continue
        for k in (i, j):
            if k not in grays:
                grays[k] = gray(imgs[k])
        M = e["H"].astype(f32).copy()
        M[8] = f32(1)
        keep, qsum = [], 0
        na = e["a"].copy()
        for k in range(nin):
            st, peak, x, y = tie_one(M, f32(e["a"]["x"][k]), f32(e["a"]["y"][k]), f32(e["b"]["x"][k]), f32(e["b"]["y"][k]), grays[i], grays[j], R, S,
                                     p["min_ncc"])
            status[r, k] = st
            ncc2[r, k] = f32(peak)
            rep["count"][st] += 1
            if st == REFINED:
                na["x"][k], na["y"][k] = x, y
                qsum += int(peak * np.float64(1048576.0))
            if not (mask >> st) & 1:
                keep.append(k)
        nout = len(keep)
        o = out[r]
        o["a"][:], o["b"][:] = np.zeros(400, SFPOINT), np.zeros(400, SFPOINT)
        o["a"][:nout], o["b"][:nout] = na[keep], e["b"][keep]
        o["n_in"] = nout
        rep["n_out"], rep["ncc_q_sum"] = nout, qsum
        if nout < nin and nout <= min_inliers:
            o["accepted"], o["ok"], o["H"] = 0, 0, np.zeros(9, f32)
            rep["flags"] = F_DEMOTED
    return out, status, ncc2, report
