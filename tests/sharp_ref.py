"""numpy restatement of frame sharpness (include/mi355_mosaic.h, "frame sharpness"; csrc/sharp.hip, csrc/sharp_solve.cpp).

Per-frame samples and cover come from gain_ref.frame_sample_maps (the oracle's refined render of each frame alone).  From them, per frame, a
gray map and a has-Laplacian mask from the five-point cover; the statistics are integer sums over the lattice; the solve builds the normal
equations densely and hands them to np.linalg.solve; rel, the status and the drop order are restated directly, connectivity by a plain BFS.

The keyword switches (centre_only, border_rule, normalise, lower_median) are the mutations tests/test_sharp_patterns_ref.py applies: each is
a plausible wrong reading of the definition, and each must show in at least one case's records.
"""
import numpy as np

PAIR = np.dtype([("a", "<i4"), ("b", "<i4"), ("n", "<i8"), ("e_a", "<i8"), ("e_b", "<i8"), ("s_a", "<i8"), ("s_b", "<i8")])
FRAME = np.dtype([("n", "<i8"), ("e", "<i8"), ("s", "<i8")])
KEPT, DROPPED, CUT_VERTEX, NO_PAIR = 0, 1, 2, 3
PRIOR = float(np.float32(0.01))


def gray(samp):
    """the integer gray of B, G, R samples [..., 3] (tie_refine.hip's tie_gray)"""
    s = samp.astype(np.int64)
    return (1868 * s[..., 0] + 9617 * s[..., 1] + 4899 * s[..., 2] + 8192) >> 14


def lap_maps(maps, centre_only=False, border_rule=True):
    """per frame None or (g [ch, cw], L [ch, cw], has [ch, cw]): the gray of its samples, the Laplacian and where it has one.  The
    neighbours are taken with np.roll, which wraps; the border rule 1 <= x <= cw - 2, 1 <= y <= ch - 2 is what keeps the wrap out."""
    out = []
    for m in maps:
        if m is None:
            out.append(None)
            continue
        samp, cover = m
        g = gray(samp)
        nb = [(0, 1), (0, -1), (1, 1), (1, -1)]                             # (axis, shift): west, east, north, south
        L = 4 * g - sum(np.roll(g, s, axis=a) for a, s in nb)
        has = cover.copy()
        if not centre_only:
            for a, s in nb:
                has &= np.roll(cover, s, axis=a)
        if border_rule:
            inner = np.zeros_like(has)
            inner[1:-1, 1:-1] = True
            has &= inner
        out.append((g, L, has))
    return out


def lattice(ch, cw, step):
    m = np.zeros((ch, cw), bool)
    m[::step, ::step] = True
    return m


def stats_ref(lm, pairs, step):
    """(PAIR records [len(pairs)], FRAME records [n]) on the lattice of `step`"""
    shape = next(m for m in lm if m is not None)[0].shape
    Lt = lattice(shape[0], shape[1], step)
    fs = np.zeros(len(lm), FRAME)
    for k, m in enumerate(lm):
        if m is None:
            continue
        at = m[2] & Lt
        fs[k] = (int(at.sum()), int((m[1][at] ** 2).sum()), int(m[0][at].sum()))
    st = np.zeros(len(pairs), PAIR)
    for i, (a, b) in enumerate(pairs):
        st[i]["a"], st[i]["b"] = a, b
        if lm[a] is None or lm[b] is None:
            continue
        at = lm[a][2] & lm[b][2] & Lt
        st[i]["n"] = int(at.sum())
        st[i]["e_a"], st[i]["e_b"] = int((lm[a][1][at] ** 2).sum()), int((lm[b][1][at] ** 2).sum())
        st[i]["s_a"], st[i]["s_b"] = int(lm[a][0][at].sum()), int(lm[b][0][at].sum())
    return st, fs


def covered_both(maps, pairs, step):
    """per pair the lattice points both frames COVER (the gain statistics' n): what the five-point rule cuts down from"""
    shape = next(m for m in maps if m is not None)[1].shape
    Lt = lattice(shape[0], shape[1], step)
    return [0 if maps[a] is None or maps[b] is None else int((maps[a][1] & maps[b][1] & Lt).sum()) for a, b in pairs]


# ---- the host half -----------------------------------------------------------------------------------------------------------------------------
def usable(st):
    return (st["n"] > 0) & (st["e_a"] > 0) & (st["e_b"] > 0) & (st["s_a"] > 0) & (st["s_b"] > 0)


def pair_d(s, normalise=True):
    d = 0.5 * (np.log(float(s["e_a"])) - np.log(float(s["e_b"])))
    if normalise:
        d -= np.log(float(s["s_a"])) - np.log(float(s["s_b"]))
    return d


def solve_ref(st, n, prior=PRIOR, normalise=True):
    """l [n] float64 (0 for a frame in no usable pair) by np.linalg.solve of the dense normal equations"""
    A, rhs, W = np.zeros((n, n)), np.zeros(n), np.zeros(n)
    for s in st[usable(st)]:
        a, b, nn, d = int(s["a"]), int(s["b"]), float(s["n"]), pair_d(s, normalise)
        A[a, a] += nn; A[b, b] += nn; A[a, b] -= nn; A[b, a] -= nn
        rhs[a] += nn * d; rhs[b] -= nn * d
        W[a] += nn; W[b] += nn
    A[np.arange(n), np.arange(n)] += prior * W
    act = np.nonzero(W > 0)[0]
    l = np.zeros(n)
    if len(act):
        l[act] = np.linalg.solve(A[np.ix_(act, act)], rhs[act])
    return l


def partners(st, n):
    part = [[] for _ in range(n)]
    for s in st[usable(st)]:
        part[int(s["a"])].append(int(s["b"]))
        part[int(s["b"])].append(int(s["a"]))
    return part


def rel_ref(l, st, n, lower_median=True):
    """rel [n]: l minus the partners' lower median (mutation: the mean of the two middle values, np.median); 0 without partners"""
    rel = np.zeros(n)
    for k, p in enumerate(partners(st, n)):
        if p:
            lp = np.sort(l[p])
            rel[k] = l[k] - (lp[(len(lp) - 1) // 2] if lower_median else np.median(lp))
    return rel


def _connected_without(part, kept, k):
    """the kept frames of k's component stay connected without k (and at least one remains)"""
    comp, todo = {k}, [k]
    while todo:                                                             # k's component among the kept frames
        for q in part[todo.pop()]:
            if kept[q] and q not in comp:
                comp.add(q); todo.append(q)
    rest = comp - {k}
    if not rest:
        return False
    start = min(rest)
    seen, todo = {start}, [start]
    while todo:
        for q in part[todo.pop()]:
            if kept[q] and q != k and q not in seen:
                seen.add(q); todo.append(q)
    return seen == rest


def select_ref(rel, st, n, blur_ratio):
    """(status [n] uint8, the drop order tried [list of k])"""
    part = partners(st, n)
    limit = np.log(float(np.float32(blur_ratio)))
    status = np.array([KEPT if p else NO_PAIR for p in part], np.uint8)
    blurred = sorted((k for k in range(n) if part[k] and rel[k] < limit), key=lambda k: (rel[k], k))
    kept = [bool(p) for p in part]
    for k in blurred:
        if _connected_without(part, kept, k):
            status[k], kept[k] = DROPPED, False
        else:
            status[k] = CUT_VERTEX
    return status, blurred


def sharp_ref(l, st, n):
    """what mi355_solve_sharpness returns as sharp: float32(exp(l)), exactly 1 for a frame in no usable pair"""
    out = np.exp(l).astype(np.float32)
    out[[not p for p in partners(st, n)]] = 1.0
    return out


def min_margin(rel, st, n, blur_ratio):
    """the least distance of a decision from its threshold: |rel - ln(blur_ratio)| over the frames with partners, and the gaps between
    the blurred frames' rel.  A case whose margin is far above the solve's 1e-9 has one status, whoever computes l."""
    part = partners(st, n)
    limit = np.log(float(np.float32(blur_ratio)))
    r = np.array([rel[k] for k in range(n) if part[k]])
    if not len(r):
        return np.inf
    m = float(np.abs(r - limit).min())
    b = np.sort(r[r < limit])
    return min(m, float(np.diff(b).min())) if len(b) > 1 else m
