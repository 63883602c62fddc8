"""numpy restatement of guided matching (include/mi355_mosaic.h, section "guided matching"): float32 scalars in the written order, the tail through
tests/oracle_lib.py's ransac2d and the record packing of the pair stage (zero tails, the min_keep convention).  Also the numpy twins of
mi355_guided_candidates and mi355_merge_pair_results (float64 in the written order).

`mut` names ONE line of the selection to get wrong -- tests/test_guided_ref.py shows that each changes a crafted case of tests/guided_cases.py:
  radius_lt   dx*dx + dy*dy <  radius*radius          no_k_tie   the largest k among equal d
  no_q_tie    the largest q among equal d1 onto one k  ratio_le   (float)d1 <= ratio^2 (float)d2
  cut_d1      the survivors ordered by d1 alone (then k, not q)"""
import numpy as np

from tests import oracle_lib as ol

SFPOINT = ol.SFPOINT
PAIR_RESULT = np.dtype([("i", "<i4"), ("j", "<i4"), ("n_in", "<i4"), ("n_selected", "<i4"), ("ok", "<i4"), ("accepted", "<i4"), ("H", "<f4", (9,)), ("_pad", "<i4"),
                        ("a", SFPOINT, (400,)), ("b", SFPOINT, (400,))])
assert PAIR_RESULT.itemsize == 9664
DEFAULTS = dict(radius=4.0, max_dist2=90000, ratio=0.8)
F = np.float32


def apply_div9(G, x, y):
    """hm::apply_div9 on float32 arrays: sums left to right, two true divisions"""
    G = np.asarray(G, F).reshape(9)
    x, y = np.asarray(x, F), np.asarray(y, F)
    with np.errstate(all="ignore"):
        den = (G[6] * x + G[7] * y) + G[8]
        return ((G[0] * x + G[1] * y) + G[2]) / den, ((G[3] * x + G[4] * y) + G[5]) / den


def select(xy_i, d_i, xy_j, d_j, G, radius=4.0, max_dist2=90000, ratio=0.8, max_selected=400, mut=""):
    """-> (a SFPOINT [n_sel], b SFPOINT [n_sel], d1 int32 [n_sel])"""
    xy_i = np.ascontiguousarray(xy_i, F).reshape(-1, 2)
    xy_j = np.ascontiguousarray(xy_j, F).reshape(-1, 2)
    d_i = np.ascontiguousarray(d_i, np.uint8).reshape(-1, 128).astype(np.int64)
    d_j = np.ascontiguousarray(d_j, np.uint8).reshape(-1, 128).astype(np.int64)
    assert len(xy_i) == len(d_i) <= 2048 and len(xy_j) == len(d_j) <= 2048
    X, Y = apply_div9(G, xy_j[:, 0], xy_j[:, 1])
    r2 = F(radius) * F(radius)
    rr = F(ratio) * F(ratio)
    best = {}                                               # k -> (d1, q) of the proposal it keeps
    with np.errstate(all="ignore"):
        for q0 in range(0, len(xy_j), 256):                 # blocks of queries: 256 x n_i float32 at a time
            dx = xy_i[None, :, 0] - X[q0:q0 + 256, None]
            dy = xy_i[None, :, 1] - Y[q0:q0 + 256, None]
            e = dx * dx + dy * dy
            hit = (e < r2) if mut == "radius_lt" else (e <= r2)          # NaN fails either way
            for qq in np.nonzero(hit.any(1))[0]:
                q = q0 + int(qq)
                ks = np.nonzero(hit[qq])[0]
                d = ((d_i[ks] - d_j[q]) ** 2).sum(1)
                order = np.lexsort((-ks if mut == "no_k_tie" else ks, d))
                d1, k1 = int(d[order[0]]), int(ks[order[0]])
                if d1 > max_dist2:
                    continue
                if len(ks) > 1 and ratio > 0:
                    d2 = int(d[order[1]])
                    ok = (F(d1) <= rr * F(d2)) if mut == "ratio_le" else (F(d1) < rr * F(d2))
                    if not ok:
                        continue
                cand = (d1, -q) if mut == "no_q_tie" else (d1, q)
                if k1 not in best or cand < best[k1]:
                    best[k1] = cand
    ties = [(d1, abs(q), k) for k, (d1, q) in best.items()]
    ties.sort(key=(lambda t: (t[0], t[2])) if mut == "cut_d1" else (lambda t: (t[0], t[1])))
    ties = ties[:max_selected]
    a, b, dd = np.zeros(len(ties), SFPOINT), np.zeros(len(ties), SFPOINT), np.zeros(len(ties), np.int32)
    for t, (d1, q, k) in enumerate(ties):
        a[t] = (xy_i[k, 0], xy_i[k, 1], k)
        b[t] = (xy_j[q, 0], xy_j[q, 1], q)
        dd[t] = d1
    return a, b, dd


def lists_400(a, b, dd):
    """the selection as mi355_guided_select_dev leaves it: 400 entries each, zero from n_sel on"""
    A, B, D = np.zeros(400, SFPOINT), np.zeros(400, SFPOINT), np.zeros(400, np.int32)
    A[:len(a)], B[:len(b)], D[:len(dd)] = a, b, dd
    return A, B, D


def pack_record(i, j, n_sel, ok, i1, i2, H, min_inliers=30):
    """a mi355_pair_result by the pair stage's convention: a rejected record keeps its real n_in and inlier lists, H all zero, ok 0"""
    r = np.zeros(1, PAIR_RESULT)[0]
    n_in = len(i1)
    r["i"], r["j"], r["n_in"], r["n_selected"] = i, j, n_in, n_sel
    r["accepted"] = int(n_in > min_inliers)
    if r["accepted"]:
        r["ok"], r["H"] = int(ok), H
    a, b = np.zeros(400, SFPOINT), np.zeros(400, SFPOINT)
    a[:n_in], b[:n_in] = i1, i2
    r["a"], r["b"] = a, b
    return r


def record(oracle, i, j, xy_i, d_i, xy_j, d_j, G, dist=2.5, seed=1, sample_times=1000, min_inliers=30, max_selected=400, **params):
    """the whole stage for one pair: select -> oracle.ransac2d -> the packed record"""
    a, b, _ = select(xy_i, d_i, xy_j, d_j, G, max_selected=max_selected, **params)
    ok, i1, i2, H = oracle.ransac2d(a, b, dist, sample_times, seed)
    return pack_record(i, j, len(a), ok, i1, i2, H, min_inliers)


def record_bytes(r):
    """a record's bytes with the diagnostic word _pad (draws that took the generic solve path: not part of the definition) cleared"""
    r = np.array(r, PAIR_RESULT).reshape(1).copy()
    r["_pad"] = 0
    return r.tobytes()


# ---- mi355_guided_candidates ------------------------------------------------------------------------------------------------------------------
def _adj3(t):
    A = [t[4] * t[8] - t[5] * t[7], t[2] * t[7] - t[1] * t[8], t[1] * t[5] - t[2] * t[4],
         t[5] * t[6] - t[3] * t[8], t[0] * t[8] - t[2] * t[6], t[2] * t[3] - t[0] * t[5],
         t[3] * t[7] - t[4] * t[6], t[1] * t[6] - t[0] * t[7], t[0] * t[4] - t[1] * t[3]]
    return A, t[0] * A[0] + t[1] * A[3] + t[2] * A[6]


def _grid_hits(M, w1, h1):
    cnt = 0
    with np.errstate(all="ignore"):
        for y in (np.float64(0.0), h1 / np.float64(2.0), h1):
            for x in (np.float64(0.0), w1 / np.float64(2.0), w1):
                den = M[6] * x + M[7] * y + M[8]
                X, Y = (M[0] * x + M[1] * y + M[2]) / den, (M[3] * x + M[4] * y + M[5]) / den
                cnt += bool(X >= 0.0 and X <= w1 and Y >= 0.0 and Y <= h1)
    return cnt


def guide_of(Ti, Tj, w, h):
    """(G float32 [9], count) of one pair, or None where the pair is skipped"""
    t = [np.float64(v) for v in np.asarray(Ti, F)]
    u = [np.float64(v) for v in np.asarray(Tj, F)]
    w1, h1 = np.float64(w - 1), np.float64(h - 1)
    with np.errstate(all="ignore"):
        A, det = _adj3(t)
        if det == 0.0 or not np.isfinite(det):
            return None
        P = [(A[3 * r] * u[c] + A[3 * r + 1] * u[3 + c] + A[3 * r + 2] * u[6 + c]) / det for r in range(3) for c in range(3)]
        if P[8] == 0.0 or not np.isfinite(P[8]):
            return None
        G = np.array([P[k] / P[8] for k in range(9)], np.float64).astype(F)
        g = [np.float64(v) for v in G]
        A2, det2 = _adj3(g)
        gi = [v / det2 for v in A2]
        return G, _grid_hits(g, w1, h1) + _grid_hits(gi, w1, h1)


def guided_candidates(w, h, transforms, have=None, min_points=0):
    t = np.ascontiguousarray(transforms, F).reshape(-1, 9)
    hv = set() if have is None else {(min(int(a), int(b)), max(int(a), int(b))) for a, b in np.asarray(have).reshape(-1, 2)}
    if min_points <= 0:
        min_points = 2
    pairs, guides = [], []
    for i in range(len(t)):
        if t[i, 8] == 0:
            continue
        for j in range(i + 1, len(t)):
            if t[j, 8] == 0 or (i, j) in hv:
                continue
            g = guide_of(t[i], t[j], w, h)
            if g is None or g[1] < min_points:
                continue
            pairs.append((i, j))
            guides.append(g[0])
    return np.array(pairs, np.int32).reshape(-1, 2), np.array(guides, F).reshape(-1, 9)


def merge_pair_results(base, extra):
    out = [r.copy() for r in base]
    at = {}
    for k, r in enumerate(out):
        at.setdefault((int(r["i"]), int(r["j"])), k)
    for e in extra:
        key = (int(e["i"]), int(e["j"]))
        if key not in at:
            at[key] = len(out)
            out.append(e.copy())
        elif int(e["n_in"]) > int(out[at[key]]["n_in"]):
            out[at[key]] = e.copy()
    res = np.zeros(len(out), base.dtype if len(base) else extra.dtype)
    for k, r in enumerate(out):
        res[k] = r
    return res


def chain_guides(results, n_images):
    """guides from accepted consecutive pairs (k, k+1), chained in float64: C[(i, j)] maps image j to image i for every j > i the chain reaches.
    A record's H maps image j to image i with H[8] holding a residual: the matrix is H with [8] = 1."""
    step = {}
    for r in results:
        if int(r["accepted"]) and int(r["j"]) == int(r["i"]) + 1:
            M = np.array(r["H"], np.float64).reshape(3, 3)
            M[2, 2] = 1.0
            step[int(r["i"])] = M
    out = {}
    for i in range(n_images):
        M = np.eye(3)
        for j in range(i + 1, n_images):
            if j - 1 not in step:
                break
            M = M @ step[j - 1]
            out[(i, j)] = (M / M[2, 2]).reshape(9).astype(F)
    return out
