"""numpy restatement of the descriptor screen (include/mi355_mosaic.h, mi355_screen_pairs; csrc/screen.hip), bit for bit.

  top-K list   a frame's min(n, top_k) keypoints in the order (response descending, index ascending); -0.0 counts as +0.0
  D(q, t)      |q - t|^2 on the u8 descriptors (exact; float64 products of integers < 2^53)
  nn(q)        argmin of D over the other list, ties -> lower position; d1 the minimum; d2 the second smallest over the multiset
               (+inf when the other list has one row)
  score        #q with nn(nn(q)) == q, both q and nn(q) passing 10000 d1 < ratio_pct^2 d2 (int64; not tested at ratio_pct == 100)
  selection    position a ranks its in-scope candidates by (score desc, position asc) and nominates the first `partners` whose score
               >= min_score (partners == 0: all of those); a pair is kept when either side nominates it
"""
import numpy as np

INF = np.int64(1) << 40          # stands for +infinity: 100^2 * INF exceeds every 10000 d1 (d1 <= 128 * 255^2)


def topk_order(response, top_k):
    """positions of a frame's top-K keypoints in list order"""
    r = np.ascontiguousarray(response, np.float32).copy()
    u = r.view(np.uint32)
    u[u == 0x80000000] = 0
    mapped = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)
    idx = np.arange(len(r))
    order = np.lexsort((idx, ~mapped))          # ~mapped ascending = response descending; then index ascending
    return order[:top_k]


def top_list(kp, desc, top_k):
    """the frame's top-K descriptors (u8 rows, list order)"""
    o = topk_order(kp["response"], top_k)
    return np.asarray(desc, np.float64).astype(np.uint8)[o] if len(o) else np.zeros((0, 128), np.uint8)


def nn_stats(Q, T):
    """(nn, d1, d2) of every row of Q among the rows of T (int64; d2 = INF with one row)"""
    q = Q.astype(np.float64)
    t = T.astype(np.float64)
    D = (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2.0 * (q @ t.T)
    D = np.rint(D).astype(np.int64)
    nn = np.argmin(D, axis=1)
    d1 = D[np.arange(len(Q)), nn]
    d2 = np.partition(D, 1, axis=1)[:, 1] if T.shape[0] >= 2 else np.full(len(Q), INF, np.int64)
    return nn, d1, d2


def passes(d1, d2, ratio_pct):
    if ratio_pct >= 100:
        return np.ones(len(d1), bool)
    return np.int64(10000) * d1 < np.int64(ratio_pct) * np.int64(ratio_pct) * d2


def score_lists(A, B, ratio_pct=80):
    """score of two top-K lists (u8 rows)"""
    if len(A) == 0 or len(B) == 0:
        return 0
    na, d1a, d2a = nn_stats(A, B)
    nb, d1b, d2b = nn_stats(B, A)
    pa, pb = passes(d1a, d2a, ratio_pct), passes(d1b, d2b, ratio_pct)
    mutual = nb[na] == np.arange(len(A))
    return int(np.count_nonzero(mutual & pa & pb[na]))


def score_matrix(lists, ratio_pct=80, window=0):
    """n x n int32 scores of the top-K lists; -1 on the diagonal and outside the window"""
    n = len(lists)
    S = np.full((n, n), -1, np.int32)
    for a in range(n):
        for b in range(a + 1, n):
            if window and b - a >= window:
                break
            S[a, b] = S[b, a] = score_lists(lists[a], lists[b], ratio_pct)
    return S


def nominations(S, partners, min_score, window=0):
    """nom[a] = the set of positions a nominates"""
    n = S.shape[0]
    nom = []
    for a in range(n):
        cand = [b for b in range(n) if b != a and (not window or abs(b - a) < window) and S[a, b] >= min_score and S[a, b] >= 0]
        cand.sort(key=lambda b: (-int(S[a, b]), b))
        nom.append(set(cand if partners == 0 else cand[:partners]))
    return nom


def select_pairs(S, partners, min_score, window=0, rank=0, world=1):
    """the screened schedule as positions [(a, b)], a < b, sorted, a mod world == rank"""
    nom = nominations(S, partners, min_score, window)
    n = S.shape[0]
    out = []
    for a in range(rank, n, world):
        for b in range(a + 1, n):
            if window and b - a >= window:
                break
            if b in nom[a] or a in nom[b]:
                out.append((a, b))
    return np.array(out, np.int32).reshape(-1, 2)
