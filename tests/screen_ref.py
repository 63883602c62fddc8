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


# ---- the batched form: many pairs of short lists at once --------------------------------------------------------------------------------------
PAIR_CHUNK = 1 << 22          # the device scores the flat pair list in launches of this many pairs; score_matrix_batched walks it the same way


def pair_list(n, window=0):
    """the in-scope pairs (a, b), a < b, in (a, b) order: the flat list the device scores (int64 arrays)"""
    win = window if window else n
    cnt = np.clip(np.minimum(n - 1 - np.arange(n, dtype=np.int64), win - 1), 0, None)
    a = np.repeat(np.arange(n, dtype=np.int64), cnt)
    off = np.concatenate([[0], np.cumsum(cnt)])
    b = a + 1 + (np.arange(len(a), dtype=np.int64) - off[a])
    return a, b


def chunk_bases(total, chunk=PAIR_CHUNK):
    """the flat index each launch starts at"""
    return list(range(0, total, chunk))


def list_codes(lists):
    """(code [n, R], DC): every distinct row gets a code, DC the exact int64 distances of the codes; the last code is the padding of a short
    list, at distance INF from everything (so a padded row is never a neighbour and a one-row list has d2 = INF)"""
    n = len(lists)
    lens = np.array([len(l) for l in lists], np.int64)
    R = max(1, int(lens.max()) if n else 1)
    rows = np.concatenate([np.asarray(l, np.uint8).reshape(-1, 128) for l in lists] + [np.zeros((0, 128), np.uint8)])
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    U = len(uniq)
    u = uniq.astype(np.int64)
    DC = np.full((U + 1, U + 1), INF, np.int64)
    DC[:U, :U] = (u * u).sum(1)[:, None] + (u * u).sum(1)[None, :] - 2 * (u @ u.T)
    code = np.full((n, R), U, np.int64)
    code[np.arange(R)[None, :] < lens[:, None]] = np.asarray(inv).reshape(-1)
    return code, DC


def _nn_batched(D, ratio_pct):
    """per pair and query row: (nn, valid and passing) over D [P, Rq, Rt]"""
    nn = np.argmin(D, axis=2)                               # the first minimum: the lower position
    d1 = np.take_along_axis(D, nn[:, :, None], 2)[:, :, 0]
    d2 = np.sort(D, axis=2)[:, :, 1] if D.shape[2] >= 2 else np.full(d1.shape, INF, np.int64)
    return nn, (d1 < INF) & passes_nd(d1, d2, ratio_pct)


def passes_nd(d1, d2, ratio_pct):
    if ratio_pct >= 100:
        return np.ones(d1.shape, bool)
    return np.int64(10000) * d1 < np.int64(ratio_pct) * np.int64(ratio_pct) * d2


def score_pairs_batched(codes, a, b, ratio_pct=80):
    """scores of the pairs (a[k], b[k]) from list_codes(lists); equal to score_lists(lists[a[k]], lists[b[k]], ratio_pct)"""
    code, DC = codes
    R = code.shape[1]
    out = np.zeros(len(a), np.int32)
    step = max(1, (1 << 21) // (R * R))
    for s in range(0, len(a), step):
        ca, cb = code[a[s:s + step]], code[b[s:s + step]]
        D = DC[ca[:, :, None], cb[:, None, :]]
        na, oka = _nn_batched(D, ratio_pct)
        nb, okb = _nn_batched(D.transpose(0, 2, 1), ratio_pct)
        back = np.take_along_axis(nb, na, 1) == np.arange(R)[None, :]
        out[s:s + step] = np.count_nonzero(oka & back & np.take_along_axis(okb, na, 1), axis=1)
    return out


def score_matrix_batched(lists, ratio_pct=80, window=0, chunk=PAIR_CHUNK):
    """score_matrix for lists of a few rows, launch by launch as the device walks the flat pair list"""
    n = len(lists)
    S = np.full((n, n), -1, np.int32)
    a, b = pair_list(n, window)
    codes = list_codes(lists)
    for base in chunk_bases(len(a), chunk):
        g = slice(base, min(base + chunk, len(a)))
        s = score_pairs_batched(codes, a[g], b[g], ratio_pct)
        S[a[g], b[g]] = s
        S[b[g], a[g]] = s
    return S
