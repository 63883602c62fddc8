"""Crafted inputs for the descriptor screen (csrc/screen.hip) at its list, tie and launch-chunk edges, with the predicates that show on the
restatement alone (tests/screen_ref.py, numpy only) that every case reaches the edge it is named for.  tests/test_screen_patterns_ref.py
evaluates the predicates on the CPU; tests/test_gpu_screen_edges.py installs the frames with SetFeatures and compares the device with the
restatement.  No frame is rendered and no SIFT runs.

A frame is {"kp": KEYPOINT records, "desc": u8 [n, 128]}; only the keypoints' responses matter to the screen.

  top-K cases      one frame of n keypoints per (response kind, n) and, per top_k, a PROBE: exact copies of the frame's true top-K list,
                   shuffled.  All descriptors are random u8 rows far from each other, so at ratio_pct 100 the score is the number of list
                   members the device found: a wrong member costs a mutual match (topk_predicate shows it for the K-th / (K+1)-th swap).
  nn cases         pairs of lists with gadgets written over random rows:
                     tie   a query c, train rows c + 3 e0, c + 3 e1 (, c + 3 e2) at chosen positions, all at distance 9, and a second query
                           equal to the LAST of them: the right tie-break (lowest position) scores 2 at ratio_pct 100, any other 1
                     dup   train rows that are equal, at distance 9 from their query: d1 == d2 over the multiset, so the query fails every
                           ratio below 100; over the set of values it would pass
                     ratio an all-zero query with train rows at distances (1, 4), (1, 5) and (0, 0): ratio_pct 50 at exact equality
  scope cases      frames of 0 .. 3 codebook rows under every window, n = 0, 1, 2, and the 2900-frame list of 4 203 550 pairs (one full
                   launch of 2^22 workgroups and a second of 9 246)
  selection cases  frames of 2 .. 3 one-hot tokens: scores are 0 .. 3 and whole rows tie; the frames below `first` share nothing with the
                   frames from `first` on, so a row's tied threshold group starts exactly there
Everything is deterministic: the same arguments give the same bytes."""
import functools

import numpy as np

from tests import screen_ref as sr

KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
W, H = 640, 480                       # the frame size SetFeatures is given; the screen does not read it
TOPK_NT = 512                         # threads of screen_topk_kernel
SEL_NT = 256                          # positions per trip of screen_select_kernel's tie scan
MAX_D = 128 * 255 * 255               # the largest distance of two u8 rows


def frame(resp, desc):
    resp = np.asarray(resp, np.float32).reshape(-1)
    kp = np.zeros(len(resp), KEYPOINT)
    kp["response"] = resp
    kp["x"], kp["y"], kp["size"] = (np.arange(len(resp)) % W).astype(np.float32), (np.arange(len(resp)) // W).astype(np.float32), 2.0
    return dict(kp=kp, desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 128))


def ordered(desc):
    """a frame whose list order is its row order (distinct descending responses)"""
    n = len(desc)
    return frame(np.arange(n, 0, -1, dtype=np.float32) / np.float32(max(n, 1)), desc)


def ref_list(f, top_k):
    return sr.top_list(f["kp"], f["desc"], top_k)


def dist(Q, T):
    q, t = np.asarray(Q, np.int64), np.asarray(T, np.int64)
    return (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2 * (q @ t.T)


# ---- top-K list cases -------------------------------------------------------------------------------------------------------------------------
TOPK_KS = (32, 96, 160, 256, 480, 512)
TOPK_KINDS = ("equal", "two_values", "last_bit", "mixed", "strong_last")
MIXED_VALUES = np.array([-1.5, -1e-3, -0.0, 0.0, 1e-40, -1e-40, 1.4e-45, np.inf, 0.02, 0.5], np.float32)


def topk_sizes(top_k):
    return sorted({1, 31, 32, 33, top_k - 1, top_k, top_k + 1, 513, 1025, 5000})


def _responses(kind, n, rng):
    if kind == "equal":
        return np.full(n, 0.0625, np.float32)
    if kind == "two_values":                                 # at most 20 strong ones: the K boundary lies inside the (larger) weak group
        r = np.full(n, 0.02, np.float32)
        r[rng.permutation(n)[:min(n // 3, 20)]] = 0.04
        return r
    if kind == "last_bit":                                   # four neighbouring float32 values
        u = np.full(n, np.float32(0.03).view(np.uint32), np.uint32) + rng.integers(0, 4, n).astype(np.uint32)
        return u.view(np.float32)
    if kind == "mixed":
        pick = np.concatenate([rng.permutation(len(MIXED_VALUES)), rng.integers(0, len(MIXED_VALUES), max(n, 10))])[:n]
        return MIXED_VALUES[pick]
    if kind == "strong_last":
        return np.arange(1, n + 1, dtype=np.float32) / np.float32(n)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def topk_frame(kind, n):
    rng = np.random.default_rng(1000 * TOPK_KINDS.index(kind) + n)
    return frame(_responses(kind, n, rng), rng.integers(0, 256, (n, 128), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def topk_probe(kind, n, top_k):
    """exact copies of the frame's true top-K list in another order"""
    f = topk_frame(kind, n)
    o = sr.topk_order(f["kp"]["response"], top_k)
    rng = np.random.default_rng(7 * n + top_k)
    return ordered(f["desc"][o][rng.permutation(len(o))])


def topk_cases(top_k):
    return [(kind, n) for kind in TOPK_KINDS for n in topk_sizes(top_k)]


def topk_predicate(kind, n, top_k):
    """the probe scores m = min(n, K) against the true list, and another score once the K-th member is swapped for the (K+1)-th keypoint (n > K)
    or dropped (n <= K): the expected score pins the list's membership"""
    f, p = topk_frame(kind, n), topk_probe(kind, n, top_k)
    order = sr.topk_order(f["kp"]["response"], n)
    m = min(n, top_k)
    P = ref_list(p, top_k)
    right = sr.score_lists(f["desc"][order[:m]], P, 100)
    other = np.concatenate([order[:m - 1], order[m:m + 1]]) if n > top_k else order[:m - 1]
    wrong = sr.score_lists(f["desc"][other], P, 100)
    return len(P) == m and right == m and wrong != right


def topk_kind_fact(kind, n, top_k):
    """what the response kind promises about the keys at the K boundary"""
    r = topk_frame(kind, n)["kp"]["response"]
    order = sr.topk_order(r, n)
    tie_at_cut = n > top_k and r[order[top_k - 1]] == r[order[top_k]]
    if kind == "equal":
        return len(np.unique(r)) == 1 and (n <= top_k or tie_at_cut)
    if kind == "two_values":
        return len(np.unique(r)) <= 2 and (n <= top_k or (tie_at_cut and r[order[top_k]] == r.min() and (r == r.min()).sum() > (r == r.max()).sum()))
    if kind == "last_bit":
        u = r.view(np.uint32)
        return int(u.max() - u.min()) <= 3 and (n < 8 or len(np.unique(u)) > 1)
    if kind == "mixed":
        u = set(r.view(np.uint32).tolist())
        want = set(MIXED_VALUES.view(np.uint32).tolist())
        return not np.isnan(r).any() and (n < 10 or want <= u)
    if kind == "strong_last":
        return (np.diff(r) > 0).all() and (n <= top_k or order[0] == n - 1)
    raise KeyError(kind)


# ---- nearest-neighbour cases ------------------------------------------------------------------------------------------------------------------
NN_KS = (32, 96, 512)
NN_RATIOS = (1, 50, 80, 99, 100)
NN_LENGTHS = {1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 511, 512}     # 1, 2, the block edges, and K - 1, K of every NN_KS


def _lists(seed, ma, mb):
    """random rows; the first rows of B are copies of rows of A with noise of growing amplitude, so d1 / d2 covers the ratios"""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 256, (ma, 128), dtype=np.uint8)
    B = rng.integers(0, 256, (mb, 128), dtype=np.uint8)
    k = min(ma, mb)
    amp = np.array([0, 2, 8, 30, 80, 120])[np.arange(k) % 6]
    noisy = np.clip(A[:k].astype(np.int64) + (rng.uniform(-1, 1, (k, 128)) * amp[:, None]).astype(np.int64), 0, 255)
    B[rng.permutation(mb)[:k]] = noisy.astype(np.uint8)
    return A, B, rng


def _center(rng):
    return rng.integers(16, 240, 128).astype(np.int64)


def _tie(rng, Q, T, q, q2, ps):
    """Q[q] = c; T[p] = c + 3 e_k for the positions ps; Q[q2] = T[ps[-1]]"""
    c = _center(rng)
    Q[q] = c
    for k, p in enumerate(ps):
        t = c.copy()
        t[k] += 3
        T[p] = t
    Q[q2] = T[ps[-1]]
    return dict(kind="tie", q=q, q2=q2, ps=tuple(ps))


def _dup(rng, Q, T, q, ps):
    """Q[q] = c; T[p] = c + 3 e_0 for every p of ps: equal rows"""
    c = _center(rng)
    Q[q] = c
    c[0] += 3
    for p in ps:
        T[p] = c
    return dict(kind="dup", q=q, ps=tuple(ps))


def gadget_holds(g, Q, T):
    """the gadget as the restatement sees it: the query's minimum (9) lies at exactly the positions ps"""
    D = dist(Q[g["q"]:g["q"] + 1], T)[0]
    at = tuple(np.flatnonzero(D == D.min()).tolist())
    ok = D.min() == 9 and at == tuple(sorted(g["ps"]))
    if g["kind"] == "tie":
        ok = ok and (Q[g["q2"]] == T[g["ps"][-1]]).all() and len({T[p].tobytes() for p in g["ps"]}) == len(g["ps"])
    else:
        ok = ok and len({T[p].tobytes() for p in g["ps"]}) == 1
    return bool(ok)


def same_lane(p, p2):
    """rows of one 32-row train block that one lane of nn_direction holds (rows 8 g + 4 hi + r: the lane's half-wave is bit 2 of the row)"""
    return p // 32 == p2 // 32 and (p >> 2) & 1 == (p2 >> 2) & 1


def _nn_case(name, A, B, gadgets=(), **facts):
    """gadgets: (direction, gadget); direction "ab": A's rows are the queries"""
    return dict(name=name, A=ordered(A), B=ordered(B), gadgets=list(gadgets), **facts)


@functools.lru_cache(maxsize=None)
def nn_cases():
    out = []
    for k, (ma, mb) in enumerate([(1, 1), (1, 2), (2, 2), (2, 31), (31, 32), (32, 33), (33, 63), (63, 64), (64, 65), (65, 95), (95, 96), (96, 511),
                                  (511, 512), (512, 512), (512, 1)]):
        A, B, _ = _lists(100 + k, ma, mb)
        out.append(_nn_case("random_%d_%d" % (ma, mb), A, B))
    # ties inside one lane: rows 1, 2 (r = 1, 2) and rows 11, 16 (g = 1, 2 of the same half-wave); the other direction: rows 9, 10
    A, B, rng = _lists(200, 33, 65)
    g = [("ab", _tie(rng, A, B, 3, 20, (1, 2))), ("ab", _tie(rng, A, B, 5, 21, (11, 16))), ("ba", _tie(rng, B, A, 40, 41, (9, 10)))]
    out.append(_nn_case("tie_lane", A, B, g, where="lane"))
    # ties across the half-waves: rows p and p + 4
    A, B, rng = _lists(201, 32, 64)
    g = [("ab", _tie(rng, A, B, 0, 1, (1, 5))), ("ba", _tie(rng, B, A, 30, 31, (26, 30)))]
    out.append(_nn_case("tie_half", A, B, g, where="half"))
    # ties across 32-row train blocks: rows p and p + 32
    A, B, rng = _lists(202, 63, 65)
    g = [("ab", _tie(rng, A, B, 2, 3, (5, 37))), ("ba", _tie(rng, B, A, 64, 63, (30, 62)))]
    out.append(_nn_case("tie_block", A, B, g, where="block"))
    # three equal smallest distances: lane, half-wave and block at once
    A, B, rng = _lists(203, 64, 96)
    g = [("ab", _tie(rng, A, B, 7, 8, (6, 10, 42))), ("ba", _tie(rng, B, A, 90, 91, (0, 33, 63)))]
    out.append(_nn_case("tie_three", A, B, g, where="three"))
    # query-side duplicates 32 and 128 positions apart (query blocks 0, 1, 4: waves 0, 1 and wave 0's second trip); as train rows of the other
    # direction they tie across blocks 0, 1, 4; ties 128 and 32 rows apart in that direction with the second query that tells them apart
    A, B, rng = _lists(204, 512, 511)
    c = _center(rng)
    A[3] = A[35] = A[131] = c
    c[0] += 3
    B[17] = c
    g = [("ba", _tie(rng, B, A, 200, 201, (40, 168))), ("ba", _tie(rng, B, A, 202, 203, (300, 332))), ("ab", _tie(rng, A, B, 400, 401, (100, 228, 510)))]
    out.append(_nn_case("dup_query_blocks", A, B, g, where="query", dup_queries=(3, 35, 131), dup_train=17))
    # equal train rows: p, p + 1 (one lane), p, p + 4 (the half-waves), p, p + 32 (two blocks), in both directions
    A, B, rng = _lists(205, 65, 95)
    g = [("ab", _dup(rng, A, B, 0, (1, 2))), ("ab", _dup(rng, A, B, 1, (9, 13))), ("ab", _dup(rng, A, B, 2, (20, 52))),
         ("ba", _dup(rng, B, A, 70, (33, 34))), ("ba", _dup(rng, B, A, 71, (3, 7))), ("ba", _dup(rng, B, A, 72, (31, 63)))]
    out.append(_nn_case("dup_train", A, B, g, where="dup"))
    # ratio_pct 50 at equality: an all-zero query, train rows at distances (1, 4): fails; (1, 5): passes; (0, 0): fails.  Two rows each, and
    # the same with the rows at the block edges (query 32, train 31 and 64)
    for tag, second in (("1_4", (0, 2, 0)), ("1_5", (0, 2, 1)), ("0_0", (0, 0, 0))):
        for (ma, mb, q, p1, p2) in ((2, 2, 0, 0, 1), (33, 65, 32, 31, 64)):
            rng = np.random.default_rng(300 + ma)
            A = rng.integers(100, 256, (ma, 128), dtype=np.uint8)
            B = rng.integers(100, 256, (mb, 128), dtype=np.uint8)
            A[q] = 0
            B[p1] = 0
            B[p2] = 0
            if tag != "0_0":
                B[p1, 0] = 1
            B[p2, 1:3] = second[1:]
            out.append(_nn_case("ratio_%s_%d_%d" % (tag, ma, mb), A, B, ratio=dict(q=q, p1=p1, p2=p2, d=(0, 0) if tag == "0_0" else (1, 4 if tag == "1_4" else 5))))
    # one train row: d2 is infinite, the copy passes at every ratio
    A, B, rng = _lists(206, 65, 1)
    B[0] = A[40]
    out.append(_nn_case("one_train_row", A, B, one_row=True))
    # the largest distance and the extreme norms
    out.append(_nn_case("zeros_vs_255", np.zeros((33, 128), np.uint8), np.full((65, 128), 255, np.uint8), extreme=True))
    A = np.zeros((64, 128), np.uint8)
    A[1::2] = 255
    B = np.zeros((63, 128), np.uint8)
    B[0::2] = 255
    out.append(_nn_case("zeros_255_mixed", A, B, extreme=True))
    return out


def nn_case(name):
    return next(c for c in nn_cases() if c["name"] == name)


def nn_frames():
    """the cases' frames in the order A0, B0, A1, B1, ... then empty frames against 0, 1 and K rows; with window 2 every case's pair is in scope"""
    fs = [f for c in nn_cases() for f in (c["A"], c["B"])]
    rng = np.random.default_rng(250)
    empty = ordered(np.zeros((0, 128), np.uint8))
    fs += [empty, empty, ordered(rng.integers(0, 256, (1, 128), dtype=np.uint8)), empty, ordered(rng.integers(0, 256, (512, 128), dtype=np.uint8))]
    return fs


def nn_predicate(c):
    """at full length (top_k 512) the case is what its name says"""
    A, B = c["A"]["desc"], c["B"]["desc"]
    ok = True
    for d, g in c["gadgets"]:
        Q, T = (A, B) if d == "ab" else (B, A)
        ok = ok and gadget_holds(g, Q, T)
        ps = g["ps"]
        if c.get("where") == "lane":
            ok = ok and same_lane(ps[0], ps[1])
        if c.get("where") == "half":
            ok = ok and ps[1] == ps[0] + 4 and ps[0] // 32 == ps[1] // 32 and not same_lane(ps[0], ps[1])
        if c.get("where") == "block":
            ok = ok and ps[1] == ps[0] + 32
        if c.get("where") == "three":
            ok = ok and len(ps) == 3
    if c.get("where") == "dup":
        shapes = sorted((g["ps"][1] - g["ps"][0]) for _, g in c["gadgets"])
        ok = ok and shapes == [1, 1, 4, 4, 32, 32]
        # every gadget query fails below 100 and passes at 100
        for d, g in c["gadgets"]:
            Q, T = (A, B) if d == "ab" else (B, A)
            _, d1, d2 = sr.nn_stats(Q[g["q"]:g["q"] + 1], T)
            ok = ok and d1[0] == d2[0] == 9 and not sr.passes(d1, d2, 99)[0] and sr.passes(d1, d2, 100)[0]
    if c.get("where") == "query":
        q0, q1, q2 = c["dup_queries"]
        nn, d1, _ = sr.nn_stats(A[[q0, q1, q2]], B)
        back, b1, b2 = sr.nn_stats(B[c["dup_train"]:c["dup_train"] + 1], A)
        ok = ok and (q1 - q0, q2 - q0) == (32, 128) and (nn == c["dup_train"]).all() and (d1 == 9).all() and back[0] == q0 and b1[0] == b2[0] == 9
    if "ratio" in c:
        r = c["ratio"]
        nn, d1, d2 = sr.nn_stats(A[r["q"]:r["q"] + 1], B)
        want = r["d"] == (1, 5)
        ok = ok and not A[r["q"]].any() and (int(d1[0]), int(d2[0])) == r["d"] and nn[0] == r["p1"] and bool(sr.passes(d1, d2, 50)[0]) == want
        ok = ok and (r["d"] != (1, 4) or 10000 * 1 == 50 * 50 * 4)
        # the case's score is the gadget's query alone: 0 or 1
        ok = ok and sr.score_lists(A, B, 50) == int(want) and sr.score_lists(A, B, 100) >= 1
    if c.get("one_row"):
        ok = ok and len(B) == 1 and all(sr.score_lists(A, B, r) == 1 for r in NN_RATIOS)
    if c.get("extreme"):
        D = dist(A, B)
        ok = ok and D.max() == MAX_D and MAX_D < (1 << 23) and set(np.unique(A)) | set(np.unique(B)) == {0, 255}
    return bool(ok)


def nn_lengths_covered():
    got = {len(c[s]["desc"]) for c in nn_cases() for s in "AB"}
    return NN_LENGTHS <= got


# ---- scope and launch cases -------------------------------------------------------------------------------------------------------------------
SCOPE_K = 32
BIG_N = 2900
BIG_PAIRS = BIG_N * (BIG_N - 1) // 2                       # 4 203 550 = 2^22 + 9 246


@functools.lru_cache(maxsize=None)
def codebook():
    """12 rows: 6 random ones and a near copy of each (noise +-4), so that different rows can pass ratio_pct 80"""
    rng = np.random.default_rng(77)
    base = rng.integers(8, 248, (6, 128))
    near = base + rng.integers(-4, 5, (6, 128))
    return np.concatenate([base, near]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def codebook_frames(n, seed, max_rows):
    """n frames of 0 .. max_rows distinct codebook rows"""
    rng = np.random.default_rng(seed)
    cb = codebook()
    out = []
    for _ in range(n):
        k = int(rng.integers(0, max_rows + 1))
        out.append(ordered(cb[rng.permutation(len(cb))[:k]]))
    return out


def scope_windows(n):
    return sorted({0, 2, 3, n - 1, n, n + 5})


def scope_frames(n):
    return codebook_frames(n, 400 + n, 3)


def big_frames():
    return codebook_frames(BIG_N, 2900, 2)


def scope_expected(frames, ratio_pct, window, top_k=SCOPE_K):
    return sr.score_matrix_batched([ref_list(f, top_k) for f in frames], ratio_pct, window)


@functools.lru_cache(maxsize=None)
def big_expected():
    S = scope_expected(big_frames(), 80, 0)
    S.setflags(write=False)
    return S


def big_predicate():
    """two launches, the second not a multiple of 8 wide, and a matrix that moves when the second launch's pairs move by one"""
    S = big_expected()
    a, b = sr.pair_list(BIG_N)
    flat = S[a, b]
    second = flat[sr.PAIR_CHUNK:]
    return (len(a) == BIG_PAIRS and sr.chunk_bases(len(a)) == [0, 1 << 22] and len(second) == 9246 and len(second) % 8 != 0
            and len(np.unique(flat)) >= 3 and len(np.unique(second)) >= 3 and bool((second[1:] != second[:-1]).any()))


# ---- selection cases --------------------------------------------------------------------------------------------------------------------------
SEL_K = 32
TOKENS = dict(L0=0, L1=1, G=2, Hh=3, X=4)


def token(j):
    t = np.zeros(128, np.uint8)
    t[2 * j:2 * j + 2] = 200
    return t


@functools.lru_cache(maxsize=None)
def select_frames(n, first):
    """positions below `first` hold {L0, L1}, the others {G, Hh}; every position with b mod 7 == 3 also holds X.  Distinct tokens are all at
    the same distance, so only equal tokens pass the ratio test: score = number of shared tokens (0 .. 3)"""
    out = []
    for b in range(n):
        names = ["L0", "L1"] if b < first else ["G", "Hh"]
        if b % 7 == 3:
            names.append("X")
        out.append(ordered(np.stack([token(TOKENS[t]) for t in names])))
    return out


@functools.lru_cache(maxsize=None)
def select_scores(n, first, window=0):
    S = scope_expected(select_frames(n, first), 80, window, SEL_K)
    S.setflags(write=False)
    return S


def _sel(n, first, partners, min_score, window=0, rank=0, world=1):
    return dict(n=n, first=first, partners=partners, min_score=min_score, window=window, rank=rank, world=world)


def select_cases():
    K = SEL_K
    return [
        _sel(700, 63, 1, 1),                                         # cut at 63 (rows > 63) and 64 (row 63)
        _sel(700, 511, 1, -5, 0, 0, 3),                              # cut at 511 and, for row 511, at 512: three trips
        _sel(700, 63, 300, 0, 0, 1, 3),                              # rows below 63: the threshold falls to min_score = 0
        _sel(700, 63, 300, 1, 0, 2, 3),                              # rows below 63: fewer than 300 candidates
        _sel(513, 255, 1, 1, 0, 0, 514),                             # cut at 255 and 256
        _sel(513, 255, 512, 0, 0, 513, 514),                         # rank n of world n + 1 owns nothing
        _sel(513, 255, 523, K + 1),                                  # min_score above top_k: nothing
        _sel(513, 255, 2, 1),                                        # cut at 256 (rows > 256)
        _sel(257, 100, 0, 1),
        _sel(257, 100, 2, 0, 257),
        _sel(257, 100, 0, -5, 2),
        _sel(256, 63, 2, 1, 5, 1, 3),
        _sel(256, 63, 300, 0, 256),
        _sel(255, 63, 254, 1, 0, 0, 3),
        _sel(255, 63, 1, K, 5, 2, 3),                                # min_score == top_k: nothing
        _sel(3, 1, 1, 0, 2),
        _sel(3, 1, 13, -5, 0, 0, 4),
        _sel(3, 1, 2, 1, 3, 3, 4),
        _sel(2, 0, 1, -5),
        _sel(2, 0, 0, 0, 2, 0, 3),
        _sel(2, 0, 12, 1, 0, 2, 3),
    ]


def select_id(c):
    return "n%d_f%d_p%d_m%d_w%d_r%dof%d" % (c["n"], c["first"], c["partners"], c["min_score"], c["window"], c["rank"], c["world"])


@functools.lru_cache(maxsize=None)
def select_expected(n, first, partners, min_score, window):
    """the world-1 list of the case (sr.select_pairs); a rank's shard is its rows"""
    out = sr.select_pairs(select_scores(n, first, window), partners, min_score, window)
    out.setflags(write=False)
    return out


def shard(pairs, rank, world):
    return pairs[pairs[:, 0] % world == rank]


@functools.lru_cache(maxsize=None)
def select_rows(n, first, partners, min_score, window):
    """per row, from sr.nominations alone: (threshold score, last nominated tied position or -1, tie is cut, candidates in scope).  The
    threshold is the lowest nominated score; the tie is cut when a candidate with that score is not nominated"""
    S = select_scores(n, first, window)
    nom = sr.nominations(S, partners, min_score, window)
    a, b = np.mgrid[0:n, 0:n]
    scope = (a != b) & (S >= max(min_score, 0))
    if window:
        scope &= np.abs(a - b) < window
    N = np.zeros((n, n), bool)
    for r, s in enumerate(nom):
        N[r, list(s)] = True
    rows = []
    for r in range(n):
        if not N[r].any():
            rows.append((None, -1, False, int(scope[r].sum())))
            continue
        t = int(S[r][N[r]].min())
        tied = scope[r] & (S[r] == t)
        cut = bool((tied & ~N[r]).any())
        rows.append((t, int(np.flatnonzero(tied & N[r]).max()) if cut else -1, cut, int(scope[r].sum())))
    return rows


def select_facts(c):
    """what the case reaches: the set of cut positions, trips of the tie scan, threshold == min_score under a cut, rows short of candidates"""
    rows = select_rows(c["n"], c["first"], c["partners"], c["min_score"], c["window"])
    lo = [max(0, a - c["window"] + 1) if c["window"] else 0 for a in range(c["n"])]
    cuts = {r[1] for r in rows if r[2]}
    trips = max([(r[1] - lo[a]) // SEL_NT + 1 for a, r in enumerate(rows) if r[2]], default=0)
    at_min = any(r[2] and r[0] == max(c["min_score"], 0) for r in rows)
    short = c["partners"] > 0 and any(r[3] < c["partners"] for r in rows)
    return dict(cuts=cuts, trips=trips, at_min=at_min, short=short)


def brute_select(S, partners, min_score, window=0, rank=0, world=1):
    """an independent statement of the selection: a stable sort of every row by score, whole-matrix nomination flags"""
    n = S.shape[0]
    a, b = np.mgrid[0:n, 0:n]
    scope = (a != b) & (S >= max(min_score, 0))
    if window:
        scope &= np.abs(a - b) < window
    key = np.where(scope, -S.astype(np.int64), 1 << 40)
    order = np.argsort(key, axis=1, kind="stable")            # score descending, position ascending, out-of-scope last
    place = np.empty_like(order)
    np.put_along_axis(place, order, np.broadcast_to(np.arange(n), (n, n)).copy(), 1)
    nom = scope & ((place < partners) | (partners == 0))
    keep = (nom | nom.T) & (a < b) & (a % world == rank)
    return np.argwhere(keep).astype(np.int32).reshape(-1, 2)
