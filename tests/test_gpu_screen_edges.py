"""GPU: the descriptor screen (csrc/screen.hip) at its list, tie and launch-chunk edges, on the crafted cases of tests/screen_patterns.py
(tests/test_screen_patterns_ref.py shows on the CPU that the cases reach those edges).  Every frame is installed with SetFeatures under an
image id that is not its position (a shuffled arithmetic progression); every comparison is of integers and exact.

  * ScreenScoresDev equals the restatement on every case; the output buffer is filled with a poison value beforehand, so an in-scope entry
    that is not written shows, and a guard row behind the matrix must keep the poison;
  * ScreenPairs equals sr.select_pairs, its scores are the matrix at the returned positions, the count-only form returns the same count,
    and the rank shards of a world (world > n too) partition the world-1 list;
  * the small cases run again after the 2900-frame case and a top_k 512 run in the same context.
"""
import ctypes as C
import time

import numpy as np
import pytest

from tests import screen_patterns as sp
from tests import screen_ref as sr

pytestmark = pytest.mark.gpu
POISON = 0x5A5A5A5A


class Env:
    def __init__(self, ctx):
        self.ctx = ctx
        self.pool = (5 + 3 * np.random.default_rng(31).permutation(20000)).astype(np.int32)       # image ids: shuffled, with gaps
        self.used = 0
        self.ids = {}

    def install(self, key, make):
        """the image id of the frame `key`, installed once"""
        if key not in self.ids:
            f = make()
            i = int(self.pool[self.used])
            self.used += 1
            self.ctx.SetFeatures(i, f["kp"], f["desc"].astype(np.float32), sp.W, sp.H)
            self.ids[key] = i
        return self.ids[key]

    def install_all(self, tag, frames):
        return np.array([self.install((tag, k), lambda f=f: f) for k, f in enumerate(frames)], np.int32)


@pytest.fixture(scope="module")
def env():
    import imagemosaicing_amd as im
    ctx = im.Context(0)
    yield Env(ctx)
    ctx.close()


def dev_scores(env, ids, **params):
    """the n x n matrix from a poisoned buffer with one guard row behind it"""
    import torch
    n = len(ids)
    buf = torch.full((n * n + max(n, 1),), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    env.ctx.ScreenScoresDev(np.asarray(ids, np.int32), buf.data_ptr(), **params)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[n * n:] == POISON).all(), "the guard row behind the matrix was written"
    return h[:n * n].reshape(n, n)


def assert_equal(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first {[(int(a), int(b), int(got[a, b]), int(want[a, b])) for a, b in bad[:6]]}"


def positions(ids, pairs):
    pos = {int(v): k for k, v in enumerate(ids)}
    return np.array([[pos[int(i)], pos[int(j)]] for i, j in pairs], np.int32).reshape(-1, 2)


# ---- top-K lists ------------------------------------------------------------------------------------------------------------------------------
def check_topk(env, top_k):
    cases = sp.topk_cases(top_k)
    ids, lists = [], []
    for kind, n in cases:
        ids.append(env.install(("topk", kind, n), lambda: sp.topk_frame(kind, n)))
        ids.append(env.install(("probe", kind, n, top_k), lambda: sp.topk_probe(kind, n, top_k)))
        lists += [sp.ref_list(sp.topk_frame(kind, n), top_k), sp.ref_list(sp.topk_probe(kind, n, top_k), top_k)]
    got = dev_scores(env, ids, window=2, top_k=top_k, ratio_pct=100)
    assert_equal(got, sr.score_matrix(lists, 100, 2), "top_k %d" % top_k)
    for k, (kind, n) in enumerate(cases):                                     # every member of the true list found: one mutual match each
        assert got[2 * k, 2 * k + 1] == min(n, top_k), (kind, n, top_k, int(got[2 * k, 2 * k + 1]))


@pytest.mark.parametrize("top_k", sp.TOPK_KS)
def test_topk_lists(env, top_k):
    check_topk(env, top_k)


# ---- nearest neighbours -----------------------------------------------------------------------------------------------------------------------
def check_nn(env, top_k, ratios):
    frames = sp.nn_frames()
    ids = env.install_all("nn", frames)
    lists = [sp.ref_list(f, top_k) for f in frames]
    for ratio in ratios:
        got = dev_scores(env, ids, window=2, top_k=top_k, ratio_pct=ratio)
        assert_equal(got, sr.score_matrix(lists, ratio, 2), "nn cases, top_k %d ratio %d" % (top_k, ratio))
    return got


@pytest.mark.parametrize("top_k", sp.NN_KS)
def test_nn_ties_ratios_and_lengths(env, top_k):
    got = check_nn(env, top_k, sp.NN_RATIOS)                                  # the last ratio is 100
    names = [c["name"] for c in sp.nn_cases()]
    if top_k == 512:                                                          # the gadgets' own statement: 2 per tie at the lowest position
        for name in ("tie_lane", "tie_half", "tie_block", "tie_three"):
            k = names.index(name)
            assert got[2 * k, 2 * k + 1] >= 2 * len(sp.nn_case(name)["gadgets"]), name
    n = len(got)
    assert (got[n - 5:, n - 5:][np.triu_indices(5, 1)][[0, 4, 7, 9]] == 0).all()          # the empty frames score 0 with 0, 1 and 512 rows


# ---- scope ------------------------------------------------------------------------------------------------------------------------------------
def check_scope(env, n):
    frames = sp.scope_frames(n)
    ids = env.install_all("scope%d" % n, frames)
    a, b = np.mgrid[0:n, 0:n]
    for w in sp.scope_windows(n):
        got = dev_scores(env, ids, window=w, top_k=sp.SCOPE_K, ratio_pct=80)
        assert_equal(got, sp.scope_expected(frames, 80, w), "n %d window %d" % (n, w))
        out = (a == b) | (np.abs(a - b) >= w if w else False)
        assert (got[out] == -1).all() and (got[~out] >= 0).all() and (got[~out] <= 3).all(), (n, w)
    return ids


@pytest.mark.parametrize("n", [7, 300])
def test_windows(env, n):
    ids = check_scope(env, n)
    if n == 7:
        lists = [sp.ref_list(f, sp.SCOPE_K) for f in sp.scope_frames(7)]
        assert_equal(dev_scores(env, ids, window=3, top_k=sp.SCOPE_K, ratio_pct=80), sr.score_matrix(lists, 80, 3), "n 7 window 3, pair by pair")


def check_tiny(env):
    frames = sp.select_frames(2, 0)
    ids = env.install_all("sel2_0", frames)
    for n in (0, 1, 2):
        got = dev_scores(env, ids[:n], top_k=sp.SEL_K, ratio_pct=80)
        assert_equal(got, sp.select_scores(2, 0)[:n, :n], "n %d" % n)
        for window in (0, 2):
            pairs, scores = env.ctx.ScreenPairs(ids[:n], window=window, top_k=sp.SEL_K, partners=1, min_score=0, return_scores=True)
            want = sr.select_pairs(sp.select_scores(2, 0)[:n, :n], 1, 0, window)
            assert np.array_equal(positions(ids[:n], pairs), want) and len(pairs) == (1 if n == 2 else 0)
            assert scores.tolist() == ([2] if n == 2 else [])


def test_n_0_1_2(env):
    check_tiny(env)


# ---- two launches -----------------------------------------------------------------------------------------------------------------------------
def run_big(env):
    frames = sp.big_frames()
    t0 = time.perf_counter()
    ids = env.install_all("big", frames)
    t1 = time.perf_counter()
    got = dev_scores(env, ids, window=0, top_k=sp.SCOPE_K, ratio_pct=80)
    t2 = time.perf_counter()
    print("2900 frames: install %.2f s, screen and copy %.2f s" % (t1 - t0, t2 - t1))
    return got


def test_2900_frames_two_launches(env):
    got = run_big(env)
    want = sp.big_expected()
    a, b = sr.pair_list(sp.BIG_N)
    assert len(a) == sp.BIG_PAIRS and len(a) - sr.PAIR_CHUNK == 9246
    second = np.zeros(len(a), bool)
    second[sr.PAIR_CHUNK:] = True
    for name, m in (("first launch", ~second), ("second launch", second)):
        bad = np.flatnonzero(got[a[m], b[m]] != want[a[m], b[m]])
        assert len(bad) == 0, f"{name}: {len(bad)} of {int(m.sum())} pairs differ, first {[(int(a[m][g]), int(b[m][g]), int(got[a[m][g], b[m][g]]), int(want[a[m][g], b[m][g]])) for g in bad[:6]]}"
    assert_equal(got, want, "2900 frames")


# ---- selection --------------------------------------------------------------------------------------------------------------------------------
def select_ids(env, n, first):
    return env.install_all("sel%d_%d" % (n, first), sp.select_frames(n, first))


def count_only(env, ids, c):
    import imagemosaicing_amd as im
    ids = np.ascontiguousarray(ids, np.int32)
    p = im.screen_params(window=c["window"], top_k=sp.SEL_K, partners=c["partners"], min_score=c["min_score"], ratio_pct=80)
    n = C.c_int(-1)
    rc = env.ctx.L.mi355_screen_pairs(env.ctx._h, ids.ctypes.data_as(C.c_void_p), len(ids), C.byref(p), c["rank"], c["world"], None, None, 0, C.byref(n))
    assert rc == 0, rc
    return n.value


def check_select(env, c):
    ids = select_ids(env, c["n"], c["first"])
    S = sp.select_scores(c["n"], c["first"], c["window"])
    pairs, scores = env.ctx.ScreenPairs(ids, window=c["window"], top_k=sp.SEL_K, partners=c["partners"], min_score=c["min_score"], ratio_pct=80,
                                        rank=c["rank"], world=c["world"], return_scores=True)
    got = positions(ids, pairs)
    want = sp.shard(sp.select_expected(c["n"], c["first"], c["partners"], c["min_score"], c["window"]), c["rank"], c["world"])
    assert np.array_equal(got, want), (sp.select_id(c), len(got), len(want), got[:5].tolist(), want[:5].tolist())
    assert np.array_equal(scores, S[got[:, 0], got[:, 1]])
    assert count_only(env, ids, c) == len(want)


@pytest.mark.parametrize("c", sp.select_cases(), ids=sp.select_id)
def test_selection(env, c):
    if c["window"] in (0, c["n"]) and c["partners"] == 1:                                        # the device's matrix behind the list, once per frame set
        assert_equal(dev_scores(env, select_ids(env, c["n"], c["first"]), window=c["window"], top_k=sp.SEL_K, ratio_pct=80),
                     sp.select_scores(c["n"], c["first"], c["window"]), sp.select_id(c))
    check_select(env, c)


@pytest.mark.parametrize("n,first,partners,min_score,world", [(700, 63, 1, 1, 3), (700, 63, 300, 0, 3), (257, 100, 2, 0, 258), (3, 1, 1, 0, 4), (2, 0, 1, -5, 3)])
def test_rank_shards_partition_the_list(env, n, first, partners, min_score, world):
    ids = select_ids(env, n, first)
    kw = dict(window=0, top_k=sp.SEL_K, partners=partners, min_score=min_score, ratio_pct=80)
    one = positions(ids, env.ctx.ScreenPairs(ids, **kw))
    assert np.array_equal(one, sp.select_expected(n, first, partners, min_score, 0)) and len(one)
    shards = [positions(ids, env.ctx.ScreenPairs(ids, rank=r, world=world, **kw)) for r in range(world)]
    for r, s in enumerate(shards):
        assert (s[:, 0] % world == r).all()
        assert np.array_equal(s, sp.shard(one, r, world)), (r, world)
    assert sum(len(s) for s in shards) == len(one)
    if world > n:
        assert all(len(shards[r]) == 0 for r in range(n - 1, world))                              # row n - 1 and the ranks past it own no pair


# ---- order independence -----------------------------------------------------------------------------------------------------------------------
def test_small_cases_after_the_large_ones(env):
    """the tables of a 2900-frame run and of a top_k 512 run are in the context's buffers when n and top_k shrink"""
    run_big(env)
    check_topk(env, 512)
    check_nn(env, 512, (80,))
    check_tiny(env)
    check_scope(env, 7)
    check_topk(env, 32)
    check_nn(env, 32, (50, 100))
    for c in sp.select_cases():
        if c["n"] <= 3:
            check_select(env, c)
    run_big(env)
    check_select(env, sp.select_cases()[0])
    check_scope(env, 7)
