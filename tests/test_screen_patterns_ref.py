"""CPU: the cases of tests/screen_patterns.py are what they claim, shown on the restatement alone (tests/screen_ref.py).

  * every case's predicate holds: the top-K probes pin the list's membership at every (response kind, n, top_k); the nn gadgets tie where they
    say (lane, half-wave, train block, three ways, query blocks); the ratio cases sit at exact equality; the 2900-frame list has two launches
    and a matrix that moves with the second launch's pairs; the selection cases cut their ties at 63, 64, 255, 256, 511 and in a third trip,
    with the threshold on min_score and with rows short of candidates;
  * the batched restatement (score_matrix_batched) equals score_lists on 2400 sampled pairs of the 2900-frame case and on whole small cases;
  * sr.select_pairs equals an independent brute-force statement;
  * sensitivity: six mutations of a COPY of the restatement each change the expected value of a named case.
"""
import importlib.util

import numpy as np
import pytest

from tests import screen_patterns as sp
from tests import screen_ref as sr


# ---- predicates -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k", sp.TOPK_KS)
def test_topk_cases_pin_membership(top_k):
    cases = sp.topk_cases(top_k)
    assert {n for _, n in cases} >= {1, 31, 32, 33, top_k - 1, top_k, top_k + 1, 513, 1025, 5000} and {k for k, _ in cases} == set(sp.TOPK_KINDS)
    for kind, n in cases:
        assert sp.topk_kind_fact(kind, n, top_k), (kind, n, top_k)
        assert sp.topk_predicate(kind, n, top_k), (kind, n, top_k)
    assert max(n for _, n in cases) > 8 * sp.TOPK_NT                  # all-equal responses: the radix select walks all eight bytes


def test_nn_cases_reach_their_edges():
    assert sp.nn_lengths_covered()
    names = [c["name"] for c in sp.nn_cases()]
    assert len(set(names)) == len(names)
    for c in sp.nn_cases():
        assert sp.nn_predicate(c), c["name"]
    for want in ("tie_lane", "tie_half", "tie_block", "tie_three", "dup_query_blocks", "dup_train", "ratio_1_4_2_2", "ratio_1_5_33_65", "ratio_0_0_2_2",
                 "one_train_row", "zeros_vs_255"):
        assert want in names
    fs = sp.nn_frames()
    assert [len(f["kp"]) for f in fs[-5:]] == [0, 0, 1, 0, 512]        # empty against 0, 1 and K rows under window 2


def test_scope_and_launch_cases():
    for n in (7, 300):
        ws = sp.scope_windows(n)
        assert set(ws) == {0, 2, 3, n - 1, n, n + 5}
        frames = sp.scope_frames(n)
        assert {len(f["kp"]) for f in frames} == {0, 1, 2, 3}
        S = sp.scope_expected(frames, 80, 3)
        a, b = np.mgrid[0:n, 0:n]
        assert (S[(a == b) | (np.abs(a - b) >= 3)] == -1).all() and (S[(a != b) & (np.abs(a - b) < 3)] >= 0).all()
        assert len(np.unique(sp.scope_expected(frames, 80, 0))) >= 3
    assert sp.big_predicate()


SELECT = sp.select_cases()


def test_selection_cases_cover_every_value():
    n_of = {c["n"] for c in SELECT}
    assert n_of == {2, 3, 255, 256, 257, 513, 700}
    assert {0, 1, 2, 300} <= {c["partners"] for c in SELECT}
    assert any(c["partners"] == c["n"] - 1 for c in SELECT) and any(c["partners"] == c["n"] + 10 for c in SELECT)
    assert {c["min_score"] for c in SELECT} == {-5, 0, 1, sp.SEL_K, sp.SEL_K + 1}
    assert {0, 2, 5} <= {c["window"] for c in SELECT} and any(c["window"] == c["n"] for c in SELECT)
    rw = {(c["rank"], c["world"]) for c in SELECT}
    assert {(0, 1), (0, 3), (1, 3), (2, 3)} <= rw
    assert any(c["rank"] == 0 and c["world"] == c["n"] + 1 for c in SELECT) and any(c["rank"] == c["n"] and c["world"] == c["n"] + 1 for c in SELECT)


def test_selection_cases_reach_their_edges():
    facts = {sp.select_id(c): sp.select_facts(c) for c in SELECT}
    cuts = set().union(*(f["cuts"] for f in facts.values()))
    assert {63, 64, 255, 256, 511} <= cuts, sorted(cuts)               # wave edge, wave start, last of trip 1, first of trip 2, last of trip 2
    assert max(f["trips"] for f in facts.values()) == 3
    assert any(f["at_min"] for f in facts.values())
    assert any(f["short"] for f in facts.values())
    f = facts[sp.select_id(SELECT[0])]
    assert {63, 64} <= f["cuts"]
    f = facts[sp.select_id(SELECT[1])]
    assert {511, 512} <= f["cuts"] and f["trips"] == 3
    assert facts[sp.select_id(SELECT[2])]["at_min"] and facts[sp.select_id(SELECT[3])]["short"]
    # the scores behind them: a small range, whole rows tied
    S = sp.select_scores(700, 63)
    assert set(np.unique(S).tolist()) == {-1, 0, 1, 2, 3}


# ---- the batched form -------------------------------------------------------------------------------------------------------------------------
def test_batched_form_equals_score_lists():
    frames = sp.big_frames()
    lists = [sp.ref_list(f, sp.SCOPE_K) for f in frames]
    S = sp.big_expected()
    a, b = sr.pair_list(sp.BIG_N)
    rng = np.random.default_rng(5)
    pick = np.concatenate([rng.integers(0, len(a), 2000), np.arange(sr.PAIR_CHUNK - 200, sr.PAIR_CHUNK + 200)])
    for g in pick:
        assert S[a[g], b[g]] == S[b[g], a[g]] == sr.score_lists(lists[a[g]], lists[b[g]], 80), (int(g), int(a[g]), int(b[g]))
    # the flat list is score_matrix's walk, with and without a window
    for n, w in ((7, 0), (7, 3), (7, 12), (2, 0), (1, 0), (0, 0)):
        a, b = sr.pair_list(n, w)
        assert list(zip(a.tolist(), b.tolist())) == [(i, j) for i in range(n) for j in range(i + 1, n) if not w or j - i < w]
    # whole matrices: scope cases, every window and ratio; selection frames; lists of different lengths with duplicates
    fr = sp.scope_frames(7)
    l7 = [sp.ref_list(f, sp.SCOPE_K) for f in fr]
    for w in sp.scope_windows(7):
        for r in sp.NN_RATIOS:
            assert np.array_equal(sr.score_matrix_batched(l7, r, w), sr.score_matrix(l7, r, w)), (w, r)
    l60 = [sp.ref_list(f, sp.SEL_K) for f in sp.select_frames(60, 20)]
    assert np.array_equal(sr.score_matrix_batched(l60, 80, 0, chunk=97), sr.score_matrix(l60, 80))
    lt = [sp.ref_list(c[s], 32)[:6] for c in sp.nn_cases()[15:22] for s in "AB"]
    for r in (50, 100):
        assert np.array_equal(sr.score_matrix_batched(lt, r), sr.score_matrix(lt, r))


# ---- the selection against a brute-force statement --------------------------------------------------------------------------------------------
def test_select_pairs_equals_brute_force():
    rng = np.random.default_rng(9)
    mats = [sp.select_scores(n, first, w) for (n, first, w) in ((2, 0, 0), (3, 1, 0), (3, 1, 2), (60, 20, 0), (60, 20, 5))]
    R = rng.integers(0, 4, (40, 40)).astype(np.int32)
    R = np.triu(R, 1) + np.triu(R, 1).T - np.eye(40, dtype=np.int32)
    mats.append(R)
    for S in mats:
        n = S.shape[0]
        w = 0 if (S[0, n - 1] >= 0 or n < 3) else next(d for d in range(1, n) if S[0, d] < 0)
        for partners in (0, 1, 2, 7, n - 1, n + 10):
            for min_score in (-5, 0, 1, 2, 33):
                for rank, world in ((0, 1), (1, 3), (0, n + 1), (n, n + 1)):
                    got = sr.select_pairs(S, partners, min_score, w, rank, world)
                    assert np.array_equal(got, sp.brute_select(S, partners, min_score, w, rank, world)), (n, w, partners, min_score, rank, world)
                    assert np.array_equal(got, sp.shard(sr.select_pairs(S, partners, min_score, w), rank, world))
    # a large case too, once
    c = SELECT[0]
    assert np.array_equal(sp.select_expected(c["n"], c["first"], c["partners"], c["min_score"], c["window"]),
                          sp.brute_select(sp.select_scores(c["n"], c["first"]), c["partners"], c["min_score"]))


# ---- sensitivity: mutations of a copy of the restatement ---------------------------------------------------------------------------------------
def mutant():
    spec = importlib.util.spec_from_file_location("screen_ref_mutant", sr.__file__)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m is not sr and m.score_lists is not sr.score_lists
    return m


def pair_score(mod, c, ratio, top_k=512):
    return mod.score_lists(mod.top_list(c["A"]["kp"], c["A"]["desc"], top_k), mod.top_list(c["B"]["kp"], c["B"]["desc"], top_k), ratio)


def test_mutation_tie_to_higher_position():
    m = mutant()

    def nn_stats(Q, T):
        nn, d1, d2 = sr.nn_stats(Q, T)
        D = sp.dist(Q, T)
        return T.shape[0] - 1 - np.argmin(D[:, ::-1], axis=1), d1, d2
    m.nn_stats = nn_stats
    for name in ("tie_lane", "tie_half", "tie_block", "tie_three", "dup_query_blocks"):
        c = sp.nn_case(name)
        assert pair_score(m, c, 100) != pair_score(sr, c, 100), name
        assert pair_score(sr, c, 100) - pair_score(m, c, 100) == len(c["gadgets"]), name     # each gadget alone loses its mutual match


def test_mutation_ratio_less_or_equal():
    m = mutant()
    m.passes = lambda d1, d2, r: np.ones(len(d1), bool) if r >= 100 else np.int64(10000) * d1 <= np.int64(r) * np.int64(r) * d2
    for name in ("ratio_1_4_2_2", "ratio_1_4_33_65", "ratio_0_0_2_2", "ratio_0_0_33_65"):
        c = sp.nn_case(name)
        assert (pair_score(sr, c, 50), pair_score(m, c, 50)) == (0, 1), name
    for name in ("ratio_1_5_2_2", "ratio_1_5_33_65"):
        c = sp.nn_case(name)
        assert (pair_score(sr, c, 50), pair_score(m, c, 50)) == (1, 1), name


def test_mutation_d2_over_the_set():
    m = mutant()

    def nn_stats(Q, T):
        nn, d1, _ = sr.nn_stats(Q, T)
        D = sp.dist(Q, T)
        d2 = np.where(D > d1[:, None], D, sr.INF).min(axis=1)
        return nn, d1, d2
    m.nn_stats = nn_stats
    c = sp.nn_case("dup_train")
    for ratio in (50, 80, 99):
        assert pair_score(m, c, ratio) - pair_score(sr, c, ratio) == len(c["gadgets"]), ratio
    assert pair_score(m, sp.nn_case("ratio_0_0_2_2"), 50) != pair_score(sr, sp.nn_case("ratio_0_0_2_2"), 50)


def test_mutation_kth_key_by_index_descending():
    m = mutant()

    def topk_order(response, top_k):
        full = sr.topk_order(response, len(response))
        r = np.asarray(response, np.float32)[full] + np.float32(0.0)         # -0 == +0
        out = full.copy()
        s = 0
        while s < len(out):                                                   # every run of equal responses in descending index order
            e = s
            while e < len(out) and r[e] == r[s]:
                e += 1
            out[s:e] = out[s:e][::-1]
            s = e
        return out[:top_k]
    m.topk_order = topk_order
    caught = set()
    for top_k in sp.TOPK_KS:
        for kind, n in sp.topk_cases(top_k):
            f, p = sp.topk_frame(kind, n), sp.topk_probe(kind, n, top_k)
            r = f["kp"]["response"]
            order = sr.topk_order(r, n)
            if n <= top_k or r[order[top_k - 1]] != r[order[top_k]]:
                continue                                                      # no tie across the K boundary: the index order cannot show
            P = sp.ref_list(p, top_k)
            right = sr.score_lists(sr.top_list(f["kp"], f["desc"], top_k), P, 100)
            wrong = m.score_lists(m.top_list(f["kp"], f["desc"], top_k), P, 100)
            assert right == top_k and wrong != right, (kind, n, top_k)
            caught.add((kind, top_k))
    assert caught >= {(kind, k) for kind in ("equal", "two_values", "last_bit", "mixed") for k in sp.TOPK_KS}


def test_mutation_tie_cut_one_late():
    m = mutant()

    def nominations(S, partners, min_score, window=0):
        nom = sr.nominations(S, partners, min_score, window)
        n = S.shape[0]
        for a in range(n):
            if not nom[a]:
                continue
            t = min(int(S[a, b]) for b in nom[a])
            last = max(b for b in nom[a] if S[a, b] == t)
            later = [b for b in range(last + 1, n) if b != a and (not window or abs(b - a) < window) and S[a, b] == t]
            if later:
                nom[a] = (nom[a] - {last}) | {later[0]}
        return nom
    m.nominations = nominations
    for k in (0, 7):
        c = SELECT[k]
        S = sp.select_scores(c["n"], c["first"], c["window"])
        want = sp.select_expected(c["n"], c["first"], c["partners"], c["min_score"], c["window"])
        assert not np.array_equal(m.select_pairs(S, c["partners"], c["min_score"], c["window"]), want), sp.select_id(c)


def test_mutation_second_launch_base_off_by_one():
    m = mutant()
    m.chunk_bases = lambda total, chunk=sr.PAIR_CHUNK: [b + (1 if b else 0) for b in sr.chunk_bases(total, chunk)]
    lists = [sp.ref_list(f, sp.SCOPE_K) for f in sp.big_frames()]
    a, b = sr.pair_list(sp.BIG_N)
    # the second launch alone, right and shifted: pair g of the launch gets the score of pair g + 1
    codes = sr.list_codes(lists)
    g0 = sr.PAIR_CHUNK
    right = sr.score_pairs_batched(codes, a[g0:], b[g0:], 80)
    assert np.array_equal(right, sp.big_expected()[a[g0:], b[g0:]])
    shifted = sr.score_pairs_batched(codes, a[g0 + 1:], b[g0 + 1:], 80)
    assert (right[:-1] != shifted).any()
    assert m.chunk_bases(len(a)) == [0, g0 + 1]
    l60 = [sp.ref_list(f, sp.SEL_K) for f in sp.select_frames(60, 20)]
    assert not np.array_equal(m.score_matrix_batched(l60, 80, 0, chunk=1000), sr.score_matrix_batched(l60, 80, 0, chunk=1000))
