"""CPU: the numpy restatement of the descriptor screen (tests/screen_ref.py) on small hand-built cases, and a g++ compile check of the
adaptor's screened GetMatchedPairsOneToAllSIFT overload against include/ alone."""
import os
import subprocess

import numpy as np
import pytest

from tests import screen_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows(*vals):
    """u8 descriptor rows whose first byte is the given value (the rest 0): D is the squared difference of the values"""
    out = np.zeros((len(vals), 128), np.uint8)
    out[:, 0] = vals
    return out


def kps(resp):
    from numpy import dtype
    kp = np.zeros(len(resp), dtype([("response", "<f4")]))
    kp["response"] = resp
    return kp


def test_topk_order_ties_in_response_go_to_lower_index():
    assert sr.topk_order(np.array([0.5, 0.9, 0.5, 0.9, 0.1], np.float32), 3).tolist() == [1, 3, 0]
    assert sr.topk_order(np.array([0.5, 0.9, 0.5, 0.9, 0.1], np.float32), 8).tolist() == [1, 3, 0, 2, 4]


def test_topk_order_negative_and_signed_zero():
    r = np.array([-0.0, 0.0, -1.0, 2.0, -0.5], np.float32)
    assert sr.topk_order(r, 5).tolist() == [3, 0, 1, 4, 2]      # -0.0 == +0.0: index order


def test_top_list_follows_the_order():
    d = rows(10, 20, 30)
    assert sr.top_list(kps([0.1, 0.3, 0.2]), d.astype(np.float32), 2)[:, 0].tolist() == [20, 30]


def test_nn_ties_in_distance_go_to_lower_position_and_d1_equals_d2():
    nn, d1, d2 = sr.nn_stats(rows(10), rows(8, 12, 30))
    assert nn.tolist() == [0] and d1.tolist() == [4] and d2.tolist() == [4]


def test_one_row_frame_has_infinite_d2():
    nn, d1, d2 = sr.nn_stats(rows(10, 50), rows(11))
    assert nn.tolist() == [0, 0] and d1.tolist() == [1, 39 * 39] and (d2 == sr.INF).all()
    assert sr.score_lists(rows(10), rows(11), 80) == 1                 # mutual, d2 = +inf on both sides
    assert sr.score_lists(rows(10), rows(11), 1) == 1


def test_ratio_test_and_ratio_100():
    A, B = rows(10, 100), rows(11, 13, 100)
    # q=10: d1 = 1, d2 = 9 -> 10000 < 6400 * 9 passes; t=11 -> nn 10 (d1 1, d2 89^2) passes; q=100 / t=100 exact (d1 0) pass
    assert sr.score_lists(A, B, 80) == 2
    # ties d1 == d2 fail every ratio < 100 and count at 100
    A, B = rows(10), rows(8, 12)
    assert sr.score_lists(A, B, 99) == 0
    assert sr.score_lists(A, B, 100) == 1                              # nn(10) = 8 (lower position), nn(8) = 10: mutual


def test_mutual_check():
    # 10 -> 12, but 12's nearest in A is 13: not mutual; 13 <-> 12 mutual
    assert sr.score_lists(rows(10, 13), rows(12), 100) == 1
    assert sr.score_lists(rows(10, 13), rows(12), 100) == sr.score_lists(rows(12), rows(10, 13), 100)


def test_empty_frame_scores_zero():
    assert sr.score_lists(rows(), rows(1, 2), 80) == 0
    assert sr.score_lists(rows(1, 2), rows(), 100) == 0
    S = sr.score_matrix([rows(1), rows(), rows(1)], 100)
    assert S.tolist() == [[-1, 0, 1], [0, -1, 0], [1, 0, -1]]


def test_one_sided_nominations_are_kept():
    S = np.array([[-1, 9, 8, 0],
                  [9, -1, 1, 1],
                  [8, 1, -1, 7],
                  [0, 1, 7, -1]], np.int32)
    nom = sr.nominations(S, 1, 1)
    assert nom == [{1}, {0}, {0}, {2}]
    # (0, 2): nominated by 2 only; (2, 3): by 3 only
    assert sr.select_pairs(S, 1, 1).tolist() == [[0, 1], [0, 2], [2, 3]]
    # partners == 0: every candidate with score >= min_score
    assert sr.select_pairs(S, 0, 7).tolist() == [[0, 1], [0, 2], [2, 3]]
    assert sr.select_pairs(S, 0, 1).tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]]


def test_score_ties_in_selection_go_to_lower_position():
    S = np.array([[-1, 5, 5, 5],
                  [5, -1, 0, 0],
                  [5, 0, -1, 0],
                  [5, 0, 0, -1]], np.int32)
    assert sr.nominations(S, 2, 1)[0] == {1, 2}
    assert sr.select_pairs(S, 2, 1).tolist() == [[0, 1], [0, 2], [0, 3]]   # (0, 3) through 3's own nomination


def test_window_scope():
    lists = [rows(v) for v in (10, 10, 10, 10, 10)]
    S = sr.score_matrix(lists, 100, window=3)
    assert S[0, 2] == 1 and S[0, 3] == -1 and S[4, 1] == -1 and S[4, 2] == 1 and S[2, 2] == -1
    got = sr.select_pairs(S, 0, 0, window=3)
    assert got.tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3], [2, 4], [3, 4]]
    shards = [sr.select_pairs(S, 0, 0, window=3, rank=r, world=2) for r in range(2)]
    assert sorted(map(tuple, np.concatenate(shards).tolist())) == sorted(map(tuple, got.tolist()))


def test_adaptor_screened_overload_compiles(tmp_path):
    src = tmp_path / "screened.cpp"
    src.write_text('#include "mi355_adaptor.h"\n'
                   'int run(int n, const int* fixed, std::vector<mi355ref::MatchPointPairs>& v) {\n'
                   '    mi355_screen_params sp; mi355_default_screen_params(&sp); sp.window = 0;\n'
                   '    int rc = mi355::GetMatchedPairsOneToAllSIFT(n, 2.5f, 1u, fixed, v, &sp);\n'
                   '    if (rc) return rc;\n'
                   '    rc = mi355::GetMatchedPairsOneToAllSIFT(n, 2.5f, 1u, fixed, v, (const mi355_screen_params*)0);\n'
                   '    return rc ? rc : mi355::GetMatchedPairsOneToAllSIFT(n, 2.5f, 1u, fixed, v, 182);\n'
                   '}\n')
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("ratio", [80, 100])
def test_score_is_symmetric_on_random_lists(ratio):
    rng = np.random.default_rng(3)
    for _ in range(5):
        A = rng.integers(0, 256, (int(rng.integers(1, 40)), 128)).astype(np.uint8)
        B = np.concatenate([A[: len(A) // 2] ^ (rng.integers(0, 2, (len(A) // 2, 128)).astype(np.uint8)),
                            rng.integers(0, 256, (int(rng.integers(0, 20)), 128)).astype(np.uint8)])
        assert sr.score_lists(A, B, ratio) == sr.score_lists(B, A, ratio)
