"""The adversarial pair-stage inputs of tests/match_patterns.py do what they are for -- checked on the CPU oracle alone, so that a GPU pass on
them (tests/test_gpu_match_edges.py) means something and none of these conditions is ever "checked" by the code under test -- and the composed
oracle (match_patterns.oracle_pair_record, the one place that takes the stage's parameters) equals the oracle's own entry points where those
exist.  oracle.select equals the reference's SelectMatchPairs on the cell-edge and cell-filling patterns wherever the reference stays inside its
label array (oracle/_ref when built, else its recorded outputs: tests/golden/ref_replay.npz)."""
import numpy as np
import pytest

from tests import match_patterns as mp
from tests import oracle_lib as ol
from tests.golden_util import bits


@pytest.fixture(scope="module")
def orc():
    return ol.load_oracle_fast()


# ---- the composition ----------------------------------------------------------------------------------------------------------------------------
def _three_pairs():
    a, b = mp.make_pair(11, 1200, 1200, outliers=0.3), mp.make_pair(12, 777, 900, outliers=0.6)
    c = dict(a, xy2=b["xy2"], d2=b["d2"])                  # unrelated: queries of one pair against the train set of the other
    return [a, b, c]


@pytest.mark.parametrize("ratio", [0.0, 0.8])
def test_composition_equals_the_oracle_entry_points(orc, ratio):
    n_in = []
    for p in _three_pairs():
        for seed in (7, 4242):
            r = mp.record_of(orc, p, mp.DIST, seed, ratio=ratio)
            args = (p["xy1"], p["d1"], p["xy2"], p["d2"], p["w"], p["h"], mp.DIST, seed)
            nin, i1, i2, H, ns = orc.match_pair(*args) if ratio == 0.0 else orc.match_pair_ratio(*args, ratio)
            assert r["n_selected"] == ns and (r["n_in"] if r["accepted"] else 0) == nin
            assert np.array_equal(r["a"], i1[:r["n_in"]]) and np.array_equal(r["b"], i2[:r["n_in"]]) and np.array_equal(bits(r["H"]), bits(H))
            n_in.append(r["n_in"])
    assert min(n_in) < 31 < max(n_in)                      # a rejected pair and accepted ones


def test_composition_of_empty_sets(orc):
    p = mp.make_pair(13, 20, 0)
    for q in (p, dict(p, xy1=p["xy2"], d1=p["d2"], xy2=p["xy1"], d2=p["d1"])):
        r = mp.record_of(orc, q, mp.DIST, 1)
        assert (r["n_selected"], r["n_in"], r["accepted"]) == (0, 0, 0)


# ---- cell edges ---------------------------------------------------------------------------------------------------------------------------------
def test_cells_next_to_the_edges_of_4000_by_3():
    """one ulp below 1333, 2666 and 3999 gives cells 0, 1, 2; the exact values give 1, 2, 3"""
    for k in (1, 2, 3):
        below, at = mp.ulps(1333 * k, -1), np.float32(1333 * k)
        assert mp.cells([[below, 0.0], [at, 0.0]], 4000, 3000, 3, 3)[1].tolist() == [k - 1, k]
        assert mp.cells([[0.0, mp.ulps(1000 * k, -1)], [0.0, 1000.0 * k]], 4000, 3000, 3, 3)[2].tolist() == [k - 1, k]


def _select_ids(orc, p, matches=None):
    m = p["matches"] if matches is None else matches
    o1, o2 = orc.select(m, p["kp1"], p["kp2"], p["nMatch"], p["w"], p["h"], p["gx"], p["gy"])
    return o1, o2


def _check_against_walk(orc, p):
    """the oracle keeps what the walk over the numpy cells keeps: its cell of every point is the numpy one"""
    o1, o2 = _select_ids(orc, p)
    want = p["matches"][p["keep"]]
    assert np.array_equal(np.stack([o1["id"], o2["id"]], 1), want), p["tag"]
    assert np.array_equal(np.stack([o1["x"], o1["y"]], 1), p["kp1"][want[:, 0]]) and np.array_equal(np.stack([o2["x"], o2["y"]], 1), p["kp2"][want[:, 1]])
    return len(o1)


def test_edge_patterns_hold_every_class_and_every_point_counts(orc):
    for p in mp.edge_select_patterns():
        w, h, gx, gy, ng = p["w"], p["h"], p["gx"], p["gy"], p["gx"] * p["gy"]
        e = slice(0, p["n_edge"])
        cell, nx, ny = mp.cells(p["kp1"][p["matches"][e, 0]], w, h, gx, gy)
        inside = (cell >= 0) & (cell < ng)
        alias = inside & ((nx < 0) | (nx >= gx))
        assert inside.sum() >= 5 and (~inside).sum() >= 8, p["tag"]
        assert (cell < 0).sum() >= 2 and (cell >= ng).sum() >= 2 and np.abs(p["kp1"]).max() == mp.FAR, p["tag"]
        if gy > 1:
            assert alias.sum() >= 2 and ((nx == gx) & (ny < gy - 1)).sum() >= 1, p["tag"]              # into the next row
        assert ((nx == gx) & (ny == gy - 1)).sum() >= 1 and (ny >= gy).sum() >= 2, p["tag"]          # out of the grid: clamped
        n = _check_against_walk(orc, p)
        assert n == p["nMatch"] == p["per_grid"] * ng <= 400, p["tag"]                                 # every cell fills
        if (gx, gy) in ((3, 3), (1, 1)):
            assert np.isin(np.arange(p["n_edge"]), p["keep"]).all(), p["tag"]                          # ... after all edge points were taken
        else:
            assert np.isin(np.arange(p["n_edge"]), p["keep"]).mean() > 0.4, p["tag"]


def test_edge_pair_selects_every_edge_point(orc):
    p = mp.edge_pair()
    r = mp.record_of(orc, p, mp.DIST, 7)
    assert (p["w"], p["h"]) == (4001, 2999) and r["n_matches"] == 1400 and r["n_selected"] == 396
    assert np.array_equal(r["kept"][:, 0], np.arange(1400))                                          # the sorted list is the query order
    assert np.isin(np.arange(p["n_edge"]), r["sel1"]["id"]).all() and r["accepted"] == 1


def test_fill_patterns(orc):
    P = {p["tag"]: p for p in mp.fill_patterns()}
    n = {t: _check_against_walk(orc, p) for t, p in P.items()}
    p = P["fill_at_lane_63_0"]
    assert p["per_grid"] == mp.LANE_P
    a, b = np.flatnonzero(p["cell"] == mp.LANE_A), np.flatnonzero(p["cell"] == mp.LANE_B)
    assert (a[mp.LANE_P - 1], a[mp.LANE_P]) == (63, 64) and (b[mp.LANE_P - 1] // 64, b[mp.LANE_P] // 64) == (1, 1) and b[mp.LANE_P] == b[mp.LANE_P - 1] + 1
    assert 63 in p["keep"] and 64 not in p["keep"] and b[mp.LANE_P - 1] in p["keep"] and b[mp.LANE_P] not in p["keep"]
    assert n["fill_at_lane_63_0"] == 45
    assert n["one_cell"] == P["one_cell"]["per_grid"] == 5
    assert n["four_cells_one_each"] == 4 and P["four_cells_one_each"]["per_grid"] == 1
    assert n["per_grid_zero"] == 0 and P["per_grid_zero"]["per_grid"] == 0 and P["per_grid_zero"]["nMatch"] > 0
    assert [n["size_%d" % M] for M in mp.FILL_SIZES] == [0, 0, 0, 18, 18, 18, 396, 396, 396]
    for (gx, gy, nm, pg) in mp.EXACT_QUOTIENTS:
        p = P["exact_%dx%d_%d" % (gx, gy, nm)]
        assert p["per_grid"] == pg and pg * gx * gy == nm and n[p["tag"]] == nm, p["tag"]             # an inexact quotient would lose one per cell
    assert len(P["exact_3x3_45"]["matches"]) == 150
    assert n["nmatch_500"] == 500


# ---- n_selected sweep, inlier counts ------------------------------------------------------------------------------------------------------------
def test_sweep_selects_exactly_n(orc):
    pairs = mp.sweep_pairs()
    assert all(len(p["d1"]) <= 1400 for p in pairs)
    recs = ol.parallel_map(lambda p: mp.record_of(orc, p, mp.DIST, 3, gx=1, gy=1), pairs)
    assert [r["n_selected"] for r in recs] == list(mp.SWEEP_N)
    assert sum(r["accepted"] for r in recs) >= 6 and sum(1 - r["accepted"] for r in recs) >= 6


@pytest.mark.parametrize("min_inliers,cases", [(30, mp.INLIER_CASES_30), (10, mp.INLIER_CASES_10)])
def test_inlier_cases_give_exactly_k(orc, min_inliers, cases):
    for K, ds in cases.items():
        c = mp.inlier_case(K, ds)
        r = mp.record_of(orc, c, mp.DIST, mp.INLIER_SEED, min_inliers=min_inliers)
        assert r["n_matches"] == mp.INLIER_M and r["n_selected"] == c["N"] == K + mp.INLIER_OUT, (K, r["n_selected"])
        assert np.array_equal(np.sort(r["sel1"]["id"]), np.arange(c["N"]))                            # selection keeps all points of the case, nothing else
        assert r["n_in"] == K and np.array_equal(r["a"]["id"], c["inliers"]), (K, r["n_in"])
        assert r["accepted"] == int(K > min_inliers)
    assert {min_inliers, min_inliers + 1} <= set(cases)


# ---- descriptor content, ratio corners ----------------------------------------------------------------------------------------------------------
def test_content_patterns(orc):
    C = mp.content_patterns()
    for nj in (33, 255, 257):
        d1, d2 = C["all128_%d" % nj]
        idx, b1, b2 = orc.bf_match(d1, d2)
        assert (d2[nj - 1] == 128).all() and (idx[::7] == nj - 1).all() and (b1[::7] == 0).all() and idx[1] == 3
    idx, b1, b2 = orc.bf_match(*C["zeros_vs_255"])
    assert b1.max() == 128 * 255 * 255 and b1.min() == 0 and (idx == 0).all()
    idx, b1, b2 = orc.bf_match(*C["all_rows_equal"])
    assert (idx == 0).all() and (b1 == 0).all() and (b2 == 0).all()
    assert np.array_equal(orc.sort_matches(idx, b1)[:, 0], np.arange(len(idx)))                       # every query ties: the sorted order is the query order
    idx, b1, b2 = orc.bf_match(*C["duplicated_train_rows"])
    assert idx[:3].tolist() == [3, 63, 3] and (b1[:3] == 0).all() and (b2[:3] == 0).all()          # the lowest index of the twins
    idx, b1, b2 = orc.bf_match(*C["duplicate_across_chunks"])
    assert idx[:2].tolist() == [2047, 2047] and b1[0] == 0 and b2[0] == 0 and b1[1] == b2[1] > 0
    idx, b1, b2 = orc.bf_match(*C["one_train_row"])
    assert (idx == 0).all() and (b2 == 0x7fffffff).all()
    assert mp.float_desc_expected(mp.FLOAT_DESC).tolist() == [0, 0, 0, 1, 2, 128, 255, 255, 255, 255]


def test_ratio_pairs(orc):
    R = mp.ratio_pairs()
    for tag in ("duplicated_train_rows", "duplicate_across_chunks"):
        p = R[tag]
        idx, b1, b2 = orc.bf_match(p["d1"], p["d2"])
        q = p["dropped"]
        assert (b1[q] == b2[q]).all() and (b1[q] == 0).any() and (b1[q] > 0).any(), tag
        r0, r = mp.record_of(orc, p, mp.DIST, 5), mp.record_of(orc, p, mp.DIST, 5, ratio=0.8)
        assert not np.isin(q, r["kept"][:, 0]).any() and r["n_kept"] < r["n_matches"], tag         # dropped ...
        assert np.isin(q, r0["sel1"]["id"]).sum() >= 20, tag                                         # ... and selected without the test
        assert r["n_selected"] > 0
    assert (orc.bf_match(R["duplicate_across_chunks"]["d1"], R["duplicate_across_chunks"]["d2"])[0][R["duplicate_across_chunks"]["dropped"]] == 2047).all()
    p = R["one_train_row"]
    r = mp.record_of(orc, p, mp.DIST, 5, ratio=0.8)
    assert r["n_kept"] == r["n_matches"] == 200 and r["n_selected"] > 0                              # second = 0x7fffffff: kept
    assert mp.record_of(orc, R["no_train_row"], mp.DIST, 5, ratio=0.8)["n_selected"] == 0


# ---- the oracle's grid walk against the reference's ---------------------------------------------------------------------------------------------
def check_select_vs_reference(oracle, ref):
    """oracle.select == the reference's SelectMatchPairs on the patterns, without the matches whose cell leaves [0, nGrids) (there the reference
    indexes label[] out of bounds; the oracle clamps: its documented divergence).  Returns (patterns, matches sent, matches held back)"""
    sent = held = 0
    pats = mp.edge_select_patterns(grids=[(3, 3), (1, 1), (5, 5)]) + mp.fill_patterns()
    for p in pats:
        m, ok = mp.inside_only(p)
        a = oracle.select(m, p["kp1"], p["kp2"], p["nMatch"], p["w"], p["h"], p["gx"], p["gy"])
        b = ref.select(m, p["kp1"], p["kp2"], p["nMatch"], p["w"], p["h"], p["gx"], p["gy"])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), p["tag"]
        sent += int(ok.sum()); held += int((~ok).sum())
    return len(pats), sent, held


def test_oracle_select_equals_reference(oracle, ref):
    n, sent, held = check_select_vs_reference(oracle, ref)
    assert n >= 20 and held > 0 and sent > 20 * held
