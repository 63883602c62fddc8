"""The sharpness cases of tests/sharp_patterns.py on the CPU: every case is what its tag claims (the predicates, on the restatement's output),
the five-point rule is exercised, all-zero cases stay a minority, and each plausible wrong reading of the definition (the mutations of
tests/sharp_ref.py) changes at least one case's records.  A case that stops being what its tag claims fails here, not quietly on the GPU
(tests/test_gpu_sharp.py).
"""
import numpy as np
import pytest

from tests import sharp_patterns as sp
from tests import sharp_ref as sr

CASES = sp.stats_cases()
IDS = [c.tag for c in CASES]
GRAPHS = sp.graph_cases()


def test_the_case_list_is_what_the_issue_names():
    tags = [c.tag for c in CASES]
    assert len(set(tags)) == len(tags)
    from tests import render_patterns as rp
    base = rp.by_tag()
    for c in CASES:
        if c.kind == "reused" and c.tag in base:                            # reused, not copied
            assert c.render is not None and all(x is y or np.array_equal(x, y) for x, y in zip(c.render.imgs, base[c.tag].imgs)) and np.array_equal(c.render.h9s, base[c.tag].h9s)
    for t in ("canvas_h1", "canvas_h2", "canvas_h3", "sharp_h8", "sharp_h9", "sharp_h17", "sharp_h257", "straddle_overlap", "twins", "m8_zero_ends", "rank_deficient",
              "sharp_overlap3", "sharp_overlap2", "sharp_row0", "sharp_east_edge", "sharp_flat", "sharp_checker1020", "sharp_steps", "sharp_pitch", "sharp_seventy"):
        assert t in tags, t
    assert {s for c in CASES for s in c.steps} >= {1, 3, 8, 64}
    assert [g.tag for g in GRAPHS] == ["chain5_middle", "grid3x3_centre", "ring6_opposite", "ring6_neighbours", "ring6_tie", "component_of_one", "unusable_only"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_predicate_holds_on_the_restatement(oracle, case):
    r = sp.restate(oracle, case)
    assert case.pred(case, r), (case.tag, case.why)
    for step in case.steps:                                                 # what every case must satisfy
        st, fs = r.stats(step)
        cov = r.covered(step)
        assert all(0 <= int(s["n"]) <= c for s, c in zip(st, cov)), case.tag
        assert all(int(s["e_a"]) <= int(s["n"]) * sp.L_MAX2 and int(s["s_a"]) <= 255 * int(s["n"]) for s in st), case.tag
        for (a, b), s in zip(r.pairs, st):                                  # a pair's points are points of both frames
            assert int(s["n"]) <= min(int(fs["n"][a]), int(fs["n"][b])), (case.tag, a, b)


def test_the_five_point_rule_is_exercised(oracle):
    """at least one reused case and every edge case (but the two whose point is that nothing is left) has a pair with 0 < n < the lattice
    points both frames cover"""
    def cut(c):
        r = sp.restate(oracle, c)
        return any(0 < int(n) < cv for s in c.steps for n, cv in zip(r.stats(s)[0]["n"], r.covered(s)))
    assert any(cut(c) for c in CASES if c.kind == "reused")
    for c in CASES:
        if c.kind == "edge" and c.tag not in ("sharp_overlap2", "sharp_row0"):
            assert cut(c), c.tag
    for c in CASES:
        if c.tag in ("sharp_overlap2", "sharp_row0"):                       # they cover common lattice points and keep none
            r = sp.restate(oracle, c)
            assert any(cv > 0 for cv in r.covered(c.steps[0])) and not r.stats(c.steps[0])[0]["n"].any(), c.tag


def test_all_zero_cases_are_at_most_a_quarter(oracle):
    zero = [c.tag for c in CASES if all(not sp.restate(oracle, c).stats(s)[0]["n"].any() for s in c.steps)]
    assert 4 * len(zero) <= len(CASES), (len(zero), len(CASES), zero)
    assert {"canvas_h1", "canvas_h2", "canvas_h3", "sharp_overlap2", "sharp_row0"} <= set(zero)


# ---- mutations: each must change at least one case's records ---------------------------------------------------------------------------------
def _stats_differ(oracle, **mut):
    changed = []
    for c in CASES:
        r = sp.restate(oracle, c)
        lm = sr.lap_maps(r.maps, **mut)
        for s in c.steps:
            st, fs = sr.stats_ref(lm, r.pairs, s)
            if st.tobytes() != r.stats(s)[0].tobytes() or fs.tobytes() != r.stats(s)[1].tobytes():
                changed.append(c.tag)
                break
    return changed


def test_mutation_centre_only_cover_shows(oracle):
    changed = _stats_differ(oracle, centre_only=True)
    assert {"sharp_overlap3", "sharp_east_edge", "sharp_west_edge_turned"} <= set(changed), changed


def test_mutation_without_the_border_rule_shows(oracle):
    changed = _stats_differ(oracle, border_rule=False)
    assert "sharp_row0" in changed, changed


def _host(g, **mut):
    l = sr.solve_ref(g.records, g.n, normalise=mut.get("normalise", True))
    rel = sr.rel_ref(l, g.records, g.n, lower_median=mut.get("lower_median", True))
    return l, rel, sr.select_ref(rel, g.records, g.n, g.blur_ratio)[0]


def test_mutation_without_brightness_normalisation_shows(oracle):
    """on the stats cases' own records: a pair of differently exposed frames"""
    changed = []
    for c in CASES:
        st = sp.restate(oracle, c).stats(c.steps[0])[0]
        if sr.usable(st).any() and not np.allclose(sr.solve_ref(st, len(c.render.imgs)), sr.solve_ref(st, len(c.render.imgs), normalise=False), atol=1e-6):
            changed.append(c.tag)
    assert changed


def test_mutation_without_the_lower_median_shows():
    changed = [g.tag for g in GRAPHS if not np.array_equal(_host(g)[2], _host(g, lower_median=False)[2])]
    assert "ring6_neighbours" in changed or "chain5_middle" in changed, changed
    assert any(not np.allclose(_host(g)[1], _host(g, lower_median=False)[1]) for g in GRAPHS)


# ---- the graph cases are what their tags claim ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GRAPHS, ids=[g.tag for g in GRAPHS])
def test_graph_case_status_is_the_hand_worked_one(g):
    l, rel, status = _host(g)
    assert tuple(int(s) for s in status) == g.status, (g.tag, rel.tolist())
    if g.tag == "ring6_tie":
        assert abs(rel[1] - rel[4]) < 1e-12
    else:
        assert sr.min_margin(rel, g.records, g.n, g.blur_ratio) > 1e-3, g.tag   # no decision hangs on the solve's last digits
    if g.tag == "unusable_only":
        assert not sr.usable(g.records).any() and (sr.sharp_ref(l, g.records, g.n) == 1.0).all()
    if g.tag == "ring6_opposite":                                           # the order decides: by index it would be the other one
        assert rel[4] < rel[1] < np.log(g.blur_ratio)
    if g.tag == "chain5_middle":                                            # a lone blurred frame comes out near d / (1 + prior)
        assert abs((l[2] - l[1]) - np.log(0.5)) < 0.02
