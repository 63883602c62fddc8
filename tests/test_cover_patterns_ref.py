"""The cover-depth cases of tests/cover_patterns.py on the CPU: every case is what its tag claims (the predicates, on the restatement's output),
the two identities of the header hold on every case, the numpy geometry equals the oracle's cover, the round rule equals the sequential
greedy on random layouts, and each plausible wrong reading of the definition (the mutations of tests/cover_ref.py) changes at least one case.
A case that stops being what its tag claims fails here, not quietly on the GPU (tests/test_gpu_cover.py).
"""
import numpy as np
import pytest

from tests import cover_patterns as cp
from tests import cover_ref as cr
from tests import gain_ref as gr
from tests import render_patterns as rp

CASES = cp.stats_cases()
IDS = [c.tag for c in CASES]
SELECTS = cp.select_cases()


def test_the_case_list_is_what_the_issue_names():
    tags = [c.tag for c in CASES]
    assert len(set(tags)) == len(tags)
    base = rp.by_tag()
    assert set(base) <= set(tags)
    for c in CASES:
        if c.tag in base:                                                   # reused, not copied
            assert c.render is base[c.tag] or (all(np.array_equal(x, y) for x, y in zip(c.render.imgs, base[c.tag].imgs)) and np.array_equal(c.h9s, base[c.tag].h9s))
    for t in ("forty", "twins", "straddle_overlap", "canvas_h1", "canvas_h257", "wide_69k", "stack_789", "list65", "list257", "list600", "horizon_inside", "edge_255_256"):
        assert t in tags, t
    assert cp.by_tag()["wide_69k"].steps == (64,)
    assert set(cp.by_tag()["edge_255_256"].steps) == {1, 3, 7, 8, 37, 64}
    assert [s.tag for s in SELECTS] == ["strip5_waits", "waiting_blocks", "two_clusters", "crit_at_max_loss", "fails_both", "leaf_frees_cut_vertex", "block3x3_depth2", "order_null",
                                        "not_examined"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_predicate_and_identities_hold_on_the_restatement(oracle, case):
    r = cp.restate(oracle, case)
    assert case.pred(case, r), (case.tag, case.why)
    n = len(case.sizes)
    for step in case.steps:
        points = ((r.cw - 1) // step + 1) * ((r.ch - 1) // step + 1)
        for keep in cp.KEEPS:
            fs, hist = r.stats(step, keep)
            at = fs["at_depth"]
            assert int(hist.sum()) == points, (case.tag, step, keep)
            for d in range(1, 8):                                           # a point d deep is credited to d frames
                assert int(at[:, d - 1].sum()) == d * int(hist[d]), (case.tag, step, keep, d)
            assert int(at[:, 7].sum()) >= 8 * int(hist[8])
            mask = cp.keep_mask(keep, n)
            for k in range(n):
                if r.covers[k] is None or (mask is not None and not mask[k]):
                    assert not at[k].any(), (case.tag, k)
        assert r.stats(step, "ones")[0].tobytes() == r.stats(step)[0].tobytes() and np.array_equal(r.stats(step, "ones")[1], r.stats(step)[1])
        assert int(r.stats(step, "zeros")[1][0]) == points and not r.stats(step, "zeros")[0]["at_depth"].any()
        if r.maps is not None:                                              # every taking-part frame kept: the gain stage's frame cover
            cover = gr.stats_ref(r.maps, [], step)[1]
            assert np.array_equal(r.stats(step)[0]["at_depth"].sum(axis=1), cover), (case.tag, step)


@pytest.mark.parametrize("case", [c for c in CASES if c.render is not None], ids=[c.tag for c in CASES if c.render is not None])
def test_numpy_geometry_is_the_oracles_cover(oracle, case):
    """the cover of the added cases and the boxes of every case come from cover_ref.geometry: on the reused cases it is the oracle's cover,
    frame for frame, and every cover lies in its box"""
    r = cp.restate(oracle, case)
    covers, boxes, (cw, ch) = cr.geometry(case.sizes, case.h9s)
    assert (cw, ch) == (r.cw, r.ch)
    for k, (mine, theirs) in enumerate(zip(covers, r.covers)):
        if theirs is None or mine is None:                                  # no inverse: the oracle gives an empty cover
            assert (mine is None or not mine.any()) and (theirs is None or not theirs.any()), (case.tag, k)
            continue
        assert np.array_equal(mine, theirs), (case.tag, k)
        ys, xs = np.nonzero(mine)
        if len(ys):
            x0, x1, y0, y1 = boxes[k]
            assert x0 <= xs.min() and xs.max() <= x1 and y0 <= ys.min() and ys.max() <= y1


# ---- selection ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SELECTS, ids=[s.tag for s in SELECTS])
def test_selection_layout_is_what_its_tag_claims(case):
    res = cp.reference(case)
    assert case.pred(case, res), (case.tag, case.why, res)
    assert res.rounds <= max(1, len(case.order) if case.order is not None else len(case.sizes))
    if case.pairs is None:
        st, ko, lost = cp.sequential(case)
        assert np.array_equal(st, res.status) and np.array_equal(ko, res.keep_out) and lost == res.lost


def _connected(n, pairs, alive):
    adj = cr._adjacency(n, pairs, alive)
    left = [k for k in range(n) if alive[k]]
    comps = []
    seen = set()
    for k in left:
        if k not in seen:
            c = cr._reach(adj, alive, k, None)
            seen |= c
            comps.append(c)
    return comps


def test_round_rule_equals_the_sequential_greedy_on_random_layouts():
    dropped = waited = 0
    for seed in cp.RANDOM_SEEDS:
        case = cp.random_layout(seed)
        res = cp.reference(case)
        st, ko, lost = cp.sequential(case)
        assert np.array_equal(st, res.status) and np.array_equal(ko, res.keep_out) and lost == res.lost, (seed, res, st)
        dropped += int((res.status == cr.DROPPED).sum())
        waited += res.rounds > 1
    assert dropped >= len(cp.RANDOM_SEEDS) // 2 and waited >= len(cp.RANDOM_SEEDS) // 10, (dropped, waited)   # the layouts do drop frames, and a tenth at least make candidates wait


def test_with_pairs_every_drop_keeps_the_graph_connected():
    cut = 0
    for seed in cp.RANDOM_SEEDS:
        case = cp.random_layout(seed, with_pairs=True)
        res = cp.reference(case)
        n = len(case.sizes)
        _, boxes, _ = cp.geometry_of(case)
        entry = [boxes[k] is not None and (case.keep is None or bool(case.keep[k])) for k in range(n)]
        before = _connected(n, case.pairs, entry)
        after = _connected(n, case.pairs, [bool(v) for v in res.keep_out])
        # every component on entry is, without its dropped frames, still one component (or empty)
        for c in before:
            left = {k for k in c if res.keep_out[k]}
            assert not left or left in after, (seed, c, after)
        cut += int((res.status == cr.CUT_VERTEX).sum())
    assert cut > 10, cut


# ---- mutations: each must change at least one case -------------------------------------------------------------------------------------------
def test_mutation_strictly_below_min_depth_shows():
    changed = [c.tag for c in SELECTS if not _same(cp.reference(c, inclusive=False), cp.reference(c))]
    assert "crit_at_max_loss" in changed and "block3x3_depth2" in changed, changed


def _same(a, b):
    return np.array_equal(a.status, b.status) and np.array_equal(a.keep_out, b.keep_out) and a.rounds == b.rounds and a.lost == b.lost


def test_mutation_blocked_boxes_without_the_waiting_candidates_shows():
    changed = [c.tag for c in SELECTS if not _same(cp.reference(c, block_waiting=False), cp.reference(c))]
    assert "order_null" in changed and "waiting_blocks" in changed, changed
    w = next(c for c in SELECTS if c.tag == "waiting_blocks")
    assert tuple(cp.reference(w, block_waiting=False).status) == (0, 1, 2, 1, 0)


def test_mutation_saturation_at_seven_shows(oracle):
    changed = []
    for c in CASES:
        r = cp.restate(oracle, c)
        fs, hist = cr.stats_ref(r.covers, None, c.steps[0], r.shape, saturate=7)
        if fs.tobytes() != r.stats(c.steps[0])[0].tobytes() or not np.array_equal(hist, r.stats(c.steps[0])[1]):
            changed.append(c.tag)
    assert {"forty", "stack_789", "list65", "list257", "list600"} <= set(changed), changed


def test_mutation_cover_without_the_box_test_shows(oracle):
    changed = []
    for c in CASES:
        if c.tag in ("wide_69k", "sparse"):                                 # large canvases, translations only: nothing to see
            continue
        loose = cr.geometry(c.sizes, c.h9s, box_test=False)[0]
        tight = cr.geometry(c.sizes, c.h9s)[0]
        if any(a is not None and not np.array_equal(a, b) for a, b in zip(loose, tight)):
            changed.append(c.tag)
    assert "horizon_inside" in changed, changed
