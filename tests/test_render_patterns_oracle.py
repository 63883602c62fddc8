"""The render edge cases of tests/render_patterns.py on the CPU: every case is what its tag claims (the predicates, on the restatements'
output), the two routes to the per-frame sample maps agree (gain_ref.frame_sample_maps through the oracle, block_gain_ref.sample_maps
through tests/warp_ref.py), and feather_ref, seamline_ref and median_ref are consistent with one another and with the oracle's refined
render.  A case that stops being what its tag claims fails here, not quietly on the GPU (tests/test_gpu_render_edges.py).
"""
import numpy as np
import pytest

from tests import render_patterns as rp
from tests import warp_patterns as wp

CASES = rp.cases()
IDS = [c.tag for c in CASES]


def _pix(canvas, cw):
    return np.ascontiguousarray(canvas[:, :3 * cw]).reshape(canvas.shape[0], cw, 3)


def test_the_case_list_is_what_the_issue_names():
    tags = [c.tag for c in CASES]
    assert len(set(tags)) == len(tags)
    base = wp.refined_cases()
    assert tags[:len(base)] == [c.tag for c in base] and not any(c.new for c in CASES[:len(base)])
    for c, b in zip(CASES, base):                                           # reused, not copied
        assert all(x is y or np.array_equal(x, y) for x, y in zip(c.imgs, b.imgs)) and np.array_equal(c.h9s, b.h9s) and c.hidden == b.hidden
    assert tags[len(base):] == ["canvas_h%d" % H for H in rp.HEIGHTS] + ["straddle_overlap"] and all(c.new for c in CASES[len(base):])
    assert rp.HEIGHTS == (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 256, 257)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_predicate_holds_on_the_restatement(oracle, case):
    r = rp.restate(oracle, case)
    assert case.pred(case, r), (case.tag, case.why)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_block_sample_maps_equal_the_oracles(oracle, case):
    """None (no coordinates) and an all-false cover are the same statement: the frame gives no pixel"""
    r = rp.restate(oracle, case)
    assert len(r.maps) == len(r.block_maps) == len(case.imgs)
    for k, (m, b) in enumerate(zip(r.maps, r.block_maps)):
        if m is None or b is None:
            assert (m is None or not m[1].any()) and (b is None or not b[1].any()), (case.tag, k)
            continue
        assert np.array_equal(m[1], b[1]) and np.array_equal(m[0], b[0]), (case.tag, k)
        assert not m[0][~m[1]].any(), (case.tag, k)                         # no sample outside the cover


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatements_are_mutually_consistent(oracle, case):
    r = rp.restate(oracle, case)
    refined = _pix(r.refined, r.cw)
    assert np.array_equal(r.top >= 0, r.layers > 0)
    assert np.array_equal(refined[r.layers == 0], np.zeros((int((r.layers == 0).sum()), 3), np.uint8))
    for ramp in rp.RAMPS:
        fcan, flayers = r.feather(ramp)
        scan, owner, scount, best, ties = r.seamline(ramp)
        assert np.array_equal(flayers, r.layers) and np.array_equal(scount, r.layers)
        assert np.array_equal(owner > 0, r.layers > 0)
        single = r.layers == 1
        assert np.array_equal(fcan[single], refined[single]) and np.array_equal(scan[single], refined[single])
        assert np.array_equal(owner[single].astype(np.int64) - 1, r.top[single])
        for depth in rp.DEPTHS:
            mcan, spread, mcount, sel, tie = r.median(ramp, depth)
            assert np.array_equal(mcount, r.layers), (ramp, depth)
            assert np.array_equal(mcan[single], refined[single]) and not spread[single].any(), (ramp, depth)
            assert np.array_equal(sel[0], owner), (ramp, depth)             # the deepest selected frame is the seamline owner
            assert np.array_equal((sel > 0).sum(axis=0), np.minimum(r.layers, depth)), (ramp, depth)
            if depth == 1:
                assert np.array_equal(mcan, scan) and not spread.any(), ramp
        assert np.array_equal(r.median(ramp, 0)[0], r.median(ramp, 5)[0])   # depth 0 is the default, 5


def test_the_cases_reach_the_paths_they_are_there_for(oracle):
    """what the summary of the GPU comparisons relies on, asserted: partial pixel groups and partial last tile rows exist for every rows-per-lane
    count, one list is longer than 32, a list-block corner has overlap, skipped frames sit at the ends of a list and one frame has no inverse"""
    tags = rp.by_tag()
    r = {t: rp.restate(oracle, tags[t]) for t in ("forty", "straddle_overlap", "m8_zero_ends", "rank_deficient", "canvas_w1", "canvas_h1")}
    assert int(r["forty"].layers.max()) > 32
    lay = r["straddle_overlap"].layers
    assert (lay[rp.BLK - 1:rp.BLK + 1, rp.BLK - 1:rp.BLK + 1] >= 2).all()
    assert rp.skipped(tags["m8_zero_ends"], r["m8_zero_ends"]) == [0, 3]
    assert rp.skipped(tags["rank_deficient"], r["rank_deficient"]) == [1] and tags["rank_deficient"].h9s[1, 8] == 1
    assert r["canvas_w1"].cw == 1 and r["canvas_h1"].ch == 1
    heights = sorted(rp.restate(oracle, c).ch for c in CASES if c.tag.startswith("canvas_h"))
    widths = sorted(rp.restate(oracle, c).cw for c in CASES if c.tag.startswith("canvas_w"))
    for th in (8, 16, 32, 256):
        assert {th - 1, th, th + 1} <= set(heights)
    assert any(w % 4 for w in widths) and {127, 128, 129, 255, 256, 257} <= set(widths)
