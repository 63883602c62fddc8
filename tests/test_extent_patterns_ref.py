"""The cases of tests/extent_patterns.py hold what they are for, without a GPU: every canvas passes the extent its name gives, its far pair
overlaps there, the records it is compared on are not all zero, and its restatement changes under each mutation of the map step that a
16-bit slip in a kernel would amount to (a wrapped coordinate, a wrapped list-block index, a launch cut at 65 535 workgroup rows).  The frame
cases have no two 256-pixel blocks alike.  The timings of the references are in CHANGELOG.md.
"""
import numpy as np
import pytest

from tests import extent_patterns as ep
from tests import render_patterns as rp

CASES = ep.canvas_cases()
IDS = [c.tag for c in CASES]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for case in CASES:                                                      # the million-row case holds a gigabyte of maps
        rp._RESTATED.pop(case.tag, None)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_predicate_holds_and_no_case_has_only_zero_records(oracle, case):
    r = rp.restate(oracle, case.render)
    assert case.pred(case, r), f"{case.tag}: {case.why}"
    assert (r.cw if case.axis == 1 else r.ch) > case.beyond > 65535, (case.tag, r.cw, r.ch)
    assert int(ep.far_overlap(case, r).sum()) > 20, case.tag
    pairs, rec = ep.records(case, r)
    i = pairs.index(case.far)
    for step in (1, 3):
        n, sa, sb = rec[("gain", step)][0][i]
        assert n > 0 and sa.all() and sb.all(), (case.tag, step)
    st, fs = rec[("sharp", ep.SHARP_STEP)]
    assert all(int(st[i][f]) > 0 for f in ("n", "e_a", "e_b", "s_a", "s_b")) and all(int(fs["n"][k]) > 0 for k in case.far), case.tag
    # no record set is all zero -- the cap on such cases is none
    for key, (pr, fr) in rec.items():
        zero = not fr.any() if key[0] == "gain" else not fr["n"].any()
        zero = zero and (all(n == 0 for n, _, _ in pr) if key[0] == "gain" else not pr["n"].any())
        assert not zero, (case.tag, key)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_changes_under_each_of_the_cases_mutations(oracle, case):
    r = rp.restate(oracle, case.render)
    assert case.mutations and set(case.mutations) <= set(ep.MUTATIONS), case.tag
    for mutate in case.mutations:
        assert not ep.survives(r.maps, mutate), f"{case.tag}: its bytes survive {mutate}"
    # and the mutations it does not name are those that cannot reach it: the other axis, or a row it does not have
    for mutate in set(ep.MUTATIONS) - set(case.mutations):
        cannot = (mutate == "wrap_x" and r.cw <= 65536) or (mutate == "wrap_y" and r.ch <= 65536) or (mutate.startswith("rows_") and r.ch <= 65535 * int(mutate[5:]))
        assert cannot and ep.survives(r.maps, mutate), (case.tag, mutate)


def test_every_mutation_is_seen_and_every_threshold_has_a_case():
    seen = set().union(*(c.mutations for c in CASES))
    assert seen == set(ep.MUTATIONS), sorted(set(ep.MUTATIONS) - seen)
    assert ep.MUTATIONS[3:] == tuple("rows_%d" % k for k in ep.ROWS_PER_WORKGROUP) and ep.ROWS_PER_WORKGROUP == (1, 4, 16)
    assert {c.tag for c in CASES} == {"wide_69k", "tall_69k", "wide_turned_far", "tall_turned_far", "ribbon_x", "ribbon_y", "far_many", "tall_262k", "tall_1m"}


def test_mutations_do_what_they_say_on_a_map_made_by_hand():
    """a 3 x 65 560 cover with one pixel on each side of 65 536 and a 65 560-row one: each mutation moves or drops exactly what it names"""
    samp = np.zeros((3, 65560, 3), np.int64)
    cover = np.zeros((3, 65560), bool)
    cover[1, 5], cover[1, 65550] = True, True
    samp[1, 5], samp[1, 65550] = 7, 9
    (s, c), = ep.mutated([(samp, cover)], "wrap_x")
    assert c[1, 5] and not c[1, 65550] and c[1, 65536 + 5] and (s[1, 65536 + 5] == 7).all() and int(c.sum()) == 2
    (s, c), = ep.mutated([(samp, cover)], "wrap_block")                     # block 256 reads block 0's list: the frame's box holds every block, nothing changes
    assert np.array_equal(c, cover) and np.array_equal(s, samp)
    far = np.zeros_like(cover)
    far[1, 65550] = True
    (s, c), = ep.mutated([(samp * far[..., None], far)], "wrap_block")      # a frame listed in block 256 alone is not in block 0's list
    assert not c.any() and not s.any()
    tall = (np.ascontiguousarray(samp.transpose(1, 0, 2)), np.ascontiguousarray(cover.T))
    (s, c), = ep.mutated([tall], "wrap_y")
    assert c[5, 1] and not c[65550, 1] and c[65536 + 5, 1] and int(c.sum()) == 2
    (s, c), = ep.mutated([tall], "rows_1")
    assert c[5, 1] and not c[65535:].any() and not s[65535:].any() and int(c.sum()) == 1
    for mutate in ("rows_4", "rows_16", "wrap_x"):
        assert ep.survives([tall], mutate), mutate
    assert list(ep.mutated([None], "wrap_x")) == [None]


@pytest.mark.parametrize("w,h", ep.FRAME_SIZES)
def test_frame_cases_have_no_two_blocks_alike(w, h):
    assert max(w, h) in (65537, 1 << 20) and min(w, h) in (2, 3)
    img = ep.frame(w, h, 5)
    assert img.shape == (h, w, 3) and ep.blocks_differ(img)
    rep = np.tile(ep.frame(256, h, 5), (1, 4, 1)) if w > h else np.tile(ep.frame(w, 256, 5), (4, 1, 1))
    assert not ep.blocks_differ(rep)                                        # the check sees a repeating pattern
    for pad in ep.FRAME_PADS:
        buf, pitch = ep.padded(img, pad)
        assert pitch == 3 * w + pad and buf.shape == (h, pitch) and np.array_equal(buf[:, :3 * w].reshape(h, w, 3), img) and (buf[:, 3 * w:] == 0xEE).all()
