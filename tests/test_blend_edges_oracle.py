"""Multiband blend at its edges, on the CPU: every case of tests/blend_edges.py is what it claims to be (its predicate holds), the oracle
(oracle/oracle_blend.c) equals the numpy restatement of its own header (tests/blend_ref.py) byte for byte on all of them, and the cases
discriminate (chip order, 16-bit wrap-around).  The GPU side is tests/test_gpu_blend_edges.py.

Not covered: more than 16 levels (MAX_BANDS) -- that needs a canvas side above 65 536, padded to 131 072 on both sides; not testable in memory.
"""
import numpy as np
import pytest

from tests import blend_edges as be
from tests import blend_ref as br

DIRECT = be.direct_cases()
SURVEY = be.survey_cases()


def _ids(cases):
    return [c.tag for c in cases]


def _by_tag(tag):
    return next(c for c in DIRECT if c.tag == tag)


def _rects(chips):
    return [(int(c["x0"]), int(c["y0"]), int(c["w"]), int(c["h"])) for c in chips]


def test_case_tags_are_unique():
    assert len(set(_ids(DIRECT))) == len(DIRECT) and len(set(_ids(SURVEY))) == len(SURVEY)


@pytest.mark.parametrize("case", DIRECT, ids=_ids(DIRECT))
def test_direct_case_is_what_it_claims(case):
    assert case.pred(case), case.why
    for (x0, y0, w, h), chip, mask in zip(*be.nonempty(case)):
        assert 0 <= x0 and 0 <= y0 and x0 + w <= case.W and y0 + h <= case.H
        assert chip.shape == (h, (3 * w + 3) & ~3) and mask.shape == (h, (w + 3) & ~3)
    # the region is never pulled back (see tests/blend_edges.py): a geometry change that makes dx, dy live must be noticed
    assert all(g["dx"] == 0 and g["dy"] == 0 for g in be.regions(case.rects, case.W, case.H, case.band))


@pytest.mark.parametrize("case", DIRECT, ids=_ids(DIRECT))
def test_oracle_equals_numpy_direct(oracle, case):
    rects, chips, masks = be.nonempty(case)
    ref, nb_ref = br.multiband_blend(rects, chips, masks, case.W, case.H, case.band)
    got, nb = oracle.multiband_blend(be.info_array(rects), chips, masks, case.W, case.H, band=case.band)
    assert nb == nb_ref == be.bands(case.W, case.H, case.band)
    assert got.shape == ref.shape and np.array_equal(got, ref), f"{case.tag}: {int((got != ref).sum())} bytes differ"


@pytest.mark.parametrize("case", SURVEY, ids=_ids(SURVEY))
def test_oracle_equals_numpy_survey(oracle, case):
    for find_masks in (True, False):
        r = oracle.chips_and_masks(case.imgs, case.h9s, keep=case.keep, find_masks=find_masks)
        rects = _rects(r["chips"])
        if find_masks:
            geo = dict(rects=rects, W=r["cw"], H=r["ch"], owned=[int((m != 0).sum()) for m in r["masks"]])
            assert case.pred(geo), (case.why, geo)
        for band in be.survey_bands(case):
            ref, nb_ref = br.multiband_blend(rects, r["chip_imgs"], r["masks"], r["cw"], r["ch"], band)
            got, nb = oracle.multiband_blend(r["chips"], r["chip_imgs"], r["masks"], r["cw"], r["ch"], band=band)
            assert nb == nb_ref
            assert np.array_equal(got, ref), f"{case.tag} find_masks={find_masks} band {band}: {int((got != ref).sum())} bytes differ"


def test_chip_order_is_part_of_the_result(oracle):
    """the canvas weight is a float sum in chip order: the same chips in another order give other bytes (a few: the sums differ in their
    last bit and that has to move a truncation)"""
    for tag in ("grey_masks", "grey_masks_extremes"):
        a, b = _by_tag(tag), _by_tag(tag + "_permuted")
        assert sorted(a.rects) == sorted(b.rects) and a.rects != b.rects
    a, b = _by_tag("grey_masks"), _by_tag("grey_masks_permuted")
    outs = [oracle.multiband_blend(be.info_array(c.rects), c.chips, c.masks, c.W, c.H, band=c.band)[0] for c in (a, b)]
    assert not np.array_equal(outs[0], outs[1])


def test_wrap_is_16_bit(oracle):
    """150 white chips: the top level's sum wraps (150 * 255 = 38 250 -> -27 286) and the mosaic is black; an accumulator wider than 16 bits
    gives a white one.  128 chips stay inside int16 (32 640), 129 do not (32 895)."""
    outs, left = {}, {}
    for n in (150, 129, 128):
        c = _by_tag("wrap_%d" % n)
        st = {}
        ref, _ = br.multiband_blend(c.rects, c.chips, c.masks, c.W, c.H, c.band, stats=st)
        outs[n], left[n] = oracle.multiband_blend(be.info_array(c.rects), c.chips, c.masks, c.W, c.H, band=c.band)[0], st["left_int16"]
        assert np.array_equal(outs[n], ref)
    assert left == {150: True, 129: True, 128: False}
    c = _by_tag("wrap_150")
    wide, _ = br.multiband_blend(c.rects, c.chips, c.masks, c.W, c.H, c.band, wide_accumulator=True)
    assert not np.array_equal(wide, outs[150])
    assert not outs[150].any() and not outs[129].any()
    assert (outs[128][:, :3 * c.W] >= 254).all() and np.array_equal(wide, outs[128])
    # without a wrap the wide accumulator is the definition
    c = _by_tag("wrap_128")
    wide128, _ = br.multiband_blend(c.rects, c.chips, c.masks, c.W, c.H, c.band, wide_accumulator=True)
    assert np.array_equal(wide128, outs[128])


def test_zero_size_entries_are_not_passed_on():
    c = _by_tag("zero_size")
    rects, chips, masks = be.nonempty(c)
    assert len(rects) == 2 and all(w > 0 and h > 0 for (_, _, w, h) in rects) and len(c.rects) == 4
