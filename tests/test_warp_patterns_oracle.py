"""The warp stage at its edges, on the CPU: every case of tests/warp_patterns.py is what it claims to be (its predicate holds on the oracle's
output), the oracle (oracle/oracle_warp.c) equals the numpy restatement (tests/warp_ref.py) byte for byte -- quad coordinates bit for bit --
and the oracle equals the reference's own code (the `ref` fixture: oracle/_ref, or its recorded outputs) wherever that code is defined.
The GPU side is tests/test_gpu_warp_edges.py.

Where the reference's code is NOT defined, and a case is left out of the third comparison:
  * a frame that takes part (m8 != 0, kept) has a homography without an inverse: the reference goes on with an uninitialised inverse;
  * a source coordinate inside a frame's box is NaN (0 / 0): the refined render and the chip loop of the reference index with int(NaN).
    (The single warp tests `0 <= x && x < w - 1` positively and rejects a NaN: it stays defined.)
Chip pixels without a sample are uninitialised memory in the reference; its harness and the oracle hand out zeros there, so no case is left
out for them.  At most a quarter of the cases may be left out (asserted below).
"""
import numpy as np
import pytest

from tests import warp_patterns as wp
from tests import warp_ref as wr
from tests.golden_util import bits
from tests.test_overlap import _same

SINGLE = wp.single_cases()
REFINED = wp.refined_cases()
CHIPS = wp.chips_cases()


def _ids(cases):
    return [c.tag for c in cases]


def test_case_tags_are_unique():
    for cases in (SINGLE, REFINED, CHIPS):
        assert len(set(_ids(cases))) == len(cases)


def test_every_content_and_size_is_used():
    tags = " ".join(_ids(SINGLE))
    assert all(name in tags for name, _ in wp.CONTENT) and all("_%dx%d_" % s in tags for s in wp.SIZES)


def test_numpy_inverse_has_the_oracles_bits(oracle):
    """tests/warp_ref.py inverts on its own; on every matrix of every case, at both thresholds in use, it gives what the oracle's
    orc_inverse_matrix gives (bit for bit, and the same refusals)"""
    hs = [c.h9 for c in SINGLE] + [m for c in REFINED for m in c.h9s] + [m for c in CHIPS for m in c.h9s]
    refused = 0
    for h9 in hs:
        for eps in (1e-6, 1e-12):
            rc, inv = oracle.inverse_matrix(np.asarray(h9, np.float32).reshape(3, 3), eps)
            mine = wr.inverse(h9, eps)
            assert (rc == 1) == (mine is not None), (h9, eps)
            refused += rc != 1
            if rc == 1:
                assert np.array_equal(bits(inv.reshape(9)), bits(mine)), (h9, eps)
    assert refused >= 2          # the rank-2 homography, at both thresholds


# ---- single warp ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SINGLE, ids=_ids(SINGLE))
def test_single_case(oracle, case):
    for img in (case.img, wp.grey(case.img)):
        o = wp.single_out(oracle, case, img)
        assert o["rc"] == 0 and o["inv"] is not None, case.tag
        if img.ndim == 3:
            assert case.pred(case, o), (case.tag, case.why, o["dw"], o["dh"])
        (buf, dw, dh, dws), _ = wr.image_projection_transform(img, case.h9, o["inv"])
        assert (dw, dh, dws) == (o["dw"], o["dh"], o["dws"]), case.tag
        assert np.array_equal(buf, o["buf"]), f"{case.tag} ({img.ndim} dims): {int((buf != o['buf']).sum())} bytes differ"


# ---- refined render -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", REFINED, ids=_ids(REFINED))
def test_refined_case(oracle, case):
    o = wp.refined_out(oracle, case)
    assert case.pred(case, o), (case.tag, case.why, o["cw"], o["ch"])
    buf, cw, ch, cws = o["numpy"]
    assert (cw, ch, cws) == (o["cw"], o["ch"], o["cws"]), case.tag
    assert np.array_equal(buf, o["canvas"]), f"{case.tag}: {int((buf != o['canvas']).sum())} bytes differ"
    if case.hidden is not None:
        assert wp._wins(o, case.hidden) == 0


# ---- chips and masks ------------------------------------------------------------------------------------------------------------------------
def _chip_invs(oracle, case):
    return [wp.inverse_of(oracle, m, 1e-12) for m in case.h9s]


@pytest.mark.parametrize("case", CHIPS, ids=_ids(CHIPS))
def test_chips_case(oracle, case):
    r = wp.chips_out(oracle, case)
    assert case.pred(case, r, lambda keep: wp.chips_out(oracle, case, keep=keep)), (case.tag, case.why, wp.owned(r), wp.valid_counts(r), wp.rects(r))
    invs = _chip_invs(oracle, case)
    for fm in (True, False):
        a = r if fm else wp.chips_out(oracle, case, find_masks=False)
        n = wr.chips_and_masks(case.imgs, case.h9s, invs, keep=case.keep, find_masks=fm)
        assert (n["cw"], n["ch"]) == (a["cw"], a["ch"]) and len(n["chips"]) == len(a["chips"]), case.tag
        assert np.array_equal(bits(n["dG"]), bits(a["dG"]))
        for k, (x, y) in enumerate(zip(n["chips"], a["chips"])):
            assert all(int(x[f]) == int(y[f]) for f in ("x0", "y0", "w", "h", "img")), (case.tag, k)
            assert np.array_equal(bits(x["quad"]), bits(y["quad"])) and bits(x["sx"]) == bits(y["sx"]) and bits(x["sy"]) == bits(y["sy"]), (case.tag, k, "quad bits")
            assert np.array_equal(n["chip_imgs"][k], a["chip_imgs"][k]), (case.tag, k, "chip pixels")
            assert np.array_equal(n["valid"][k], a["valid"][k]), (case.tag, k, "validity")
            assert np.array_equal(n["masks"][k], a["masks"][k]), (case.tag, fm, k, "ownership")
    # a canvas pixel has at most one owner
    cover = np.zeros((r["ch"], r["cw"]), np.int32)
    for (x0, y0, w, h), m in zip(wp.rects(r), r["masks"]):
        cover[y0:y0 + h, x0:x0 + w] += m[:, :w] != 0
    assert cover.max() <= 1


# ---- the reference's own code ---------------------------------------------------------------------------------------------------------------
def single_defined(oracle, case):
    return wp.inverse_of(oracle, case.h9, 1e-6) is not None


def refined_defined(oracle, case):
    o = wp.refined_out(oracle, case)
    return not o["nan_seen"] and all(inv is not None for m, inv in zip(case.h9s, o["invs"]) if m[8] != 0)


def chips_defined(oracle, case):
    invs = _chip_invs(oracle, case)
    live = [k for k in range(len(case.imgs)) if (case.keep is None or case.keep[k]) and case.h9s[k, 8] != 0]
    if any(invs[k] is None for k in live):
        return False
    return not wr.chips_and_masks(case.imgs, case.h9s, invs, keep=case.keep, find_masks=False)["nan_seen"]


def check_single_vs_reference(oracle, ref):
    left_out = 0
    for case in SINGLE:
        if not single_defined(oracle, case):
            left_out += 1
            continue
        for img in (case.img, wp.grey(case.img)):
            r1, a = oracle.image_projection_transform(img, case.h9)
            r2, b = ref.image_projection_transform(img, case.h9)
            assert r1 == r2 == 0 and tuple(a[1:]) == tuple(b[1:]) and np.array_equal(a[0], b[0]), case.tag
    return left_out


def check_refined_vs_reference(oracle, ref):
    left_out = 0
    for case in REFINED:
        if not refined_defined(oracle, case):
            left_out += 1
            continue
        r1, a = oracle.mosaic_images_refined(case.imgs, case.h9s)
        r2, b = ref.mosaic_images_refined(case.imgs, case.h9s)
        assert r1 == r2 == 0 and tuple(a[1:]) == tuple(b[1:]) and np.array_equal(a[0], b[0]), case.tag
    return left_out


def check_chips_vs_reference(oracle, ref):
    left_out = 0
    for case in CHIPS:
        if not chips_defined(oracle, case):
            left_out += 1
            continue
        keep = np.ones(len(case.imgs), np.uint8) if case.keep is None else case.keep
        for fm in (True, False):
            a = oracle.chips_and_masks(case.imgs, case.h9s, keep=keep, find_masks=fm)
            b = ref.chips_and_masks(case.imgs, case.h9s, keep=keep, find_masks=fm)
            _same(a, b, f"{case.tag} find_masks={fm}")
    return left_out


def check_all_vs_reference(oracle, ref):
    return (check_single_vs_reference(oracle, ref), check_refined_vs_reference(oracle, ref), check_chips_vs_reference(oracle, ref))


def test_oracle_equals_reference_single(oracle, ref):
    assert 4 * check_single_vs_reference(oracle, ref) <= len(SINGLE)


def test_oracle_equals_reference_refined(oracle, ref):
    assert 4 * check_refined_vs_reference(oracle, ref) <= len(REFINED)


def test_oracle_equals_reference_chips(oracle, ref):
    assert 4 * check_chips_vs_reference(oracle, ref) <= len(CHIPS)


def test_horizon_stays_in_the_reference_comparison(oracle):
    """no destination pixel of the horizon cases gives 0 / 0 (computed in numpy from the inverse): they are compared with the reference"""
    for tag in ("horizon", "near_horizon"):
        case = next(c for c in SINGLE if c.tag == tag)
        o = wp.single_out(oracle, case, case.img)
        _, (xs, ys, ok, xf, yf) = wr.image_projection_transform(case.img, case.h9, o["inv"])
        assert not np.isnan(xs).any() and not np.isnan(ys).any() and single_defined(oracle, case)
    assert [c.tag for c in REFINED if not refined_defined(oracle, c)] == ["rank_deficient"]
    assert all(chips_defined(oracle, c) for c in CHIPS)


# ---- the cases discriminate -----------------------------------------------------------------------------------------------------------------
def test_first_wins_and_last_wins_differ_on_the_twins(oracle):
    """ownership: the first of two equal chips; refined render: the last of two equal frames -- the opposite rule changes the output"""
    case = next(c for c in REFINED if c.tag == "twins")
    o = wp.refined_out(oracle, case)
    swapped = wp.refined_out(oracle, case._replace(imgs=[case.imgs[0], case.imgs[2], case.imgs[1]]))
    assert not np.array_equal(o["canvas"], swapped["canvas"])
    case = next(c for c in CHIPS if c.tag == "duplicates")
    r = wp.chips_out(oracle, case)
    # `>=` instead of `>`: the later twin owns what the earlier one owned, and the masks are not the oracle's
    wrong, _ = wr.ownership(r["valid"], r["chips"], r["cw"], r["ch"], strict=False)
    right, _ = wr.ownership(r["valid"], r["chips"], r["cw"], r["ch"])
    assert all(np.array_equal(a, b) for a, b in zip(right, r["masks"]))
    assert not np.array_equal(wrong[0], r["masks"][0]) and not np.array_equal(wrong[1], r["masks"][1])
    assert not wrong[0].any() and wrong[1].any() and r["masks"][0].any() and not r["masks"][1].any()
