"""The warp stage at its edges, on the GPU: csrc/warp.hip (ImageProjectionTransform, the one-launch MosaicImagesRefined canvas and its stripe
cover, the chip warps, distmax_kernel / owner_kernel / mask_bbox_kernel) against the oracle on the cases of tests/warp_patterns.py --
quarter turns, mirrors, m8 = 2 and -1, horizons, 0 / 255 content, twins, 70 chips on one block, chips without a valid pixel.  Every
comparison is np.array_equal on the output bytes (quad coordinates: on their bits); there are no tolerances and nothing is filtered at run
time.  (tests/test_warp_patterns_oracle.py checks the oracle itself against a numpy restatement and against the reference's own code.)
"""
import numpy as np
import pytest

from tests import warp_patterns as wp
from tests import warp_ref as wr
from tests.golden_util import bits

pytestmark = pytest.mark.gpu

SINGLE = wp.single_cases()
REFINED = wp.refined_cases()
CHIPS = wp.chips_cases()
SENTINEL = 0xA5


def _ids(cases):
    return [c.tag for c in cases]


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


def _src(h9, x, y):
    """source coordinate of destination point (x, y) under h9, in double precision: for the failure reports only"""
    try:
        v = np.linalg.inv(np.asarray(h9, np.float64).reshape(3, 3)) @ np.array([x, y, 1.0])
        return "(%.4f, %.4f)" % (v[0] / v[2], v[1] / v[2])
    except (np.linalg.LinAlgError, ZeroDivisionError, FloatingPointError):
        return "(no inverse)"


def _first_difference(got, ref, ch, what, where=None):
    """where two buffers differ first: pixel, channel, both values, the extent of the differences; where(x, y) adds the frame / chip and the
    source coordinate"""
    if got.shape != ref.shape:
        return f"{what}: shape {got.shape} != {ref.shape}"
    d = np.argwhere(got != ref)
    if not len(d):
        return f"{what}: equal"
    y, b = (int(v) for v in d[0])
    return (f"{what}: {len(d)} bytes differ, first at x {b // ch} y {y} channel {b % ch}: got {int(got[y, b])}, expected {int(ref[y, b])}; "
            f"rows {int(d[:, 0].min())}..{int(d[:, 0].max())}, columns {int(d[:, 1].min()) // ch}..{int(d[:, 1].max()) // ch}"
            + (("; " + where(b // ch, y)) if where else ""))


# ---- ImageProjectionTransform ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SINGLE, ids=_ids(SINGLE))
def test_gpu_single_warp_equals_oracle(ctx, oracle, case):
    for img in (case.img, wp.grey(case.img)):
        ch = 3 if img.ndim == 3 else 1
        o = wp.single_out(oracle, case, img)
        buf, dw, dh, dws = ctx.ImageProjectionTransform(img, case.h9)
        assert (dw, dh, dws) == (o["dw"], o["dh"], o["dws"]), case.tag
        X, Y = wr.project(case.h9, *wr.corners(img.shape[1], img.shape[0]))

        def where(x, y, X=X, Y=Y):
            return f"source {_src(case.h9, x + float(np.nanmin(X)), y + float(np.nanmin(Y)))} of the {img.shape[1]} x {img.shape[0]} frame"
        assert np.array_equal(buf, o["buf"]), _first_difference(buf, o["buf"], ch, f"{case.tag} {ch} channel(s) {dw} x {dh}", where)      # row padding included


# ---- MosaicImagesRefined --------------------------------------------------------------------------------------------------------------------
def _device_frames(imgs, withhold=None):
    import torch
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in imgs]
    ptrs = [0 if k == withhold else t.data_ptr() for k, t in enumerate(d)]
    return d, ptrs, [a.shape[1] for a in imgs], [a.shape[0] for a in imgs], [np.ascontiguousarray(a).strides[0] for a in imgs]


def _refined_where(case, o):
    def where(x, y):
        k = int(o["winner"][y, x]) if x < o["cw"] else -1
        if k < 0:
            return "no frame has a sample there"
        import imagemosaicing_amd as im
        dG = im.mosaic_layout([a.shape[1] for a in case.imgs], [a.shape[0] for a in case.imgs], case.h9s)[3]
        return f"the oracle's sample comes from frame {k} at source {_src(case.h9s[k], x - float(dG[0]), y - float(dG[1]))}"
    return where


def _render_rows(ctx, case, o, ptrs, wv, hv, wsv, row0, rows, cws):
    """the canvas after rendering rows [row0, row0 + rows) into a sentinel-filled buffer of row stride cws"""
    import torch
    can = torch.full((o["ch"], cws), SENTINEL, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.MosaicImagesRefinedDev(ptrs, wv, hv, wsv, case.h9s, can.data_ptr(), o["cw"], o["ch"], cws, row0, rows)
    ctx.synchronize()
    return can.cpu().numpy()


def _check_rows(got, o, row0, rows, what, where):
    cw, ch = o["cw"], o["ch"]
    inside = got[row0:row0 + rows]
    assert np.array_equal(inside[:, :3 * cw], o["canvas"][row0:row0 + rows, :3 * cw]), _first_difference(
        np.ascontiguousarray(inside[:, :3 * cw]), np.ascontiguousarray(o["canvas"][row0:row0 + rows, :3 * cw]), 3, what, lambda x, y: where(x, y + row0))
    assert not inside[:, 3 * cw:].any(), f"{what}: row padding not cleared"
    assert (got[:row0] == SENTINEL).all() and (got[row0 + rows:] == SENTINEL).all(), f"{what}: rows outside the stripe were written"


def _stripe_list(case, ch):
    if ch <= 64:
        return [(y, 1) for y in range(ch)]
    s = [(0, 7), (7, 250), (257, ch - 257), (255, 2), (ch - 1, 1), (17, 1)]
    return [(a, n) for a, n in s if n >= 1 and a + n <= ch]


@pytest.mark.parametrize("case", REFINED, ids=_ids(REFINED))
def test_gpu_refined_equals_oracle(ctx, oracle, case):
    o = wp.refined_out(oracle, case)
    where = _refined_where(case, o)
    got, cw, ch, cws = ctx.MosaicImagesRefined(case.imgs, case.h9s)
    assert (cw, ch, cws) == (o["cw"], o["ch"], o["cws"]), case.tag
    assert np.array_equal(got, o["canvas"]), _first_difference(got, o["canvas"], 3, f"{case.tag} MosaicImagesRefined", where)
    d, ptrs, wv, hv, wsv = _device_frames(case.imgs)
    _check_rows(_render_rows(ctx, case, o, ptrs, wv, hv, wsv, 0, ch, cws), o, 0, ch, f"{case.tag} MosaicImagesRefinedDev", where)
    # a caller's row stride wider than the layout's: padding and uncovered pixels zero, nothing outside the rows touched
    wide = cws + 12
    _check_rows(_render_rows(ctx, case, o, ptrs, wv, hv, wsv, 0, ch, wide), o, 0, ch, f"{case.tag} row stride {wide}", where)
    r0, rn = ch // 3, max(1, ch // 2)
    _check_rows(_render_rows(ctx, case, o, ptrs, wv, hv, wsv, r0, rn, wide), o, r0, rn, f"{case.tag} rows {r0}..{r0 + rn - 1} row stride {wide}", where)
    if case.hidden is not None:
        d2, p2, _, _, _ = _device_frames(case.imgs, withhold=case.hidden)
        _check_rows(_render_rows(ctx, case, o, p2, wv, hv, wsv, 0, ch, cws), o, 0, ch, f"{case.tag} without a pointer to frame {case.hidden}", where)


@pytest.mark.parametrize("case", REFINED, ids=_ids(REFINED))
def test_gpu_refined_stripes_equal_oracle(ctx, oracle, case):
    """every row on its own for canvases of up to 64 rows; cuts off the multiples of 16 and 256 for the large sparse canvas"""
    o = wp.refined_out(oracle, case)
    where = _refined_where(case, o)
    d, ptrs, wv, hv, wsv = _device_frames(case.imgs)
    assert o["ch"] <= 64 or case.tag == "sparse"
    for a, n in _stripe_list(case, o["ch"]):
        _check_rows(_render_rows(ctx, case, o, ptrs, wv, hv, wsv, a, n, o["cws"]), o, a, n, f"{case.tag} rows {a}..{a + n - 1}", where)


@pytest.mark.parametrize("case", REFINED, ids=_ids(REFINED))
def test_gpu_exact_stripe_cover_is_the_set_of_winners(ctx, oracle, case):
    """mi355_mosaic_stripe_cover, exact mode: precisely the frames that own at least one pixel of the rows in the oracle's canvas (the winner
    map of tests/warp_ref.py, whose canvas the CPU suite proves equal to the oracle's)"""
    o = wp.refined_out(oracle, case)
    wv, hv = [a.shape[1] for a in case.imgs], [a.shape[0] for a in case.imgs]
    ch = o["ch"]
    stripes = [(0, ch), (0, 1), (ch - 1, 1), (ch // 3, max(1, ch // 2))] + ([(7, 250), (257, ch - 257)] if ch > 257 else [])
    for a, n in stripes:
        need = ctx.StripeCover(wv, hv, case.h9s, a, n, exact=True)
        want = np.zeros(len(case.imgs), np.uint8)
        for k in np.unique(o["winner"][a:a + n]):
            if k >= 0:
                want[k] = 1
        assert np.array_equal(need, want), (case.tag, a, n, need.tolist(), want.tolist())
    if case.tag == "twins":
        need = ctx.StripeCover(wv, hv, case.h9s, 0, ch, exact=True)
        assert need[1] == 0 and need[2] == 1


# ---- ChipsAndMasks --------------------------------------------------------------------------------------------------------------------------
def _chip_where(case, o, k):
    c = o["chips"][k]
    f = int(c["img"])

    def where(x, y):
        X = x + int(c["x0"]) - float(o["dG"][0]) - float(c["sx"])
        Y = y + int(c["y0"]) - float(o["dG"][1]) - float(c["sy"])
        return f"chip {k} (frame {f}, rectangle {int(c['x0'])}, {int(c['y0'])}, {int(c['w'])} x {int(c['h'])}) at source {_src(case.h9s[f], X, Y)}"
    return where


def _check_chips(ctx, oracle, case, find_masks, o=None):
    o = o or wp.chips_out(oracle, case, find_masks=find_masks)
    r = ctx.ChipsAndMasks(case.imgs, case.h9s, keep=case.keep, find_masks=find_masks)
    what = f"{case.tag} find_masks={find_masks}"
    assert (r["cw"], r["ch"]) == (o["cw"], o["ch"]) and len(r["chips"]) == len(o["chips"]), what
    cover = np.zeros((o["ch"], o["cw"]), np.int32)
    for k, (a, b) in enumerate(zip(r["chips"], o["chips"])):
        assert all(int(a[f]) == int(b[f]) for f in ("x0", "y0", "w", "h", "img")), (what, k, a, b)
        assert np.array_equal(bits(a["quad"]), bits(b["quad"])) and bits(a["sx"]) == bits(b["sx"]) and bits(a["sy"]) == bits(b["sy"]), (what, k, "quad bits")
        where = _chip_where(case, o, k)
        assert np.array_equal(r["chip_imgs"][k], o["chip_imgs"][k]), _first_difference(r["chip_imgs"][k], o["chip_imgs"][k], 3, f"{what} chip {k} pixels", where)
        assert np.array_equal(r["masks"][k], o["masks"][k]), _first_difference(r["masks"][k], o["masks"][k], 1, f"{what} chip {k} {'ownership' if find_masks else 'validity'}", where)
        x0, y0, w, h = (int(b[f]) for f in ("x0", "y0", "w", "h"))
        cover[y0:y0 + h, x0:x0 + w] += r["masks"][k][:, :w] != 0
    if find_masks:
        assert cover.max() <= 1, f"{what}: a canvas pixel with {int(cover.max())} owners"
    return o


@pytest.mark.parametrize("find_masks", (True, False), ids=("owners", "validity"))
@pytest.mark.parametrize("case", CHIPS, ids=_ids(CHIPS))
def test_gpu_chips_and_masks_equal_oracle(ctx, oracle, case, find_masks):
    _check_chips(ctx, oracle, case, find_masks)


def _blend_stripes(tag, ch):
    if tag == "straddle":
        s = [(0, 250), (250, 13), (255, 2), (256, 1), (263, ch - 263)]
    else:
        s = [(0, 1), (1, 1), (ch - 1, 1), (ch // 2, 1), (17, 1), (0, 23), (23, ch - 23)]
    return [(a, n) for a, n in s if n >= 1 and a >= 0 and a + n <= ch]


@pytest.mark.parametrize("tag", ("seventy", "straddle", "duplicates", "thin"))
def test_gpu_striped_ownership_equals_the_whole(ctx, oracle, tag):
    """the striped form of the chips stage (row_lo .. row_hi) is reached through the one-call blend: a stripe of the blended canvas is the rows
    of the whole, and the whole is the oracle's blend of the oracle's chips and ownership masks"""
    case = next(c for c in CHIPS if c.tag == tag)
    o = wp.chips_out(oracle, case)
    cw, ch = o["cw"], o["ch"]
    d, ptrs, wv, hv, wsv = _device_frames(case.imgs)
    for band in (5, 1):
        ref, _ = oracle.multiband_blend(o["chips"], o["chip_imgs"], o["masks"], cw, ch, band=band)
        whole, cw2, ch2, cws = ctx.MosaicBlendedDev(ptrs, wv, hv, wsv, case.h9s, keep=case.keep, band=band)
        whole = whole.cpu().numpy()
        assert (cw2, ch2) == (cw, ch) and np.array_equal(whole[:, :3 * cw], ref[:, :3 * cw]), _first_difference(
            np.ascontiguousarray(whole[:, :3 * cw]), np.ascontiguousarray(ref[:, :3 * cw]), 3, f"{tag} band {band} whole canvas")
        for a, n in _blend_stripes(tag, ch):
            got, cw3, ch3, cws3 = ctx.MosaicBlendedDev(ptrs, wv, hv, wsv, case.h9s, keep=case.keep, band=band, row0=a, rows=n)
            assert (cw3, ch3, cws3) == (cw, ch, cws) and tuple(got.shape) == (n, cws)
            got = got.cpu().numpy()
            assert np.array_equal(got, whole[a:a + n]), _first_difference(got, np.ascontiguousarray(whole[a:a + n]), 3, f"{tag} band {band} rows {a}..{a + n - 1}")


# ---- one context across large and tiny cases ------------------------------------------------------------------------------------------------
def test_gpu_one_context_large_tiny_large(oracle):
    """buffers the context keeps (chip_masks, chip_imgs, mosaic_lists, mosaic_frames) must not leak from a large case into a tiny one or back:
    one fresh context runs large, tiny, large"""
    import imagemosaicing_amd as im
    chips = {c.tag: c for c in CHIPS}
    refined = {c.tag: c for c in REFINED}
    single = {c.tag: c for c in SINGLE}
    ctx = im.Context(0)
    try:
        for ctag, rtag, stag in (("straddle", "sparse", "up300"), ("thin", "canvas_w1", "width_1"), ("seventy", "forty", "horizon"),
                                 ("no_valid_pixel", "canvas_w2", "turn90_2x2_white"), ("straddle", "sparse", "up300")):
            _check_chips(ctx, oracle, chips[ctag], True)
            _check_chips(ctx, oracle, chips[ctag], False)
            rc = refined[rtag]
            o = wp.refined_out(oracle, rc)
            got, cw, ch, cws = ctx.MosaicImagesRefined(rc.imgs, rc.h9s)
            assert (cw, ch, cws) == (o["cw"], o["ch"], o["cws"]) and np.array_equal(got, o["canvas"]), _first_difference(got, o["canvas"], 3, f"{rtag} after {ctag}")
            sc = single[stag]
            so = wp.single_out(oracle, sc, sc.img)
            buf, dw, dh, dws = ctx.ImageProjectionTransform(sc.img, sc.h9)
            assert (dw, dh, dws) == (so["dw"], so["dh"], so["dws"]) and np.array_equal(buf, so["buf"]), _first_difference(buf, so["buf"], 3, f"{stag} after {rtag}")
    finally:
        ctx.close()
