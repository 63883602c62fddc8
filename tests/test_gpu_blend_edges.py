"""Multiband blend at its edges, on the GPU: the HIP paths (csrc/blend.hip) against the oracle on the cases of tests/blend_edges.py -- canvases
narrower than 2^band, chips of a few pixels, level counts set by the canvas, grey masks, 16-bit wrap-around, odd pyramid offsets inside a
batch, tiny / projective / strip-shaped surveys, stripes down to single rows.  Every comparison is np.array_equal on the output bytes plus
the canvas size; nothing is skipped or filtered at run time.  (tests/test_blend_edges_oracle.py checks the oracle itself against a numpy
restatement of its definition on the same cases.)

Not covered: more than 16 levels (MAX_BANDS) -- that needs a canvas side above 65 536, padded to 131 072 on both sides; not testable in memory.
"""
import numpy as np
import pytest

from tests import blend_edges as be

pytestmark = pytest.mark.gpu

DIRECT = be.direct_cases()
SURVEY = be.survey_cases()


def _ids(cases):
    return [c.tag for c in cases]


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


def _first_difference(got, ref, W, what):
    """where two canvases differ first: pixel, channel, both values -- enough to find the level and the column class from the geometry"""
    if got.shape != ref.shape:
        return f"{what}: shape {got.shape} != {ref.shape}"
    d = np.argwhere(got != ref)
    if not len(d):
        return f"{what}: equal"
    y, b = (int(v) for v in d[0])
    return (f"{what}: {len(d)} bytes differ, first at x {b // 3} y {y} channel {b % 3} (canvas width {W}): got {int(got[y, b])}, expected {int(ref[y, b])}; "
            f"rows {int(d[:, 0].min())}..{int(d[:, 0].max())}, columns {int(d[:, 1].min()) // 3}..{int(d[:, 1].max()) // 3}")


def _direct_oracle(oracle, case):
    rects, chips, masks = be.nonempty(case)
    return oracle.multiband_blend(be.info_array(rects), chips, masks, case.W, case.H, band=case.band)


def _check_direct(ctx, oracle, case, ref=None):
    if ref is None:
        ref, _ = _direct_oracle(oracle, case)
    got, ow, oh, ows = ctx.MultiBandBlend(be.info_array(case.rects), case.chips, case.masks, case.W, case.H, band=case.band)
    assert (ow, oh) == (case.W, case.H) and ows == ref.shape[1]
    assert np.array_equal(got, ref), _first_difference(got, ref, case.W, case.tag)


@pytest.mark.parametrize("case", DIRECT, ids=_ids(DIRECT))
def test_gpu_direct_case_equals_oracle(ctx, oracle, case):
    _check_direct(ctx, oracle, case)


def _device_frames(imgs):
    import torch
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in imgs]
    return d, [t.data_ptr() for t in d], [a.shape[1] for a in imgs], [a.shape[0] for a in imgs], [np.ascontiguousarray(a).strides[0] for a in imgs]


@pytest.mark.parametrize("case", SURVEY, ids=_ids(SURVEY))
def test_gpu_survey_case_equals_oracle(ctx, oracle, case):
    o = oracle.chips_and_masks(case.imgs, case.h9s, keep=case.keep, find_masks=True)
    r = ctx.ChipsAndMasks(case.imgs, case.h9s, keep=case.keep, find_masks=True)
    cw, ch = o["cw"], o["ch"]
    assert (r["cw"], r["ch"]) == (cw, ch) and len(r["chips"]) == len(o["chips"])
    for k, (a, b) in enumerate(zip(r["chips"], o["chips"])):
        assert all(int(a[f]) == int(b[f]) for f in ("x0", "y0", "w", "h", "img")), (k, a, b)
        assert np.array_equal(r["chip_imgs"][k], o["chip_imgs"][k]), f"{case.tag}: chip {k} pixels"
        assert np.array_equal(r["masks"][k], o["masks"][k]), f"{case.tag}: chip {k} mask"
    o2 = oracle.chips_and_masks(case.imgs, case.h9s, keep=case.keep, find_masks=False)
    r2 = ctx.ChipsAndMasks(case.imgs, case.h9s, keep=case.keep, find_masks=False)
    for k in range(len(o2["chips"])):
        assert np.array_equal(r2["masks"][k], o2["masks"][k]), f"{case.tag}: chip {k} validity mask"
    d_imgs, ptrs, wv, hv, wsv = _device_frames(case.imgs)
    for band in be.survey_bands(case):
        ref, _ = oracle.multiband_blend(o["chips"], o["chip_imgs"], o["masks"], cw, ch, band=band)
        got, ow, oh, _ = ctx.MultiBandBlend(r["chips"], r["chip_imgs"], r["masks"], cw, ch, band=band)
        assert (ow, oh) == (cw, ch) and np.array_equal(got, ref), _first_difference(got, ref, cw, f"{case.tag} band {band} MultiBandBlend")
        got, ow, oh, _ = ctx.MosaicBlended(case.imgs, case.h9s, keep=case.keep, band=band)
        assert (ow, oh) == (cw, ch) and np.array_equal(got, ref), _first_difference(got, ref, cw, f"{case.tag} band {band} MosaicBlended")
        got, dw_, dh_, dws = ctx.MosaicBlendedDev(ptrs, wv, hv, wsv, case.h9s, keep=case.keep, band=band)
        got = got.cpu().numpy()
        assert (dw_, dh_) == (cw, ch) and np.array_equal(got[:, :3 * cw], ref[:, :3 * cw]), _first_difference(got, ref, cw, f"{case.tag} band {band} MosaicBlendedDev")
        ref2, _ = oracle.multiband_blend(o2["chips"], o2["chip_imgs"], o2["masks"], cw, ch, band=band)
        got, ow, oh, _ = ctx.MultiBandBlend(r2["chips"], r2["chip_imgs"], r2["masks"], cw, ch, band=band)
        assert (ow, oh) == (cw, ch) and np.array_equal(got, ref2), _first_difference(got, ref2, cw, f"{case.tag} band {band} validity masks")


def _stripes(ch, band, every_row):
    """(row0, rows): single rows at 0, 1, ch - 1 and ch // 2, the two parts of a cut inside one 2^band block, and every row on its own"""
    al = 1 << min(band, 10)
    cut = al + al // 2 + 1
    if cut >= ch:
        cut = max(1, ch // 2)
    s = [(0, 1), (1, 1), (ch - 1, 1), (ch // 2, 1), (0, cut), (cut, ch - cut)]
    if every_row:
        s += [(y, 1) for y in range(ch)]
    out = []
    for a, n in s:
        if 0 <= a and n >= 1 and a + n <= ch and (a, n) not in out:
            out.append((a, n))
    return out


@pytest.mark.parametrize("case", SURVEY, ids=_ids(SURVEY))
def test_gpu_survey_stripes_equal_whole_canvas(ctx, oracle, case):
    """stripes through MosaicBlendedDev(row0, rows) are the rows of the whole canvas -- which is the oracle's (asserted here as well).  band 0
    (and any stripe when no pyramid is left) takes the path that forms the whole canvas and copies the stripe out."""
    o = oracle.chips_and_masks(case.imgs, case.h9s, keep=case.keep, find_masks=True)
    cw, ch = o["cw"], o["ch"]
    d_imgs, ptrs, wv, hv, wsv = _device_frames(case.imgs)
    small = case.tag in ("tiny_only", "narrow")
    bands = be.survey_bands(case) + ((0,) if case.tag in ("tiny_only", "strip") else ())
    for band in bands:
        ref, _ = oracle.multiband_blend(o["chips"], o["chip_imgs"], o["masks"], cw, ch, band=band)
        whole, cw2, ch2, cws = ctx.MosaicBlendedDev(ptrs, wv, hv, wsv, case.h9s, keep=case.keep, band=band)
        whole = whole.cpu().numpy()
        assert (cw2, ch2) == (cw, ch) and np.array_equal(whole[:, :3 * cw], ref[:, :3 * cw]), _first_difference(whole, ref, cw, f"{case.tag} band {band}")
        for a, n in _stripes(ch, band, every_row=small and band in (5, 1, 0)):
            got, cw3, ch3, cws3 = ctx.MosaicBlendedDev(ptrs, wv, hv, wsv, case.h9s, keep=case.keep, band=band, row0=a, rows=n)
            assert (cw3, ch3, cws3) == (cw, ch, cws) and tuple(got.shape) == (n, cws)
            got = got.cpu().numpy()
            assert np.array_equal(got, whole[a:a + n]), _first_difference(got, whole[a:a + n], cw, f"{case.tag} band {band} rows {a}..{a + n - 1}")


def test_gpu_one_context_across_large_and_small_canvases(oracle):
    """buffers kept by the context from a larger case must not leak into a smaller one: one fresh context, the cases ordered so that large and
    small canvases alternate (direct and survey cases interleaved), then the first case again"""
    import imagemosaicing_amd as im
    by_size = sorted(DIRECT, key=lambda c: c.W * c.H)
    order = []
    while by_size:
        order.append(by_size.pop())                 # largest left
        if by_size:
            order.append(by_size.pop(0))            # smallest left
    surveys = sorted(SURVEY, key=lambda s: sum(a.size for a in s.imgs), reverse=True)
    ctx = im.Context(0)
    try:
        refs = {}
        for i, case in enumerate(order + order[:1]):
            if case.tag not in refs:
                refs[case.tag] = _direct_oracle(oracle, case)[0]
            _check_direct(ctx, oracle, case, refs[case.tag])
            if i % 4 == 1 and surveys:
                s = surveys.pop(0) if (i // 4) % 2 == 0 else surveys.pop()
                o = oracle.chips_and_masks(s.imgs, s.h9s, keep=s.keep, find_masks=True)
                ref, _ = oracle.multiband_blend(o["chips"], o["chip_imgs"], o["masks"], o["cw"], o["ch"], band=5)
                got, ow, oh, _ = ctx.MosaicBlended(s.imgs, s.h9s, keep=s.keep, band=5)
                assert (ow, oh) == (o["cw"], o["ch"]) and np.array_equal(got, ref), _first_difference(got, ref, o["cw"], f"{s.tag} after {case.tag}")
        assert not surveys
    finally:
        ctx.close()
