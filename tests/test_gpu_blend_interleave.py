"""GPU: the entry points of the multiband blend -- ChipsAndMasks, MultiBandBlend, MosaicBlended, MosaicBlendedDev (whole canvas, stripes, the
whole-canvas fallback of a stripe), StripeCover(blended) and MosaicBlendedInto -- share the chip stage and the context's chip, mask, warp
argument and pyramid buffers.  The suites of each pin it alone; this one runs them interleaved on ONE context, over surveys of 2 to 70
chips, and holds every result to the bytes of the same call on a fresh context: nothing the chip stage of one entry point leaves behind --
deferred warp arguments, launch extents, owned boxes, offsets -- may reach the next one.  (In the pattern of
tests/test_gpu_render_interleave.py; all frames are at most 320 x 240.)
"""
import numpy as np
import pytest

from tests import blend_edges as be
from tests import warp_patterns as wp

pytestmark = pytest.mark.gpu

BAND = 5


class Dev:
    """a survey with its frames in HBM"""

    def __init__(self, torch, case):
        self.case = case
        self.imgs = [np.ascontiguousarray(a) for a in case.imgs]
        self.t = [torch.from_numpy(a).cuda() for a in self.imgs]
        torch.cuda.synchronize()
        self.ptrs = [t.data_ptr() for t in self.t]
        self.w = [a.shape[1] for a in self.imgs]; self.h = [a.shape[0] for a in self.imgs]; self.ws = [a.strides[0] for a in self.imgs]

    def blended(self, ctx, ptrs=None, **kw):
        got, cw, ch, cws = ctx.MosaicBlendedDev(self.ptrs if ptrs is None else ptrs, self.w, self.h, self.ws, self.case.h9s, keep=self.case.keep, **kw)
        return got.cpu().numpy(), cw, ch, cws


def _oracle_canvas(oracle, case, band):
    o = oracle.chips_and_masks(case.imgs, case.h9s, keep=case.keep, find_masks=True)
    ref, _ = oracle.multiband_blend(o["chips"], o["chip_imgs"], o["masks"], o["cw"], o["ch"], band=band)
    return ref, o["cw"], o["ch"]


def test_interleaved_blend_calls_equal_fresh_contexts(oracle):
    import torch
    import imagemosaicing_amd as im
    surveys = {s.tag: s for s in be.survey_cases()}
    strip, tiny, keep = Dev(torch, surveys["strip"]), Dev(torch, surveys["tiny_only"]), surveys["keep"]
    projective, downscaled = surveys["projective"], surveys["downscaled"]
    seventy = Dev(torch, next(c for c in wp.chips_cases() if c.tag == "seventy"))
    assert max(max(a.shape[:2]) for s in list(surveys.values()) + [seventy.case] for a in s.imgs) <= 320
    ch = im.blend_layout(strip.w, strip.h, strip.case.h9s, strip.case.keep)[1]
    cut = 32 + 16 + 1                                                       # inside the second 2^5 block of rows
    assert 32 < cut < 64 <= ch, ch
    held = {}                                                               # the chips of step 2, for step 3

    def chips_of(case, find_masks, hold=False):
        def f(ctx):
            r = ctx.ChipsAndMasks(case.imgs, case.h9s, keep=case.keep, find_masks=find_masks)
            if hold:
                held.setdefault("chips", r)
            info = np.array([[int(c[k]) for k in ("x0", "y0", "w", "h", "img")] for c in r["chips"]], np.int64)
            return [info, np.array([r["cw"], r["ch"]])] + list(r["chip_imgs"]) + list(r["masks"])
        return f

    def blend_held(ctx):
        r = held["chips"]
        got, ow, oh, ows = ctx.MultiBandBlend(r["chips"], r["chip_imgs"], r["masks"], r["cw"], r["ch"], band=BAND)
        return [got, np.array([ow, oh, ows])]

    def into(ctx):
        cw, chh, _ = im.blend_layout([a.shape[1] for a in keep.imgs], [a.shape[0] for a in keep.imgs], keep.h9s, keep.keep)
        out = np.full((chh, 3 * cw + 13), 201, np.uint8)                  # the bytes past 3 cw stay the caller's
        ctx.MosaicBlendedInto(keep.imgs, None, keep.h9s, keep=keep.keep, band=BAND, out=out)
        return [out]

    steps = [
        ("1 strip, device", lambda ctx: list(strip.blended(ctx, band=BAND)[:1])),
        ("2 chips of projective", chips_of(projective, True, hold=True)),
        ("3 blend of those chips", blend_held),
        ("4 strip, a stripe cut inside a block", lambda ctx: list(strip.blended(ctx, band=BAND, row0=cut, rows=ch - cut)[:1])),
        ("5 cover of that stripe", lambda ctx: [ctx.StripeCover(strip.w, strip.h, strip.case.h9s, cut, ch - cut, blended=True, band=BAND)]),
        ("6 tiny_only, one row at band 0", lambda ctx: list(tiny.blended(ctx, band=0, row0=1, rows=1)[:1])),
        ("7 downscaled, host frames, band 3", lambda ctx: [np.array(v) for v in ctx.MosaicBlended(downscaled.imgs, downscaled.h9s, keep=downscaled.keep, band=3)]),
        ("8 validity chips of strip", chips_of(strip.case, False)),
        ("9 keep, into host rows", into),
        ("10 seventy, device", lambda ctx: list(seventy.blended(ctx, band=BAND)[:1])),
        ("11 strip, device, again", lambda ctx: list(strip.blended(ctx, band=BAND)[:1])),
    ]
    ctx = im.Context(0)
    shared = [call(ctx) for _, call in steps]
    ctx.close()
    for (name, call), got in zip(steps, shared):
        fresh = im.Context(0)
        want = call(fresh)
        fresh.close()
        assert len(got) == len(want) > 0, name
        for a, b in zip(got, want):
            a, b = np.asarray(a), np.asarray(b)
            assert a.shape == b.shape and np.array_equal(a, b), "%s: %d values differ from a fresh context's" % (name, int((a != b).sum()))
    res = dict(zip([n.split()[0] for n, _ in steps], shared))
    # steps 1, 3 and 7 are the oracle's canvases
    ref, cw, och = _oracle_canvas(oracle, strip.case, BAND)
    assert och == ch and np.array_equal(res["1"][0][:, :3 * cw], ref[:, :3 * cw]) and np.array_equal(res["11"][0], res["1"][0])
    ref, _, _ = _oracle_canvas(oracle, projective, BAND)
    assert np.array_equal(res["3"][0], ref)
    ref, _, _ = _oracle_canvas(oracle, downscaled, 3)
    assert np.array_equal(res["7"][0], ref)
    # the stripe is those rows of the whole canvas; the single row of the fallback is the oracle's
    assert res["4"][0].shape[0] == ch - cut and np.array_equal(res["4"][0], res["1"][0][cut:])
    ref, tcw, tch = _oracle_canvas(oracle, tiny.case, 0)
    assert tch >= 2 and np.array_equal(res["6"][0][:, :3 * tcw], ref[1:2, :3 * tcw])
    ref, kcw, _ = _oracle_canvas(oracle, keep, BAND)
    assert np.array_equal(res["9"][0][:, :3 * kcw], ref[:, :3 * kcw]) and np.all(res["9"][0][:, 3 * kcw:] == 201)
    # three batches in step 10: more than 64 chips own something
    o = oracle.chips_and_masks(seventy.case.imgs, seventy.case.h9s, keep=None, find_masks=True)
    assert sum(1 for m in o["masks"] if m.any()) > 64
    # The cover marks exactly the frames whose pointers the stripe needs: with the others NULL (and the statement checked: strict_frames)
    # the stripe is the same, and without any one of the marked frames the call is refused.
    need = res["5"][0]
    assert need.shape == (len(strip.ptrs),) and need.any()
    fresh = im.Context(0)
    fresh.set_option("strict_frames", 1)
    got = strip.blended(fresh, ptrs=[p if n else 0 for p, n in zip(strip.ptrs, need)], band=BAND, row0=cut, rows=ch - cut)[0]
    assert np.array_equal(got, res["4"][0])
    for k in np.flatnonzero(need):
        with pytest.raises(im.Mi355Error):
            strip.blended(fresh, ptrs=[0 if i == k else p for i, p in enumerate(strip.ptrs)], band=BAND, row0=cut, rows=ch - cut)
    fresh.close()
