"""GPU: the median render (mi355_mosaic_median / _dev / _into / _cover, csrc/median.hip): canvas, spread map and count map byte for byte against
tests/median_ref.py (numpy on the oracle's refined render), with pre-filled outputs so that unwritten bytes show and row padding is zero.

  * the reference's committed 20-frame run (tests/golden, decimated) at depth 1, 2, 3, 5, 9 (every instantiation, and depths below their K) with
    ramp 0, depth 5 also with ramp 1, 16 and 1000; depth 1 is the seamline render's canvas, count == 1 the refined render's bytes;
  * the 10-frame case of tests/test_gpu_gain.py (projective frames, a skipped frame, a far-away frame) at depth 0 (the default), 4 (an even m on
    the K = 5 kernel) and 9;
  * odd pitches with poisoned padding, mixed frame sizes down to 2 x 2 and 3 x 2 (tests/pitched.py);
  * stripes of 1, 7 and 256 rows put side by side equal the whole canvas, for all three outputs; a stripe writes its own rows only;
  * the host form, the _into form (kept frames and host images mixed, a caller pitch wider than 3 cw) and the device form agree;
  * after GainCompensateDev the render is the restatement on the LUT'd frames;
  * 300 frames stacked on one spot at depth 1, 5, 9: weight ties by the dozen at every selection boundary; MedianCover is the set of frames
    in the restatement's selected sets; NULL for every frame outside it gives the same bytes, NULL for a frame inside is MI355_ERR_ARG naming
    it, nothing written, and the ctx goes on working;
  * maps without frames; the moving-object case and the built boundary tie of tests/test_median_ref.py; every refusal of the header.
"""
import numpy as np
import pytest

from tests import gain_ref as gr
from tests import median_ref as mr
from tests import seamline_ref as sr

pytestmark = pytest.mark.gpu
FILL = (7, 0x33, 0x5555)                                                    # canvas, spread, count before a call


@pytest.fixture(scope="module")
def golden(oracle):
    imgs, h9s = sr.golden_survey()
    maps = gr.frame_sample_maps(oracle, imgs, h9s)
    return imgs, h9s, maps, {}


def _golden_ref(oracle, golden, ramp, depth):
    """the restatement on the golden survey, the weight maps of a ramp made once"""
    imgs, h9s, maps, wcache = golden
    if ramp not in wcache:
        wcache[ramp] = sr.weight_maps(oracle, imgs, h9s, ramp, maps)
    return mr.pick(maps, wcache[ramp], depth)


@pytest.fixture(scope="module")
def case(oracle):
    from tests.test_gpu_gain import _case
    imgs, h9s, pairs = _case()
    return imgs, h9s, pairs, gr.frame_sample_maps(oracle, imgs, h9s)


def _upload(torch, imgs):
    from tests.test_gpu_gain import _upload as up
    return up(torch, imgs)


class Out:
    """device canvas [ch, cws] uint8, spread [ch, cw] uint8 and count [ch, cw] (int16 storage, read as uint16), pre-filled so that unwritten
    bytes show"""
    def __init__(self, torch, im, w, h, h9s, cws=None, canvas=True, spread=True, count=True):
        self.cw, self.ch, lws, _ = im.mosaic_layout(w, h, h9s)
        self.cws = cws or lws
        self.canvas = torch.full((self.ch, self.cws), FILL[0], dtype=torch.uint8, device="cuda") if canvas else None
        self.spread = torch.full((self.ch, self.cw), FILL[1], dtype=torch.uint8, device="cuda") if spread else None
        self.count = torch.full((self.ch, self.cw), FILL[2], dtype=torch.int16, device="cuda") if count else None
        torch.cuda.synchronize()                                            # the fills run on torch's stream, the library on the ctx's own

    def render(self, ctx, ptrs, w, h, ws, h9s, row0=0, rows=-1, **kw):
        ctx.MosaicMedianDev(ptrs, w, h, ws, h9s, self.canvas.data_ptr() if self.canvas is not None else 0, self.cw, self.ch, self.cws, row0, rows,
                            d_spread=self.spread.data_ptr() if self.spread is not None else 0,
                            d_count=self.count.data_ptr() if self.count is not None else 0, **kw)
        return self

    def host(self):
        return (None if self.canvas is None else self.canvas.cpu().numpy(), None if self.spread is None else self.spread.cpu().numpy(),
                None if self.count is None else self.count.cpu().numpy().view(np.uint16))

    def untouched(self):
        return all(a is None or np.all(a == fill) for a, fill in zip(self.host(), FILL))


def _pix(a, cw):
    return np.ascontiguousarray(a[:, :3 * cw]).reshape(a.shape[0], cw, 3)


def _same(got, ref, cw, what=""):
    canvas, spread, count = got
    for name, a, b in (("count", count, ref[2]), ("spread", spread, ref[1]), ("canvas", _pix(canvas, cw), ref[0])):
        bad = (a != b)
        bad = bad.any(axis=2) if bad.ndim == 3 else bad
        assert a.shape == b.shape and not bad.any(), "%s %s: %d pixels differ, first %s" % (what, name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert not canvas[:, 3 * cw:].any()                                     # row padding zeroed


@pytest.mark.parametrize("ramp,depth", [(0, 1), (0, 2), (0, 3), (0, 5), (0, 9), (1, 5), (16, 5), (1000, 5)])
def test_golden_equals_restatement(golden, oracle, ramp, depth):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s = golden[:2]
    ref = _golden_ref(oracle, golden, ramp, depth)
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, ramp=ramp, depth=depth)
    assert (o.ch, o.cw) == ref[0].shape[:2]
    _same(o.host(), ref, o.cw, "ramp %d depth %d" % (ramp, depth))
    assert ref[2].max() >= 4 and (ref[2] >= 3).sum() > 10000
    # a caller's wider row: the padding is cleared up to cws
    o2 = Out(torch, im, w, h, h9s, cws=o.cws + 32).render(ctx, ptrs, w, h, ws, h9s, ramp=ramp, depth=depth)
    _same(o2.host(), ref, o.cw, "wide rows, ramp %d depth %d" % (ramp, depth))
    if depth == 1:
        # the seamline render, which is pinned to the oracle on its own
        s = torch.full((o.ch, o.cws), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.MosaicSeamlineDev(ptrs, w, h, ws, h9s, s.data_ptr(), o.cw, o.ch, o.cws, ramp=ramp)
        assert torch.equal(s, o.canvas)
    if depth == 5 and ramp == 0:
        # the refined render wherever one frame covers
        r = torch.full((o.ch, o.cws), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.MosaicImagesRefinedDev(ptrs, w, h, ws, h9s, r.data_ptr(), o.cw, o.ch, o.cws)
        single = ref[2] == 1
        assert single.sum() > 1000 and np.array_equal(_pix(r.cpu().numpy(), o.cw)[single], _pix(o.host()[0], o.cw)[single])
    ctx.close()


@pytest.mark.parametrize("depth", [0, 4, 9])
def test_case_equals_restatement(case, oracle, depth):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    for ramp in (0, 16):
        ref = mr.median_ref(oracle, imgs, h9s, ramp, depth, maps)
        o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, ramp=ramp, depth=depth)
        _same(o.host(), ref, o.cw, "ramp %d depth %d" % (ramp, depth))
    assert (ref[2] >= 4).sum() > 100                                        # depth 4: medians of four, an even m
    ctx.close()


def test_pitches_and_mixed_sizes(oracle):
    import torch
    import imagemosaicing_amd as im
    from tests import pitched as pf
    sizes = pf.MIXED_SIZES + [(3, 2), (2, 3), (2, 2)]
    imgs = pf.mixed_images(sizes, seed=3)
    h9s = pf.mixed_h9s(sizes, seed=6)
    h9s[-1] = [3, 0, 100.25, 0, 3, 80.5, 0, 0, 1]                          # a 2 x 2 frame magnified: its one texel cell spans 3 x 3 canvas pixels
    maps = gr.frame_sample_maps(oracle, imgs, h9s)
    refs = {(ramp, depth): mr.median_ref(oracle, imgs, h9s, ramp, depth, maps) for ramp, depth in ((0, 3), (5, 0))}
    for shift in (0, 2):
        F = pf.PitchedFrames(imgs, pf.mixed_pitches(sizes, shift=shift), offsets=[k % 4 for k in range(len(sizes))], seed=11 + shift)
        t, ptrs = F.to_device(torch)
        w, h, ws = F.geom()
        ctx = im.Context(0)
        for (ramp, depth), ref in refs.items():
            o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, ramp=ramp, depth=depth)
            _same(o.host(), ref, o.cw, "shift %d ramp %d depth %d" % (shift, ramp, depth))
            assert ref[2].max() >= 3 and (ref[2] > 1).sum() > 10000
        assert np.array_equal(F.device_bytes(t), F.buf)                      # the frames and their padding are read only
        ctx.close()


def test_after_gain_compensation(golden, oracle):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s = golden[:2]
    pairs = [(k, k + 1) for k in range(len(imgs) - 1)]
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    g = ctx.GainCompensateDev(ptrs, w, h, ws, h9s, pairs, step=4)
    assert not np.all(g == 1.0)
    lutd = [gr.apply_lut(imgs[k], g[k]) for k in range(len(imgs))]
    ref = mr.median_ref(oracle, lutd, h9s, 0, 3)
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, depth=3)
    _same(o.host(), ref, o.cw, "compensated")
    ctx.close()


def test_stripes_equal_the_whole_canvas(golden):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s = golden[:2]
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    whole = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s).host()
    ch = whole[0].shape[0]
    assert ch > 256
    for cut in (1, 7, 256):
        o = Out(torch, im, w, h, h9s)
        for row0 in range(0, ch, cut):
            o.render(ctx, ptrs, w, h, ws, h9s, row0, min(cut, ch - row0))
        for a, b in zip(o.host(), whole):
            assert np.array_equal(a, b), cut
    # a stripe call writes its own rows only, in all three outputs
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, 100, 50)
    for a, b, fill in zip(o.host(), whole, FILL):
        assert np.array_equal(a[100:150], b[100:150]) and np.all(a[:100] == fill) and np.all(a[150:] == fill)
    ctx.close()


def test_host_into_and_device_forms_agree(case, oracle):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    n = len(imgs)
    ref = mr.median_ref(oracle, imgs, h9s, 16, 3, maps)
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, ramp=16, depth=3)
    dev = o.host()
    cw, ch = o.cw, o.ch
    _same(dev, ref, cw)
    host, cw2, ch2, cws2, spr = ctx.MosaicMedian(imgs, h9s, ramp=16, depth=3, want_spread=True)
    assert (cw2, ch2) == (cw, ch) and np.array_equal(host, dev[0]) and np.array_equal(spr, ref[1])
    host2, _, _, _ = ctx.MosaicMedian(imgs, h9s, ramp=16, depth=3)
    assert np.array_equal(host2, host)
    # _into: host sources, a caller pitch wider than 3 cw whose tail stays as it is
    pitch = 3 * cw + 29
    out = np.full((ch, pitch), 201, np.uint8)
    out, cw3, ch3 = ctx.MosaicMedianInto(imgs, None, h9s, out=out, ramp=16, depth=3)
    assert (cw3, ch3) == (cw, ch) and np.array_equal(_pix(out, cw), ref[0]) and np.all(out[:, 3 * cw:] == 201)
    # _into: kept frames (the caller's arrays hold garbage by the time of the render), and a mix of both sources
    ctx.set_option("keep_frames", 1)
    for k in range(n):
        ctx.SiftExtractHost(k, imgs[k].copy())
    ctx.synchronize()
    ids = np.arange(n, dtype=np.int32)
    garbage = [np.full_like(f, 77) for f in imgs]
    out, _, _ = ctx.MosaicMedianInto(garbage, ids, h9s, ramp=16, depth=3)
    assert np.array_equal(_pix(out, cw), ref[0])
    mixed = np.where(ids % 2 == 0, ids, -1).astype(np.int32)
    out, _, _ = ctx.MosaicMedianInto([None if mixed[k] >= 0 else imgs[k] for k in range(n)], mixed, h9s, ramp=16, depth=3)
    assert np.array_equal(_pix(out, cw), ref[0])
    ctx.close()


def _heavy(n=300):
    from tests.synth import texture
    rng = np.random.default_rng(12)
    imgs = [texture(24, 20, seed=200 + k) for k in range(n)]
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (n, 1))
    h9s[:, 2] = rng.integers(0, 7, n)
    h9s[:, 5] = rng.integers(0, 5, n)
    h9s[1::3, 0] = 1.05
    return imgs, h9s


def test_heavy_overlap_and_withheld_frames(oracle):
    """300 small frames on one spot, as the seamline tests build them: hundreds of frames per pixel and weight ties by the dozen at every
    selection boundary, so that the index decides who is selected nearly everywhere"""
    import torch
    import imagemosaicing_amd as im
    imgs, h9s = _heavy()
    n = len(imgs)
    maps = gr.frame_sample_maps(oracle, imgs, h9s)
    wmaps = sr.weight_maps(oracle, imgs, h9s, 0, maps)
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    for depth in (1, 5, 9):
        out, spread, count, sel, tie = mr.pick(maps, wmaps, depth)
        assert count.max() > 250 and tie.sum() > 100                        # the boundary ties are there
        o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, depth=depth)
        _same(o.host(), (out, spread, count), o.cw, "heavy, depth %d" % depth)
        inside = np.unique(sel[sel > 0]).astype(int) - 1
        need = ctx.MedianCover(w, h, h9s, depth=depth)
        assert np.array_equal(np.flatnonzero(need), inside), depth
    # depth 5: withholding is really exercised
    ref = mr.pick(maps, wmaps, 5)
    inside = np.unique(ref[3][ref[3] > 0]).astype(int) - 1
    need = ctx.MedianCover(w, h, h9s, depth=5)
    idle = [k for k in range(n) if not need[k]]
    assert n - len(inside) >= n // 4 and len(idle) == n - len(inside)
    assert ctx.StripeCover(w, h, h9s, 0, ref[0].shape[0])[idle].all()       # their boxes do meet the rows: no pixel selects them
    # NULL for every frame outside the cover: the same bytes
    held = [0 if not need[k] else p for k, p in enumerate(ptrs)]
    o = Out(torch, im, w, h, h9s).render(ctx, held, w, h, ws, h9s, depth=5)
    _same(o.host(), ref, o.cw, "outsiders withheld")
    # NULL for one frame inside: refused, naming it, before anything is written; the ctx goes on working
    for k in (int(inside[0]), int(inside[len(inside) // 2]), int(inside[-1])):
        bad = list(held)
        bad[k] = 0
        o2 = Out(torch, im, w, h, h9s)
        with pytest.raises(im.Mi355Error) as e:
            o2.render(ctx, bad, w, h, ws, h9s, depth=5)
        assert e.value.code == -1 and "image %d " % k in str(e.value), str(e.value)
        assert o2.untouched()
        _same(Out(torch, im, w, h, h9s).render(ctx, held, w, h, ws, h9s, depth=5).host(), ref, o.cw, "after the refusal")
    ctx.close()


def test_cover_and_maps_without_frames(case, oracle):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    depth = 2
    ref = mr.median_ref(oracle, imgs, h9s, 0, depth, maps, full=True)
    sel = ref[3]
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, depth=depth)
    canvas, spread, count = o.host()
    _same((canvas, spread, count), ref, o.cw)
    ch = o.ch
    for row0, rows in ((0, ch), (0, 60), (100, 1), (37, 200), (ch - 5, 5), (250, 300)):
        need = ctx.MedianCover(w, h, h9s, row0, rows, depth=depth)
        want = np.unique(sel[:, row0:row0 + rows]).astype(int)
        want = want[want > 0] - 1
        assert np.array_equal(np.flatnonzero(need), want), (row0, rows)
        assert not need[8]                                                  # skipped (h9[8] == 0)
        # NULL for everything outside the cover
        held = [p if need[k] else 0 for k, p in enumerate(ptrs)]
        s = Out(torch, im, w, h, h9s).render(ctx, held, w, h, ws, h9s, row0, rows, depth=depth).host()
        for a, b in zip(s, (canvas, spread, count)):
            assert np.array_equal(a[row0:row0 + rows], b[row0:row0 + rows]), (row0, rows)
    assert np.array_equal(ctx.MedianCover(w, h, h9s, ramp=16), ctx.MedianCover(w, h, h9s, 0, ch, ramp=16))
    # d_canvas == NULL and d_spread == NULL: nothing is sampled; d_imgs and ws may be NULL altogether
    m = Out(torch, im, w, h, h9s, canvas=False, spread=False).render(ctx, None, w, h, None, h9s, depth=depth).host()
    assert np.array_equal(m[2], count)
    m = Out(torch, im, w, h, h9s, canvas=False, spread=False).render(ctx, [0] * len(w), w, h, ws, h9s, depth=depth).host()
    assert np.array_equal(m[2], count)
    # each output alone, and the spread map without a canvas
    m = Out(torch, im, w, h, h9s, spread=False, count=False).render(ctx, ptrs, w, h, ws, h9s, depth=depth).host()
    assert np.array_equal(m[0], canvas)
    m = Out(torch, im, w, h, h9s, canvas=False, count=False).render(ctx, ptrs, w, h, ws, h9s, depth=depth).host()
    assert np.array_equal(m[1], spread)
    ctx.close()


def test_a_moving_object_drops_out(oracle):
    import torch
    import imagemosaicing_amd as im
    clean, dirty, h9s, (bx, by, block) = mr.moving_object_case()
    c_ref = mr.median_ref(oracle, clean, h9s, 0, 9)
    d_ref = mr.median_ref(oracle, dirty, h9s, 0, 9)
    ctx = im.Context(0)
    got = []
    for imgs, ref in ((clean, c_ref), (dirty, d_ref)):
        ts, ptrs, w, h, ws = _upload(torch, imgs)
        o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, depth=9)
        _same(o.host(), ref, o.cw)
        got.append(o.host())
    cw = c_ref[0].shape[1]
    assert np.array_equal(got[0][0], got[1][0])                             # the block is gone from the canvas
    foot = got[1][1] > 0
    assert foot.sum() == block * block and foot[by:by + block, bx:bx + block].all() and not got[0][1].any()
    ts, ptrs, w, h, ws = _upload(torch, dirty)
    f = torch.zeros((c_ref[0].shape[0], got[0][0].shape[1]), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.MosaicFeatheredDev(ptrs, w, h, ws, h9s, f.data_ptr(), cw, f.shape[0], f.shape[1])
    assert (_pix(f.cpu().numpy(), cw)[foot] != c_ref[0][foot]).any(axis=1).all()       # which the feathered mean keeps as a ghost
    ctx.close()


def test_the_index_decides_a_tie_at_the_selection_boundary(oracle):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, col, rows = mr.boundary_tie_case()
    ref = mr.median_ref(oracle, imgs, h9s, 0, 2, full=True)
    assert ref[4][rows, col].all() and (ref[3][1, rows, col] == 2).all()
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, depth=2)
    _same(o.host(), ref[:3], o.cw)
    need = ctx.MedianCover(w, h, h9s, 32, 1, depth=2)                      # one row through the tie
    assert np.array_equal(np.flatnonzero(need), np.unique(ref[3][:, 32][ref[3][:, 32] > 0]).astype(int) - 1)
    ctx.close()


def test_refusals(case):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    o = Out(torch, im, w, h, h9s)
    whole = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s).host()

    def err(fn, code, match=""):
        with pytest.raises(im.Mi355Error) as e:
            fn()
        assert e.value.code == code and match in str(e.value), str(e.value)

    err(lambda: o.render(ctx, ptrs, w, h, ws, h9s, ramp=-1), -1, "ramp=-1")
    err(lambda: ctx.MedianCover(w, h, h9s, ramp=-3), -1, "ramp=-3")
    err(lambda: ctx.MosaicMedian(imgs, h9s, ramp=-1), -1, "ramp=-1")
    err(lambda: ctx.MosaicMedianInto(imgs, None, h9s, ramp=-1), -1, "ramp=-1")
    # depth outside 0 .. MI355_MEDIAN_MAX_DEPTH
    err(lambda: o.render(ctx, ptrs, w, h, ws, h9s, depth=-1), -1, "depth=-1")
    err(lambda: o.render(ctx, ptrs, w, h, ws, h9s, depth=10), -1, "depth=10")
    err(lambda: ctx.MedianCover(w, h, h9s, depth=10), -1, "depth=10")
    err(lambda: ctx.MosaicMedian(imgs, h9s, depth=-2), -1, "depth=-2")
    err(lambda: ctx.MosaicMedianInto(imgs, None, h9s, depth=12), -1, "depth=12")
    # all three outputs NULL; a canvas or a spread map without frames
    err(lambda: ctx.MosaicMedianDev(ptrs, w, h, ws, h9s, 0, o.cw, o.ch, o.cws), -1, "all NULL")
    err(lambda: ctx.MosaicMedianDev(None, w, h, ws, h9s, o.canvas.data_ptr(), o.cw, o.ch, o.cws), -1, "d_imgs")
    err(lambda: ctx.MosaicMedianDev(None, w, h, ws, h9s, 0, o.cw, o.ch, o.cws, d_spread=o.spread.data_ptr()), -1, "d_imgs")
    err(lambda: ctx.MosaicMedianDev(ptrs, w, h, None, h9s, 0, o.cw, o.ch, o.cws, d_spread=o.spread.data_ptr()), -1, "d_imgs")
    # a canvas geometry that is not the layout's
    err(lambda: ctx.MosaicMedianDev(ptrs, w, h, ws, h9s, o.canvas.data_ptr(), o.cw + 1, o.ch, o.cws), -1, "canvas geometry")
    err(lambda: ctx.MosaicMedianDev(ptrs, w, h, ws, h9s, o.canvas.data_ptr(), o.cw, o.ch - 1, o.cws), -1, "canvas geometry")
    err(lambda: ctx.MosaicMedianDev(ptrs, w, h, ws, h9s, o.canvas.data_ptr(), o.cw, o.ch, 3 * o.cw - 4), -1, "canvas geometry")
    err(lambda: ctx.MosaicMedianDev(None, w, h, None, h9s, 0, o.cw + 1, o.ch, o.cws, d_count=o.count.data_ptr()), -1, "canvas geometry")
    # frame geometry: a pitch below 3 w, a side beyond 2^20
    bad_ws = list(ws)
    bad_ws[1] = 3 * w[1] - 1
    err(lambda: o.render(ctx, ptrs, w, h, bad_ws, h9s), -1, "bad image geometry")
    big_w = [(1 << 20) + 1, 4]
    big_h9 = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    err(lambda: ctx.MedianCover(big_w, [2, 2], big_h9), -1, "bad image geometry")
    # the frame limit
    big = 65536
    err(lambda: ctx.MedianCover([8] * big, [8] * big, np.tile(np.eye(3, dtype=np.float32).reshape(9), (big, 1))), -1, "65535")
    # n <= 1 in the host forms, as mi355_mosaic_refined
    err(lambda: ctx.MosaicMedian(imgs[:1], h9s[:1]), -2)
    err(lambda: ctx.MosaicMedianInto(imgs[:1], None, h9s[:1]), -2)
    # _into: a destination that is not the layout's
    err(lambda: ctx.MosaicMedianInto(imgs, None, h9s, out=np.zeros((o.ch, 3 * o.cw - 3), np.uint8), pitch=3 * o.cw - 3), -1, "dst_pitch")
    assert o.untouched()                                                    # no refusal wrote anything
    got = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s).host()  # the ctx still works after the refusals
    assert all(np.array_equal(a, b) for a, b in zip(got, whole))
    ctx.close()
