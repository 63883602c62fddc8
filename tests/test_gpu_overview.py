"""GPU: the overview levels (mi355_mosaic_overview / _dev, csrc/overview.hip) and the striped preview (mi355_mosaic_preview_into), byte for
byte against tests/overview_ref.py: the levels, the coverage maps and the zeroed row padding.

  * the committed 20-frame survey: seamline, refined and feathered canvases with the seamline count map, levels 1..7, all three no-data modes;
  * adversarial device buffers: noise with a sparse map, all-invalid, one valid pixel in a 128 x 128 block, saturated 255, a 0 / 255
    checkerboard under NODATA_ZERO, canvases of 1 x 1, 1 x 300, 300 x 1, 129 x 257, a wide caller pitch with poisoned padding, a stripe
    pointer at 4 mod 16;
  * stripes of 2^levels, 3 * 2^levels and the rest equal the whole; a stripe writes its own output rows only;
  * host form = device form; every refusal, each followed by a call that works;
  * the preview for render x nodata on the survey and on the 10-frame projective case equals the restatement of the full render (itself
    from the _dev calls), with kept frames and host images mixed and a wide dst pitch; "preview_stripe_rows" 2^level, 1024, 0 agree; after
    GainCompensateDev it is the preview of the compensated frames;
  * C3 at its own size (500 x 4000x3000): the level-3 seamline preview on 512 x 512 output windows.
"""
import numpy as np
import pytest

from tests import overview_ref as ovr
from tests import seamline_ref as sr

pytestmark = pytest.mark.gpu
FILL8, FILL16 = 0xA5, 0xA5A5


def _upload(torch, imgs):
    from tests.test_gpu_gain import _upload as up
    return up(torch, imgs)


class Levels:
    """prefilled device outputs of levels 1 .. levels: [oh, ows] uint8 and [oh, ow] covers (int16 storage, read as uint16)"""
    def __init__(self, torch, cw, ch, levels, covers=True):
        self.geo = ovr.layout(cw, ch, levels)
        self.lv = [torch.full((oh, ows), FILL8, dtype=torch.uint8, device="cuda") for ow, oh, ows in self.geo]
        self.cv = [torch.full((oh, ow), FILL16 - 65536, dtype=torch.int16, device="cuda") for ow, oh, ows in self.geo] if covers else None
        torch.cuda.synchronize()                                            # the fills run on torch's stream, the library on the ctx's own

    def ptrs(self):
        return [t.data_ptr() for t in self.lv], (None if self.cv is None else [t.data_ptr() for t in self.cv])

    def host(self):
        return [(self.lv[l].cpu().numpy(), None if self.cv is None else self.cv[l].cpu().numpy().view(np.uint16)) for l in range(len(self.lv))]


def _run(ctx, torch, canvas_t, cw, levels, nodata=0, vmap_t=None, covers=True, row0=0, rows=-1, out=None):
    """canvas_t: device [ch, cws] uint8; vmap_t: device [ch, cw] int16 or None.  The stripe pointers are those of row row0."""
    ch, cws = canvas_t.shape
    out = out or Levels(torch, cw, ch, levels, covers)
    lv, cv = out.ptrs()
    ctx.MosaicOverviewDev(canvas_t.data_ptr() + row0 * cws, cw, ch, cws, levels, lv, cv,
                          d_valid_rows=0 if vmap_t is None else vmap_t.data_ptr() + 2 * row0 * cw, nodata=nodata, row0=row0, rows=rows)
    ctx.synchronize()
    return out


def _same(got, ref, what=""):
    assert len(got) == len(ref)
    for l, ((g, gc), (r, rc)) in enumerate(zip(got, ref), 1):
        assert g.shape == r.shape, (what, l, g.shape, r.shape)
        bad = g != r
        assert not bad.any(), "%s level %d: %d bytes differ, first %s" % (what, l, int(bad.sum()), np.argwhere(bad)[:5].tolist())
        if gc is not None:
            bad = gc != rc
            assert not bad.any(), "%s level %d: %d cover values differ, first %s" % (what, l, int(bad.sum()), np.argwhere(bad)[:5].tolist())


def _dev16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).cuda()


def _full_renders(ctx, torch, im, imgs, h9s, ramp=0):
    """the three full-size canvases [ch, cws] and the seamline count map [ch, cw], all through the existing _dev calls (device tensors)"""
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    cw, ch, cws, _ = im.mosaic_layout(w, h, h9s)
    can = [torch.full((ch, cws), 7, dtype=torch.uint8, device="cuda") for _ in range(3)]
    count = torch.zeros((ch, cw), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx.MosaicImagesRefinedDev(ptrs, w, h, ws, h9s, can[0].data_ptr(), cw, ch, cws)
    ctx.MosaicFeatheredDev(ptrs, w, h, ws, h9s, can[1].data_ptr(), cw, ch, cws, ramp=ramp)
    ctx.MosaicSeamlineDev(ptrs, w, h, ws, h9s, can[2].data_ptr(), cw, ch, cws, d_count=count.data_ptr(), ramp=ramp)
    ctx.synchronize()
    return can, count, cw, ch, cws


@pytest.fixture(scope="module")
def golden():
    return sr.golden_survey()


@pytest.fixture(scope="module")
def case():
    from tests.test_gpu_gain import _case
    return _case()


@pytest.mark.parametrize("render", [2, 0, 1])
def test_golden_survey_all_levels_all_modes(golden, render):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s = golden
    ctx = im.Context(0)
    can, count, cw, ch, cws = _full_renders(ctx, torch, im, imgs, h9s)
    canvas, cnt = can[render].cpu().numpy(), count.cpu().numpy().view(np.uint16)
    assert (cnt > 0).any() and (cnt == 0).any()
    for nodata in (0, 1, 2):
        got = _run(ctx, torch, can[render], cw, 7, nodata, count).host()
        _same(got, ovr.overview_ref(canvas, cw, 7, nodata, cnt), "render %d nodata %d" % (render, nodata))
    # fewer levels are the first levels; no covers asked for
    got = _run(ctx, torch, can[render], cw, 3, 2, count, covers=False).host()
    ref = ovr.overview_ref(canvas, cw, 3, 2, cnt)
    assert all(np.array_equal(g[0], r[0]) for g, r in zip(got, ref))
    ctx.close()


def _adversarial():
    rng = np.random.default_rng(17)
    out = []

    def add(name, pix, vmap=None, modes=(0, 1, 2), **kw):
        ch, cw = pix.shape[:2]
        if vmap is None:
            vmap = (rng.random((ch, cw)) < 0.5).astype(np.uint16) * rng.integers(1, 65536, (ch, cw)).astype(np.uint16)
        out.append((name, pix.astype(np.uint8), vmap.astype(np.uint16), modes, kw))
    noise = rng.integers(0, 256, (517, 389, 3))
    noise[rng.random((517, 389)) < 0.2] = 0
    add("noise, sparse map", noise, (rng.random((517, 389)) < 0.07).astype(np.uint16) * 9)
    add("all invalid", np.zeros((260, 300, 3)), np.zeros((260, 300)), modes=(1, 2))
    one = np.zeros((256, 384, 3)); onem = np.zeros((256, 384)); one[200, 300] = (1, 0, 255); onem[200, 300] = 65535
    add("one valid pixel", one, onem)
    add("saturated", np.full((256, 257, 3), 255), np.ones((256, 257)))
    yy, xx = np.mgrid[:300, :263]
    add("checkerboard", (((xx + yy) & 1) * 255)[..., None].repeat(3, 2), modes=(1, 0))
    for cw, ch in ((1, 1), (1, 300), (300, 1), (129, 257)):
        add("%d x %d" % (cw, ch), rng.integers(0, 256, (ch, cw, 3)))
    add("wide pitch", rng.integers(0, 256, (200, 131, 3)), pitch=131 * 3 + 3 + 40)
    add("pointer 4 mod 16", rng.integers(0, 256, (384, 202, 3)), shift=4)
    return out


def test_adversarial_buffers():
    import torch
    import imagemosaicing_amd as im
    ctx = im.Context(0)
    for name, pix, vmap, modes, kw in _adversarial():
        ch, cw = pix.shape[:2]
        cws = kw.get("pitch", (3 * cw + 3) & ~3)
        shift = kw.get("shift", 0)
        host = np.full(ch * cws + 64, 0xEE, np.uint8)                      # poisoned padding, and room to move the first row
        rows = host[shift:shift + ch * cws].reshape(ch, cws)
        rows[:, :3 * cw] = pix.reshape(ch, 3 * cw)
        dev = torch.from_numpy(host).cuda()
        canvas_t = dev[shift:shift + ch * cws].view(ch, cws)
        if shift:
            assert canvas_t.data_ptr() % 16 == shift
        vt = _dev16(torch, vmap)
        torch.cuda.synchronize()
        for nodata in modes:
            got = _run(ctx, torch, canvas_t, cw, 7, nodata, vt).host()
            _same(got, ovr.overview_ref(pix, cw, 7, nodata, vmap), "%s, nodata %d" % (name, nodata))
        assert np.array_equal(dev.cpu().numpy(), host)                       # the canvas and its padding are read only
    ctx.close()


@pytest.mark.parametrize("levels", [1, 4, 7])
def test_stripes_equal_the_whole_and_write_their_own_rows(levels):
    import torch
    import imagemosaicing_amd as im
    rng = np.random.default_rng(levels)
    cw, ch = 333, 1111
    pix = rng.integers(0, 256, (ch, cw, 3), dtype=np.uint8)
    pix[rng.random((ch, cw)) < 0.3] = 0
    vmap = (rng.random((ch, cw)) < 0.4).astype(np.uint16)
    cws = (3 * cw + 3) & ~3
    rows = np.zeros((ch, cws), np.uint8); rows[:, :3 * cw] = pix.reshape(ch, 3 * cw)
    ct, vt = torch.from_numpy(rows).cuda(), _dev16(torch, vmap)
    ctx = im.Context(0)
    u = 1 << levels
    cuts = [0, u, 4 * u, ch]                                                # stripes of 2^levels, 3 * 2^levels and the rest
    for nodata in (0, 1, 2):
        whole = ovr.overview_ref(pix, cw, levels, nodata, vmap)
        out = Levels(torch, cw, ch, levels)
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            _run(ctx, torch, ct, cw, levels, nodata, vt, row0=r0, rows=r1 - r0, out=out)
        _same(out.host(), whole, "stripes, nodata %d" % nodata)
        # a stripe buffer of its own (not a window of the whole canvas) serves as well
        part = Levels(torch, cw, ch, levels)
        st, sv = ct[u:4 * u].clone(), vt[u:4 * u].clone()
        torch.cuda.synchronize()
        lv, cv = part.ptrs()
        ctx.MosaicOverviewDev(st.data_ptr(), cw, ch, cws, levels, lv, cv, d_valid_rows=sv.data_ptr(), nodata=nodata, row0=u, rows=3 * u)
        ctx.synchronize()
        for l, ((g, gc), (r, rc)) in enumerate(zip(part.host(), whole), 1):
            y0, y1 = u >> l, (4 * u) >> l
            assert np.array_equal(g[y0:y1], r[y0:y1]) and np.array_equal(gc[y0:y1], rc[y0:y1]), (nodata, l)
            assert np.all(g[:y0] == FILL8) and np.all(g[y1:] == FILL8) and np.all(gc[:y0] == FILL16) and np.all(gc[y1:] == FILL16), (nodata, l)
    ctx.close()


def test_host_form_equals_device_form_and_refusals(golden):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s = golden
    ctx = im.Context(0)
    can, count, cw, ch, cws = _full_renders(ctx, torch, im, imgs, h9s)
    canvas, cnt = can[2].cpu().numpy(), count.cpu().numpy().view(np.uint16)
    for nodata in (0, 1, 2):
        dev = _run(ctx, torch, can[2], cw, 5, nodata, count).host()
        lv, cv = ctx.MosaicOverview(canvas, cw, 5, valid=cnt, nodata=nodata, want_covers=True)
        _same(list(zip(lv, cv)), dev, "host form, nodata %d" % nodata)
    lv = ctx.MosaicOverview(canvas, cw, 2, nodata=1)
    assert len(lv) == 2 and np.array_equal(lv[1], ovr.overview_ref(canvas, cw, 2, 1)[1][0])
    good = ovr.overview_ref(canvas, cw, 3, 2, cnt)

    def err(fn, code=-1, match=""):
        with pytest.raises(im.Mi355Error) as e:
            fn()
        assert e.value.code == code and match in str(e.value), str(e.value)
        _same(_run(ctx, torch, can[2], cw, 3, 2, count).host(), good, "after a refusal")       # the ctx goes on working

    out = Levels(torch, cw, ch, 7)
    lvp, cvp = out.ptrs()
    call = lambda **kw: ctx.MosaicOverviewDev(**dict(dict(d_rows=can[2].data_ptr(), cw=cw, ch=ch, cws=cws, levels=3, d_levels=lvp[:3], d_covers=cvp[:3],
                                                          d_valid_rows=count.data_ptr(), nodata=2, row0=0, rows=-1), **kw))
    err(lambda: call(levels=0, d_levels=[]), match="levels=0")
    err(lambda: call(levels=8, d_levels=lvp + [0]), match="levels=8")
    err(lambda: call(nodata=3), match="nodata=3")
    err(lambda: call(nodata=-1), match="nodata=-1")
    err(lambda: call(d_valid_rows=0), match="without a map")
    err(lambda: call(row0=4, rows=8), match="multiples of 2^levels")
    err(lambda: call(d_rows=can[2].data_ptr() + 8 * cws, row0=8, rows=12), match="multiples of 2^levels")
    err(lambda: call(row0=8, rows=ch), match="rows")
    err(lambda: call(d_levels=None), match="NULL")
    err(lambda: call(d_levels=[lvp[0], 0, lvp[2]]), match="d_levels[1]")
    err(lambda: call(cws=3 * cw - 4), match="geometry")
    err(lambda: call(cws=cws + 2), match="geometry")
    err(lambda: call(d_rows=can[2].data_ptr() + 2), match="geometry")
    err(lambda: call(cw=0), match="geometry")
    err(lambda: ctx.MosaicOverview(canvas, cw, 8))
    err(lambda: ctx.MosaicOverview(canvas, cw, 3, nodata=2))
    assert all(np.all(g == FILL8) and np.all(c == FILL16) for g, c in out.host())              # no refusal wrote anything
    # NULL covers, and a single NULL entry, are fine
    call(d_covers=None); call(d_covers=[cvp[0], 0, cvp[2]]); ctx.synchronize()
    got = out.host()
    assert all(np.array_equal(got[l][0], good[l][0]) for l in range(3)) and np.array_equal(got[0][1], good[0][1]) and np.array_equal(got[2][1], good[2][1])
    assert np.all(got[1][1] == FILL16)
    ctx.close()


def _mixed_sources(ctx, imgs):
    """even frames kept in HBM (the host arrays handed over hold garbage), odd frames as host images"""
    n = len(imgs)
    ctx.set_option("keep_frames", 1)
    for k in range(0, n, 2):
        ctx.SiftExtractHost(k, imgs[k].copy())
    ctx.synchronize()
    ids = np.where(np.arange(n) % 2 == 0, np.arange(n), -1).astype(np.int32)
    return [None if ids[k] >= 0 else imgs[k] for k in range(n)], ids


@pytest.mark.parametrize("which,level,ramp", [("golden", 3, 0), ("case", 2, 16)])
def test_preview_equals_the_restatement_of_the_full_render(golden, case, which, level, ramp):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s = golden if which == "golden" else case[:2]
    ctx = im.Context(0)
    can, count, cw, ch, cws = _full_renders(ctx, torch, im, imgs, h9s, ramp)
    cnt = count.cpu().numpy().view(np.uint16)
    srcs, ids = _mixed_sources(ctx, imgs)
    ow, oh, ows = ovr.layout(cw, ch, level)[-1]
    pitch = 3 * ow + 29
    seen = {}
    for render in (0, 1, 2):
        canvas = can[render].cpu().numpy()
        for nodata in (0, 1, 2):
            ref, rcov = ovr.overview_ref(canvas, cw, level, nodata, cnt)[level - 1]
            out = np.full((oh, pitch), 201, np.uint8)
            out, gw, gh, cover = ctx.MosaicPreviewInto(srcs, ids, h9s, out=out, want_cover=True, render=render, ramp=ramp, level=level, nodata=nodata)
            assert (gw, gh) == (ow, oh)
            bad = out[:, :3 * ow] != ref[:, :3 * ow]
            assert not bad.any(), "%s render %d nodata %d: %d bytes differ, first %s" % (which, render, nodata, int(bad.sum()), np.argwhere(bad)[:5].tolist())
            assert np.all(out[:, 3 * ow:] == 201) and np.array_equal(cover, rcov), (render, nodata)
            seen[(render, nodata)] = out[:, :3 * ow].copy()
    assert (seen[(0, 2)] != seen[(1, 2)]).any() and (seen[(0, 2)] != seen[(2, 2)]).any() and (seen[(2, 0)] != seen[(2, 2)]).any()
    # the stripe height does not show: 2^level, 1024 and the whole canvas
    assert ch > 2 << level
    for stripe in (1 << level, 1024, 0, 1):
        ctx.set_option("preview_stripe_rows", stripe)
        for render in (0, 1, 2):
            out, _, _ = ctx.MosaicPreviewInto(srcs, ids, h9s, render=render, ramp=ramp, level=level, nodata=2)
            assert np.array_equal(out[:, :3 * ow], seen[(render, 2)]), (stripe, render)
    ctx.close()


def test_preview_refusals(case):
    import imagemosaicing_amd as im
    imgs, h9s = case[:2]
    ctx = im.Context(0)
    good, ow, oh = ctx.MosaicPreviewInto(imgs, None, h9s, render=2, level=3)

    def err(fn, code=-1, match=""):
        with pytest.raises(im.Mi355Error) as e:
            fn()
        assert e.value.code == code and match in str(e.value), str(e.value)
        assert np.array_equal(ctx.MosaicPreviewInto(imgs, None, h9s, render=2, level=3)[0], good)

    err(lambda: ctx.MosaicPreviewInto(imgs, None, h9s, render=3), match="render=3")
    err(lambda: ctx.MosaicPreviewInto(imgs, None, h9s, render=-1), match="render=-1")
    err(lambda: ctx.MosaicPreviewInto(imgs, None, h9s, level=0), match="level=0")
    err(lambda: ctx.MosaicPreviewInto(imgs, None, h9s, level=8), match="level=8")
    err(lambda: ctx.MosaicPreviewInto(imgs, None, h9s, nodata=3), match="nodata=3")
    err(lambda: ctx.MosaicPreviewInto(imgs, None, h9s, render=1, ramp=-1), match="ramp=-1")
    err(lambda: ctx.MosaicPreviewInto(imgs[:1], None, h9s[:1]), code=-2)
    err(lambda: ctx.MosaicPreviewInto(imgs, None, h9s, level=3, dims=(ow + 1, oh), out=np.zeros((oh, 3 * ow + 8), np.uint8)), match="layout")
    err(lambda: ctx.MosaicPreviewInto(imgs, None, h9s, level=3, dims=(ow, oh - 1)), match="layout")
    err(lambda: ctx.MosaicPreviewInto(imgs, None, h9s, level=3, out=np.zeros((oh, 3 * ow), np.uint8), pitch=3 * ow - 1), match="dst_pitch")
    err(lambda: ctx.MosaicPreviewInto(imgs, np.full(len(imgs), 99, np.int32), h9s, geom=[(320, 240, 960)] * len(imgs)), match="holds no kept frame")
    err(lambda: ctx.set_option("preview_stripe_rows", -1))
    ctx.close()


def test_preview_after_gain_compensation(golden):
    """the kept frames are compensated in place (their device addresses go to GainCompensateDev): the preview through their ids is the
    restatement of the full render of the compensated frames"""
    import torch
    import imagemosaicing_amd as im
    imgs, h9s = golden
    n = len(imgs)
    ctx = im.Context(0)
    ctx.set_option("keep_frames", 1)
    for k in range(n):
        ctx.SiftExtractHost(k, imgs[k].copy())
    ctx.synchronize()
    fr = [ctx.FrameDev(k) for k in range(n)]
    ptrs, w, h, ws = [f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr], [f[3] for f in fr]
    g = ctx.GainCompensateDev(ptrs, w, h, ws, h9s, [(k, k + 1) for k in range(n - 1)], step=4)
    assert not np.all(g == 1.0)
    cw, ch, cws, _ = im.mosaic_layout(w, h, h9s)
    canvas = torch.zeros((ch, cws), dtype=torch.uint8, device="cuda")
    count = torch.zeros((ch, cw), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx.MosaicSeamlineDev(ptrs, w, h, ws, h9s, canvas.data_ptr(), cw, ch, cws, d_count=count.data_ptr())
    ctx.synchronize()
    ref, rcov = ovr.overview_ref(canvas.cpu().numpy(), cw, 3, 2, count.cpu().numpy().view(np.uint16))[2]
    out, ow, oh, cover = ctx.MosaicPreviewInto(None, np.arange(n, dtype=np.int32), h9s, want_cover=True, render=2, level=3, nodata=2)
    assert np.array_equal(out[:, :3 * ow], ref[:, :3 * ow]) and np.array_equal(cover, rcov)
    plain, _, _ = ctx.MosaicPreviewInto(imgs, None, h9s, render=2, level=3, nodata=2)       # the uncompensated host images
    assert (plain != out).any()
    ctx.close()


def test_c3_full_size():
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import frame_layout
    from tests.test_gpu_gain import _h9s, _render
    W, H, F, level = 4000, 3000, 500, 3
    ctx = im.Context(0)
    A, gains = frame_layout(F, W, H)
    frames, ws = _render(ctx, torch, A, gains, W, H)
    assert ws == 3 * W
    h9s = _h9s(A)
    ptrs = [frames[k].data_ptr() for k in range(F)]
    wv, hv, wsv = [W] * F, [H] * F, [ws] * F
    cw, ch, cws, _ = im.mosaic_layout(wv, hv, h9s)
    canvas = torch.empty((ch, cws), dtype=torch.uint8, device="cuda")
    count = torch.empty((ch, cw), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx.MosaicSeamlineDev(ptrs, wv, hv, wsv, h9s, canvas.data_ptr(), cw, ch, cws, d_count=count.data_ptr())
    ctx.synchronize()
    host = frames.cpu().numpy()
    del frames
    torch.cuda.empty_cache()
    imgs = [host[k].reshape(H, W, 3) for k in range(F)]
    out, ow, oh, cover = ctx.MosaicPreviewInto(imgs, None, h9s, want_cover=True, render=2, level=level, nodata=2)
    assert (ow, oh) == ovr.layout(cw, ch, level)[-1][:2] and ow > 1024 and oh > 1024
    ctx.set_option("preview_stripe_rows", 0)
    whole, _, _ = ctx.MosaicPreviewInto(imgs, None, h9s, render=2, level=level, nodata=2)
    assert np.array_equal(whole, out), "C3: one stripe and stripes of 1024 rows differ"
    rng = np.random.default_rng(31)
    S, b = 512, 1 << level
    wins = [(0, 0), (ow - S, oh - S)] + [(int(rng.integers(0, ow - S)), int(rng.integers(0, oh - S))) for _ in range(2)]
    for X0, Y0 in wins:
        y1, x1 = min((Y0 + S) * b, ch), min((X0 + S) * b, cw)
        win = canvas[Y0 * b:y1, 3 * X0 * b:3 * x1].cpu().numpy().reshape(y1 - Y0 * b, x1 - X0 * b, 3)
        cnt = count[Y0 * b:y1, X0 * b:x1].cpu().numpy().view(np.uint16)
        ref, rcov = ovr.overview_ref(win, win.shape[1], level, 2, cnt)[level - 1]
        got = out[Y0:Y0 + S, 3 * X0:3 * (X0 + S)]
        print("C3 window (%d, %d): %d of %d output pixels covered" % (X0, Y0, int((rcov > 0).sum()), S * S))
        assert np.array_equal(got, ref[:, :3 * S]), "C3 window (%d, %d): %d bytes differ" % (X0, Y0, int((got != ref[:, :3 * S]).sum()))
        assert np.array_equal(cover[Y0:Y0 + S, X0:X0 + S], rcov)
    del canvas, count
    torch.cuda.empty_cache()
    ctx.close()
