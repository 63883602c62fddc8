"""GPU: the seamline render (mi355_mosaic_seamline / _dev / _into / _cover, csrc/seamline.hip): canvas, owner map and count map byte for byte
against tests/seamline_ref.py (numpy on the oracle's refined render).

  * the reference's committed 20-frame run (tests/golden, decimated) at ramp 0, 1, 16 and 1000 (longer than the frame), and after
    GainCompensateDev; the 10-frame case of tests/test_gpu_gain.py (projective frames, a skipped frame, a far-away frame);
  * odd pitches with poisoned padding, mixed frame sizes down to 2 x 2 and 3 x 2 (tests/pitched.py);
  * stripes of 1, 7 and 256 rows put side by side equal the whole canvas, for all three outputs; a stripe writes its own rows only;
  * the host form, the _into form (kept frames and host images mixed, a caller pitch wider than 3 cw) and the device form agree;
  * withheld frames: NULL for every frame that owns nothing gives the same bytes, NULL for an owner is MI355_ERR_ARG naming it and the ctx
    goes on working; SeamlineCover is unique(owner) - 1 of the rows; d_canvas == NULL with d_imgs == NULL gives the same maps;
  * the built tie (the index decides), 300 frames stacked on one spot, every refusal of the header;
  * C3 at its own size (500 x 4000x3000): two calls, two contexts, 8 stripes, 512 x 512 windows against the restatement.
"""
import numpy as np
import pytest

from tests import gain_ref as gr
from tests import seamline_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(oracle):
    imgs, h9s = sr.golden_survey()
    return imgs, h9s, gr.frame_sample_maps(oracle, imgs, h9s)


@pytest.fixture(scope="module")
def case(oracle):
    from tests.test_gpu_gain import _case
    imgs, h9s, pairs = _case()
    return imgs, h9s, pairs, gr.frame_sample_maps(oracle, imgs, h9s)


def _upload(torch, imgs):
    from tests.test_gpu_gain import _upload as up
    return up(torch, imgs)


class Out:
    """device canvas [ch, cws] uint8 and maps [ch, cw] (int16 storage, read as uint16), pre-filled so that unwritten bytes show"""
    def __init__(self, torch, im, w, h, h9s, cws=None, canvas=True, owner=True, count=True):
        self.cw, self.ch, lws, _ = im.mosaic_layout(w, h, h9s)
        self.cws = cws or lws
        self.canvas = torch.full((self.ch, self.cws), 7, dtype=torch.uint8, device="cuda") if canvas else None
        self.owner = torch.full((self.ch, self.cw), 0x5555, dtype=torch.int16, device="cuda") if owner else None
        self.count = torch.full((self.ch, self.cw), 0x5555, dtype=torch.int16, device="cuda") if count else None
        torch.cuda.synchronize()                                            # the fills run on torch's stream, the library on the ctx's own

    def render(self, ctx, ptrs, w, h, ws, h9s, row0=0, rows=-1, **kw):
        ctx.MosaicSeamlineDev(ptrs, w, h, ws, h9s, self.canvas.data_ptr() if self.canvas is not None else 0, self.cw, self.ch, self.cws, row0, rows,
                              d_owner=self.owner.data_ptr() if self.owner is not None else 0,
                              d_count=self.count.data_ptr() if self.count is not None else 0, **kw)
        return self

    def host(self):
        m = lambda t: None if t is None else t.cpu().numpy().view(np.uint16)
        return (None if self.canvas is None else self.canvas.cpu().numpy()), m(self.owner), m(self.count)


def _pix(a, cw):
    return np.ascontiguousarray(a[:, :3 * cw]).reshape(a.shape[0], cw, 3)


def _same(got, ref, cw, what=""):
    canvas, owner, count = got
    for name, a, b in (("count", count, ref[2]), ("owner", owner, ref[1]), ("canvas", _pix(canvas, cw), ref[0])):
        bad = (a != b)
        bad = bad.any(axis=2) if bad.ndim == 3 else bad
        assert a.shape == b.shape and not bad.any(), "%s %s: %d pixels differ, first %s" % (what, name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert not canvas[:, 3 * cw:].any()                                     # row padding zeroed


@pytest.mark.parametrize("ramp", [0, 1, 16, 1000])
def test_golden_equals_restatement(golden, oracle, ramp):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, maps = golden
    ref = sr.seamline_ref(oracle, imgs, h9s, ramp, maps)
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, ramp=ramp)
    assert (o.ch, o.cw) == ref[0].shape[:2]
    _same(o.host(), ref, o.cw, "ramp %d" % ramp)
    assert ref[2].max() >= 4 and (ref[2] >= 3).sum() > 10000
    # a caller's wider row: the padding is cleared up to cws
    o2 = Out(torch, im, w, h, h9s, cws=o.cws + 32).render(ctx, ptrs, w, h, ws, h9s, ramp=ramp)
    _same(o2.host(), ref, o.cw, "wide rows, ramp %d" % ramp)
    ctx.close()


@pytest.mark.parametrize("ramp", [0, 16])
def test_case_equals_restatement(case, oracle, ramp):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    ref = sr.seamline_ref(oracle, imgs, h9s, ramp, maps)
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, ramp=ramp)
    _same(o.host(), ref, o.cw, "ramp %d" % ramp)
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
    for shift in (0, 2):
        F = pf.PitchedFrames(imgs, pf.mixed_pitches(sizes, shift=shift), offsets=[k % 4 for k in range(len(sizes))], seed=11 + shift)
        t, ptrs = F.to_device(torch)
        w, h, ws = F.geom()
        ctx = im.Context(0)
        for ramp in (0, 5):
            ref = sr.seamline_ref(oracle, imgs, h9s, ramp, maps)
            o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, ramp=ramp)
            _same(o.host(), ref, o.cw, "shift %d ramp %d" % (shift, ramp))
            assert ref[2].max() >= 3 and (ref[2] > 1).sum() > 10000
        assert np.array_equal(F.device_bytes(t), F.buf)                      # the frames and their padding are read only
        ctx.close()


def test_after_gain_compensation(golden, oracle):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, maps = golden
    pairs = [(k, k + 1) for k in range(len(imgs) - 1)]
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    g = ctx.GainCompensateDev(ptrs, w, h, ws, h9s, pairs, step=4)
    assert not np.all(g == 1.0)
    lutd = [gr.apply_lut(imgs[k], g[k]) for k in range(len(imgs))]
    ref = sr.seamline_ref(oracle, lutd, h9s, 0)
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s)
    _same(o.host(), ref, o.cw, "compensated")
    ctx.close()


def test_stripes_equal_the_whole_canvas(golden):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, maps = golden
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
    for a, b, fill in zip(o.host(), whole, (7, 0x5555, 0x5555)):
        assert np.array_equal(a[100:150], b[100:150]) and np.all(a[:100] == fill) and np.all(a[150:] == fill)
    ctx.close()


def test_host_into_and_device_forms_agree(case, oracle):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    n = len(imgs)
    ref = sr.seamline_ref(oracle, imgs, h9s, 16, maps)
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s, ramp=16)
    dev = o.host()
    cw, ch = o.cw, o.ch
    _same(dev, ref, cw)
    host, cw2, ch2, cws2, own = ctx.MosaicSeamline(imgs, h9s, ramp=16, want_owner=True)
    assert (cw2, ch2) == (cw, ch) and np.array_equal(host, dev[0]) and np.array_equal(own, ref[1])
    host2, _, _, _ = ctx.MosaicSeamline(imgs, h9s, ramp=16)
    assert np.array_equal(host2, host)
    # _into: host sources, a caller pitch wider than 3 cw whose tail stays as it is
    pitch = 3 * cw + 29
    out = np.full((ch, pitch), 201, np.uint8)
    out, cw3, ch3 = ctx.MosaicSeamlineInto(imgs, None, h9s, out=out, ramp=16)
    assert (cw3, ch3) == (cw, ch) and np.array_equal(_pix(out, cw), ref[0]) and np.all(out[:, 3 * cw:] == 201)
    # _into: kept frames (the caller's arrays hold garbage by the time of the render), and a mix of both sources
    ctx.set_option("keep_frames", 1)
    for k in range(n):
        ctx.SiftExtractHost(k, imgs[k].copy())
    ctx.synchronize()
    ids = np.arange(n, dtype=np.int32)
    garbage = [np.full_like(f, 77) for f in imgs]
    out, _, _ = ctx.MosaicSeamlineInto(garbage, ids, h9s, ramp=16)
    assert np.array_equal(_pix(out, cw), ref[0])
    mixed = np.where(ids % 2 == 0, ids, -1).astype(np.int32)
    out, _, _ = ctx.MosaicSeamlineInto([None if mixed[k] >= 0 else imgs[k] for k in range(n)], mixed, h9s, ramp=16)
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
    """300 small frames on one spot, as the feather tests build them: dozens of frames per pixel, most of which own nothing"""
    import torch
    import imagemosaicing_amd as im
    imgs, h9s = _heavy()
    n = len(imgs)
    ref = sr.seamline_ref(oracle, imgs, h9s, 0)
    assert ref[2].max() > 250
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s)
    whole = o.host()
    _same(whole, ref, o.cw, "heavy")
    owners = np.unique(ref[1][ref[1] > 0]).astype(int) - 1
    need = ctx.SeamlineCover(w, h, h9s)
    assert np.array_equal(np.flatnonzero(need), owners)
    idle = [k for k in range(n) if not need[k]]
    assert len(idle) > 100 and ctx.StripeCover(w, h, h9s, 0, o.ch)[idle].all()          # their boxes do meet the rows: they lose every pixel
    # NULL for every frame that owns nothing: the same bytes
    held = [0 if not need[k] else p for k, p in enumerate(ptrs)]
    _same(Out(torch, im, w, h, h9s).render(ctx, held, w, h, ws, h9s).host(), ref, o.cw, "non-owners withheld")
    # NULL for one owner: refused, naming it, before anything is written; the ctx goes on working
    for k in (int(owners[0]), int(owners[len(owners) // 2]), int(owners[-1])):
        bad = list(held)
        bad[k] = 0
        o2 = Out(torch, im, w, h, h9s)
        with pytest.raises(im.Mi355Error) as e:
            o2.render(ctx, bad, w, h, ws, h9s)
        assert e.value.code == -1 and "image %d " % k in str(e.value), str(e.value)
        assert all(np.all(a == fill) for a, fill in zip(o2.host(), (7, 0x5555, 0x5555)))
        _same(Out(torch, im, w, h, h9s).render(ctx, held, w, h, ws, h9s).host(), ref, o.cw, "after the refusal")
    ctx.close()


def test_cover_and_maps_without_frames(case):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    o = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s)
    canvas, owner, count = o.host()
    ch = o.ch
    for row0, rows in ((0, ch), (0, 60), (100, 1), (37, 200), (ch - 5, 5), (250, 300)):
        need = ctx.SeamlineCover(w, h, h9s, row0, rows)
        want = np.unique(owner[row0:row0 + rows]).astype(int)
        want = want[want > 0] - 1
        assert np.array_equal(np.flatnonzero(need), want), (row0, rows)
        assert not need[8]                                                  # skipped (h9[8] == 0)
        # NULL for everything outside the cover
        held = [p if need[k] else 0 for k, p in enumerate(ptrs)]
        s = Out(torch, im, w, h, h9s).render(ctx, held, w, h, ws, h9s, row0, rows).host()
        for a, b in zip(s, (canvas, owner, count)):
            assert np.array_equal(a[row0:row0 + rows], b[row0:row0 + rows]), (row0, rows)
    assert np.array_equal(ctx.SeamlineCover(w, h, h9s, ramp=16), ctx.SeamlineCover(w, h, h9s, 0, ch, ramp=16))
    # d_canvas == NULL: nothing is sampled; d_imgs and ws may be NULL altogether; either map alone
    m = Out(torch, im, w, h, h9s, canvas=False).render(ctx, None, w, h, None, h9s).host()
    assert np.array_equal(m[1], owner) and np.array_equal(m[2], count)
    m = Out(torch, im, w, h, h9s, canvas=False, count=False).render(ctx, None, w, h, None, h9s).host()
    assert np.array_equal(m[1], owner)
    m = Out(torch, im, w, h, h9s, canvas=False, owner=False).render(ctx, [0] * len(w), w, h, ws, h9s).host()
    assert np.array_equal(m[2], count)
    m = Out(torch, im, w, h, h9s, owner=False, count=False).render(ctx, ptrs, w, h, ws, h9s).host()
    assert np.array_equal(m[0], canvas)
    ctx.close()


def test_the_index_decides_a_built_tie(oracle):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, xm = sr.tie_case()
    ctx = im.Context(0)
    for order in ([0, 1], [1, 0]):
        ii, hh = [imgs[k] for k in order], h9s[order]
        ref = sr.seamline_ref(oracle, ii, hh, 0, full=True)
        assert ref[4][32, xm] and ref[1][32, xm] == 2
        ts, ptrs, w, h, ws = _upload(torch, ii)
        o = Out(torch, im, w, h, hh).render(ctx, ptrs, w, h, ws, hh)
        _same(o.host(), ref[:3], o.cw, "order %s" % order)
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
    err(lambda: ctx.SeamlineCover(w, h, h9s, ramp=-3), -1, "ramp=-3")
    err(lambda: ctx.MosaicSeamline(imgs, h9s, ramp=-1), -1, "ramp=-1")
    err(lambda: ctx.MosaicSeamlineInto(imgs, None, h9s, ramp=-1), -1, "ramp=-1")
    # all three outputs NULL; a canvas without frames
    err(lambda: ctx.MosaicSeamlineDev(ptrs, w, h, ws, h9s, 0, o.cw, o.ch, o.cws), -1, "all NULL")
    err(lambda: ctx.MosaicSeamlineDev(None, w, h, ws, h9s, o.canvas.data_ptr(), o.cw, o.ch, o.cws), -1, "d_imgs")
    # a canvas geometry that is not the layout's
    err(lambda: ctx.MosaicSeamlineDev(ptrs, w, h, ws, h9s, o.canvas.data_ptr(), o.cw + 1, o.ch, o.cws), -1, "canvas geometry")
    err(lambda: ctx.MosaicSeamlineDev(ptrs, w, h, ws, h9s, o.canvas.data_ptr(), o.cw, o.ch - 1, o.cws), -1, "canvas geometry")
    err(lambda: ctx.MosaicSeamlineDev(ptrs, w, h, ws, h9s, o.canvas.data_ptr(), o.cw, o.ch, 3 * o.cw - 4), -1, "canvas geometry")
    err(lambda: ctx.MosaicSeamlineDev(None, w, h, None, h9s, 0, o.cw + 1, o.ch, o.cws, d_count=o.count.data_ptr()), -1, "canvas geometry")
    # frame geometry: a pitch below 3 w, a side beyond 2^20
    bad_ws = list(ws)
    bad_ws[1] = 3 * w[1] - 1
    err(lambda: o.render(ctx, ptrs, w, h, bad_ws, h9s), -1, "bad image geometry")
    big_w = [(1 << 20) + 1, 4]
    big_h9 = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    err(lambda: ctx.SeamlineCover(big_w, [2, 2], big_h9), -1, "bad image geometry")
    # the frame limit
    big = 65536
    err(lambda: ctx.SeamlineCover([8] * big, [8] * big, np.tile(np.eye(3, dtype=np.float32).reshape(9), (big, 1))), -1, "65535")
    # n <= 1 in the host forms, as mi355_mosaic_refined
    err(lambda: ctx.MosaicSeamline(imgs[:1], h9s[:1]), -2)
    err(lambda: ctx.MosaicSeamlineInto(imgs[:1], None, h9s[:1]), -2)
    # _into: a destination that is not the layout's
    err(lambda: ctx.MosaicSeamlineInto(imgs, None, h9s, out=np.zeros((o.ch, 3 * o.cw - 3), np.uint8), pitch=3 * o.cw - 3), -1, "dst_pitch")
    assert all(np.all(a == fill) for a, fill in zip(o.host(), (7, 0x5555, 0x5555)))      # no refusal wrote anything
    got = Out(torch, im, w, h, h9s).render(ctx, ptrs, w, h, ws, h9s).host()  # the ctx still works after the refusals
    assert all(np.array_equal(a, b) for a, b in zip(got, whole))
    ctx.close()


def test_c3_full_size():
    import torch
    import imagemosaicing_amd as im
    from tests import oracle_lib as ol
    from tests.synth_survey import frame_layout, host_image
    from tests.test_gpu_gain import _h9s, _render
    orc = ol.load_oracle_fast()
    W, H, F = 4000, 3000, 500
    c1, c2 = im.Context(0), im.Context(0)
    A, gains = frame_layout(F, W, H)
    frames, ws = _render(c1, torch, A, gains, W, H)
    h9s = _h9s(A)
    ptrs = [frames[k].data_ptr() for k in range(F)]
    wv, hv, wsv = [W] * F, [H] * F, [ws] * F
    a = Out(torch, im, wv, hv, h9s).render(c1, ptrs, wv, hv, wsv, h9s)
    b = Out(torch, im, wv, hv, h9s).render(c1, ptrs, wv, hv, wsv, h9s)
    same = lambda x, y: torch.equal(x.canvas, y.canvas) and torch.equal(x.owner, y.owner) and torch.equal(x.count, y.count)
    assert same(a, b), "C3: two calls differ"
    del b
    b = Out(torch, im, wv, hv, h9s).render(c2, ptrs, wv, hv, wsv, h9s)
    assert same(a, b), "C3: two contexts differ"
    del b
    b = Out(torch, im, wv, hv, h9s)
    G, cw, ch = 8, a.cw, a.ch
    need_all = np.zeros(F, bool)
    for r in range(G):
        row0 = (ch * r) // G
        rows = (ch * (r + 1)) // G - row0
        need = c1.SeamlineCover(wv, hv, h9s, row0, rows)
        need_all |= need != 0
        b.render(c1, [p if need[k] else 0 for k, p in enumerate(ptrs)], wv, hv, wsv, h9s, row0, rows)
    assert same(a, b), "C3: 8 stripes (each given its cover only) differ from the whole canvas"
    del b
    owners = torch.unique(a.owner).cpu().numpy().view(np.uint16).astype(int)
    assert np.array_equal(np.flatnonzero(need_all), np.sort(owners[owners > 0]) - 1)
    rng = np.random.default_rng(31)
    S = 512
    wins = [(int(rng.integers(0, cw - S)), int(rng.integers(0, ch - S))) for _ in range(3)]
    for x0, y0 in wins:
        ref, rown, rcnt, nsub = sr.window_ref(orc, lambda k: host_image(frames, k, W, H, ws), W, H, h9s, (x0, y0, S, S), 0, threads=8)
        got = a.canvas[y0:y0 + S, 3 * x0:3 * (x0 + S)].cpu().numpy().reshape(S, S, 3)
        gown = a.owner[y0:y0 + S, x0:x0 + S].cpu().numpy().view(np.uint16)
        gcnt = a.count[y0:y0 + S, x0:x0 + S].cpu().numpy().view(np.uint16)
        print("C3 window (%d, %d): %d frames rendered, up to %d per pixel" % (x0, y0, nsub, int(rcnt.max())))
        assert nsub >= 1 and np.array_equal(gcnt, rcnt), "C3 window (%d, %d): %d counts differ" % (x0, y0, int((gcnt != rcnt).sum()))
        assert np.array_equal(gown, rown), "C3 window (%d, %d): %d owners differ" % (x0, y0, int((gown != rown).sum()))
        assert np.array_equal(got, ref), "C3 window (%d, %d): %d bytes differ (%d frames)" % (x0, y0, int((got != ref).sum()), nsub)
    del a, frames
    torch.cuda.empty_cache()
    c1.close(); c2.close()
