"""GPU: weighted (feather) blending (mi355_mosaic_feathered / _dev / _into, csrc/feather.hip), byte for byte against tests/feather_ref.py
(numpy on the oracle's refined render).

  * the 10-frame case of tests/test_gpu_gain.py (affine and projective frames, a skipped frame, a far-away frame, clipped boxes) at ramp 0, 1,
    16 and 1000 (longer than the frame);
  * odd pitches with poisoned padding, mixed frame sizes down to 2 x 2 and 3 x 2;
  * stripes of 1, 7 and 256 rows put side by side equal the whole canvas; a withheld frame inside the box cover is MI355_ERR_ARG, outside it fine;
  * the host form, the _into form (kept frames, a caller pitch wider than 3 cw) and the device form give the same bytes;
  * 300 frames stacked on one spot, and 65535 all-255 frames at ramp 1: the accumulators at their arithmetic limit;
  * after GainCompensateDev the canvas is the restatement on the host-LUT'd frames;
  * C3 at its own size (500 x 4000x3000): two calls, two contexts, 8 stripes, four 512 x 512 windows against the restatement.
"""
import numpy as np
import pytest

from tests import feather_ref as fr
from tests import gain_ref as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(oracle):
    from tests.test_gpu_gain import _case
    imgs, h9s, pairs = _case()
    return imgs, h9s, pairs, gr.frame_sample_maps(oracle, imgs, h9s)


def _upload(torch, imgs):
    from tests.test_gpu_gain import _upload as up
    return up(torch, imgs)


def _render_dev(ctx, torch, im, ptrs, w, h, ws, h9s, fill=7, cws=None, **kw):
    """the device form on a canvas pre-filled with `fill`: ([ch, cws] numpy, cw, ch)"""
    cw, ch, lws, _ = im.mosaic_layout(w, h, h9s)
    cws = cws or lws
    canvas = torch.full((ch, cws), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                                # the fill runs on torch's stream, the library on the ctx's own
    ctx.MosaicFeatheredDev(ptrs, w, h, ws, h9s, canvas.data_ptr(), cw, ch, cws, **kw)
    return canvas.cpu().numpy(), cw, ch


def _pix(a, cw):
    return np.ascontiguousarray(a[:, :3 * cw]).reshape(a.shape[0], cw, 3)


@pytest.mark.parametrize("ramp", [0, 1, 16, 1000])
def test_case_equals_restatement(case, oracle, ramp):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    ref, layers = fr.feather_ref(oracle, imgs, h9s, ramp, maps)
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    got, cw, ch = _render_dev(ctx, torch, im, ptrs, w, h, ws, h9s, ramp=ramp)
    assert (ch, cw) == ref.shape[:2]
    bad = (_pix(got, cw) != ref).any(axis=2)
    assert not bad.any(), "ramp %d: %d pixels differ, first %s" % (ramp, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert not got[:, 3 * cw:].any()                                        # row padding zeroed
    assert layers.max() >= 4 and (layers > 1).sum() > 10000
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
    tiny = [k for k, (w_, h_) in enumerate(sizes) if min(w_, h_) == 2 and k != 3]      # frame 3 (2 x 2, scattered) gives no pixel a sample
    assert len(tiny) == 5 and all(maps[k][1].sum() > 0 for k in tiny), [int(maps[k][1].sum()) for k in tiny]
    for shift in (0, 2):
        F = pf.PitchedFrames(imgs, pf.mixed_pitches(sizes, shift=shift), offsets=[k % 4 for k in range(len(sizes))], seed=11 + shift)
        t, ptrs = F.to_device(torch)
        w, h, ws = F.geom()
        ctx = im.Context(0)
        for ramp in (0, 5):
            ref, layers = fr.feather_ref(oracle, imgs, h9s, ramp, maps)
            got, cw, ch = _render_dev(ctx, torch, im, ptrs, w, h, ws, h9s, ramp=ramp)
            assert np.array_equal(_pix(got, cw), ref), (shift, ramp, int((_pix(got, cw) != ref).sum()))
            assert layers.max() >= 3 and (layers > 1).sum() > 10000
        assert np.array_equal(F.device_bytes(t), F.buf)                      # the frames and their padding are read only
        ctx.close()


def test_stripes_equal_the_whole_canvas(case):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    whole, cw, ch = _render_dev(ctx, torch, im, ptrs, w, h, ws, h9s)
    assert ch > 256
    cws = whole.shape[1]
    for cut in (1, 7, 256):
        canvas = torch.full((ch, cws), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for row0 in range(0, ch, cut):
            ctx.MosaicFeatheredDev(ptrs, w, h, ws, h9s, canvas.data_ptr(), cw, ch, cws, row0, min(cut, ch - row0))
        assert np.array_equal(canvas.cpu().numpy(), whole), cut
    # a stripe call writes its own rows only
    canvas = torch.full((ch, cws), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.MosaicFeatheredDev(ptrs, w, h, ws, h9s, canvas.data_ptr(), cw, ch, cws, 100, 50)
    a = canvas.cpu().numpy()
    assert np.array_equal(a[100:150], whole[100:150]) and np.all(a[:100] == 9) and np.all(a[150:] == 9)
    ctx.close()


def test_withheld_frames(case):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    whole, cw, ch = _render_dev(ctx, torch, im, ptrs, w, h, ws, h9s)
    cws = whole.shape[1]
    row0, rows = 0, 60
    need = ctx.StripeCover(w, h, h9s, row0, rows)                           # MI355_COVER_REFINED: the box cover is this render's cover
    inside, outside = np.flatnonzero(need != 0), np.flatnonzero(need == 0)
    assert len(inside) >= 3 and len(outside) >= 3 and 8 in outside            # frame 8 is skipped (h9[8] == 0)
    canvas = torch.full((ch, cws), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    held = [0 if k in outside else p for k, p in enumerate(ptrs)]
    ctx.MosaicFeatheredDev(held, w, h, ws, h9s, canvas.data_ptr(), cw, ch, cws, row0, rows)
    assert np.array_equal(canvas.cpu().numpy()[row0:row0 + rows], whole[row0:row0 + rows])
    for strict in (0, 1):
        ctx.set_option("strict_frames", strict)
        for k in inside:
            held = list(ptrs)
            held[k] = 0
            with pytest.raises(im.Mi355Error) as e:
                ctx.MosaicFeatheredDev(held, w, h, ws, h9s, canvas.data_ptr(), cw, ch, cws, row0, rows)
            assert e.value.code == -1 and "image %d" % k in str(e.value), str(e.value)
    with pytest.raises(im.Mi355Error) as e:
        ctx.MosaicFeatheredDev(ptrs, w, h, ws, h9s, canvas.data_ptr(), cw, ch, cws, ramp=-1)
    assert e.value.code == -1 and "ramp=-1" in str(e.value)
    with pytest.raises(im.Mi355Error) as e:
        ctx.MosaicFeathered(imgs[:1], h9s[:1])
    assert e.value.code == -2                                               # n <= 1, as mi355_mosaic_refined
    got, _, _ = _render_dev(ctx, torch, im, ptrs, w, h, ws, h9s)            # the ctx still works after the refusals
    assert np.array_equal(got, whole)
    ctx.close()


def test_host_into_and_device_forms_agree(case, oracle):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    n = len(imgs)
    ref, _ = fr.feather_ref(oracle, imgs, h9s, 16, maps)
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    dev, cw, ch = _render_dev(ctx, torch, im, ptrs, w, h, ws, h9s, ramp=16)
    assert np.array_equal(_pix(dev, cw), ref)
    host, cw2, ch2, cws2 = ctx.MosaicFeathered(imgs, h9s, ramp=16)
    assert (cw2, ch2) == (cw, ch) and np.array_equal(host, dev)
    # _into: host sources, a caller pitch wider than 3 cw whose tail stays as it is
    pitch = 3 * cw + 29
    out = np.full((ch, pitch), 201, np.uint8)
    out, cw3, ch3 = ctx.MosaicFeatheredInto(imgs, None, h9s, out=out, ramp=16)
    assert (cw3, ch3) == (cw, ch) and np.array_equal(_pix(out, cw), ref) and np.all(out[:, 3 * cw:] == 201)
    # _into: kept frames (the caller's arrays hold garbage by the time of the render), and a mix of both sources
    ctx.set_option("keep_frames", 1)
    for k in range(n):
        ctx.SiftExtractHost(k, imgs[k].copy())
    ctx.synchronize()
    ids = np.arange(n, dtype=np.int32)
    garbage = [np.full_like(f, 77) for f in imgs]
    out, _, _ = ctx.MosaicFeatheredInto(garbage, ids, h9s, ramp=16)
    assert np.array_equal(_pix(out, cw), ref)
    mixed = np.where(ids % 2 == 0, ids, -1).astype(np.int32)
    out, _, _ = ctx.MosaicFeatheredInto([None if mixed[k] >= 0 else imgs[k] for k in range(n)], mixed, h9s, ramp=16)
    assert np.array_equal(_pix(out, cw), ref)
    ctx.close()


def test_heavy_overlap(oracle):
    """300 small frames on one spot: weighted sums far beyond 16 bits"""
    import torch
    import imagemosaicing_amd as im
    from tests.synth import texture
    rng = np.random.default_rng(12)
    n = 300
    imgs = [texture(24, 20, seed=200 + k) for k in range(n)]
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (n, 1))
    h9s[:, 2] = rng.integers(0, 7, n)
    h9s[:, 5] = rng.integers(0, 5, n)
    h9s[1::3, 0] = 1.05
    ref, layers = fr.feather_ref(oracle, imgs, h9s, 0)
    assert layers.max() > 250
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    got, cw, ch = _render_dev(ctx, torch, im, ptrs, w, h, ws, h9s)
    assert np.array_equal(_pix(got, cw), ref), int((_pix(got, cw) != ref).sum())
    ctx.close()


def test_accumulators_hold_at_the_arithmetic_limit():
    """65535 all-255 frames on one spot at ramp 1: omega = 255 wherever the four texels lie off the border, so a pixel's sums reach
    65535 * 255 * 255 + 65535 * 255 / 2 = 4 269 748 612 < 2^32.  The mean of equal samples is the sample: every covered byte is 255."""
    import torch
    import imagemosaicing_amd as im
    n = 65535
    frame = torch.full((8, 24), 255, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w, h, ws = [8] * n, [8] * n, [24] * n
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (n, 1))
    ctx = im.Context(0)
    got, cw, ch = _render_dev(ctx, torch, im, [frame.data_ptr()] * n, w, h, ws, h9s, ramp=1)
    assert (cw, ch) == (8, 8)
    want = np.zeros((8, 8, 3), np.uint8)
    want[:7, :7] = 255                                                      # samples exist on [0, w - 1) x [0, h - 1)
    assert np.array_equal(_pix(got, cw), want)
    ctx.close()


def test_after_gain_compensation(case, oracle):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    g = ctx.GainCompensateDev(ptrs, w, h, ws, h9s, pairs, step=4)
    assert not np.all(g == 1.0)
    lutd = [gr.apply_lut(imgs[k], g[k]) for k in range(len(imgs))]
    ref, _ = fr.feather_ref(oracle, lutd, h9s, 0)
    got, cw, ch = _render_dev(ctx, torch, im, ptrs, w, h, ws, h9s)
    assert np.array_equal(_pix(got, cw), ref)
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
    cw, ch, cws, _ = im.mosaic_layout(wv, hv, h9s)
    whole = torch.full((ch, cws), 7, dtype=torch.uint8, device="cuda")
    other = torch.full((ch, cws), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    c1.MosaicFeatheredDev(ptrs, wv, hv, wsv, h9s, whole.data_ptr(), cw, ch, cws)
    c1.MosaicFeatheredDev(ptrs, wv, hv, wsv, h9s, other.data_ptr(), cw, ch, cws)
    assert torch.equal(whole, other), "C3: two calls differ"
    other.fill_(9)
    torch.cuda.synchronize()
    c2.MosaicFeatheredDev(ptrs, wv, hv, wsv, h9s, other.data_ptr(), cw, ch, cws)
    assert torch.equal(whole, other), "C3: two contexts differ"
    other.fill_(9)
    torch.cuda.synchronize()
    G = 8
    for r in range(G):
        row0 = (ch * r) // G
        c1.MosaicFeatheredDev(ptrs, wv, hv, wsv, h9s, other.data_ptr(), cw, ch, cws, row0, (ch * (r + 1)) // G - row0)
    assert torch.equal(whole, other), "C3: 8 stripes differ from the whole canvas"
    del other
    rng = np.random.default_rng(31)
    S = 512
    wins = [(int(rng.integers(0, cw - S)), int(rng.integers(0, ch - S))) for _ in range(4)]
    for x0, y0 in wins:
        ref, nsub = fr.window_ref(orc, lambda k: host_image(frames, k, W, H, ws), W, H, h9s, (x0, y0, S, S), 0, threads=4)
        got = whole[y0:y0 + S, 3 * x0:3 * (x0 + S)].cpu().numpy().reshape(S, S, 3)
        print("C3 window (%d, %d): %d frames rendered" % (x0, y0, nsub))
        assert nsub >= 1 and np.array_equal(got, ref), "C3 window (%d, %d): %d bytes differ (%d frames)" % (x0, y0, int((got != ref).sum()), nsub)
    del whole, frames
    torch.cuda.empty_cache()
    c1.close(); c2.close()
