"""GPU: exposure gain compensation (mi355_gain_stats_dev / mi355_apply_gains_dev / mi355_gain_compensate_dev, csrc/gain.hip).

  * stats: equal to tests/gain_ref.py (samples and cover from the oracle's refined render) on 10 frames of 320x240 at step 1, 4 and 8:
    affine and projective frames, a skipped frame (h9[8] = 0), a listed pair without overlap, boxes clipped at the canvas edge;
  * apply: the numpy LUT byte for byte, out of place and in place, pitch padding untouched;
  * canvas identity: the refined and blended renders of the compensated frames equal the renders of the host-LUT'd frames;
  * ground truth: 40 frames of 1280x960 with known gains in [0.85, 1.15];
  * determinism across calls and contexts; C3 at full size (500 x 4000x3000).
"""
import numpy as np
import pytest

from tests import gain_ref as gr

pytestmark = pytest.mark.gpu


def _case():
    from tests.synth import texture, warp_cases
    Hs = warp_cases()
    n = 10
    imgs = [(texture(320, 240, 40 + k).astype(np.float64) * (0.88 + 0.03 * k)).clip(0, 255).astype(np.uint8) for k in range(n)]
    h9s = np.zeros((n, 9), np.float32)
    off = [(0, 0), (140, 10), (280, -20), (60, 150), (200, 170), (330, 140), (-40, 90), (120, 60), (250, 90), (2000, 0)]
    for k in range(n):
        h9s[k] = Hs[[0, 2, 1, 3, 4, 5, 2, 3, 1, 0][k]]
        h9s[k, 2] += off[k][0]
        h9s[k, 5] += off[k][1]
    h9s[8, 8] = 0.0                                         # skipped by the render
    pairs = [(0, 1), (1, 2), (0, 3), (3, 4), (4, 5), (1, 4), (2, 5), (0, 6), (6, 3), (7, 0), (7, 1), (7, 4), (3, 7), (8, 7), (0, 9), (5, 9), (2, 8)]
    return imgs, h9s, pairs


@pytest.fixture(scope="module")
def case(oracle):
    imgs, h9s, pairs = _case()
    return imgs, h9s, pairs, gr.frame_sample_maps(oracle, imgs, h9s)


def _upload(torch, imgs, pad=0, fill=None):
    """device copies [h, 3w + pad] of host images (pad bytes set to `fill` or 0); returns (tensors, ptrs, w, h, ws)"""
    ts = []
    for im_ in imgs:
        h, w = im_.shape[:2]
        a = np.full((h, 3 * w + pad), 0 if fill is None else fill, np.uint8)
        a[:, :3 * w] = im_.reshape(h, 3 * w)
        ts.append(torch.from_numpy(a).cuda())
    torch.cuda.synchronize()
    w = [i.shape[1] for i in imgs]; h = [i.shape[0] for i in imgs]; ws = [t.shape[1] for t in ts]
    return ts, [t.data_ptr() for t in ts], w, h, ws


def _host(t, w):
    a = t.cpu().numpy()
    return a[:, :3 * w].reshape(a.shape[0], w, 3)


@pytest.mark.parametrize("step", [1, 4, 8])
def test_stats_equal_restatement(case, step):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    st, cover = ctx.GainStatsDev(ptrs, w, h, ws, h9s, pairs, step)
    recs, cov_ref = gr.stats_ref(maps, pairs, step)
    assert np.array_equal(cover, cov_ref), (cover, cov_ref)
    for i, (a, b) in enumerate(pairs):
        nn, sa, sb = recs[i]
        assert (st[i]["a"], st[i]["b"]) == (a, b)
        assert st[i]["n"] == nn and np.array_equal(st[i]["sum_a"], sa) and np.array_equal(st[i]["sum_b"], sb), (i, a, b, st[i], recs[i])
    # the case covers what it claims: a skipped frame, a listed pair without overlap, overlapping pairs, clipped boxes
    assert cover[8] == 0 and st[pairs.index((0, 9))]["n"] == 0 and st[pairs.index((8, 7))]["n"] == 0
    assert sum(int(r[0] > 0) for r in recs) >= 10
    ctx.close()


def test_apply_equals_lut(case):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    ctx = im.Context(0)
    n = len(imgs)
    rng = np.random.default_rng(3)
    g = rng.uniform(0.7, 1.4, (n, 3)).astype(np.float32)
    g[2] = 1.0
    g[5] = [0.0, 3.0, 1.0]                                     # clamps at both ends
    src, sp, w, h, ws = _upload(torch, imgs, pad=13, fill=77)   # odd pitch: rows start unaligned
    dst, dp, _, _, _ = _upload(torch, [np.zeros_like(i) for i in imgs], pad=13, fill=201)
    ctx.ApplyGainsDev(sp, dp, w, h, ws, g)
    for k in range(n):
        a = dst[k].cpu().numpy()
        assert np.array_equal(_host(dst[k], w[k]), gr.apply_lut(imgs[k], g[k])), k
        assert np.all(a[:, 3 * w[k]:] == 201), k                 # pitch padding untouched
        assert np.array_equal(_host(src[k], w[k]), imgs[k])     # source unchanged
    # in place
    ctx.ApplyGainsDev(sp, sp, w, h, ws, g)
    for k in range(n):
        assert np.array_equal(_host(src[k], w[k]), gr.apply_lut(imgs[k], g[k])), k
        assert np.all(src[k].cpu().numpy()[:, 3 * w[k]:] == 77)
    # aligned pitch (the 16-byte path for whole rows)
    src2, sp2, w2, h2, ws2 = _upload(torch, imgs, pad=64 - (3 * 320) % 64)
    ctx.ApplyGainsDev(sp2, sp2, w2, h2, ws2, g)
    for k in range(n):
        assert np.array_equal(_host(src2[k], w2[k]), gr.apply_lut(imgs[k], g[k])), k
    # ragged frames in one launch: rows shorter than the 16-byte head, heights off the 16-row blocks, unequal block counts, mixed pitches
    # and base pointers (tests/pitched.py; padding and the gaps between frames are garbage that must stay as it is)
    from tests import pitched as pf
    from tests.synth import texture
    sizes = [(1, 1), (2, 17), (5, 15), (7, 241), (320, 33), (333, 257)]
    rimgs = [texture(w, h, seed=60 + k) for k, (w, h) in enumerate(sizes)]
    rg = rng.uniform(0.6, 1.5, (len(sizes), 3)).astype(np.float32)
    pitches = [pf.pitch_kinds(w)[k % 5] for k, (w, h) in enumerate(sizes)]
    fs = pf.PitchedFrames(rimgs, pitches, offsets=[k % 4 for k in range(len(sizes))], seed=7)
    fd = pf.PitchedFrames([np.zeros_like(i) for i in rimgs], pitches, offsets=[(k + 1) % 4 for k in range(len(sizes))], seed=8)
    ts, sp3 = fs.to_device(torch)
    td, dp3 = fd.to_device(torch)
    rw, rh, rws = fs.geom()
    pix_s, pix_d = np.zeros(fs.nbytes, bool), np.zeros(fd.nbytes, bool)
    for k in range(len(sizes)):
        fs.view(k, pix_s)[:, :fs.row_bytes(k)] = True
        fd.view(k, pix_d)[:, :fd.row_bytes(k)] = True
    ctx.ApplyGainsDev(sp3, dp3, rw, rh, rws, rg)
    got_s, got_d = fs.device_bytes(ts), fd.device_bytes(td)
    for k in range(len(sizes)):
        assert np.array_equal(fd.pixels(k, got_d), gr.apply_lut(rimgs[k], rg[k])), sizes[k]
    assert np.array_equal(got_d[~pix_d], fd.buf[~pix_d]) and np.array_equal(got_s, fs.buf)
    ctx.ApplyGainsDev(sp3, sp3, rw, rh, rws, rg)
    got_s = fs.device_bytes(ts)
    for k in range(len(sizes)):
        assert np.array_equal(fs.pixels(k, got_s), gr.apply_lut(rimgs[k], rg[k])), sizes[k]
    assert np.array_equal(got_s[~pix_s], fs.buf[~pix_s])
    ctx.close()


def test_canvas_identity(case, oracle):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    g = ctx.GainCompensateDev(ptrs, w, h, ws, h9s, pairs, step=4)
    assert np.all(g[8] == 1.0) and not np.all(g == 1.0)
    lutd = [gr.apply_lut(imgs[k], g[k]) for k in range(len(imgs))]
    for k in range(len(imgs)):
        assert np.array_equal(_host(ts[k], w[k]), lutd[k]), k
    cw, ch, cws, _ = im.mosaic_layout(w, h, h9s)
    canvas = torch.empty((ch, cws), dtype=torch.uint8, device="cuda")
    ctx.MosaicImagesRefinedDev(ptrs, w, h, ws, h9s, canvas.data_ptr(), cw, ch, cws)
    ctx.synchronize()
    rc, ref = oracle.mosaic_images_refined(lutd, h9s)
    assert rc == 0 and np.array_equal(canvas.cpu().numpy()[:, :3 * cw], ref[0][:, :3 * cw])
    # blended: the GPU's own blended render of the host-LUT'd frames
    t2, p2, _, _, _ = _upload(torch, lutd)
    b1, bw, _, _ = ctx.MosaicBlendedDev(ptrs, w, h, ws, h9s)
    b2, _, _, _ = ctx.MosaicBlendedDev(p2, w, h, ws, h9s)
    assert np.array_equal(b1.cpu().numpy()[:, :3 * bw], b2.cpu().numpy()[:, :3 * bw])
    ctx.close()


def test_determinism_and_second_context(case):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    c1, c2 = im.Context(0), im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    s1, v1 = c1.GainStatsDev(ptrs, w, h, ws, h9s, pairs, 2)
    s2, v2 = c1.GainStatsDev(ptrs, w, h, ws, h9s, pairs, 2)
    s3, v3 = c2.GainStatsDev(ptrs, w, h, ws, h9s, pairs, 2)
    assert s1.tobytes() == s2.tobytes() == s3.tobytes() and np.array_equal(v1, v2) and np.array_equal(v1, v3)
    g1 = im.solve_gains(s1, v1)
    assert im.solve_gains(s3, v3).tobytes() == g1.tobytes()
    a, pa, _, _, _ = _upload(torch, imgs)
    b, pb, _, _, _ = _upload(torch, imgs)
    ga = c1.GainCompensateDev(pa, w, h, ws, h9s, pairs, step=2)
    gb = c2.GainCompensateDev(pb, w, h, ws, h9s, pairs, step=2)
    assert ga.tobytes() == gb.tobytes() == g1.tobytes()
    c1.close(); c2.close()


def test_argument_errors(case):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, maps = case
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)

    def err(fn, match):
        with pytest.raises(im.Mi355Error) as e:
            fn()
        assert e.value.code == -1 and match in str(e.value), str(e.value)

    err(lambda: ctx.GainStatsDev(ptrs, w, h, ws, h9s, [(1, 1)]), "pair 0 (1, 1): a == b")
    err(lambda: ctx.GainStatsDev(ptrs, w, h, ws, h9s, [(0, 1), (2, 10)]), "pair 1 (2, 10): position outside [0, 10)")
    err(lambda: ctx.GainStatsDev(ptrs, w, h, ws, h9s, [(0, 1), (1, 0)]), "pair 1 (1, 0) repeats pair 0")
    err(lambda: ctx.GainStatsDev(ptrs, w, h, ws, h9s, pairs, 0), "step=0")
    err(lambda: ctx.GainStatsDev(ptrs, w, h, ws, h9s, pairs, 65), "step=65")
    err(lambda: ctx.GainCompensateDev(ptrs, w, h, ws, h9s, pairs, channels=2), "channels=2")
    err(lambda: ctx.GainCompensateDev(ptrs, w, h, ws, h9s, pairs, sigma_n=0.0), "sigma_n=")
    err(lambda: ctx.GainCompensateDev(ptrs, w, h, ws, h9s, pairs, sigma_g=-0.1), "sigma_g=")
    err(lambda: ctx.GainCompensateDev(ptrs, w, h, ws, h9s, pairs, step=100), "step=100")
    big = 65536
    err(lambda: ctx.GainStatsDev([ptrs[0]] * big, [w[0]] * big, [h[0]] * big, [ws[0]] * big, np.tile(h9s[:1], (big, 1)), []), "n=65536")
    g = np.ones((2, 3), np.float32) * 1.1
    # overlapping src / dst that are not equal: dst of frame 0 starts 3 bytes into its own src
    err(lambda: ctx.ApplyGainsDev(ptrs[:1], [ptrs[0] + 3], w[:1], h[:1], ws[:1], g[:1]), "overlaps src of frame 0")
    err(lambda: ctx.ApplyGainsDev(ptrs[:2], [ptrs[1], ptrs[1]], w[:2], h[:2], ws[:2], g), "overlaps")
    assert cover_of(ctx, ptrs, w, h, ws, h9s) is not None        # the ctx still works after the refusals
    ctx.close()


def cover_of(ctx, ptrs, w, h, ws, h9s):
    return ctx.GainStatsDev(ptrs, w, h, ws, h9s, [], 8)[1]


def _render(ctx, torch, A, gains, w, h, tseed=0xC0FFEE):
    ws = (3 * w + 3) & ~3
    n = len(A)
    frames = torch.empty((n, h * ws), dtype=torch.uint8, device="cuda")
    for k in range(n):
        ctx.SynthFrameDev(frames[k].data_ptr(), w, h, ws, A[k], tseed, k, float(gains[k]), 2.0)
    ctx.synchronize()
    return frames, ws


def _h9s(A):
    from tests.synth_survey import affine3
    return np.stack([affine3(a).reshape(9) for a in A]).astype(np.float32)


def test_ground_truth_gains():
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import frame_layout
    W, H, F = 1280, 960, 40
    ctx = im.Context(0)
    A, _ = frame_layout(F, W, H, per_row=10)
    gains = np.random.default_rng(21).uniform(0.85, 1.15, F)
    frames, ws = _render(ctx, torch, A, gains, W, H)
    sat = float(((frames == 0) | (frames == 255)).float().mean().item())
    print("ground truth: saturated byte fraction %.2e" % sat)
    assert sat < 1e-3                                        # measured 1.7e-4 (0 or 255 bytes): too few to bias an overlap mean
    h9s = _h9s(A)
    ptrs = [frames[k].data_ptr() for k in range(F)]
    wv, hv, wsv = [W] * F, [H] * F, [ws] * F
    pairs = [(a, b) for a in range(F) for b in range(a + 1, F)]
    st, cover = ctx.GainStatsDev(ptrs, wv, hv, wsv, h9s, pairs, 8)
    keep = st["n"] > 0
    st = st[keep]
    print("ground truth: %d overlapping pairs of %d" % (len(st), len(pairs)))
    g_weak = im.solve_gains(st, cover, sigma_g=10.0)
    prod = g_weak.astype(np.float64) * gains[:, None]
    spread = float((prod.max(axis=0) / prod.min(axis=0)).max())
    g_def = im.solve_gains(st, cover)

    def mismatch(g):
        n = st["n"].astype(np.float64)[:, None]
        Iab, Iba = st["sum_a"] / n, st["sum_b"] / n
        return float((n * (g[st["a"]] * Iab - g[st["b"]] * Iba) ** 2).sum())

    m1, md = mismatch(np.ones((F, 3))), mismatch(g_def.astype(np.float64))
    print("ground truth: spread max/min of g*gain (sigma_g 10) %.4f; mismatch gains=1 %.4g, defaults %.4g (x%.1f)" % (spread, m1, md, m1 / md))
    assert spread <= 1.02
    assert md * 2 <= m1
    ctx.close()


def test_c3_full_size():
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import frame_layout
    W, H, F = 4000, 3000, 500
    ctx = im.Context(0)
    A, gains = frame_layout(F, W, H)
    frames, ws = _render(ctx, torch, A, gains, W, H)
    h9s = _h9s(A)
    ptrs = [frames[k].data_ptr() for k in range(F)]
    pairs = [(k, k + 1) for k in range(F - 1)]
    st, cover = ctx.GainStatsDev(ptrs, [W] * F, [H] * F, [ws] * F, h9s, pairs, 8)
    weak = im.solve_gains(st, cover, sigma_g=10.0)
    g = ctx.GainCompensateDev(ptrs, [W] * F, [H] * F, [ws] * F, h9s, pairs)
    assert g.tobytes() == im.solve_gains(st, cover).tobytes()
    r = [float(np.corrcoef(g[:, c], 1.0 / gains)[0, 1]) for c in range(3)]
    rw = [float(np.corrcoef(weak[:, c], 1.0 / gains)[0, 1]) for c in range(3)]
    print("C3: corr(g, 1/gain) per channel", r, "g range", float(g.min()), float(g.max()), "; sigma_g 10:", rw)
    # measured 0.870 with the defaults: sigma_g = 0.1 pulls every gain toward 1 and a chain of adjacent pairs gives each frame two
    # neighbours only, so the gains follow 1/gain_k locally and shrink its slow drift along the strip
    assert min(r) > 0.8
    del frames
    torch.cuda.empty_cache()
    ctx.close()
