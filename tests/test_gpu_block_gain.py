"""GPU: block gain compensation (mi355_block_gain_stats_dev / mi355_apply_block_gains_dev / mi355_block_gain_compensate_dev, csrc/gain.hip)
against the numpy restatement (tests/block_gain_ref.py).

  * stats: record for record on the 10 frames of tests/test_gpu_gain.py at step 1, 4, 8 and grids 1x1, 4x3, 5x7, 16x16, on a quarter-turn frame,
    on a frame of exactly the grid's size; the two identities against GainStatsDev in the same context;
  * apply: byte for byte over widths 1..320 (and one above the column table), heights 1..240, odd pitches, unlike alignments, in and out of
    place, padding untouched; hand-set maps (1.0, 0, 7.99, a 16x16 checkerboard, 1x1);
  * compensate = stats -> solve -> apply; the refined render of the compensated frames; the vignetting ranking; determinism; every refusal;
  * C3 at full size: the two identities and a sane time.
"""
import time

import numpy as np
import pytest

from tests import block_gain_ref as br
from tests import gain_ref as gr

pytestmark = pytest.mark.gpu

GRIDS = [(1, 1), (4, 3), (5, 7), (16, 16)]


@pytest.fixture(scope="module")
def case(oracle):
    imgs, h9s, pairs = br.ten_frames()
    sizes = [(i.shape[1], i.shape[0]) for i in imgs]
    coords, _ = br.coord_maps(sizes, h9s)
    return imgs, h9s, pairs, sizes, coords, gr.frame_sample_maps(oracle, imgs, h9s)


def _upload(torch, imgs, pad=0, fill=0):
    ts = []
    for im_ in imgs:
        h, w = im_.shape[:2]
        a = np.full((h, 3 * w + pad), fill, np.uint8)
        a[:, :3 * w] = im_.reshape(h, 3 * w)
        ts.append(torch.from_numpy(a).cuda())
    torch.cuda.synchronize()
    w = [i.shape[1] for i in imgs]; h = [i.shape[0] for i in imgs]; ws = [t.shape[1] for t in ts]
    return ts, [t.data_ptr() for t in ts], w, h, ws


def _host(t, w):
    a = t.cpu().numpy()
    return a[:, :3 * w].reshape(a.shape[0], w, 3)


def _same_records(st, ref):
    assert len(st) == len(ref), (len(st), len(ref))
    for f in ("pair", "cell_a", "cell_b", "n", "sum_a", "sum_b"):
        assert np.array_equal(st[f], ref[f]), f
    assert np.all(st["n"] > 0) and np.all(st["reserved"] == 0)
    key = list(zip(st["pair"].tolist(), st["cell_a"].tolist(), st["cell_b"].tolist()))
    assert key == sorted(key) and len(set(key)) == len(key)


def _identities(ctx, st, cover, ptrs, w, h, ws, h9s, pairs, step):
    fs, fcov = ctx.GainStatsDev(ptrs, w, h, ws, h9s, pairs, step)
    assert np.array_equal(cover.sum(axis=1), fcov)
    for f in ("n", "sum_a", "sum_b"):
        tot = np.zeros(fs[f].shape, np.int64)
        np.add.at(tot, st["pair"], st[f])
        assert np.array_equal(tot, fs[f]), f


@pytest.mark.parametrize("gx,gy", GRIDS)
@pytest.mark.parametrize("step", [1, 4, 8])
def test_stats_equal_restatement(case, step, gx, gy):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, sizes, coords, maps = case
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    st, cover = ctx.BlockGainStatsDev(ptrs, w, h, ws, h9s, pairs, step, gx, gy)
    ref, cov_ref = br.stats_ref(maps, coords, sizes, pairs, step, gx, gy)
    assert np.array_equal(cover, cov_ref)
    _same_records(st, ref)
    _identities(ctx, st, cover, ptrs, w, h, ws, h9s, pairs, step)
    # the case covers what it claims: a skipped frame, listed pairs without overlap, many cell combinations per pair on the finer grids
    assert cover[8].sum() == 0 and not np.any(st["pair"] == pairs.index((0, 9))) and not np.any(st["pair"] == pairs.index((8, 7)))
    assert gx * gy == 1 or len(st) > len(pairs)
    ctx.close()


def test_stats_quarter_turn_and_grid_sized_frame(oracle):
    """frame 1 is turned by a quarter, so its cell rows run along frame 0's cell columns; frame 2 has exactly 5 x 7 pixels (a pixel per cell)"""
    import torch
    import imagemosaicing_amd as im
    from tests.synth import texture
    imgs = [texture(200, 150, 3), texture(150, 200, 4), texture(5, 7, 5), texture(120, 90, 6)]
    h9s = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1], [0, -1, 230, 1, 0, 10, 0, 0, 1], [1, 0, 50.5, 0, 1, 60.25, 0, 0, 1], [1.1, 0.1, 40, -0.1, 0.9, 30, 1e-4, 0, 1]], np.float32)
    pairs = [(0, 1), (2, 0), (1, 3), (3, 0), (2, 1)]
    sizes = [(i.shape[1], i.shape[0]) for i in imgs]
    coords, _ = br.coord_maps(sizes, h9s)
    maps = gr.frame_sample_maps(oracle, imgs, h9s)
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    for step in (1, 3):
        st, cover = ctx.BlockGainStatsDev(ptrs, w, h, ws, h9s, pairs, step, 5, 7)
        ref, cov_ref = br.stats_ref(maps, coords, sizes, pairs, step, 5, 7)
        assert np.array_equal(cover, cov_ref)
        _same_records(st, ref)
        _identities(ctx, st, cover, ptrs, w, h, ws, h9s, pairs, step)
    st, cover = ctx.BlockGainStatsDev(ptrs, w, h, ws, h9s, pairs, 1, 5, 7)
    p01 = st[st["pair"] == 0]
    assert len(p01) > 20 and np.all(st["n"][st["pair"] == 1] >= 1) and np.any(st["pair"] == 1)
    # a quarter turn: along frame 0's columns (cell_a % 5 grows) frame 1's rows (cell_b // 5) change
    assert len(set((p01["cell_a"] % 5).tolist())) > 1 and len(set((p01["cell_b"] // 5).tolist())) > 1
    assert np.count_nonzero(cover[2]) >= 12                     # a 5 x 7 frame has samples in [0, 4) x [0, 6): 24 cells at most
    # one pixel smaller than the grid: refused, naming the frame, its size and the grid
    for gx, gy in ((6, 7), (5, 8)):
        with pytest.raises(im.Mi355Error) as e:
            ctx.BlockGainStatsDev(ptrs, w, h, ws, h9s, pairs, 1, gx, gy)
        assert e.value.code == -1 and "frame 2 (5x7) is smaller than the %dx%d grid" % (gx, gy) in str(e.value), str(e.value)
    ctx.close()


APPLY_W = [1, 2, 3, 15, 16, 17, 255, 257, 320]
APPLY_H = [1, 2, 17, 240]


@pytest.mark.parametrize("gx,gy", [(1, 1), (4, 3), (8, 6), (16, 16)])
def test_apply_equals_restatement(gx, gy):
    """every width x height in one launch, plus a row wider than the kernel's column table; mixed pitches (3w, IplImage, 3w + 1, 3w + 13, 256) and
    base offsets that align source and destination differently; gaps and padding are garbage that must stay"""
    import torch
    import imagemosaicing_amd as im
    from tests import pitched as pf
    from tests.synth import texture
    ctx = im.Context(0)
    rng = np.random.default_rng(gx * 17 + gy)
    sizes = [(w, h) for h in APPLY_H for w in APPLY_W] + [(8200, 3)]
    imgs = [texture(w, h, seed=60 + k) for k, (w, h) in enumerate(sizes)]
    n = len(sizes)
    g = rng.uniform(0.5, 1.7, (n, gy, gx, 3)).astype(np.float32)
    want = [br.apply_ref(imgs[k], g[k]) for k in range(n)]
    pitches = [pf.pitch_kinds(w)[k % 5] for k, (w, h) in enumerate(sizes)]
    fs = pf.PitchedFrames(imgs, pitches, offsets=[k % 4 for k in range(n)], seed=7)
    fd = pf.PitchedFrames([np.zeros_like(i) for i in imgs], pitches, offsets=[(k + 1) % 4 for k in range(n)], seed=8)
    ts, sp = fs.to_device(torch)
    td, dp = fd.to_device(torch)
    w, h, ws = fs.geom()
    pix_s, pix_d = np.zeros(fs.nbytes, bool), np.zeros(fd.nbytes, bool)
    for k in range(n):
        fs.view(k, pix_s)[:, :fs.row_bytes(k)] = True
        fd.view(k, pix_d)[:, :fd.row_bytes(k)] = True
    ctx.ApplyBlockGainsDev(sp, dp, w, h, ws, g)
    got_s, got_d = fs.device_bytes(ts), fd.device_bytes(td)
    for k in range(n):
        assert np.array_equal(fd.pixels(k, got_d), want[k]), sizes[k]
    assert np.array_equal(got_d[~pix_d], fd.buf[~pix_d]) and np.array_equal(got_s, fs.buf)
    ctx.ApplyBlockGainsDev(sp, sp, w, h, ws, g)                  # in place
    got_s = fs.device_bytes(ts)
    for k in range(n):
        assert np.array_equal(fs.pixels(k, got_s), want[k]), sizes[k]
    assert np.array_equal(got_s[~pix_s], fs.buf[~pix_s])
    # source and destination aligned alike on a 16-byte pitch: whole rows through the 16-byte path, sentinel padding
    a_s, pa, wa, ha, wsa = _upload(torch, imgs[-10:-1], pad=64 - (3 * 320) % 64, fill=77)
    a_d, pd, _, _, _ = _upload(torch, [np.zeros_like(i) for i in imgs[-10:-1]], pad=64 - (3 * 320) % 64, fill=201)
    ctx.ApplyBlockGainsDev(pa, pd, wa, ha, wsa, g[-10:-1])
    for j, k in enumerate(range(n - 10, n - 1)):
        assert np.array_equal(_host(a_d[j], wa[j]), want[k]), sizes[k]
        assert np.all(a_d[j].cpu().numpy()[:, 3 * wa[j]:] == 201) and np.all(a_s[j].cpu().numpy()[:, 3 * wa[j]:] == 77)
    ctx.close()


def test_apply_hand_set_maps():
    import torch
    import imagemosaicing_amd as im
    ctx = im.Context(0)
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for (w, h) in [(320, 240), (257, 17), (64, 64)]]
    n = len(imgs)

    def run(g, in_place):
        src, sp, w, h, ws = _upload(torch, imgs, pad=13, fill=77)
        dst, dp, _, _, _ = _upload(torch, [np.full_like(i, 9) for i in imgs], pad=13, fill=201)
        ctx.ApplyBlockGainsDev(sp, sp if in_place else dp, w, h, ws, g)
        out = src if in_place else dst
        return [_host(out[k], w[k]) for k in range(n)], [out[k].cpu().numpy()[:, 3 * w[k]:] for k in range(n)]

    for gx, gy in ((1, 1), (8, 6), (16, 16)):
        for in_place in (False, True):
            got, pad = run(np.ones((n, gy, gx, 3), np.float32), in_place)           # a map of 1.0: the bytes as they were
            assert all(np.array_equal(got[k], imgs[k]) for k in range(n)) and all(np.all(p == (77 if in_place else 201)) for p in pad)
    g = np.ones((n, 3, 4, 3), np.float32)
    g[0, :, :2] = 0.0; g[0, :, 2:] = 7.99                        # both ends of Q12: black, and saturation through 32727 / 4096
    g[1, 1] = [0.0, 7.99, 1.0]
    g[2, 0, 0] = 9.5                                              # clamped to 32767 / 4096
    got, _ = run(g, False)
    for k in range(n):
        assert np.array_equal(got[k], br.apply_ref(imgs[k], g[k])), k
    assert np.all(got[0][:, :40] == 0) and np.all(got[0][:, 300:][imgs[0][:, 300:] >= 32] == 255)
    board = np.ones((n, 16, 16, 3), np.float32)
    board[:, ::2, ::2] = 0.25; board[:, 1::2, 1::2] = 0.25; board[..., 1] *= 2.0; board[..., 2] += 0.1
    for in_place in (False, True):
        got, _ = run(board, in_place)
        for k in range(n):
            assert np.array_equal(got[k], br.apply_ref(imgs[k], board[k])), k
    one = rng.uniform(0.6, 1.5, (n, 1, 1, 3)).astype(np.float32)                    # grid 1 x 1: one Q12 gain per channel
    got, _ = run(one, True)
    for k in range(n):
        assert np.array_equal(got[k], br.apply_ref(imgs[k], one[k])), k
        q = np.floor(one[k, 0, 0].astype(np.float64) * 4096 + 0.5).astype(np.int64)
        assert np.array_equal(got[k], np.minimum(255, (q * 256 * imgs[k].astype(np.int64) + (1 << 19)) >> 20))
    ctx.close()


def test_compensate_equals_stats_solve_apply_and_canvas(case, oracle):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, sizes, coords, maps = case
    ctx = im.Context(0)
    n = len(imgs)
    kw = dict(step=4, grid_x=4, grid_y=3, smooth=1)
    ts, ptrs, w, h, ws = _upload(torch, imgs, pad=5, fill=77)
    st, cover = ctx.BlockGainStatsDev(ptrs, w, h, ws, h9s, pairs, 4, 4, 3)
    g = im.solve_block_gains(st, pairs, cover, **kw)
    ref = br.gains_ref(*br.stats_ref(maps, coords, sizes, pairs, 4, 4, 3)[:1], pairs, cover, 4, 3, 1)
    assert np.max(np.abs(g.astype(np.float64) - ref)) <= 2e-7   # both are float32 roundings of solutions within 1e-9: an ulp near 1 apart at most
    assert np.all(g[8] == 1.0) and np.ptp(g[0]) > 0
    dst, dp, _, _, _ = _upload(torch, [np.zeros_like(i) for i in imgs], pad=5, fill=201)
    ctx.ApplyBlockGainsDev(ptrs, dp, w, h, ws, g)
    ptrs_skip = list(ptrs); ptrs_skip[8] = 0                     # the skipped frame may be withheld
    g2 = ctx.BlockGainCompensateDev(ptrs_skip, w, h, ws, h9s, pairs, **kw)
    assert g2.tobytes() == g.tobytes()
    comp = [br.apply_ref(imgs[k], g[k]) for k in range(n)]
    for k in range(n):
        assert np.array_equal(_host(ts[k], w[k]), _host(dst[k], w[k])) and np.array_equal(_host(ts[k], w[k]), comp[k]), k
        assert np.all(ts[k].cpu().numpy()[:, 3 * w[k]:] == 77)
    assert np.array_equal(comp[8], imgs[8])
    # the refined render of the compensated frames is the oracle's render of the restatement's compensated frames
    cw, ch, cws, _ = im.mosaic_layout(w, h, h9s)
    canvas = torch.empty((ch, cws), dtype=torch.uint8, device="cuda")
    ctx.MosaicImagesRefinedDev(ptrs, w, h, ws, h9s, canvas.data_ptr(), cw, ch, cws)
    ctx.synchronize()
    rc, r = oracle.mosaic_images_refined(comp, h9s)
    assert rc == 0 and np.array_equal(canvas.cpu().numpy()[:, :3 * cw], r[0][:, :3 * cw])
    ctx.close()


def test_vignetting_ranking_through_the_library():
    import torch
    import imagemosaicing_amd as im
    ctx = im.Context(0)

    def block(imgs, h9s, pairs, maps_ref):
        ts, ptrs, w, h, ws = _upload(torch, imgs)
        g = ctx.BlockGainCompensateDev(ptrs, w, h, ws, h9s, pairs, step=4, grid_x=8, grid_y=6, smooth=2)
        assert np.max(np.abs(g.astype(np.float64) - maps_ref)) <= 2e-7
        return [_host(ts[k], w[k]) for k in range(len(imgs))]

    def frame(imgs, h9s, pairs, gains_ref):
        ts, ptrs, w, h, ws = _upload(torch, imgs)
        g = ctx.GainCompensateDev(ptrs, w, h, ws, h9s, pairs, step=4)
        assert np.max(np.abs(g.astype(np.float64) - gains_ref)) <= 2e-7
        return [_host(ts[k], w[k]) for k in range(len(imgs))]

    mad = br.vignette_ranking(block, frame)
    print("vignetting through the library: mean |a - b| over the overlaps: block %.3f, frame %.3f, none %.3f" % tuple(mad))
    assert mad[0] < 0.8 * mad[1] and mad[1] < mad[2]
    ctx.close()


def test_determinism_and_second_context(case):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, sizes, coords, maps = case
    c1, c2 = im.Context(0), im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)
    s1, v1 = c1.BlockGainStatsDev(ptrs, w, h, ws, h9s, pairs, 2, 16, 16)            # two table batches
    s2, v2 = c1.BlockGainStatsDev(ptrs, w, h, ws, h9s, pairs, 2, 16, 16)
    s3, v3 = c2.BlockGainStatsDev(ptrs, w, h, ws, h9s, pairs, 2, 16, 16)
    assert s1.tobytes() == s2.tobytes() == s3.tobytes() and np.array_equal(v1, v2) and np.array_equal(v1, v3)
    kw = dict(step=2, grid_x=5, grid_y=7)
    a, pa, _, _, _ = _upload(torch, imgs)
    b, pb, _, _, _ = _upload(torch, imgs)
    ga = c1.BlockGainCompensateDev(pa, w, h, ws, h9s, pairs, **kw)
    gb = c2.BlockGainCompensateDev(pb, w, h, ws, h9s, pairs, **kw)
    assert ga.tobytes() == gb.tobytes()
    assert all(np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in range(len(imgs)))
    c1.close(); c2.close()


def test_argument_errors(case):
    import torch
    import imagemosaicing_amd as im
    imgs, h9s, pairs, sizes, coords, maps = case
    ctx = im.Context(0)
    ts, ptrs, w, h, ws = _upload(torch, imgs)

    def err(fn, match):
        with pytest.raises(im.Mi355Error) as e:
            fn()
        assert e.value.code == -1 and match in str(e.value), str(e.value)

    S, A, Cp = ctx.BlockGainStatsDev, ctx.ApplyBlockGainsDev, ctx.BlockGainCompensateDev
    err(lambda: S(ptrs, w, h, ws, h9s, [(1, 1)]), "pair 0 (1, 1): a == b")
    err(lambda: S(ptrs, w, h, ws, h9s, [(0, 1), (2, 10)]), "pair 1 (2, 10): position outside [0, 10)")
    err(lambda: S(ptrs, w, h, ws, h9s, [(0, 1), (1, 0)]), "pair 1 (1, 0) repeats pair 0")
    err(lambda: S(ptrs, w, h, ws, h9s, pairs, 0), "step=0")
    err(lambda: S(ptrs, w, h, ws, h9s, pairs, 65), "step=65")
    err(lambda: S(ptrs, w, h, ws, h9s, pairs, 8, 0, 3), "grid 0x3")
    err(lambda: S(ptrs, w, h, ws, h9s, pairs, 8, 4, 17), "grid 4x17")
    err(lambda: S([0] + ptrs[1:], w, h, ws, h9s, pairs), "frame 0 takes part but its pointer is NULL")
    err(lambda: S(ptrs, w, h, [3 * 320 - 1] + ws[1:], h9s, pairs), "frame 0: bad geometry")
    err(lambda: Cp(ptrs, w, h, ws, h9s, pairs, channels=2), "channels=2")
    err(lambda: Cp(ptrs, w, h, ws, h9s, pairs, sigma_n=0.0), "sigma_n=")
    err(lambda: Cp(ptrs, w, h, ws, h9s, pairs, sigma_g=-0.1), "sigma_g=")
    err(lambda: Cp(ptrs, w, h, ws, h9s, pairs, step=100), "step=100")
    err(lambda: Cp(ptrs, w, h, ws, h9s, pairs, smooth=9), "smooth=9")
    err(lambda: Cp(ptrs, w, h, ws, h9s, pairs, grid_x=17), "grid 17x6")
    big = 65536
    err(lambda: S([ptrs[0]] * big, [w[0]] * big, [h[0]] * big, [ws[0]] * big, np.tile(h9s[:1], (big, 1)), []), "n=65536")
    g = np.full((2, 3, 4, 3), 1.1, np.float32)
    err(lambda: A(ptrs[:1], [ptrs[0] + 3], w[:1], h[:1], ws[:1], g[:1]), "overlaps src of frame 0")
    err(lambda: A(ptrs[:2], [ptrs[1], ptrs[1]], w[:2], h[:2], ws[:2], g), "overlaps")
    err(lambda: A(ptrs[:2], [ptrs[0], 0], w[:2], h[:2], ws[:2], g), "frame 1: NULL pointer")
    bad = g.copy(); bad[1, 2, 3, 1] = np.inf
    err(lambda: A(ptrs[:2], ptrs[:2], w[:2], h[:2], ws[:2], bad), "frame 1: gain[34] is not finite")
    bad = g.copy(); bad[0, 0, 0, 0] = np.nan
    err(lambda: A(ptrs[:2], ptrs[:2], w[:2], h[:2], ws[:2], bad), "frame 0: gain[0] is not finite")
    err(lambda: A(ptrs[:1], ptrs[:1], [(1 << 20) + 1], [1], [3 * ((1 << 20) + 1)], g[:1]), "above 2^20")
    err(lambda: A(ptrs[:1], ptrs[:1], w[:1], h[:1], ws[:1], np.ones((1, 17, 4, 3), np.float32)), "grid 4x17")
    for k in range(len(imgs)):                                  # nothing was written by a refused call
        assert np.array_equal(_host(ts[k], w[k]), imgs[k])
    assert ctx.BlockGainStatsDev(ptrs, w, h, ws, h9s, [], 8)[0].shape == (0,)        # the ctx still works, and no pairs is no records
    ctx.close()


def test_c3_full_size():
    import torch
    import imagemosaicing_amd as im
    from tests.synth_survey import affine3, frame_layout
    W, H, F = 4000, 3000, 500
    ctx = im.Context(0)
    A, gains = frame_layout(F, W, H)
    ws = (3 * W + 3) & ~3
    frames = torch.empty((F, H * ws), dtype=torch.uint8, device="cuda")
    for k in range(F):
        ctx.SynthFrameDev(frames[k].data_ptr(), W, H, ws, A[k], 0xC0FFEE, k, float(gains[k]), 2.0)
    ctx.synchronize()
    h9s = np.stack([affine3(a).reshape(9) for a in A]).astype(np.float32)
    ptrs = [frames[k].data_ptr() for k in range(F)]
    pairs = [(k, k + 1) for k in range(F - 1)]
    wv, hv, wsv = [W] * F, [H] * F, [ws] * F
    ctx.BlockGainStatsDev(ptrs, wv, hv, wsv, h9s, pairs[:4])   # buffers and code objects
    t0 = time.perf_counter()
    st, cover = ctx.BlockGainStatsDev(ptrs, wv, hv, wsv, h9s, pairs)
    dt = time.perf_counter() - t0
    _identities(ctx, st, cover, ptrs, wv, hv, wsv, h9s, pairs, 8)
    print("C3: %d block records of %d pairs, stats call %.1f ms" % (len(st), len(pairs), dt * 1e3))
    assert len(st) > len(pairs) and np.all(cover.sum(axis=1) > 0)
    # sanity, not a benchmark: 499 pairs at 8 x 6 are two table batches over a few thousand tiles; a call that takes a second has lost its way
    assert dt < 1.0
    del frames
    torch.cuda.empty_cache()
    ctx.close()
