"""GPU: every kernel that reads a caller's frame takes it by (w, h, ws) -- rows of ws bytes, IplImage / BitmapImage layout
(include/mi355_mosaic.h).  Here the frames are padded (3w + 1, 3w + 13, the IplImage pitch, 256-byte rows), odd (w % 4 of 1, 2, 3), tiny
(2 x 2, 2 x N, N x 2), of different sizes within one call, and on the device at base pointers +1, +2, +3 (tests/pitched.py); all padding is
non-zero garbage.  Every output equals, bit for bit, the oracle (or the host entry point) on the contiguous copies, and output pitches the
caller owns keep their padding.  tests/test_oracle_pitch.py checks the oracle itself on the same frames."""
import ctypes as C

import numpy as np
import pytest

from tests import gain_ref as gr
from tests import oracle_lib as ol
from tests import pitched as pf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def im():
    import imagemosaicing_amd
    return imagemosaicing_amd


@pytest.fixture(scope="module")
def ctx(im):
    c = im.Context(0)
    yield c
    c.close()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _rows(buf, cw):
    return np.ascontiguousarray(buf[:, :3 * cw])


def _chk(ctx, rc):
    assert rc == 0, (rc, (ctx.L.mi355_last_error(ctx._h) or b"").decode())


@pytest.fixture(scope="module")
def mixed():
    """the mixed frame set of tests/pitched.py: contiguous images, the refined render's h9s (one frame skipped), the blended form's h9s and
    keep[] (the same frame dropped through keep instead), and two pitched layouts of it"""
    sizes = pf.MIXED_SIZES
    imgs = pf.mixed_images(sizes, seed=1)
    h9s = pf.mixed_h9s(sizes)
    bh9s = h9s.copy()
    bh9s[pf.MIXED_SKIP, 8] = 1.0
    keep = np.ones(len(sizes), np.uint8)
    keep[pf.MIXED_SKIP] = 0
    fa = pf.PitchedFrames(imgs, pf.mixed_pitches(sizes, 3, 0), offsets=[k % 4 for k in range(len(sizes))], seed=21)
    fb = pf.PitchedFrames(imgs, pf.mixed_pitches(sizes, 3, 2), offsets=[(k + 1) % 4 for k in range(len(sizes))], seed=22)
    return dict(imgs=imgs, h9s=h9s, bh9s=bh9s, keep=keep, fa=fa, fb=fb)


# ---------------------------------------------------------------------------------------------- 1. warp
def test_warp_padded_and_odd_frames(ctx, oracle):
    rng = np.random.default_rng(31)
    sizes = [(2, 2), (2, 9), (9, 2), (7, 5), (333, 257), (201, 150), (130, 97), (642, 31)]
    for ch in (3, 1):
        imgs = pf.mixed_images(sizes, seed=8, ch=ch)
        for shift in (0, 1, 2, 3, 4):
            fr = pf.PitchedFrames(imgs, pf.mixed_pitches(sizes, ch, shift), offsets=[(k + shift) % 4 for k in range(len(sizes))], seed=shift)
            for k in range(len(sizes)):
                H = np.eye(3) + rng.normal(0, 0.06, (3, 3))
                H[0, 2], H[1, 2] = rng.uniform(-30, 30), rng.uniform(-30, 30)
                H[2, 0], H[2, 1], H[2, 2] = rng.normal(0, 1e-4), rng.normal(0, 1e-4), 1
                h9 = H.reshape(9).astype(np.float32)
                dst = C.c_void_p()
                dw, dh, dws = C.c_int(), C.c_int(), C.c_int()
                _chk(ctx, ctx.L.mi355_warp_image(ctx._h, C.c_void_p(fr.host_ptrs()[k]), int(fr.w[k]), int(fr.h[k]), int(fr.ws[k]), ch, _vp(h9),
                                                 C.byref(dst), C.byref(dw), C.byref(dh), C.byref(dws)))
                buf = np.ctypeslib.as_array(C.cast(dst, ol.u8p), shape=(dh.value, dws.value)).copy()
                ctx.L.mi355_free(dst)
                rc, ref = oracle.image_projection_transform(imgs[k], h9)
                tag = (ch, sizes[k], int(fr.ws[k]), fr.base[k] % 4)
                assert rc == 0 and (dw.value, dh.value, dws.value) == ref[1:], tag
                assert np.array_equal(buf, ref[0]), (tag, int((buf != ref[0]).sum()))


# ---------------------------------------------------------------------------------------------- 2. refined render
def test_refined_render_all_forms(im, ctx, oracle, mixed):
    import torch
    imgs, h9s = mixed["imgs"], mixed["h9s"]
    n = len(imgs)
    rc, ref = oracle.mosaic_images_refined(imgs, h9s)
    assert rc == 0
    want, cw, ch, cws = ref
    for fr in (mixed["fa"], mixed["fb"]):
        w, h, ws = fr.geom()
        # host form (the skipped frame's pointer is NULL: it is never read)
        canvas = C.c_void_p()
        cwv, chv, cwsv = C.c_int(), C.c_int(), C.c_int()
        _chk(ctx, ctx.L.mi355_mosaic_refined(ctx._h, fr.host_ptr_array(skip={pf.MIXED_SKIP}), _vp(w), _vp(h), _vp(ws), n, _vp(h9s),
                                             C.byref(canvas), C.byref(cwv), C.byref(chv), C.byref(cwsv)))
        got = np.ctypeslib.as_array(C.cast(canvas, ol.u8p), shape=(chv.value, cwsv.value)).copy()
        ctx.L.mi355_free(canvas)
        assert (cwv.value, chv.value, cwsv.value) == (cw, ch, cws)
        assert np.array_equal(_rows(got, cw), _rows(want, cw)), int((_rows(got, cw) != _rows(want, cw)).sum())
        # into: host sources, a destination with its own padding
        pitch = 3 * cw + 11
        dst = np.full((ch, pitch), 0xA5, np.uint8)
        _chk(ctx, ctx.L.mi355_mosaic_refined_into(ctx._h, fr.host_ptr_array(), None, _vp(w), _vp(h), _vp(ws), n, _vp(h9s),
                                                  _vp(dst), pitch, cw, ch))
        assert np.array_equal(dst[:, :3 * cw], _rows(want, cw)) and (dst[:, 3 * cw:] == 0xA5).all()
        # device form: frames at odd base pointers, the whole canvas and random stripes
        t, ptrs = fr.to_device(torch)
        d_canvas = torch.full((ch, cws), 77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.MosaicImagesRefinedDev(ptrs, w, h, ws, h9s, d_canvas.data_ptr(), cw, ch, cws)
        ctx.synchronize()
        assert np.array_equal(_rows(d_canvas.cpu().numpy(), cw), _rows(want, cw))
        d_canvas.fill_(77)
        torch.cuda.synchronize()
        cuts = [0] + sorted(np.random.default_rng(int(fr.ws[0])).choice(np.arange(1, ch), 5, replace=False).tolist()) + [ch]
        for a, b in zip(cuts[:-1], cuts[1:]):
            ctx.MosaicImagesRefinedDev(ptrs, w, h, ws, h9s, d_canvas.data_ptr(), cw, ch, cws, a, b - a)
        ctx.synchronize()
        assert np.array_equal(_rows(d_canvas.cpu().numpy(), cw), _rows(want, cw)), cuts
        assert np.array_equal(fr.device_bytes(t), fr.buf)         # sources untouched
        del t


# ---------------------------------------------------------------------------------------------- 3. chips, masks, blend
def _chips_and_masks(ctx, fr, h9s, keep, find_masks):
    """mi355_chips_and_masks on the pitched host frames (what Context.ChipsAndMasks does on contiguous ones)"""
    w, h, ws = fr.geom()
    nch = C.c_int(0)
    chips = C.c_void_p()
    cimgs = C.POINTER(C.c_void_p)()
    masks = C.POINTER(C.c_void_p)()
    cw, ch = C.c_int(), C.c_int()
    _chk(ctx, ctx.L.mi355_chips_and_masks(ctx._h, fr.host_ptr_array(), _vp(w), _vp(h), _vp(ws), fr.n, _vp(h9s), _vp(keep), int(find_masks),
                                          C.byref(nch), C.byref(chips), C.byref(cimgs), C.byref(masks), C.byref(cw), C.byref(ch)))
    nv = nch.value
    info = np.ctypeslib.as_array(C.cast(chips, ol.u8p), shape=(max(nv, 1) * ol.CHIPINFO.itemsize,))[:nv * ol.CHIPINFO.itemsize].copy().view(ol.CHIPINFO)
    out_c, out_m = [], []
    for v in range(nv):
        cwv, chv = int(info[v]["w"]), int(info[v]["h"])
        ccws, mws = (cwv * 3 + 3) & ~3, (cwv + 3) & ~3
        out_c.append(np.ctypeslib.as_array(C.cast(cimgs[v], ol.u8p), shape=(chv * ccws,)).copy().reshape(chv, ccws))
        out_m.append(np.ctypeslib.as_array(C.cast(masks[v], ol.u8p), shape=(chv * mws,)).copy().reshape(chv, mws))
        ctx.L.mi355_free(C.c_void_p(cimgs[v]))
        ctx.L.mi355_free(C.c_void_p(masks[v]))
    ctx.L.mi355_free(chips)
    ctx.L.mi355_free(C.cast(cimgs, C.c_void_p))
    ctx.L.mi355_free(C.cast(masks, C.c_void_p))
    return dict(cw=cw.value, ch=ch.value, chips=info, chip_imgs=out_c, masks=out_m)


def test_chips_masks_and_blend_all_forms(im, ctx, oracle, mixed):
    import torch
    imgs, h9s, keep = mixed["imgs"], mixed["bh9s"], mixed["keep"]
    n = len(imgs)
    ref = oracle.chips_and_masks(imgs, h9s, keep=keep)
    cw, ch = ref["cw"], ref["ch"]
    assert len(ref["chips"]) == n - 1
    for fr in (mixed["fa"], mixed["fb"]):
        for find_masks, key in ((1, "masks"), (0, "valid")):
            got = _chips_and_masks(ctx, fr, h9s, keep, find_masks)
            assert (got["cw"], got["ch"]) == (cw, ch) and len(got["chips"]) == len(ref["chips"])
            for v in range(len(ref["chips"])):
                for f in ("x0", "y0", "w", "h", "img"):
                    assert int(got["chips"][v][f]) == int(ref["chips"][v][f]), (v, f)
                assert np.array_equal(got["chips"][v]["quad"].view(np.uint32), ref["chips"][v]["quad"].view(np.uint32)), v
                assert np.array_equal(got["chip_imgs"][v], ref["chip_imgs"][v]), (v, int(ref["chips"][v]["img"]))
                assert np.array_equal(got["masks"][v], ref[key][v]), (v, key)
    w, h, ws = mixed["fa"].geom()
    t, ptrs = mixed["fa"].to_device(torch)
    for band in (5, 1):
        want, _ = oracle.multiband_blend(ref["chips"], ref["chip_imgs"], ref["masks"], cw, ch, band=band)
        for fr in (mixed["fa"], mixed["fb"]):
            fw, fh, fws = fr.geom()
            out = C.c_void_p()
            ow, oh, ows = C.c_int(), C.c_int(), C.c_int()
            _chk(ctx, ctx.L.mi355_mosaic_blended(ctx._h, fr.host_ptr_array(), _vp(fw), _vp(fh), _vp(fws), n, _vp(h9s), _vp(keep), band,
                                                 C.byref(out), C.byref(ow), C.byref(oh), C.byref(ows)))
            got = np.ctypeslib.as_array(C.cast(out, ol.u8p), shape=(oh.value * ows.value,)).copy().reshape(oh.value, ows.value)
            ctx.L.mi355_free(out)
            assert (ow.value, oh.value) == (cw, ch) and np.array_equal(_rows(got, cw), _rows(want, cw)), (band, int((_rows(got, cw) != _rows(want, cw)).sum()))
            pitch = 3 * cw + 7
            dst = np.full((ch, pitch), 0x5A, np.uint8)
            _chk(ctx, ctx.L.mi355_mosaic_blended_into(ctx._h, fr.host_ptr_array(skip={pf.MIXED_SKIP}), None, _vp(fw), _vp(fh), _vp(fws), n,
                                                      _vp(h9s), _vp(keep), band, _vp(dst), pitch, cw, ch))
            assert np.array_equal(dst[:, :3 * cw], _rows(want, cw)) and (dst[:, 3 * cw:] == 0x5A).all(), band
        d_out, bw, bh, _ = ctx.MosaicBlendedDev(ptrs, w, h, ws, h9s, keep=keep, band=band)
        assert (bw, bh) == (cw, ch) and np.array_equal(_rows(d_out.cpu().numpy(), cw), _rows(want, cw)), band
        cuts = [0, 1, ch // 3, ch // 3 + 17, ch]
        stripes = [ctx.MosaicBlendedDev(ptrs, w, h, ws, h9s, keep=keep, band=band, row0=a, rows=b - a)[0].cpu().numpy() for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(_rows(np.concatenate(stripes), cw), _rows(want, cw)), band
    assert np.array_equal(mixed["fa"].device_bytes(t), mixed["fa"].buf)
    del t


# ---------------------------------------------------------------------------------------------- 4. gain compensation
def _gain_set():
    sizes = pf.MIXED_SIZES
    imgs = [(i.astype(np.float64) * (0.86 + 0.035 * k)).clip(0, 255).astype(np.uint8) for k, i in enumerate(pf.mixed_images(sizes, seed=3))]
    h9s = pf.mixed_h9s(sizes)
    pairs = [(0, 1), (0, 2), (1, 2), (0, 3), (2, 4), (0, 5), (1, 6), (0, 7), (7, 9), (1, 9), (2, 7), (8, 0), (8, 7), (6, 7), (4, 5), (3, 9)]
    return imgs, h9s, pairs


@pytest.mark.parametrize("step", [1, 3])
def test_gain_stats_mixed_geometry(ctx, oracle, step):
    import torch
    imgs, h9s, pairs = _gain_set()
    maps = gr.frame_sample_maps(oracle, imgs, h9s)
    recs, cov_ref = gr.stats_ref(maps, pairs, step)
    fr = pf.PitchedFrames(imgs, pf.mixed_pitches(pf.MIXED_SIZES, 3, step), offsets=[(k * step) % 4 for k in range(len(imgs))], seed=40 + step)
    t, ptrs = fr.to_device(torch)
    ptrs[pf.MIXED_SKIP] = 0                                  # the skipped frame takes no part: NULL
    w, h, ws = fr.geom()
    st, cover = ctx.GainStatsDev(ptrs, w, h, ws, h9s, pairs, step)
    assert np.array_equal(cover, cov_ref), (cover, cov_ref)
    for i, (a, b) in enumerate(pairs):
        nn, sa, sb = recs[i]
        assert (st[i]["a"], st[i]["b"]) == (a, b)
        assert st[i]["n"] == nn and np.array_equal(st[i]["sum_a"], sa) and np.array_equal(st[i]["sum_b"], sb), (i, a, b, st[i], recs[i])
    assert sum(int(r[0] > 0) for r in recs) >= 8 and cover[pf.MIXED_SKIP] == 0
    del t


def test_gain_compensate_null_skipped_frame_and_canvas_identity(im, ctx, oracle):
    import torch
    imgs, h9s, pairs = _gain_set()
    fr = pf.PitchedFrames(imgs, pf.mixed_pitches(pf.MIXED_SIZES, 3, 4), offsets=[(k + 2) % 4 for k in range(len(imgs))], seed=50)
    t, ptrs = fr.to_device(torch)
    ptrs[pf.MIXED_SKIP] = 0
    w, h, ws = fr.geom()
    g = ctx.GainCompensateDev(ptrs, w, h, ws, h9s, pairs, step=2)
    assert np.all(g[pf.MIXED_SKIP] == 1.0) and not np.all(g == 1.0)
    after = fr.device_bytes(t)
    lutd = [gr.apply_lut(imgs[k], g[k]) for k in range(len(imgs))]
    for k in range(len(imgs)):
        assert np.array_equal(fr.pixels(k, after), lutd[k] if k != pf.MIXED_SKIP else imgs[k]), k
    outside = np.ones(fr.nbytes, bool)
    for k in range(len(imgs)):
        fr.view(k, outside)[:, :fr.row_bytes(k)] = False
    assert np.array_equal(after[outside], fr.buf[outside]), "bytes outside the pixels written"
    cw, ch, cws, _ = im.mosaic_layout(w, h, h9s)
    canvas = torch.empty((ch, cws), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.MosaicImagesRefinedDev(ptrs, w, h, ws, h9s, canvas.data_ptr(), cw, ch, cws)
    ctx.synchronize()
    rc, ref = oracle.mosaic_images_refined(lutd, h9s)
    assert rc == 0 and np.array_equal(_rows(canvas.cpu().numpy(), cw), _rows(ref[0], cw))
    del t


# ---------------------------------------------------------------------------------------------- 5. SIFT device batches
def _sift_refs(imgs):
    orc = ol.load_oracle_fast()
    return ol.parallel_map(lambda i: orc.sift(i), imgs)


def _same_features(kp, desc, ref, tag):
    okp, odesc = ref
    assert len(kp) == len(okp), (tag, len(kp), len(okp))
    assert np.array_equal(kp.view(np.uint8), okp.view(np.uint8)), tag
    assert np.array_equal(desc, desc.astype(np.uint8).astype(np.float32)) and np.array_equal(desc.astype(np.uint8), odesc), tag


def _sift_batch(im, fr, ids):
    """the frames of fr as one device batch of a fresh context (sift_batch 4); returns (features, gauss_stream launches, gauss launches)"""
    import torch
    c = im.Context(0)
    c.set_option("sift_batch", 4)
    c.profile_enable(True)
    t, ptrs = fr.to_device(torch)
    c.profile_reset()
    for k in range(fr.n):
        c.SiftExtractDev(ids[k], ptrs[k], int(fr.w[k]), int(fr.h[k]), int(fr.ws[k]))
    feats = [c.GetFeatures(ids[k]) for k in range(fr.n)]
    ns = c.profile_get("gauss_stream")[1]
    ng = c.profile_get("gauss")[1]
    c.close()
    del t
    return feats, ns, ng


def test_sift_device_batches_pitch_and_alignment(im, ctx):
    from tests.synth_frames import terrain
    big = [terrain(1100, 780, seed=70 + k) for k in range(4)]
    odd = [terrain(1101, 700, seed=80 + k) for k in range(4)]
    refs = _sift_refs(big + odd)
    rb, ro = refs[:4], refs[4:]
    routes = {}
    for name, pitches, offs in [("aligned", [3328] * 4, [0] * 4),             # stream route, rows 3328 bytes apart (not 3 w = 3300)
                                ("pitch2", [3328, 3328, 3330, 3328], [0] * 4),  # one frame with ws % 4 == 2: the whole batch on the tile route
                                ("ptr2", [3328] * 4, [0, 2, 0, 0])]:            # one frame at a +2 base pointer: likewise
        fr = pf.PitchedFrames(big, pitches, offsets=offs, seed=len(name))
        feats, ns, ng = _sift_batch(im, fr, [10, 11, 12, 13])
        for k in range(4):
            _same_features(*feats[k], rb[k], (name, k))
        routes[name] = (ns, ng)
    ns0, ng0 = routes["aligned"]
    assert ns0 > 0, routes
    for name in ("pitch2", "ptr2"):
        assert routes[name] == (ns0 - 1, ng0 + 1), routes      # the base level (one launch for the batch) moves from gauss_stream to gauss
    fr = pf.PitchedFrames(odd, [pf.ipl_pitch(1101)] * 4, offsets=[0, 1, 2, 3], seed=9)
    feats, _, _ = _sift_batch(im, fr, [20, 21, 22, 23])
    for k in range(4):
        _same_features(*feats[k], ro[k], ("ipl1101", k))
    # the host form: one padded frame of more than 512 columns at an odd address
    fr = pf.PitchedFrames(big[:1], [3331], offsets=[1], seed=3)
    kp = np.zeros(2048, im.KEYPOINT)
    desc = np.zeros((2048, 128), np.float32)
    n = C.c_int(0)
    _chk(ctx, ctx.L.mi355_sift_extract(ctx._h, 30, C.c_void_p(fr.host_ptrs()[0]), 1100, 780, 3331, _vp(kp), _vp(desc), 2048, C.byref(n)))
    _same_features(kp[:n.value], desc[:n.value], rb[0], "host")


# ---------------------------------------------------------------------------------------------- 6. SURF
def test_surf_padded_frames_host_and_device(im, ctx):
    import torch
    from tests.synth_frames import terrain
    imgs = [terrain(640, 480, seed=90), terrain(333, 257, seed=91)]
    orc = ol.load_oracle_fast()
    refs = ol.parallel_map(lambda i: orc.surf(i, 50.0, 4096), imgs)
    fr = pf.PitchedFrames(imgs, [1936, 1000], offsets=[1, 3], seed=12)
    t, ptrs = fr.to_device(torch)
    for k in range(2):
        okp, od = refs[k]
        assert len(okp) > 100
        for form in ("host", "dev"):
            kp = np.zeros(4096, im.KEYPOINT)
            desc = np.zeros((4096, 128), np.float32)
            n = C.c_int(0)
            if form == "host":
                _chk(ctx, ctx.L.mi355_surf_extract(ctx._h, 40 + k, C.c_void_p(fr.host_ptrs()[k]), int(fr.w[k]), int(fr.h[k]), int(fr.ws[k]),
                                                   C.c_float(50.0), 4096, _vp(kp), _vp(desc), C.byref(n)))
            else:
                _chk(ctx, ctx.L.mi355_surf_extract_dev(ctx._h, 50 + k, C.c_void_p(ptrs[k]), int(fr.w[k]), int(fr.h[k]), int(fr.ws[k]),
                                                       C.c_float(50.0), 4096, None))
                _chk(ctx, ctx.L.mi355_surf_get_features(ctx._h, 50 + k, _vp(kp), _vp(desc), 4096, C.byref(n)))
            m = n.value
            assert m == len(okp), (form, k, m, len(okp))
            assert np.array_equal(kp[:m].view(np.uint8), okp.view(np.uint8)), (form, k)
            assert np.array_equal(desc[:m].view(np.uint32), od.view(np.uint32)), (form, k)
    del t


# ---------------------------------------------------------------------------------------------- 7. kept frames
def test_kept_ipl_frames_render_into(im):
    from tests.synth_frames import terrain
    sizes = [(333, 257)] * 4
    imgs = [terrain(w, h, seed=100 + k) for k, (w, h) in enumerate(sizes)]
    h9s = pf.mixed_h9s(sizes, seed=7, skip=None)
    ws = pf.ipl_pitch(333)
    assert ws == 1000
    fr = pf.PitchedFrames(imgs, [ws] * 4, offsets=[0, 1, 2, 3], seed=13)
    ctx = im.Context(0)
    ctx.set_option("keep_frames", 1)
    ctx.set_option("sift_batch", 2)
    kp = np.zeros(2048, im.KEYPOINT)
    desc = np.zeros((2048, 128), np.float32)
    n = C.c_int(0)
    for k in range(4):
        p = C.c_void_p(fr.host_ptrs()[k])
        if k % 2:                                            # deferred: through the staging ring
            _chk(ctx, ctx.L.mi355_sift_extract(ctx._h, k, p, 333, 257, ws, None, None, 0, None))
        else:
            _chk(ctx, ctx.L.mi355_sift_extract(ctx._h, k, p, 333, 257, ws, _vp(kp), _vp(desc), 2048, C.byref(n)))
    ctx.synchronize()
    for k in range(4):
        assert ctx.FrameDev(k)[1:] == (333, 257, ws), k
    ref_r, cw, ch, _ = ctx.MosaicImagesRefined(imgs, h9s)
    ref_b, bw, bh, _ = ctx.MosaicBlended(imgs, h9s)
    ids = np.arange(4, dtype=np.int32)
    geom = [(333, 257, ws)] * 4
    dst = np.full((ch, 3 * cw + 9), 0xC3, np.uint8)
    ctx.MosaicImagesRefinedInto(None, ids, h9s, out=dst, geom=geom)
    assert np.array_equal(dst[:, :3 * cw], _rows(ref_r, cw)) and (dst[:, 3 * cw:] == 0xC3).all()
    dst = np.full((bh, 3 * bw + 6), 0x3C, np.uint8)
    ctx.MosaicBlendedInto(None, ids, h9s, out=dst, geom=geom)
    assert np.array_equal(dst[:, :3 * bw], _rows(ref_b, bw)) and (dst[:, 3 * bw:] == 0x3C).all()
    ctx.close()


# ---------------------------------------------------------------------------------------------- 8. the drop-in caller
def test_cxx_adaptor_odd_width_frames(tmp_path, im, oracle):
    """tests/cxx/adaptor_driver.cpp on 333- and 201-wide frames: cvCreateImage8U pads their widthStep (1000, 604)"""
    from tests.test_gpu_cxx import build_driver, read_image, run
    exe = build_driver(str(tmp_path))
    sizes = [(333, 257), (201, 150), (333, 257), (201, 150)]
    imgs = pf.mixed_images(sizes, seed=5)
    h9s = pf.mixed_h9s(sizes, seed=3, skip=None)
    fr = pf.PitchedFrames(imgs, [pf.ipl_pitch(w) for w, _ in sizes], seed=14)

    def write(k_list, hs):
        with open(tmp_path / "images.bin", "wb") as f:
            f.write(np.int32(len(k_list)).tobytes())
            for k, h9 in zip(k_list, hs):
                f.write(np.array([fr.w[k], fr.h[k], fr.ws[k]], np.int32).tobytes())
                f.write(fr.view(k).tobytes())
                f.write(np.ascontiguousarray(h9, np.float32).tobytes())

    for k in (0, 1):                                         # the warp mode warps image 0 of the file by its h9 (here a projective one)
        write([k], [h9s[3]])
        run(exe, tmp_path, "warp")
        buf, dw, dh, dws = read_image(tmp_path / "warp.out")
        rc, ref = oracle.image_projection_transform(imgs[k], h9s[3])
        assert rc == 0 and (dw, dh, dws) == ref[1:] and np.array_equal(buf, ref[0]), k
    write(range(4), h9s)
    run(exe, tmp_path, "mosaic")
    buf, cw, ch, cws = read_image(tmp_path / "mosaic.out")
    rc, ref = oracle.mosaic_images_refined(imgs, h9s)
    assert rc == 0 and (cw, ch) == ref[1:3] and np.array_equal(_rows(buf, cw), _rows(ref[0], cw))
    run(exe, tmp_path, "blend")
    buf, bw, bh, bws = read_image(tmp_path / "blend.out")
    keep = im.resample_by_overlap([w for w, _ in sizes], [h for _, h in sizes], h9s, 0.7)
    c = im.Context(0)
    want, ww, wh, _ = c.MosaicBlended(imgs, h9s, keep=keep, band=5)
    c.close()
    assert (bw, bh) == (ww, wh) and np.array_equal(_rows(buf, bw), _rows(want, ww))
