"""GPU: frames kept in HBM after their extraction (option "keep_frames") and the renders that write straight into caller memory
(mi355_mosaic_refined_into / mi355_mosaic_blended_into).  The reference's driver extracts features from its host frames and renders the
same frames with the same indices (MosaicWithoutPos.cpp:4430-4679); these tests hold the new path to the bytes of the host entry points
mi355_mosaic_refined / mi355_mosaic_blended (themselves held to the oracle elsewhere, and here once more on the small strip)."""
import numpy as np
import pytest

from tests.synth_frames import strip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def im():
    import imagemosaicing_amd
    return imagemosaicing_amd


@pytest.fixture(scope="module")
def small():
    frames, Hs = strip(6, 640, 480, seed=11)
    return frames, np.stack([H.reshape(9) for H in Hs]).astype(np.float32)


@pytest.fixture(scope="module")
def medium():
    # a canvas of ~24 MB: dozens of 1 MB download chunks and a partial last one
    frames, Hs = strip(8, 1600, 1200, seed=5)
    return frames, np.stack([H.reshape(9) for H in Hs]).astype(np.float32)


def _ctx(im, keep=1, batch=None):
    ctx = im.Context(0)
    ctx.set_option("keep_frames", keep)
    if batch:
        ctx.set_option("sift_batch", batch)
    return ctx


def _rows(buf, cw):
    return np.ascontiguousarray(buf[:, :3 * cw])


def _extract(ctx, frames, deferred_ids):
    for k, f in enumerate(frames):
        if k in deferred_ids:
            ctx.SiftExtractHost(k, f)
        else:
            ctx.SiftExtract(k, f)
    ctx.synchronize()


def test_kept_frames_are_used_and_match_the_host_entry_points(im, small, oracle):
    frames, h9s = small
    n = len(frames)
    orig = [f.copy() for f in frames]
    ctx = _ctx(im, batch=4)
    _extract(ctx, [f.copy() for f in frames], deferred_ids={0, 2, 3, 5})       # both forms: deferred (batched) and synchronous
    ref_r, cw, ch, _ = ctx.MosaicImagesRefined(orig, h9s)
    ref_b, bw, bh, _ = ctx.MosaicBlended(orig, h9s)
    # the oracle once on this strip: the host entry point is what the new path must equal
    _, oref = oracle.mosaic_images_refined(orig, h9s)
    assert np.array_equal(_rows(ref_r, cw), _rows(oref[0], cw))
    # the caller's arrays are overwritten after extraction: a render that uploads again would see the garbage
    garbage = [np.full_like(f, 77) for f in frames]
    ids = np.arange(n, dtype=np.int32)
    out, cw2, ch2 = ctx.MosaicImagesRefinedInto(garbage, ids, h9s)
    assert (cw2, ch2) == (cw, ch)
    assert np.array_equal(_rows(out, cw), _rows(ref_r, cw))
    outb, bw2, bh2 = ctx.MosaicBlendedInto(garbage, ids, h9s)
    assert (bw2, bh2) == (bw, bh)
    assert np.array_equal(_rows(outb, bw), _rows(ref_b, bw))
    # no host pointers at all
    out, _, _ = ctx.MosaicImagesRefinedInto(None, ids, h9s)
    assert np.array_equal(_rows(out, cw), _rows(ref_r, cw))
    # mixed sources: even images from their kept frames, odd ones from the host
    mixed = np.where(ids % 2 == 0, ids, -1).astype(np.int32)
    src = [None if mixed[k] >= 0 else orig[k] for k in range(n)]
    out, _, _ = ctx.MosaicImagesRefinedInto(src, mixed, h9s)
    assert np.array_equal(_rows(out, cw), _rows(ref_r, cw))
    outb, _, _ = ctx.MosaicBlendedInto(src, mixed, h9s)
    assert np.array_equal(_rows(outb, bw), _rows(ref_b, bw))
    # all from the host (img_ids None): the old path through the new destination
    out, _, _ = ctx.MosaicImagesRefinedInto(orig, None, h9s)
    assert np.array_equal(_rows(out, cw), _rows(ref_r, cw))
    ctx.close()


def test_destination_pitch_padding_and_chunks(im, medium):
    frames, h9s = medium
    n = len(frames)
    ctx = _ctx(im)
    _extract(ctx, frames, deferred_ids=set(range(n)))
    ref_r, cw, ch, _ = ctx.MosaicImagesRefined(frames, h9s)
    ref_b, bw, bh, _ = ctx.MosaicBlended(frames, h9s)
    ids = np.arange(n, dtype=np.int32)
    for chunk_mb in (64, 1):
        ctx.set_option("download_chunk_mb", chunk_mb)
        if chunk_mb == 1:
            assert ch * ((3 * cw + 3) & ~3) > 20 * (1 << 20) and (ch * ((3 * cw + 3) & ~3)) % (1 << 20) != 0      # dozens of chunks, a partial last one
        for threads in (1, 4):
            ctx.set_option("download_threads", threads)
            pitch = 3 * cw + 37
            dst = np.full((ch, pitch), 0xA5, np.uint8)
            out, _, _ = ctx.MosaicImagesRefinedInto(None, ids, h9s, out=dst)
            assert out is dst
            assert np.array_equal(dst[:, :3 * cw], _rows(ref_r, cw))
            assert (dst[:, 3 * cw:] == 0xA5).all(), "row padding written"
            pitch = 3 * bw + 5
            dstb = np.full((bh, pitch), 0x5A, np.uint8)
            ctx.MosaicBlendedInto(None, ids, h9s, out=dstb)
            assert np.array_equal(dstb[:, :3 * bw], _rows(ref_b, bw))
            assert (dstb[:, 3 * bw:] == 0x5A).all(), "row padding written"
    # the measurement modes give the same bytes
    for mode in (1, 2):
        ctx.set_option("download_mode", mode)
        dst = np.full((ch, 3 * cw + 11), 0xA5, np.uint8)
        ctx.MosaicImagesRefinedInto(None, ids, h9s, out=dst)
        assert np.array_equal(dst[:, :3 * cw], _rows(ref_r, cw)) and (dst[:, 3 * cw:] == 0xA5).all()
    ctx.close()


def test_replacement_follows_the_second_frame(im, small):
    frames, h9s = small
    a, b = frames[3], frames[4]          # same geometry, different pixels
    ctx = _ctx(im, batch=8)
    ref = _ctx(im, keep=0)
    for k in range(3):
        ctx.SiftExtractHost(k, frames[k])
    ctx.SiftExtractHost(3, a.copy())     # parked in a batch that has not run yet ...
    ctx.SiftExtractHost(3, b.copy())     # ... and replaced at once
    ctx.synchronize()
    kb, db = ref.SiftExtract(3, b)
    k3, d3 = ctx.GetFeatures(3)
    assert len(k3) == len(kb) and np.array_equal(k3.view(np.uint8), kb.view(np.uint8)) and np.array_equal(d3, db)
    srcs = [frames[0], frames[1], frames[2], b]
    sub = h9s[:4].copy()
    want, cw, ch, _ = ref.MosaicImagesRefined(srcs, sub)
    out, _, _ = ctx.MosaicImagesRefinedInto(None, np.arange(4, dtype=np.int32), sub)
    assert np.array_equal(_rows(out, cw), _rows(want, cw))
    wantb, bw, _, _ = ref.MosaicBlended(srcs, sub)
    outb, _, _ = ctx.MosaicBlendedInto(None, np.arange(4, dtype=np.int32), sub)
    assert np.array_equal(_rows(outb, bw), _rows(wantb, bw))
    ctx.close(); ref.close()


def test_keep_frames_does_not_change_features(im, small):
    frames, _ = small
    n = len(frames)
    pairs = im.pair_schedule(n, 182)
    got = []
    for keep in (0, 1):
        ctx = _ctx(im, keep=keep, batch=4)
        _extract(ctx, frames, deferred_ids={1, 2, 4})
        feats = [ctx.GetFeatures(k) for k in range(n)]
        res = ctx.MatchPairs(pairs, 2.5, 7)
        got.append((feats, res))
        ctx.close()
    (f0, r0), (f1, r1) = got
    for (ka, da), (kb, db) in zip(f0, f1):
        assert np.array_equal(ka.view(np.uint8), kb.view(np.uint8)) and np.array_equal(da, db)
    assert r0.tobytes() == r1.tobytes()


def test_frame_dev_feeds_the_dev_entry_points(im, small):
    import torch
    frames, h9s = small
    n = len(frames)
    ctx = _ctx(im)
    _extract(ctx, frames, deferred_ids=set(range(n)))
    ref_r, cw, ch, cws = ctx.MosaicImagesRefined(frames, h9s)
    ref_b, bw, bh, bws = ctx.MosaicBlended(frames, h9s)
    fd = [ctx.FrameDev(k) for k in range(n)]
    for k, (d, w, h, ws) in enumerate(fd):
        assert d and (w, h, ws) == (frames[k].shape[1], frames[k].shape[0], frames[k].strides[0])
    d_ptrs = [x[0] for x in fd]
    w = [x[1] for x in fd]; h = [x[2] for x in fd]; ws = [x[3] for x in fd]
    canvas = torch.empty((ch, cws), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    half = ch // 2
    ctx.MosaicImagesRefinedDev(d_ptrs, w, h, ws, h9s, canvas.data_ptr(), cw, ch, cws, 0, half)
    ctx.MosaicImagesRefinedDev(d_ptrs, w, h, ws, h9s, canvas.data_ptr(), cw, ch, cws, half, ch - half)
    ctx.synchronize()
    got = canvas.cpu().numpy()
    assert np.array_equal(_rows(got, cw), _rows(ref_r, cw))
    parts = []
    for r0, rows in ((0, bh // 3), (bh // 3, bh - bh // 3)):
        t, _, _, _ = ctx.MosaicBlendedDev(d_ptrs, w, h, ws, h9s, row0=r0, rows=rows)
        parts.append(t.cpu().numpy())
    assert np.array_equal(_rows(np.concatenate(parts), bw), _rows(ref_b, bw))
    ctx.close()


def test_errors_name_their_cause(im, small):
    import ctypes as C
    frames, h9s = small
    n = len(frames)
    ctx = im.Context(0)
    # keep_frames never set: nothing is kept
    ctx.SiftExtract(0, frames[0])
    with pytest.raises(im.Mi355Error) as e:
        ctx.FrameDev(0)
    assert e.value.code == -1 and "no kept frame" in str(e.value)
    ctx.set_option("keep_frames", 1)
    _extract(ctx, frames, deferred_ids=set(range(n)))
    ids = np.arange(n, dtype=np.int32)
    # unknown id
    bad = ids.copy(); bad[2] = 99
    geom = [(f.shape[1], f.shape[0], f.strides[0]) for f in frames]
    with pytest.raises(im.Mi355Error) as e:
        ctx.MosaicImagesRefinedInto(None, bad, h9s, geom=geom)
    assert e.value.code == -1 and "image 2" in str(e.value) and "id 99" in str(e.value)
    with pytest.raises(im.Mi355Error) as e:
        ctx.MosaicBlendedInto(None, bad, h9s, geom=geom)
    assert e.value.code == -1 and "image 2" in str(e.value) and "id 99" in str(e.value)
    # geometry mismatch: image 1 said to be its own kept frame, but the kept frame of id 1 is said to be narrower
    g2 = list(geom); g2[1] = (geom[1][0] - 4, geom[1][1], geom[1][2])
    with pytest.raises(im.Mi355Error) as e:
        ctx.MosaicImagesRefinedInto(None, ids, h9s, geom=g2)
    assert e.value.code == -1 and "image 1" in str(e.value) and "id 1" in str(e.value)
    # a skipped image is neither read nor checked
    hs = h9s.copy(); hs[2, 8] = 0.0
    ctx.MosaicImagesRefinedInto(None, bad, hs, geom=geom)
    # wrong cw / ch, dst_pitch < 3 * cw: straight through the C ABI
    L = ctx.L
    w = np.array([g[0] for g in geom], np.int32); h = np.array([g[1] for g in geom], np.int32); ws = np.array([g[2] for g in geom], np.int32)
    cw, ch, cws, _ = im.mosaic_layout(w, h, h9s)
    dst = np.zeros((ch + 1, cws + 8), np.uint8)
    args = lambda: (ctx._h, None, ids.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p),
                    ws.ctypes.data_as(C.c_void_p), n, h9s.ctypes.data_as(C.c_void_p))
    err = lambda: (L.mi355_last_error(ctx._h) or b"").decode()
    assert L.mi355_mosaic_refined_into(*args(), C.c_void_p(dst.ctypes.data), cws, cw + 1, ch) == -1 and "layout" in err()
    assert L.mi355_mosaic_refined_into(*args(), C.c_void_p(dst.ctypes.data), cws, cw, ch - 1) == -1 and "layout" in err()
    assert L.mi355_mosaic_refined_into(*args(), C.c_void_p(dst.ctypes.data), 3 * cw - 1, cw, ch) == -1 and "dst_pitch" in err()
    bw, bh, bws = im.blend_layout(w, h, h9s)
    dstb = np.zeros((bh + 1, bws + 8), np.uint8)
    assert L.mi355_mosaic_blended_into(*args(), None, 5, C.c_void_p(dstb.ctypes.data), bws, bw, bh + 1) == -1 and "layout" in err()
    assert L.mi355_mosaic_blended_into(*args(), None, 5, C.c_void_p(dstb.ctypes.data), 3 * bw - 1, bw, bh) == -1 and "dst_pitch" in err()
    # the refined form keeps mi355_mosaic_refined's n <= 1 convention
    assert L.mi355_mosaic_refined_into(ctx._h, None, ids.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p),
                                       ws.ctypes.data_as(C.c_void_p), 1, h9s.ctypes.data_as(C.c_void_p), C.c_void_p(dst.ctypes.data), cws, cw, ch) == -2
    # dropped frames are gone; the others stay
    ctx.DropFrames(3)
    with pytest.raises(im.Mi355Error) as e:
        ctx.FrameDev(3)
    assert e.value.code == -1 and "3" in str(e.value)
    assert ctx.FrameDev(4)[0]
    ctx.DropFrames(-1)
    for k in range(n):
        with pytest.raises(im.Mi355Error):
            ctx.FrameDev(k)
    # features outlive the frames (mi355_drop_frames is not mi355_drop_features)
    assert len(ctx.GetFeatures(1)[0]) > 0
    ctx.close()


def test_surf_extraction_keeps_frames(im, small):
    frames, h9s = small
    n = len(frames)
    ctx = _ctx(im)
    for k in range(n):
        ctx.SurfExtract(k, frames[k])
    ref, cw, _, _ = ctx.MosaicImagesRefined(frames, h9s)
    out, _, _ = ctx.MosaicImagesRefinedInto([np.zeros_like(f) for f in frames], np.arange(n, dtype=np.int32), h9s)
    assert np.array_equal(_rows(out, cw), _rows(ref, cw))
    ctx.close()


def test_full_size_strip_kept_vs_host_entry_point(im):
    """20 frames of 4000 x 3000 along a C3-like strip: kept frames + _into vs mi355_mosaic_refined on the host frames, byte for byte"""
    import torch
    from tests.synth_survey import render_frames, host_image, affine3
    n, w, h = 20, 4000, 3000
    ctx = _ctx(im)
    fr, A, _, ws = render_frames(ctx, torch, n, w, h, per_row=25)
    imgs = [host_image(fr, k, w, h, ws) for k in range(n)]
    del fr
    torch.cuda.empty_cache()
    for k in range(n):
        ctx.SiftExtractHost(k, imgs[k])
    ctx.synchronize()
    h9s = np.stack([affine3(A[k]).reshape(9) for k in range(n)]).astype(np.float32)
    ref, cw, ch, _ = ctx.MosaicImagesRefined(imgs, h9s)
    dst = np.empty((ch, 3 * cw), np.uint8)
    ctx.MosaicImagesRefinedInto(None, np.arange(n, dtype=np.int32), h9s, out=dst)
    assert cw > 30000 and np.array_equal(dst, _rows(ref, cw))
    ctx.close()
