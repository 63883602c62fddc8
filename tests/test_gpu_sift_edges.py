"""GPU: SIFT detect+describe (HIP) vs oracle/oracle_sift.c, bit for bit, at the size limits and on adversarial content.
tests/test_sift_patterns_oracle.py shows on the oracle alone that these inputs hold what they are for (tie groups, several orientations
at one location, clamped and saturated descriptors, keypoints at IMG_BORDER) and that none but `ramp` and `checker(2)` is empty.

Which levels go through blur16_stream, from the rule in blur_streams() (w % 4 == 0, w >= 512, h >= 64, last strip w % 256 == 0 or > 16;
the decimation is fused into level 3 only on an even height), not from a run -- every level of an octave is admitted or refused together:
  512x64   octave 0 streams, level 3 with the fused decimation; octave 1 = 256x32 does not (width)
  512x65   octave 0 streams, level 3 without the decimation (odd height); octave 1 no
  512x63   nothing streams (height)          508x64  nothing streams (width)
  516x64   nothing streams (last strip 4)    528x64  nothing streams (last strip 16 = MAX_R)
  532x64   octave 0 streams (last strip 20); octave 1 = 266x32 no
  532x129  octave 0 streams, no fused decimation (odd height); octave 1 = 266x64 no (width)
  1024x64  octave 0 streams; octave 1 = 512x32 no (height)
  1024x127 octave 0 streams, no fused decimation; octave 1 = 512x63 no (height)
  4096x64  octave 0 streams (16 strips, one row segment); octave 1 = 2048x32 no (height)
  4096x66  octave 0 streams with the fused decimation; octave 1 = 2048x33 no
  2048x100, 2048x104  octave 0 streams; octave 1 = 1024x50 / 1024x52 no (height); octave 3 is 12 / 13 rows high
  1024x208 octaves 0 and 1 (512x104) stream; octave 4 = 64x13
  4000x16  nothing streams (height), one octave; 16x4000 likewise"""
import numpy as np
import pytest

from tests import sift_patterns as sp
from tests.synth_frames import terrain
from tests.test_gpu_sift import _check

pytestmark = pytest.mark.gpu
KEEPALL_CAP = 32768


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_keepall():
    import imagemosaicing_amd as im
    p = im.default_params()
    p.nfeatures = 0
    c = im.Context(0, p)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_nostream():
    import imagemosaicing_amd as im
    c = im.Context(0)
    c.set_option("blur_stream", 0)
    yield c
    c.close()


def _pmap(fn, items):
    from tests import oracle_lib
    return oracle_lib.parallel_map(fn, items)


def _same(a, b, tag):
    assert len(a[0]) == len(b[0]), f"{tag}: {len(a[0])} vs {len(b[0])} keypoints"
    assert np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8)), f"{tag}: keypoints differ"
    assert np.array_equal(np.asarray(a[1]).astype(np.uint8), np.asarray(b[1]).astype(np.uint8)), f"{tag}: descriptors differ"


def _check_keepall(ctx_keepall, oracle, img, tag):
    kp, desc = ctx_keepall.SiftExtract(8, img, max_kp=KEEPALL_CAP)
    okp, odesc = oracle.sift(img, 0, KEEPALL_CAP)
    d8 = desc.astype(np.uint8)
    assert np.array_equal(desc, d8.astype(np.float32)), "descriptors are not integer valued"
    _same((kp, d8), (okp, odesc), tag + " keep-all")


def _shape_inputs(sizes):
    """terrain at every size, one tiled and one binary_noise frame per group (at its first and last size)"""
    out = [(f"terrain {w}x{h}", terrain(w, h, seed=sp.shape_seed(w, h))) for (w, h) in sizes]
    (w, h), (w2, h2) = sizes[0], sizes[-1]
    out.append((f"tiled {w}x{h}", sp.tiled(w, h, 5, 32)))
    out.append((f"binary_noise {w2}x{h2}", sp.binary_noise(w2, h2, 17)))
    return out


# ---- content ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(320, 240), (333, 257)])
def test_content_default_and_keepall(ctx, ctx_keepall, oracle, size):
    """every pattern, nfeatures = 2000 and keep-all; 333x257 has an odd width: tile blur on every level, no fused decimation.  checker(16)
    ties more than 2048 keypoints at the nfeatures cut: the default mode refuses it (documented limit, include/mi355_mosaic.h) and goes on
    working, keep-all takes it"""
    import imagemosaicing_amd as im
    w, h = size
    total = 0
    for name, img in sp.content_matrix(w, h).items():
        _check_keepall(ctx_keepall, oracle, img, f"{name} {w}x{h}")
        if name in sp.OVER_2048_TIES:
            assert len(oracle.sift(img, 2000, 8192)[0]) > 2048
            with pytest.raises(im.Mi355Error, match="overflow"):
                ctx.SiftExtract(7, img)
            continue
        kp, _ = _check(ctx, oracle, img, f"{name} {w}x{h}")
        assert (len(kp) == 0) == (name in sp.ZERO_KEYPOINT_PATTERNS), name
        total += len(kp)
    assert total > 4000


def test_tie_cut_inside_a_group(ctx, oracle):
    """more than nfeatures keypoints come back: the cut at the 2000th response falls inside a group of bit-equal responses"""
    kp, _ = _check(ctx, oracle, sp.tiled(*sp.TIE_CUT_SIZE, 5, 32), "tiled tie cut")
    assert 2000 < len(kp) <= 2048


@pytest.mark.parametrize("size", [(1100, 780), (1024, 768)])
def test_content_streamed_route(ctx, ctx_nostream, oracle, size):
    """levels >= 512 columns through blur16_stream (1100: partial last strip): against the oracle and a blur_stream = 0 context; then as one
    batch through the streamed extrema kernel (xstream_min_w lowered as in test_sift_streamed_extrema), where checker / tiled frames are
    full of tied extrema that are kept"""
    import torch
    import imagemosaicing_amd as im
    w, h = size
    m = sp.streamed_contents(w, h)
    want = _pmap(lambda img: oracle.sift(img), list(m.values()))
    ref = []
    for (name, img), o in zip(m.items(), want):
        got = ctx.SiftExtract(7, img)
        _same(got, o, f"{name} {w}x{h}")
        _same(ctx_nostream.SiftExtract(7, img), got, f"{name} {w}x{h} blur_stream=0")
        ref.append(got)
    c = im.Context(0)
    c.set_option("xstream_min_w", 1000); c.set_option("xstream_min_frames", 1); c.set_option("sift_batch", len(m))
    dev = [torch.from_numpy(np.ascontiguousarray(i)).cuda() for i in m.values()]
    torch.cuda.synchronize()
    for k, d in enumerate(dev):
        c.SiftExtractDev(k, d.data_ptr(), w, h, 3 * w)
    for k, name in enumerate(m):
        _same(c.GetFeatures(k), ref[k], f"{name} {w}x{h} streamed extrema")
    c.close()


def test_tiled32_streamed_route_keepall(oracle):
    """tiled(P = 32) at the streamed sizes: tie groups of hundreds of keypoints, which only the keep-all mode holds -- against the oracle, a
    blur_stream = 0 context, and as a batch through the streamed extrema kernel"""
    import torch
    import imagemosaicing_amd as im
    p = im.default_params()
    p.nfeatures = 0
    sizes = [(1100, 780), (1024, 768)]
    imgs = [sp.tiled(w, h, 5, 32) for (w, h) in sizes]
    want = _pmap(lambda img: oracle.sift(img, 0, KEEPALL_CAP), imgs)
    c, c0, cx = im.Context(0, p), im.Context(0, p), im.Context(0, p)
    c0.set_option("blur_stream", 0)
    cx.set_option("xstream_min_w", 1000); cx.set_option("xstream_min_frames", 1); cx.set_option("sift_batch", 2)
    for k, ((w, h), img, o) in enumerate(zip(sizes, imgs, want)):
        assert len(o[0]) > 4096 and np.unique(o[0]["response"].view(np.uint32), return_counts=True)[1].max() >= 100
        got = c.SiftExtract(7, img, max_kp=KEEPALL_CAP)
        _same(got, o, f"tiled32 {w}x{h} keep-all")
        _same(c0.SiftExtract(7, img, max_kp=KEEPALL_CAP), got, f"tiled32 {w}x{h} keep-all blur_stream=0")
        dev = [torch.from_numpy(np.ascontiguousarray(img)).cuda() for _ in range(2)]
        torch.cuda.synchronize()
        for j, d in enumerate(dev):
            cx.SiftExtractDev(10 * k + j, d.data_ptr(), w, h, 3 * w)
        for j in range(2):
            _same(cx.GetFeatures(10 * k + j, max_kp=KEEPALL_CAP), got, f"tiled32 {w}x{h} keep-all streamed extrema")
    c.close(); c0.close(); cx.close()


# ---- shape --------------------------------------------------------------------------------------------------------------------------
def _run_shapes(ctx, oracle, sizes, other=None):
    items = _shape_inputs(sizes)
    want = _pmap(lambda it: oracle.sift(it[1]), items)
    for (tag, img), o in zip(items, want):
        got = ctx.SiftExtract(7, img)
        d8 = got[1].astype(np.uint8)
        assert np.array_equal(got[1], d8.astype(np.float32)), "descriptors are not integer valued"
        _same(got, o, tag)
        if min(img.shape[:2]) >= 32 and tag.startswith("terrain"):
            assert len(got[0]) >= 1, tag
        if other is not None:
            _same(other.SiftExtract(7, img), got, tag + " blur_stream=0")


def test_minimum_size_and_refusals(ctx, oracle):
    """16 samples is the accepted minimum on either side; below it the call is refused on the host, before any launch, and the context goes on
    working"""
    import imagemosaicing_amd as im
    _run_shapes(ctx, oracle, sp.MIN_ACCEPTED)
    normal = terrain(200, 160, seed=31)
    first = _check(ctx, oracle, normal, "200x160")
    for (w, h) in sp.REFUSED:
        with pytest.raises(im.Mi355Error):
            ctx.SiftExtract(7, np.full((h, w, 3), 90, np.uint8))
        again = ctx.SiftExtract(7, normal)
        assert np.array_equal(again[0].view(np.uint8), first[0].view(np.uint8)) and np.array_equal(again[1].astype(np.uint8), first[1])


def test_octave_count_boundaries(ctx, oracle):
    """min(w, h) either side of every rounding step of cvRound(log2(min) - 2)"""
    _run_shapes(ctx, oracle, sp.OCTAVE_BOUNDARY)


def test_octaves_of_12_and_13_samples(ctx, ctx_nostream, oracle):
    """the last octave is 12 or 13 samples wide / high, the largest blur radius is 13: reflect-101 folds twice and the halo is wider than the
    image; the three wide sizes stream their big octaves first"""
    _run_shapes(ctx, oracle, sp.SMALL_OCTAVE, ctx_nostream)


def test_streaming_admission_sizes(ctx, ctx_nostream, oracle):
    """either side of every term of blur_streams() (see the table in the module docstring), blur_stream on and off"""
    _run_shapes(ctx, oracle, sp.STREAM_ADMISSION, ctx_nostream)


@pytest.mark.parametrize("batch,slots", [(3, 1), (3, 3), (8, 1), (8, 3)])
def test_mixed_size_batches_equal_single(ctx, batch, slots):
    """the shape matrix through SiftExtractDev: runs of equal sizes (which share a batch) broken by size changes inside a batch, the smallest
    frame next to the largest"""
    import torch
    import imagemosaicing_amd as im
    sizes = ([(16, 16)] * 2 + [(4096, 66)] + [(16, 16)] + [(4000, 16)] * 2 + [(16, 4000)] + [(24, 24)] * 3 + [(2048, 104)] * 2 + [(26, 300)]
             + [(300, 25)] * 2 + [(532, 64)] * 4 + [(528, 64)] + [(512, 65)] * 2 + [(1024, 208)] * 3 + [(23, 23), (22, 22), (46, 260)]
             + [(111, 111)] * 2 + [(1024, 127)] * 2 + [(55, 300)])
    imgs = [terrain(w, h, seed=300 + k) if k % 5 else sp.tiled(w, h, 5 + k, 32) for k, (w, h) in enumerate(sizes)]
    ref = [ctx.SiftExtract(900 + k, img) for k, img in enumerate(imgs)]
    c = im.Context(0)
    c.set_option("sift_batch", batch); c.set_option("sift_slots", slots)
    dev = [torch.from_numpy(np.ascontiguousarray(i)).cuda() for i in imgs]
    torch.cuda.synchronize()
    for k, d in enumerate(dev):
        c.SiftExtractDev(k, d.data_ptr(), sizes[k][0], sizes[k][1], sizes[k][0] * 3)
    for k in range(len(imgs)):
        _same(c.GetFeatures(k), ref[k], f"batch {batch} slots {slots}: frame {k} ({sizes[k][0]}x{sizes[k][1]})")
    c.close()


# ---- pair stage on tied features ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sp.TILED_PAIRS)
def test_pair_stage_on_periodic_frames(ctx, oracle, pair):
    """two views of one tiled texture: many descriptor distances are equal, so the matcher's lowest-index rule and the order of the sorted
    match list decide the records -- on real SIFT output (sift_patterns.TILED_PAIRS says what each pair ends with)"""
    w, h = 320, 240
    seed, P, dx, dy = pair
    f0, f1 = sp.tiled(w, h, seed, P), sp.tiled_shifted(w, h, seed, P, dx, dy)
    (k0, d0), (k1, d1) = _check(ctx, oracle, f0, "tiled"), _check(ctx, oracle, f1, "tiled shifted")
    ctx.SiftExtract(0, f0); ctx.SiftExtract(1, f1)
    res = ctx.MatchPairs([(0, 1)], 2.5, 1)[0]
    nin, i1, i2, Ho, ns = oracle.match_pair(np.stack([k0["x"], k0["y"]], 1), d0, np.stack([k1["x"], k1["y"]], 1), d1, w, h, 2.5, 1)
    assert ns >= 100
    n_in = int(res["n_in"])                              # the record keeps the raw count, the oracle returns 0 for a pair below 31 inliers
    assert (n_in if n_in > 30 else 0) == nin and int(res["accepted"]) == int(nin > 0) and ns == int(res["n_selected"])
    assert np.array_equal(res["a"][:nin], i1[:nin]) and np.array_equal(res["b"][:nin], i2[:nin])
    if nin > 0:                                          # a rejected pair's record carries no H
        assert np.array_equal(res["H"].view(np.uint32), Ho.view(np.uint32))
