"""GPU: extrema_stream hands every candidate's 3x3x3 DoG neighbourhood to refine_kernel (wave-private LDS ring of DoG rows -> the work
area's cube buffer) -- SIFT detect+describe through the streamed extrema route against oracle/oracle_sift.c, bit for bit.

The streamed route is forced with xstream_min_w = 256 and xstream_min_frames = 1 (as test_content_streamed_route does with 1000), which
admits every octave at least 256 x 192 with a width that is a multiple of 4.  What the sizes give, from extrema_launch() in sift_plan.cpp:
  512x384    octave 0: three strips of 172 columns x six segments of 64 rows = 18 waves (regions 0..17); octave 1 (256x192): 2 x 3
  1100x780   octave 0: five strips of 220 columns x thirteen segments (the last 12 rows high); octave 1 is 550 wide: tiled kernel
  744x1408   octave 0: three strips of 248 columns x 22 segments = 66 waves on 64 regions; octave 1 (372x704): 2 x 11
Keep-all (nfeatures = 0) returns every refined point, so it checks every candidate's first Newton step, not only the strongest 2000."""
import numpy as np
import pytest

from tests import sift_patterns as sp
from tests.synth_frames import terrain
from tests.test_gpu_sift_edges import KEEPALL_CAP, _pmap, _same

pytestmark = pytest.mark.gpu
XSTREAM_W = 256


def _context(batch, keepall=False, streamed=True):
    import imagemosaicing_amd as im
    p = im.default_params()
    if keepall:
        p.nfeatures = 0
    c = im.Context(0, p)
    if streamed:
        c.set_option("xstream_min_w", XSTREAM_W); c.set_option("xstream_min_frames", 1)
    else:
        c.set_option("blur_stream", 0)
    c.set_option("sift_batch", batch)
    return c


def _extract(c, imgs, max_kp=4096):
    """the frames as ONE batch through SiftExtractDev (the context's sift_batch is len(imgs)); (keypoints, u8 descriptors) per frame and the
    stage counters of the last frame"""
    import torch
    dev = [torch.from_numpy(np.ascontiguousarray(i)).cuda() for i in imgs]
    torch.cuda.synchronize()
    for k, (d, i) in enumerate(zip(dev, imgs)):
        c.SiftExtractDev(k, d.data_ptr(), i.shape[1], i.shape[0], 3 * i.shape[1])
    out = []
    for k in range(len(imgs)):
        kp, desc = c.GetFeatures(k, max_kp=max_kp)
        d8 = desc.astype(np.uint8)
        assert np.array_equal(desc, d8.astype(np.float32)), "descriptors are not integer valued"
        out.append((kp, d8))
    return out, c.last_sift_counters()


def _banded(w, h, seed, period=6, first=12, rows=40, every=64):
    """terrain with a band of 0/255 bars `period` wide (the value changes along x) in rows first .. first + rows - 1 of every 64-row segment.
    Bars 6 wide put the DoG maximum of a bar on its two centre columns, with equal values, in layer 2 (DoG amplitudes of a period-12 square
    wave at sigma = 1.6 * 2^(l/3): 0.131, 0.160, 0.167, 0.138, 0.079 of the step), and every row repeats it: 4 columns of 12 are tied extrema,
    57 per row of a 172-column strip.  The terrain above and below reaches about 4 sigma = 16 rows into a band through the blurs (beyond
    that its weight is below half a unit of the 16-bit levels), so the six rows in the middle of a 40-row band at least are pure bars: a
    wave that walks through them has more candidates in three rows than its list holds."""
    img = terrain(w, h, seed=seed).copy()
    bars = sp.bars(w, h, period, 0)
    for y0 in range(first, h, every):
        img[y0:y0 + rows] = bars[y0:y0 + rows]
    return np.ascontiguousarray(img)


def _small_contents(w, h):
    return {"terrain": terrain(w, h, seed=sp.shape_seed(w, h)), "tiled32": sp.tiled(w, h, 5, 32), "binary_noise": sp.binary_noise(w, h, 17)}


@pytest.fixture(scope="module")
def small():
    """512x384: the contents, and the oracle's default and keep-all results (shared by the tests below, never modified)"""
    from tests import oracle_lib
    o = oracle_lib.load_oracle()
    m = _small_contents(512, 384)
    m["banded"] = _banded(512, 384, 41)
    m["bars6"] = sp.bars(512, 384, 6, 0)
    imgs = list(m.values())
    return m, dict(zip(m, _pmap(lambda i: o.sift(i), imgs))), dict(zip(m, _pmap(lambda i: o.sift(i, 0, KEEPALL_CAP), imgs)))


@pytest.mark.parametrize("keepall", [False, True])
def test_smallest_streamed_shape(small, keepall):
    """512x384, each frame a launch of its own.  terrain: sparse candidates; tiled32: every candidate repeats on a 32-pixel grid, so they
    fall on the first and last rows of the 64-row segments and on the first and last columns of the 172-column strips (neither is a multiple
    of 32 away from the next), where the ring's priming rows and the neighbour lanes' columns are read; binary_noise: saturated 0 | 255 levels, the extremes of the
    16-bit differences the ring holds"""
    m, want, want_all = small
    c = _context(1, keepall)
    for name in ("terrain", "tiled32", "binary_noise"):
        got, cnt = _extract(c, [m[name]], KEEPALL_CAP if keepall else 4096)
        o = (want_all if keepall else want)[name]
        assert len(o[0]) >= 100, name
        print(f"{name} 512x384 keepall={keepall}: extrema {cnt[0]}, refined {cnt[1]}, keypoints {len(o[0])}")
        _same(got[0], o, f"{name} 512x384 streamed extrema" + (" keep-all" if keepall else ""))
    c.close()


def test_partial_last_segment_against_tiled_route(oracle):
    """1100x780: strips of 220 columns (lanes 56 .. 63 of every wave lie outside their strip), a last segment of 12 rows; octave 1 is not
    admitted (550 columns: not a multiple of 4) and stays with the tiled kernel.  Equal to a blur_stream = 0 context, whose extrema come
    from the tiled kernel and its own cubes, and to the oracle.  tiled32 in keep-all only: its tie group at the nfeatures cut does not fit
    the default mode's record (sift_patterns.streamed_contents)"""
    w, h = 1100, 780
    m = _small_contents(w, h)
    for keepall, names in ((False, ("terrain", "binary_noise")), (True, ("terrain", "tiled32", "binary_noise"))):
        imgs = [m[n] for n in names]
        cap = KEEPALL_CAP if keepall else 4096
        want = _pmap(lambda i: oracle.sift(i, 0, KEEPALL_CAP) if keepall else oracle.sift(i), imgs)
        cs, ct = _context(len(imgs), keepall), _context(len(imgs), keepall, streamed=False)
        got, _ = _extract(cs, imgs, cap)
        tiled, _ = _extract(ct, imgs, cap)
        for n, g, t, o in zip(names, got, tiled, want):
            assert len(o[0]) >= 500, n
            _same(g, o, f"{n} {w}x{h} keepall={keepall} streamed extrema")
            _same(t, g, f"{n} {w}x{h} keepall={keepall} blur_stream=0")
        cs.close(); ct.close()


@pytest.mark.parametrize("keepall", [False, True])
def test_list_overflow_mixes_records_with_and_without_cube(small, keepall):
    """`banded` (see _banded): every wave of octave 0 meets 57 tied extrema per row in the middle of rows 12 .. 51 of its segment -- more in
    three rows than the 144 records its list holds -- and finishes the segment in the plain loop, whose records carry no cube: every region
    then holds terrain candidates with a cube (rows 0 .. 11) and without (rows 52 .. 63); the oracle has keypoints on both sides.  `bars6`
    is the band alone (no keypoint survives the edge test); binary_noise has few extrema and stays in the row loop.  The extrema counts are the check
    that the bars are what they are meant to be: a third of the tested pixels of bars6, and in `banded` at least the six pure rows x six
    segments x (502 columns / 3) = 5940."""
    m, want, want_all = small
    c = _context(1, keepall)
    for name in ("banded", "bars6", "binary_noise"):
        got, cnt = _extract(c, [m[name]], KEEPALL_CAP if keepall else 4096)
        o = (want_all if keepall else want)[name]
        print(f"{name} 512x384 keepall={keepall}: extrema {cnt[0]}, refined {cnt[1]}, keypoints {len(o[0])}")
        if name == "banded":
            assert cnt[0] > 5940 and len(o[0]) >= 300
        if name == "bars6":
            assert cnt[0] > 0.3 * 502 * 374
        _same(got[0], o, f"{name} 512x384 list overflow" + (" keep-all" if keepall else ""))
    c.close()


def test_cube_overflow(oracle):
    """744x1408, bars 6 wide except for a band of terrain in rows 640 .. 831.  cube_cap = 744 * 1408 / 256 + 4096 = 8188 cubes per region.
    From the period (see _banded): a third of the 238 / 248 / 238 tested columns of a strip are tied extrema in every tested row, 79 to 83
    per row.  Regions 0 and 1 receive two waves each, segment 0 (rows 5 .. 63) and segment 21 (rows 1344 .. 1402): 2 x 59 rows x 79 = 9322
    candidates at least, more than cube_cap; every other region receives one wave, at most 64 x 83 = 5312.  The frame's extrema count is
    asserted at that density.  With ties this dense a wave leaves the row loop after three rows, so most records behind a region's
    cube_cap come from the plain loop; which of the row loop's flushes land behind it is a matter of timing, and either way they must leave
    without the cube bit.  The terrain band gives the keypoints (segments 10 .. 12, regions 30 .. 38)."""
    w, h = 744, 1408
    img = sp.bars(w, h, 6, 0)
    img[640:832] = terrain(w, 192, seed=43)
    img = np.ascontiguousarray(img)
    for keepall in (False, True):
        o = oracle.sift(img, 0, KEEPALL_CAP) if keepall else oracle.sift(img)
        assert len(o[0]) >= 500
        c = _context(1, keepall)
        got, cnt = _extract(c, [img], KEEPALL_CAP if keepall else 4096)
        print(f"bars6 + terrain band {w}x{h} keepall={keepall}: extrema {cnt[0]}, refined {cnt[1]}, keypoints {len(o[0])}")
        assert cnt[0] > 0.3 * (w - 10) * (h - 10 - 192)
        _same(got[0], o, f"cube overflow {w}x{h} keepall={keepall}")
        c.close()


def test_batch_of_four_equals_single_frames(small):
    """four different contents in one launch: each frame equals its single-frame result (the oracle's), which checks the per-frame stride of
    the cube buffer and of the region counters"""
    m, want, want_all = small
    names = ("terrain", "tiled32", "binary_noise", "banded")
    for keepall in (False, True):
        c = _context(4, keepall)
        got, _ = _extract(c, [m[n] for n in names], KEEPALL_CAP if keepall else 4096)
        for n, g in zip(names, got):
            _same(g, (want_all if keepall else want)[n], f"{n} 512x384 in a batch of four, keepall={keepall}")
        c.close()
