"""GPU: the narrow octaves' routes (option "narrow_routes", sift_plan::Routes::narrow) against oracle/oracle_sift.c, bit for bit, and
against the same context with the option off.

What the shapes give, from blur_streams() / blur_launch() / extrema_launch() in sift_plan.cpp with narrow = 1 (tests/test_sift_plan_narrow.py
checks those rules on the host); segments for batches of 1, 2 and 4 are STREAM_NARROW_MIN_L = 16 rows at all of these heights but 66 / 67:
  384x288, 384x289   the smallest streamed width: two strips, the second 128 columns (lanes 32 .. 63 store nothing), 18 segments + one of
                     one row at 289; 288: level 3 writes octave 1 (192x144, tiled) on the way out, 289: downsample16 does
  388x291            that width + 4: second strip 132 columns, last segment 3 rows
  380x285            just under: every level through blur16_tile, either way
  500x375, 500x376   the 12 MP frames' octave 3: second strip 244 columns, 24 segments (the last 7 / 8 rows)
  508x66, 508x67     second strip 252 columns (the widest partial one); 66 / 67 rows: five segments of 16, the last 2 / 3 rows, where
                     narrow = 0 keeps it tiled (under 512 columns)
  250x187, 127x95    stay with blur16_tile (127: width no multiple of 4; its last octave is 31x23, one tile that reflects 13 columns and rows deep)
  1000x750, 1000x751 in a batch of 4: octave 0 takes extrema_stream at the default xstream_min_w = 1000 (five strips of 200 columns x 12
                     segments), its blurs 16-row segments (4 strips x 4 frames); octave 1 = 500x375 is seeded by the ds copy (750) or by
                     downsample16 (751) and streams in 16-row segments
Contents: terrain (sparse candidates) and binary noise (saturated levels, dense candidates: the tiled extrema kernel's and the streamed
waves' lists overflow), as tests/test_gpu_sift_handoff.py uses them."""
import numpy as np
import pytest

from tests import sift_patterns as sp
from tests.synth_frames import terrain
from tests.test_gpu_sift_edges import _pmap, _same

pytestmark = pytest.mark.gpu

SHAPES = [(384, 288), (384, 289), (388, 291), (380, 285), (500, 375), (500, 376), (508, 66), (508, 67), (250, 187), (127, 95)]


def _frames(w, h, count):
    s = sp.shape_seed(w, h)
    return [terrain(w, h, seed=s + k) if k % 2 == 0 else sp.binary_noise(w, h, 17 + k) for k in range(count)]


def _extract(c, imgs):
    """the frames as one batch (sift_batch = len(imgs)) through SiftExtractDev"""
    import torch
    c.set_option("sift_batch", len(imgs))
    dev = [torch.from_numpy(np.ascontiguousarray(i)).cuda() for i in imgs]
    torch.cuda.synchronize()
    for k, (d, i) in enumerate(zip(dev, imgs)):
        c.SiftExtractDev(k, d.data_ptr(), i.shape[1], i.shape[0], 3 * i.shape[1])
    out = []
    for k in range(len(imgs)):
        kp, desc = c.GetFeatures(k, max_kp=4096)
        d8 = desc.astype(np.uint8)
        assert np.array_equal(desc, d8.astype(np.float32)), "descriptors are not integer valued"
        out.append((kp, d8))
    return out


def _both_ways(c, imgs, want, tag):
    for narrow in (1, 0, 1):
        c.set_option("narrow_routes", narrow)
        got = _extract(c, imgs)
        for k, (g, o) in enumerate(zip(got, want)):
            _same(g, o, f"{tag} frame {k} of {len(imgs)}, narrow_routes={narrow}")


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_narrow_shapes_in_batches_of_1_2_4(ctx, oracle, size):
    """four frames per shape (terrain, noise, terrain, noise): alone, as a pair and all four in one launch, narrow_routes on, off and on
    again on one context; every result equals the oracle's"""
    w, h = size
    imgs = _frames(w, h, 4)
    want = _pmap(lambda i: oracle.sift(i), imgs)
    assert len(want[0][0]) >= 50 and len(want[1][0]) >= 5, (w, h, len(want[0][0]), len(want[1][0]))      # noise: few candidates pass the edge test
    for n in (1, 2, 4):
        _both_ways(ctx, imgs[:n], want[:n], f"{w}x{h}")


@pytest.mark.parametrize("size", [(1000, 750), (1000, 751)], ids=lambda s: "%dx%d" % s)
def test_octave2_shape_in_a_batch_of_four(ctx, oracle, size):
    """library defaults: streamed extrema on octave 0, octave 1 = 500x375 through the short segments"""
    w, h = size
    imgs = _frames(w, h, 4)
    want = _pmap(lambda i: oracle.sift(i), imgs)
    assert all(len(o[0]) >= 500 for o in want)
    _both_ways(ctx, imgs, want, f"{w}x{h}")
