"""The adversarial SIFT inputs of tests/sift_patterns.py do what they are for -- checked on the CPU oracle alone, so that a GPU pass
on them (tests/test_gpu_sift_edges.py) means something and none of these conditions is ever "checked" by the code under test.

Zero keypoints are allowed for two contents only, plain `ramp` (no extremum anywhere) and `checker(2)` (a period below the smallest
SIFT scale blurs to a flat grey).  checker(3) and 0/255 bars are flat or one-dimensional in every level as well (the edge test rejects
every bar), so the content matrix carries them cut into patches (`windowed`) and next to faint blobs (`bars_blobs`), where they do
give keypoints on the saturated texture."""
import numpy as np
import pytest

from tests import sift_patterns as sp
from tests.synth_frames import terrain

IMG_BORDER = 5
TIE_CUT_SIZE = sp.TIE_CUT_SIZE


def _response_groups(kp):
    _, c = np.unique(kp["response"].view(np.uint32), return_counts=True)
    return c


def _multi_peak(kp):
    """locations (octave, x, y bits) that carry more than one keypoint, with different angles"""
    key = np.stack([kp["octave"].astype(np.int64), kp["x"].view(np.uint32).astype(np.int64), kp["y"].view(np.uint32).astype(np.int64)], 1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    n = 0
    for g in np.where(cnt > 1)[0]:
        a = kp["angle"][inv == g]
        n += int(len(np.unique(a.view(np.uint32))) > 1)
    return n


def _octave_xy(kp, w, h):
    """keypoint coordinates in the samples of their own octave, and that octave's size"""
    o = (kp["octave"] & 255).astype(np.int64)
    s = 1.0 / (1 << o).astype(np.float64)
    return kp["x"] * s, kp["y"] * s, (w >> o), (h >> o)


def test_tiled_has_tie_groups_and_the_cut_falls_inside_one(oracle):
    kp, _ = oracle.sift(sp.tiled(320, 240, 5, 32))
    assert _response_groups(kp).max() >= 8
    kp, _ = oracle.sift(sp.tiled(320, 240, 6, 48))
    assert _response_groups(kp).max() >= 8
    w, h = TIE_CUT_SIZE
    kp, _ = oracle.sift(sp.tiled(w, h, 5, 32), 2000)
    assert 2000 < len(kp) <= 2048, len(kp)
    r = np.abs(kp["response"])
    assert (r == r.min()).sum() >= 2                    # the keypoints past the 2000th are ties with it


@pytest.mark.parametrize("name", ["discs", "checker16"])
def test_symmetric_shapes_give_several_orientations_at_one_location(oracle, name):
    img = sp.discs(320, 240) if name == "discs" else sp.checker(320, 240, 16)
    kp, _ = oracle.sift(img)
    assert _multi_peak(kp) >= 4, _multi_peak(kp)


def test_one_direction_gradients_clamp_and_saturate_descriptors(oracle):
    n255 = nclamp = 0
    for img in (sp.bars_blobs(320, 240, 40), sp.ramp_blobs(320, 240, 0, seed=3), sp.clipped(320, 240, sp.CLIP_GAIN, seed=10)):
        _, d = oracle.sift(img)
        assert len(d) > 0
        n255 += int((d == 255).any(1).sum())
        nclamp += int(((d == d.max(1, keepdims=True)).sum(1) >= 2).sum())      # several equal largest bytes: all were cut at 0.2
    assert n255 >= 1 and nclamp >= 1, (n255, nclamp)
    _, d = oracle.sift(sp.bars_blobs(320, 240, 40))
    assert (d == 255).any(1).sum() >= 8                 # what bars_blobs is built for


def test_edge_dots_reach_the_border_and_never_cross_it(oracle):
    near = 0
    for (w, h) in [(320, 240), (333, 257)]:
        for d in (4, 5, 6, 7):
            kp, _ = oracle.sift(sp.edge_dots(w, h, d))
            assert len(kp) > 0, (w, h, d)
            x, y, ow, oh = _octave_xy(kp, w, h)
            # adjustLocalExtrema keeps integer sample positions IMG_BORDER <= c < n - IMG_BORDER; the sub-sample offset is below 0.5
            assert (x > IMG_BORDER - 0.5).all() and (y > IMG_BORDER - 0.5).all()
            assert (x < ow - IMG_BORDER - 0.5).all() and (y < oh - IMG_BORDER - 0.5).all()
            near += int(((x < IMG_BORDER + 1) | (y < IMG_BORDER + 1) | (x > ow - 1 - IMG_BORDER - 1) | (y > oh - 1 - IMG_BORDER - 1)).sum())
    assert near >= 50, near


def test_ramp_and_checker2_counts_are_stable(oracle):
    for img, want in [(sp.ramp(320, 240, 0), 0), (sp.ramp(333, 257, 1), 0), (sp.checker(320, 240, 2), 0), (sp.checker(333, 257, 2), 0)]:
        a, _ = oracle.sift(img)
        b, _ = oracle.sift(img)
        assert len(a) == want and len(b) == want


@pytest.mark.parametrize("size", [(320, 240), (333, 257)])
def test_content_matrix_is_not_empty(oracle, size):
    """at most the two named patterns give no keypoints, in the default and in the keep-all mode"""
    m = sp.content_matrix(*size)
    zero = [n for n, img in m.items() if len(oracle.sift(img)[0]) == 0]
    assert set(zero) <= set(sp.ZERO_KEYPOINT_PATTERNS), zero
    zero = [n for n, img in m.items() if len(oracle.sift(img, 0, 60000)[0]) == 0]
    assert set(zero) <= set(sp.ZERO_KEYPOINT_PATTERNS), zero
    over = [n for n, img in m.items() if len(oracle.sift(img, 2000, 8192)[0]) > 2048]       # nfeatures + ties beyond a feature record
    assert over == list(sp.OVER_2048_TIES), over


def test_streamed_contents_are_not_empty(oracle):
    for (w, h) in [(1100, 780), (1024, 768)]:
        for name, img in sp.streamed_contents(w, h).items():
            kp, _ = oracle.sift(img)
            assert len(kp) >= (1 if name == "checker8" else 50), (name, w, h, len(kp))      # checker(8): a handful at the frame corners only


def test_shape_matrix_runs_and_terrain_gives_keypoints(oracle):
    sizes = sp.MIN_ACCEPTED + sp.OCTAVE_BOUNDARY + sp.SMALL_OCTAVE + sp.STREAM_ADMISSION
    for k, (w, h) in enumerate(sizes):
        kp, d = oracle.sift(terrain(w, h, seed=sp.shape_seed(w, h)))
        f, b = oracle.sift_last_octaves()
        assert f == sp.n_octaves(w, h) and b == sp.n_octaves_built(w, h), (w, h, f, b)
        if min(w, h) >= 32:
            assert len(kp) >= 1, (w, h)


def test_octave_count_steps_at_the_rounding_boundaries(oracle):
    """cvRound(log2(min) - 2) steps by one across 22|23, 45|46, 90|91, 181|182 -- and the octaves actually built do not: the loop stops
    below 12 samples, which is reached first for every size (min >> o >= 12 needs o <= log2(min) - 3.58), so the rounding of the formula can
    never cost a keypoint.  The pairs stay in the GPU matrix to pin exactly that."""
    for lo, hi, n_lo in [(22, 23, 2), (45, 46, 3), (90, 91, 4), (181, 182, 5)]:
        for mk in (lambda n: (n, n), lambda n: (n, 300), lambda n: (300, n)):
            got = []
            for n in (lo, hi):
                w, h = mk(n)
                oracle.sift(terrain(w, h, seed=1))
                got.append(oracle.sift_last_octaves())
            assert got[0][0] == n_lo and got[1][0] == n_lo + 1, got
            assert got[0][1] == got[1][1] == sp.n_octaves_built(lo, lo), got


def test_small_octave_sizes_end_in_a_12_or_13_sample_octave():
    for (w, h) in sp.SMALL_OCTAVE:
        last = sp.n_octaves_built(w, h) - 1
        assert min(w >> last, h >> last) in (12, 13), (w, h)


def test_periodic_pairs_have_equal_descriptors_matches_and_inliers(oracle):
    """the inputs of the GPU pair test: identical descriptors inside a frame (equal match distances for certain), matches selected on both
    pairs, inliers on the whole-period shift"""
    w, h = 320, 240
    nins = []
    for (seed, P, dx, dy) in sp.TILED_PAIRS:
        k0, d0 = oracle.sift(sp.tiled(w, h, seed, P))
        k1, d1 = oracle.sift(sp.tiled_shifted(w, h, seed, P, dx, dy))
        _, c = np.unique(d0, axis=0, return_counts=True)
        assert c.max() >= 4
        nin, i1, i2, H, ns = oracle.match_pair(np.stack([k0["x"], k0["y"]], 1), d0, np.stack([k1["x"], k1["y"]], 1), d1, w, h, 2.5, 1)
        assert ns >= 100, ns
        nins.append(nin)
    assert nins[1] >= 8, nins
