"""Seeded adversarial inputs for SURF detect+describe and its pair stage (numpy / the terrain generator / tests/sift_patterns.py only).

What each is for (tests/test_surf_patterns_oracle.py checks on the oracle alone that the inputs do it):
  tiled / impulses / discs / checker3_windowed : groups of keypoints with bit-equal response -- the tie order (octave, layer, row, column) of
                                                 the 64-bit sort key, and a max_kp cut that falls inside a group (TIE_CUT)
  binary_noise at 16383x40 / 40x16383          : keypoints past column / row 8191 -- the 14-bit row and column fields of that key
  bright                                       : a gray sum above 2^32 -- the integral image modulo 2^32, keypoints below the wrap row
  the shape matrix                             : frames where only some filter sizes (9, 15, 21, 27) << o fit, frames smaller than the 64 x 16
                                                 tile of the octave-0 Hessian kernel and frames that end one sample either side of a tile edge
  dup_pair                                     : one patch pasted several times into the train frame -- bit-equal train descriptors, queries whose
                                                 minimum distance is attained by several train rows, in a pair that still selects matches
  tiled pair / self pair                       : every query ties; the threshold walk runs down to distT <= 0 and ends with nothing selected
Everything is deterministic: the same arguments give the same bytes."""
import numpy as np

from tests import sift_patterns as sp
from tests.synth_frames import terrain

THR = 50.0                        # minHessian of the reference (MosaicWithoutPos.h:71)
THR_SHAPE = 1.0                   # the shape matrix: tiny frames, every maximum counts
KEEP_ALL = 1 << 16                # more than any frame here returns


def flat(w, h, level=90):
    return np.full((h, w, 3), level, np.uint8)


def content_matrix(w, h):
    """name -> frame: every content class at one size.  Pure checkers and the plain ramp give no SURF keypoint at any period (the box
    Hessian of a checker is zero at every sample), so they appear cut into patches only"""
    m = {}
    m["checker3_windowed"] = sp.windowed(sp.checker(w, h, 3), 2)
    m["checker8_windowed"] = sp.windowed(sp.checker(w, h, 8), 5)
    m["checker16_windowed"] = sp.windowed(sp.checker(w, h, 16), 6)
    m["bars7_y_windowed"] = sp.windowed(sp.bars(w, h, 7, 1), 3)
    m["bars40_blobs"] = sp.bars_blobs(w, h, 40)
    m["binary_noise"] = sp.binary_noise(w, h, 11)
    m["impulses_255_on_0"] = sp.impulses(w, h, 0, 255)
    m["impulses_0_on_255"] = sp.impulses(w, h, 255, 0)
    m["tiled32"] = sp.tiled(w, h, 5, 32)
    m["tiled48"] = sp.tiled(w, h, 6, 48)
    m["discs"] = sp.discs(w, h)
    m["ramp_blobs_x"] = sp.ramp_blobs(w, h, 0, seed=3)
    m["edge_dots5"] = sp.edge_dots(w, h, 5)
    m["mono_g_0"] = sp.mono(w, h, 1, 0, seed=7)
    m["mono_r_255"] = sp.mono(w, h, 2, 255, seed=8)
    m["clipped"] = sp.clipped(w, h, sp.CLIP_GAIN, seed=10)
    m["flat"] = flat(w, h)
    return m


ZERO_KEYPOINT_PATTERNS = ("flat",)                # the only content allowed to give no keypoints
TIE_PATTERNS = ("tiled32", "tiled48", "impulses_255_on_0", "impulses_0_on_255", "discs", "checker3_windowed")      # tie groups of 8 or more
# (w, h, patch seed, P, max_kp): the oracle's sorted list of tiled(640, 480, 6, 48) holds one tie group at positions 2564 .. 2680; the
# cut at 2600 keeps 36 of its 117 members, the ones first in (octave, layer, row, column) order
TIE_CUT = (640, 480, 6, 48, 2600)
TIE_CUT_GROUP = (2564, 2680)


def tie_cut_frame():
    w, h, seed, P, _ = TIE_CUT
    return sp.tiled(w, h, seed, P)


# ---- limit shapes ---------------------------------------------------------------------------------------------------------------------
# (w, h, content, threshold, max_kp): the host accepts 16 <= w, h < 16384
LIMIT_SHAPES = [(16383, 40, "binary_noise", 1.0, KEEP_ALL), (40, 16383, "binary_noise", 1.0, KEEP_ALL), (16383, 300, "binary_noise", 400.0, 20000),
                (16, 4000, "terrain", 1.0, KEEP_ALL), (4000, 16, "terrain", 1.0, KEEP_ALL)]


def limit_frame(w, h, content):
    return sp.binary_noise(w, h, 3 + (w % 7)) if content == "binary_noise" else terrain(w, h, seed=sp.shape_seed(w, h))


BRIGHT = (4600, 4400, 250)        # 4600 * 4400 * 250 = 5.06e9 > 2^32 = 4.29e9: the running sum wraps near row 3735


def bright(w=BRIGHT[0], h=BRIGHT[1], level=BRIGHT[2], n=4000, seed=0):
    """a frame at `level` with n dark Gaussian blobs (sigma 1.5 .. 4) at seeded places, 64 of them in the last rows where a maximum is
    still possible (centres 14 .. 30 rows above the lower edge)"""
    rng = np.random.default_rng(seed)
    g = np.full((h, w), level, np.uint8)
    R = 12
    yy, xx = np.mgrid[-R:R + 1, -R:R + 1].astype(np.float32)
    for k in range(n):
        s, amp = rng.uniform(1.5, 4.0), rng.uniform(60.0, float(level))
        cx = int(rng.integers(R, w - R))
        cy = int(rng.integers(R, h - R)) if k >= 64 else h - 1 - int(rng.integers(14, 31))
        blob = amp * np.exp(-0.5 * (xx * xx + yy * yy) / (s * s))
        win = g[cy - R:cy + R + 1, cx - R:cx + R + 1]
        win[...] = np.minimum(win, np.clip(np.rint(level - blob), 0, 255).astype(np.uint8))
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))


# ---- the small-size matrix --------------------------------------------------------------------------------------------------------------
# min(w, h): the accepted minimum; 21 .. 34, where the filters 21 and 27 and then the first interior samples of the two middle layers of
# octave 0 appear (a maximum needs (size_above / 2) / step + 1 samples of margin on each side: 23 and 29 samples for layers 1 and 2); the
# same steps of octaves 1 (46 / 58), 2 (92 / 116) and 3 (184 / 232); the filter sizes themselves (42 54 | 84 108 | 168 216) and 2 x 27
SMALL_N = [16, 20, 21, 22, 23, 26, 27, 28, 29, 30, 31, 32, 33, 34, 41, 42, 45, 46, 47, 51, 52, 53, 54, 55, 57, 58, 59, 83, 84, 91, 92, 93,
           107, 108, 109, 115, 116, 117, 167, 168, 183, 184, 185, 215, 216, 217, 231, 232, 233]
# the octave-0 Hessian kernel works on 64 x 16 tiles of samples and reads a 92 x 44 window of the integral image ((w + 1) x (h + 1) sums)
TILE_W = [63, 64, 65, 91, 92, 93]
TILE_H = [16, 17, 43, 44, 45]
SHAPES = ([(n, n) for n in SMALL_N] + [(n, 300) for n in SMALL_N] + [(300, n) for n in SMALL_N] + [(w, h) for w in TILE_W for h in TILE_H])


def shape_frames(w, h):
    """the two frames of a shape-matrix size: terrain and binary noise"""
    return {"terrain": terrain(w, h, seed=sp.shape_seed(w, h)), "binary_noise": sp.binary_noise(w, h, 17 + (w * 3 + h) % 11)}


def layer_mask(w, h):
    """per octave, bit l set when the filter (9 + 6 l) << o fits a w x h frame"""
    return tuple(sum(1 << l for l in range(4) if ((9 + 6 * l) << o) <= min(w, h)) for o in range(4))


def interior(w, h, o, l):
    """samples of middle layer l (1 or 2) of octave o that have their 26 neighbours inside the margin, along the shorter side"""
    step = 1 << o
    margin = ((((9 + 6 * (l + 1)) << o) // 2) // step) + 1
    return max(0, min(w, h) // step - 2 * margin)


def octaves_possible(w, h):
    """octaves in which a maximum is possible at all: the three filters of middle layer 1 fit and it has an interior sample"""
    return tuple(o for o in range(4) if (layer_mask(w, h)[o] & 7) == 7 and interior(w, h, o, 1) > 0)


# Zero keypoints are allowed for a shape-matrix frame in two cases only.  (1) octaves_possible(w, h) is empty: no middle layer has its three
# filters inside the frame and an interior sample (min(w, h) < 23), whatever the content.  (2) The frames listed here, found on the oracle:
# the interior is 1 .. 19 samples wide (min(w, h) <= 41) and this content puts no accepted maximum on it
ZERO_BY_CONTENT = {("terrain", 23, 23), ("binary_noise", 23, 23), ("binary_noise", 26, 26), ("binary_noise", 27, 27), ("terrain", 28, 28),
                   ("binary_noise", 28, 28), ("terrain", 29, 29), ("binary_noise", 29, 29), ("terrain", 30, 30), ("binary_noise", 30, 30),
                   ("terrain", 31, 31), ("binary_noise", 32, 32), ("terrain", 34, 34), ("terrain", 41, 41), ("terrain", 23, 300),
                   ("terrain", 300, 23)}

# the "more than 2^21 Hessian maxima" refusal: a 0 / 255 lattice of single pixels 4 apart gives 0.059 maxima per pixel at threshold 0
# (binary noise: 0.030); at 6000 x 6000 that is 2.23e6 > 2^21 = 2 097 152.  Device memory by the plane arithmetic of the extraction:
# det + trace planes 2 * 4 B * 5.3125 w h, integral image 4 w h, gray w h, frame 3 w h = 50.5 B per pixel = 1.82 GB
LATTICE = (6000, 6000, 4)


def lattice(w=LATTICE[0], h=LATTICE[1], p=LATTICE[2]):
    g = np.zeros((h, w), np.uint8)
    g[::p, ::p] = 255
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))


# ---- pair stage -----------------------------------------------------------------------------------------------------------------------
def _dup_patch(P=88):
    """flat 110 with three Gaussian blobs of different weight: a keypoint whose descriptor window lies inside the patch sees the same
    pixels wherever the patch is pasted"""
    g = np.full((P, P), 110.0, np.float32)
    yy, xx = np.mgrid[0:P, 0:P].astype(np.float32)
    for (cx, cy, s, a) in ((44, 44, 3.0, 120.0), (52, 40, 2.0, -70.0), (38, 50, 2.2, 60.0)):
        g += a * np.exp(-0.5 * ((xx - cx) ** 2 + (yy - cy) ** 2) / (s * s))
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


DUP_SIZE = (520, 400)
# the second patch of frame i lands at DUP_AT_J[0] in frame j under the pair's motion, and DUP_AT_J[0] is the first of the twins in (row, column)
# order: the matcher's "first of equal distances" rule makes that match an inlier, any other choice loses it
DUP_AT_I = [(150, 140), (330, 40)]
DUP_AT_J = [(127, 43), (140, 136), (280, 136), (140, 260), (280, 260), (400, 200)]


def dup_pair():
    """two overlapping views of one terrain (synth_frames.strip); the same patch pasted twice into frame i and six times into frame j"""
    from tests.synth_frames import strip
    w, h = DUP_SIZE
    fi, fj = (np.ascontiguousarray(f).copy() for f in strip(2, w, h, seed=3)[0])
    p = _dup_patch()[:, :, None]
    for (x, y) in DUP_AT_I:
        fi[y:y + p.shape[0], x:x + p.shape[1]] = p
    for (x, y) in DUP_AT_J:
        fj[y:y + p.shape[0], x:x + p.shape[1]] = p
    return fi, fj


# (match_dist, max_features) on the dup pair -> the walk ends with 1 .. 3 matches (the oracle decides; checked in the oracle test)
FEW_SELECTED = [(0.5, 3), (0.12, 3)]
# (match_dist, max_features) on the dup pair: three matches lie below 0.05, two of them at distance 0.  The walk 0.1 -> 0.05 -> next step
# ends at (float)((double)0.05f - 0.05) = 7.45e-10 > 0 and selects the two; stepping in float would give 0.0 and select nothing
WALK_TO_EPS = [(0.1, 2), (0.05, 2)]
TILED_PAIR = (6, 48, 48, 0)       # (patch seed, P, dx, dy) at 320x240: every query ties, the walk ends at distT <= 0 with nothing selected
FEATURE_COUNTS = (1, 63, 64, 65, 255, 256, 257)       # n_i / n_j either side of the 64-row train tile and the 256-query workgroup of the matcher


def count_frames():
    """two overlapping views of one terrain: extracted with max_kp = n they give exactly n features each"""
    from tests.synth_frames import strip
    a, b = strip(2, 320, 240, seed=5)[0]
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


RING_N = 40                       # the ring schedule of 40 frames has 40 * 15 = 600 pairs: more than the 512 of one batch
RING_MAX_KP = (700, 1, 64, 300, 65, 2, 257, 40, 63, 500, 256, 5, 120, 255)


def ring_frames():
    """[(frame, threshold, max_kp)] * 40: 128x96 .. 176x132 views of one terrain 6 px apart, so that neighbours match; feature counts from
    0 (two flat frames) to several hundred, set by max_kp"""
    big = terrain(176 + 6 * RING_N, 140, seed=29)
    out = []
    for k in range(RING_N):
        w, h = (128, 96) if k % 3 == 0 else ((160, 120) if k % 3 == 1 else (176, 132))
        img = np.ascontiguousarray(big[:h, 6 * k:6 * k + w])
        if k in (7, 23):
            img = flat(w, h)
        out.append((img, 2.0, RING_MAX_KP[k % len(RING_MAX_KP)]))
    return out
