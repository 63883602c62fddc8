"""Seeded adversarial inputs for SIFT detect+describe (numpy / the terrain generator only): BGR u8 frames of a given (w, h).

What each is for (tests/test_sift_patterns_oracle.py checks on the oracle alone that the inputs do it):
  checker / bars / binary_noise / impulses : saturated 0 | 255 steps -- the extremes of the x48 16-bit pyramid and its rounding
  tiled                                    : one patch repeated -- groups of keypoints with bit-equal response (tie order, the nfeatures cut)
  discs / checker(16)                      : rotational and four-fold symmetry -- several orientation peaks at one location
  bars / ramp_blobs / clipped              : one-direction gradients -- the descriptor's 0.2 clamp and the *512 saturation to 255
  edge_dots                                : structure at IMG_BORDER (5 px from an edge)
  mono                                     : single-channel colour through the fixed-point BGR2GRAY
Everything is deterministic: the same arguments give the same bytes."""
import numpy as np

from tests.synth_frames import terrain


def _bgr(g):
    g = np.ascontiguousarray(g, np.uint8)
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))


def checker(w, h, period):
    """0/255 checkerboard: squares of `period` pixels"""
    yy, xx = np.mgrid[0:h, 0:w]
    return _bgr((((xx // period) + (yy // period)) & 1) * 255)


def bars(w, h, period, axis):
    """0/255 bars `period` pixels wide; axis 0: the value changes along x (vertical bars), axis 1: along y"""
    yy, xx = np.mgrid[0:h, 0:w]
    return _bgr((((xx if axis == 0 else yy) // period) & 1) * 255)


def binary_noise(w, h, seed):
    """independent 0/255 pixels"""
    rng = np.random.default_rng(seed)
    return _bgr(rng.integers(0, 2, (h, w)) * 255)


def impulses(w, h, bg, fg, seed=0, cell=8):
    """isolated single pixels and 3x3 squares of `fg` on a `bg` field: one per 8 x 8 cell at a seeded position inside it, half of the
    cells left empty (no two touch; the uneven density is what gives the coarser octaves something to find)"""
    rng = np.random.default_rng(seed)
    g = np.full((h, w), bg, np.int32)
    for y0 in range(0, h - cell + 1, cell):
        for x0 in range(0, w - cell + 1, cell):
            on, sq, dx, dy = rng.random() < 0.5, rng.random() < 0.5, int(rng.integers(2, cell - 2)), int(rng.integers(2, cell - 2))
            if not on:
                continue
            cx, cy = x0 + dx, y0 + dy
            if sq:
                g[cy - 1:cy + 2, cx - 1:cx + 2] = fg
            else:
                g[cy, cx] = fg
    return _bgr(g)


def windowed(img, seed, n=10):
    """img inside n seeded rectangles (12 .. 59 px a side), 0 outside: a pattern finer than the smallest SIFT scale blurs to a flat grey
    and gives no keypoint anywhere; cut into patches its levels keep the saturated texture and the patch corners give keypoints on it"""
    rng = np.random.default_rng(seed)
    h, w = img.shape[:2]
    m = np.zeros((h, w), bool)
    for _ in range(n):
        rw, rh = int(rng.integers(12, min(60, w))), int(rng.integers(12, min(60, h)))
        x0, y0 = int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1))
        m[y0:y0 + rh, x0:x0 + rw] = True
    return np.ascontiguousarray(img * m[..., None].astype(np.uint8))


def bars_blobs(w, h, period, amp=10.0, sigma=2.3):
    """0/255 bars along x with one faint Gaussian blob 6 .. 19 px in front of every edge, every 24 rows.  The blob gives the keypoint, the
    saturated step next to it all of the gradient energy in its descriptor window: the energy lands in the four cells of one column and one
    orientation bin, every one of them is cut at 0.2, and the renormalised value 0.2 / sqrt(4 * 0.04) * 512 = 256 saturates the byte"""
    g = bars(w, h, period, 0)[..., 0].astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    k = 0
    for cy in range(20, h - 20, 24):
        for ex in range(period, w - period, period):
            cx = ex - (6 + k % 14)
            k += 1
            sign = 1.0 if g[cy, ex - 2] == 0 else -1.0
            g += sign * amp * np.exp(-0.5 * ((xx - cx) ** 2 + (yy - cy) ** 2) / (sigma * sigma))
    return _bgr(np.clip(np.rint(g), 0, 255))


def tiled(w, h, patch_seed, P):
    """one P x P patch of terrain repeated over the frame"""
    patch = terrain(P, P, seed=patch_seed)
    reps = ((h + P - 1) // P, (w + P - 1) // P, 1)
    return np.ascontiguousarray(np.tile(patch, reps)[:h, :w])


def tiled_shifted(w, h, patch_seed, P, dx, dy):
    """the frame `tiled` would give if its origin lay (dx, dy) pixels further right / down: pixel (x, y) here = pixel (x + dx, y + dy) there"""
    big = tiled(w + dx, h + dy, patch_seed, P)
    return np.ascontiguousarray(big[dy:dy + h, dx:dx + w])


def discs(w, h, radii=(3, 5, 8), pitch=40):
    """filled discs, rings and plus-shapes (255 on 0, every fourth 0 on a 255 square) on a grid"""
    g = np.zeros((h, w), np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    k = 0
    for cy in range(pitch // 2, h, pitch):
        for cx in range(pitch // 2, w, pitch):
            r = radii[(k // 3) % len(radii)]
            d2 = (xx - cx) ** 2 + (yy - cy) ** 2
            fg, bgv = 255, 0
            if k % 4 == 3:
                g[max(cy - pitch // 2 + 2, 0):cy + pitch // 2 - 2, max(cx - pitch // 2 + 2, 0):cx + pitch // 2 - 2] = 255
                fg, bgv = 0, 255
            kind = k % 3
            if kind == 0:
                g[d2 <= r * r] = fg
            elif kind == 1:
                g[(d2 <= r * r) & (d2 >= (r - 2) * (r - 2))] = fg
            else:
                t = max(1, r // 3)
                g[(np.abs(xx - cx) <= t) & (np.abs(yy - cy) <= r)] = fg
                g[(np.abs(yy - cy) <= t) & (np.abs(xx - cx) <= r)] = fg
            del bgv
            k += 1
    return _bgr(g)


def ramp(w, h, axis):
    """linear 0 .. 255 ramp along x (axis 0) or y (axis 1)"""
    n = w if axis == 0 else h
    v = (np.arange(n) * 255) // max(n - 1, 1)
    g = np.broadcast_to(v[None, :] if axis == 0 else v[:, None], (h, w))
    return _bgr(g)


def ramp_blobs(w, h, axis, seed=0, amp=60.0):
    """ramp plus small Gaussian blobs (sigma 1.5 .. 3) of either sign"""
    rng = np.random.default_rng(seed)
    g = ramp(w, h, axis)[..., 0].astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    for _ in range(max(6, (w * h) // 900)):
        cx, cy, s = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(1.5, 3.0)
        g += (amp if rng.random() < 0.5 else -amp) * np.exp(-0.5 * ((xx - cx) ** 2 + (yy - cy) ** 2) / (s * s))
    return _bgr(np.clip(np.rint(g), 0, 255))


def edge_dots(w, h, d, sigma=2.6, pitch=32):
    """Gaussian dots (255 on 40) whose centres lie d px from each of the four edges (every `pitch` px along it) and the four corners, and
    one at the frame centre (at d = 4 every extremum at the edge falls inside IMG_BORDER and is dropped)"""
    g = np.full((h, w), 40.0, np.float32)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    cs = [(d, d), (w - 1 - d, d), (d, h - 1 - d), (w - 1 - d, h - 1 - d), (w // 2, h // 2)]
    for cx in range(d + pitch, w - 1 - d - pitch // 2, pitch):
        cs += [(cx, d), (cx, h - 1 - d)]
    for cy in range(d + pitch, h - 1 - d - pitch // 2, pitch):
        cs += [(d, cy), (w - 1 - d, cy)]
    for (cx, cy) in cs:
        g = np.maximum(g, 40.0 + 215.0 * np.exp(-0.5 * ((xx - cx) ** 2 + (yy - cy) ** 2) / (sigma * sigma)))
    return _bgr(np.rint(g))


def mono(w, h, channel, other, seed=0):
    """terrain with the two channels that are not `channel` set to `other` (0 or 255)"""
    img = terrain(w, h, seed=seed).copy()
    for c in range(3):
        if c != channel:
            img[..., c] = other
    return img


def clipped(w, h, gain, seed=0):
    """terrain pushed through a gain about its median so that about a third of the pixels saturate at 0 or 255"""
    t = terrain(w, h, seed=seed).astype(np.float32)
    med = np.median(t)
    return np.clip(np.rint((t - med) * gain + 128.0), 0, 255).astype(np.uint8)


def content_matrix(w, h):
    """name -> frame: every content class at one size (the GPU content tests and the oracle-side caps walk this list)"""
    m = {}
    for p in (2, 8, 16):
        m[f"checker{p}"] = checker(w, h, p)
    m["checker3_windowed"] = windowed(checker(w, h, 3), 2)
    m["bars4_x_windowed"] = windowed(bars(w, h, 4, 0), 1)
    m["bars7_y_windowed"] = windowed(bars(w, h, 7, 1), 3)
    m["bars40_blobs"] = bars_blobs(w, h, 40)
    m["binary_noise"] = binary_noise(w, h, 11)
    m["impulses_255_on_0"] = impulses(w, h, 0, 255)
    m["impulses_0_on_255"] = impulses(w, h, 255, 0)
    m["tiled32"] = tiled(w, h, 5, 32)
    m["tiled48"] = tiled(w, h, 6, 48)
    m["discs"] = discs(w, h)
    m["ramp_x"] = ramp(w, h, 0)
    m["ramp_blobs_x"] = ramp_blobs(w, h, 0, seed=3)
    m["ramp_blobs_y"] = ramp_blobs(w, h, 1, seed=4)
    for d in (4, 5, 6, 7):
        m[f"edge_dots{d}"] = edge_dots(w, h, d)
    m["mono_g_0"] = mono(w, h, 1, 0, seed=7)
    m["mono_r_255"] = mono(w, h, 2, 255, seed=8)
    m["mono_b_0"] = mono(w, h, 0, 0, seed=9)
    m["clipped"] = clipped(w, h, CLIP_GAIN, seed=10)
    return m


CLIP_GAIN = 6.0
TIE_CUT_SIZE = (640, 480)         # tiled(.., 5, 32) here: more than nfeatures = 2000 keypoints come back, the cut falls inside a tie group
ZERO_KEYPOINT_PATTERNS = ("ramp_x", "checker2")       # the only contents allowed to give no keypoints
# retainBest keeps every keypoint tied with the 2000th response: here that is more than the 2048 rows a feature record holds, which the
# library refuses (MI355_ERR_FAILED, "overflow") instead of cutting the group; keep-all mode takes the frame
OVER_2048_TIES = ("checker16",)


# ---- shape matrix (tests/test_gpu_sift_edges.py runs these on the GPU, tests/test_sift_patterns_oracle.py on the oracle) ----
MIN_ACCEPTED = [(16, 16), (16, 17), (17, 16), (16, 4000), (4000, 16)]
REFUSED = [(15, 16), (16, 15), (1, 1)]
# nOctaves = cvRound(log2(min(w, h)) - 2) steps between 22|23 (2|3), 45|46 (3|4), 90|91 (4|5), 181|182 (5|6)
OCTAVE_BOUNDARY = [(22, 22), (23, 23), (45, 45), (46, 46), (90, 90), (91, 91), (181, 181), (182, 182),
                   (22, 300), (300, 23), (45, 260), (260, 46), (90, 400), (400, 91), (181, 640), (640, 182)]
# sizes whose pyramid ends in an octave 12 or 13 samples wide / high (n >> o for the last octave kept): the largest blur radius is 13,
# so reflect-101 folds twice there
SMALL_OCTAVE_N = [24, 25, 26, 27, 48, 50, 52, 55, 96, 100, 104, 111]
SMALL_OCTAVE = ([(n, n) for n in SMALL_OCTAVE_N] + [(n, 300) for n in SMALL_OCTAVE_N] + [(300, n) for n in SMALL_OCTAVE_N]
                + [(2048, 100), (2048, 104), (1024, 208)])
STREAM_ADMISSION = [(512, 64), (512, 65), (512, 63), (508, 64), (516, 64), (528, 64), (532, 64), (532, 129), (1024, 64), (1024, 127),
                    (4096, 64), (4096, 66)]


def n_octaves(w, h):
    """cv::SIFT's octave count for a w x h frame (no doubled base image in the reference's build)"""
    return int(np.rint(np.log2(min(w, h)) - 2.0))


def n_octaves_built(w, h):
    """octaves that exist in the pyramid: the loop over n_octaves() stops at the first octave below 2 * IMG_BORDER + 2 = 12 samples"""
    n = 0
    while n < n_octaves(w, h) and min(w >> n, h >> n) >= 12:
        n += 1
    return n


def shape_seed(w, h):
    """terrain seed of a shape-matrix frame"""
    return 100 + (w * 31 + h) % 97


def streamed_contents(w, h):
    """name -> frame: the contents that go through the streamed blur / streamed extrema at 1100x780 and 1024x768.  The tiled patch is 160 px
    here: groups of up to 6 x 4 equal responses.  With P = 32 a group has hundreds of members at this size, the group at the nfeatures cut
    does not fit the 2048-row feature record and the default mode refuses the frame (see OVER_2048_TIES); P = 32 runs in keep-all mode"""
    return {"tiled160": tiled(w, h, 5, 160), "checker8": checker(w, h, 8), "binary_noise": binary_noise(w, h, 12),
            "clipped": clipped(w, h, CLIP_GAIN, seed=13), "edge_dots5": edge_dots(w, h, 5)}


# (patch seed, P, dx, dy) of the tiled pairs of the pair-stage test.  Periodic frames defeat RANSAC unless the shift is a whole period: the
# first pair ends with matches selected and no inlier (the record and the H of the failed fit are still compared bit for bit, and any change
# in the order of tied matches changes them), the second with inlier lists
TILED_PAIRS = [(5, 32, 7, 3), (6, 48, 48, 0)]
