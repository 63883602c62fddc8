"""Edge cases of the warp stage (csrc/warp.hip vs oracle/oracle_warp.c vs tests/warp_ref.py): pure numpy, seeded, no GPU, no oracle.

Three lists: single warps (ImageProjectionTransform), refined renders (MosaicImagesRefined) and chip surveys (ChipsAndMasks).  Every case
carries a tag, one line on why it is there, and a predicate over the ORACLE'S output, so that a later edit of a size or a matrix cannot
quietly turn it into an ordinary case.  tests/test_warp_patterns_oracle.py asserts the predicates, compares the oracle with the numpy
restatement and with the reference's own code; tests/test_gpu_warp_edges.py compares the HIP paths with the oracle.

What a predicate is given:
  single   pred(case, out)       out = dict(buf, dw, dh, dws, inv)                       inv: the 3 x 3 inverse the warp used (float32[9])
  refined  pred(case, out)       out = dict(canvas, cw, ch, cws, winner, invs)           winner[y, x]: the frame whose sample the pixel holds, -1 = none
  chips    pred(case, r, run)    r = Oracle.chips_and_masks(...) (find_masks=True) + r["valid"]; run(keep) renders the same survey with other flags
"""
from typing import Callable, List, NamedTuple, Optional

import numpy as np

from tests import warp_ref as wr
from tests.synth import texture

NE = 32                        # candidates per batch in owner_kernel
BLK = 256                      # candidate lists are kept per 256 x 256 block of the canvas (both renders)


class Single(NamedTuple):
    tag: str
    img: np.ndarray            # [h, w, 3]; the 1-channel form is channel 0 (grey())
    h9: np.ndarray
    why: str
    pred: Callable


class Refined(NamedTuple):
    tag: str
    imgs: list
    h9s: np.ndarray
    why: str
    pred: Callable
    hidden: Optional[int] = None     # a frame that gives no pixel although its box lies in the canvas: may be withheld (NULL pointer)


class Chips(NamedTuple):
    tag: str
    imgs: list
    h9s: np.ndarray
    keep: Optional[np.ndarray]
    why: str
    pred: Callable


def grey(img):
    return np.ascontiguousarray(img[:, :, 0])


# ---- content --------------------------------------------------------------------------------------------------------------------------------
def _rgb(a):
    return np.ascontiguousarray(np.repeat(np.asarray(a, np.uint8)[:, :, None], 3, 2))


def white(w, h, seed=0):
    return np.full((h, w, 3), 255, np.uint8)


def impulses(w, h, seed=0):
    """0 with single 255 pixels: corners, centre, last column and row (one channel each, so that a swapped channel shows)"""
    a = np.zeros((h, w, 3), np.uint8)
    for i, (x, y) in enumerate(((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2), (w - 1, h // 2), (w // 2, h - 1))):
        a[y, x, i % 3] = 255
    return a


def checker(period):
    def f(w, h, seed=0):
        yy, xx = np.mgrid[0:h, 0:w]
        return _rgb((((xx // period) + (yy // period)) & 1) * 255)
    return f


def noise(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def ramp(w, h, seed=0):
    """value = column index: a wrong neighbour is visible in the byte"""
    return _rgb(np.tile((np.arange(w) & 255).astype(np.uint8), (h, 1)))


CONTENT = [("white", white), ("impulses", impulses), ("checker1", checker(1)), ("checker3", checker(3)), ("noise", noise), ("ramp", ramp),
           ("texture", lambda w, h, seed=0: texture(w, h, seed=seed))]


# ---- homographies ---------------------------------------------------------------------------------------------------------------------------
def H(a=1.0, b=0.0, c=0.0, d=0.0, e=1.0, f=0.0, g=0.0, h=0.0, i=1.0):
    return np.array([a, b, c, d, e, f, g, h, i], np.float32)


def turn(deg, tx=0.0, ty=0.0):
    """exact quarter turns: integer cosine and sine"""
    c, s = {0: (1, 0), 90: (0, 1), 180: (-1, 0), 270: (0, -1)}[deg]
    return H(c, -s, tx, s, c, ty)


def mirror_x(tx=0.0, ty=0.0):
    return H(-1, 0, tx, 0, 1, ty)


def mirror_y(tx=0.0, ty=0.0):
    return H(1, 0, tx, 0, -1, ty)


def yaw(deg, s=1.0, tx=0.0, ty=0.0):
    c, sn = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return H(s * c, -s * sn, tx, s * sn, s * c, ty)


def scale(sx, sy=None, tx=0.0, ty=0.0):
    return H(sx, 0, tx, 0, sx if sy is None else sy, ty)


def shear(k=0.5):
    return H(1, k, 0, 0, 1, 0)


def shift(tx, ty):
    return H(1, 0, tx, 0, 1, ty)


def times(h9, k):
    """the whole matrix multiplied: the same map, m8 = k"""
    return (np.asarray(h9, np.float32) * np.float32(k)).astype(np.float32)


def det2(h9):
    return float(h9[0]) * float(h9[4]) - float(h9[1]) * float(h9[3])


# ---- single warps ---------------------------------------------------------------------------------------------------------------------------
SIZES = [(2, 2), (2, 9), (9, 2), (3, 3), (5, 7), (257, 3), (37, 23)]


def _dims(fn):
    return lambda c, o: (o["dw"], o["dh"]) == fn(c.img.shape[1], c.img.shape[0])


def _affine_not_unit(k):
    return lambda c, o: o["inv"][6] == 0 and o["inv"][7] == 0 and o["inv"][8] != 1 and c.h9[8] == k and c.h9[6] == 0 and c.h9[7] == 0


def _neg_zero(c, o):
    return bool(np.signbit(o["inv"][6]) and np.signbit(o["inv"][7]) and o["inv"][6] == 0 and o["inv"][7] == 0 and o["inv"][8] == -1)


def _positive(c, o):
    return o["dw"] >= 1 and o["dh"] >= 1


GEOMS = [
    ("turn90", lambda w, h: turn(90), "quarter turn, integer cosine and sine", _dims(lambda w, h: (h, w))),
    ("turn180", lambda w, h: turn(180), "half turn", _dims(lambda w, h: (w, h))),
    ("turn270", lambda w, h: turn(270), "three quarter turns", _dims(lambda w, h: (h, w))),
    ("mirror_x", lambda w, h: mirror_x(), "mirror, det < 0", lambda c, o: det2(c.h9) < 0 and (o["dw"], o["dh"]) == (c.img.shape[1], c.img.shape[0])),
    ("mirror_y", lambda w, h: mirror_y(), "mirror, det < 0", lambda c, o: det2(c.h9) < 0 and (o["dw"], o["dh"]) == (c.img.shape[1], c.img.shape[0])),
    ("yaw45", lambda w, h: yaw(45), "yaw 45: the box is a diamond's, most of it has no sample", _positive),
    ("aniso", lambda w, h: scale(3, 0.3), "scale 3 x 0.3", _dims(lambda w, h: (int(3 * (w - 1) + 1.5), int(np.float32(0.3) * np.float32(h - 1) + np.float32(1.5))))),
    ("shear", lambda w, h: shear(0.5), "shear", _positive),
    ("shift_int", lambda w, h: shift(7, -3), "integer translation", _dims(lambda w, h: (w, h))),
    ("shift_half", lambda w, h: shift(0.5, -2.5), "half-pixel translation", _dims(lambda w, h: (w, h))),
    ("times2", lambda w, h: times(yaw(17, 1.3, 2.5, 1.25), 2), "the matrix times 2: affine with m8 = 2, no unit denominator", _affine_not_unit(2)),
    ("times_m1", lambda w, h: times(yaw(17, 1.3, 2.5, 1.25), -1), "the matrix times -1: m8 = -1, the inverse has -0.0 in 6 and 7", _neg_zero),
    ("m8_m1", lambda w, h: H(1, 0, 3, 0, 1, 2, 0, 0, -1), "m8 = -1 alone: a half turn through a denominator of -1", _neg_zero),
]


def _both_254_255(c, o):
    v = o["buf"][:, :o["dw"] * 3]
    return bool((v == 254).any() and (v == 255).any())


def _wrong_neighbour_shows(c, o):
    """the result with the neighbour at xi + 1 differs from the oracle's"""
    bad, _ = wr.image_projection_transform(c.img, c.h9, o["inv"], xi_shift=1)
    return bad[0].shape == o["buf"].shape and not np.array_equal(bad[0], o["buf"])


def _den_signs(c, o):
    """destination pixels with denominators of both signs, and none with 0 / 0 (the reference's code stays defined)"""
    _, (xs, ys, ok, xf, yf) = wr.image_projection_transform(c.img, c.h9, o["inv"])
    den = wr.denominators(o["inv"], xf, yf)
    return bool((den > 0).any() and (den < 0).any() and not np.isnan(xs).any() and not np.isnan(ys).any())


def _width_case(W):
    src_w = 37
    sx = (W - 1 + 0.3) / (src_w - 1)
    return Single("width_%d" % W, noise(src_w, 5, 900 + W), scale(sx, 1.0), "destination width %d: group-of-4 / wave-of-256-pixels boundary" % W,
                  lambda c, o, W=W: o["dw"] == W and o["dh"] == 5)


def single_cases() -> List[Single]:
    out = []
    for gi, (gtag, make, why, pred) in enumerate(GEOMS):
        for si, (w, h) in enumerate(SIZES):
            ctag, gen = CONTENT[(gi + si) % len(CONTENT)]
            out.append(Single("%s_%dx%d_%s" % (gtag, w, h, ctag), gen(w, h, seed=100 + 7 * gi + si), make(w, h), why, pred))
    y17 = yaw(17, 1.3)
    out.append(Single("white_yaw17", white(50, 40), y17, "constant 255: the truncating cast sits on a boundary, a re-associated sum moves bytes", _both_254_255))
    out.append(Single("white_times2", white(50, 40), times(y17, 2), "the same through m8 = 2", lambda c, o: _both_254_255(c, o) and _affine_not_unit(2)(c, o)))
    out.append(Single("ramp_yaw17", ramp(37, 23), y17, "ramp: a neighbour one pixel off changes bytes", _wrong_neighbour_shows))
    out.append(Single("ramp_shear", ramp(37, 23), shear(0.5), "ramp under shear", _wrong_neighbour_shows))
    out.append(Single("ramp_turn90", ramp(37, 23), H(0, -1.5, 0, 1.5, 0, 0),
                      "ramp under a quarter turn with scale 1.5", _wrong_neighbour_shows))
    out.append(Single("impulses_up", impulses(9, 7), scale(1.5, 2.5), "single 255 pixels, magnified", lambda c, o: 0 < int((o["buf"] != 0).sum()) < o["buf"].size // 2))
    out.append(Single("checker1_yaw", checker(1)(37, 23), yaw(33, 0.7), "period-1 checkerboard, minified and turned", _positive))
    out.append(Single("checker3_proj", checker(3)(37, 23), H(1, 0.1, 0, -0.05, 1, 0, 2e-3, -1e-3, 1), "period-3 checkerboard, projective", _positive))
    out.append(Single("up300", noise(2, 2, 5), scale(300), "a 2 x 2 frame magnified 300 times: one source cell", lambda c, o: (o["dw"], o["dh"]) == (301, 301)))
    out.append(Single("down004", noise(300, 200, 6), scale(0.004), "300 x 200 minified to 2 x 2", lambda c, o: (o["dw"], o["dh"]) == (2, 2)))
    out.append(Single("horizon", noise(64, 48, 7), H(g=-1.0 / 40), "the horizon m6 x + 1 = 0 crosses the frame: denominators of both signs",
                      lambda c, o: (o["dw"], o["dh"]) == (111, 130) and _den_signs(c, o)))
    out.append(Single("near_horizon", noise(64, 48, 8), H(g=-1.0 / 80, h=-1.0 / 90), "the frame ends just before the horizon",
                      lambda c, o: (o["dw"], o["dh"]) == (501, 251)))
    for W in (1, 2, 3, 4, 5, 6, 7, 8, 9, 127, 128, 129, 255, 256, 257):
        out.append(_width_case(W))
    return out


# ---- refined renders ------------------------------------------------------------------------------------------------------------------------
def _wins(o, k):
    return int((o["winner"] == k).sum())


def _all_win(c, o):
    return all(_wins(o, k) > 0 for k in range(len(c.imgs)))


def _refined_width(W):
    if W == 1:
        imgs = [noise(2, 5, 700), noise(2, 3, 701)]
        h9s = np.stack([scale(0.4, 1.0), scale(0.4, 1.0, 0, 1.5)])
    else:
        imgs = [noise(W, 5, 700 + W), noise(W, 3, 701 + W)]
        h9s = np.stack([shift(0, 0), shift(0, 1.5)])
    return Refined("canvas_w%d" % W, imgs, h9s, "canvas width %d: pixel groups, row padding and the 128-pixel tile at their edges" % W,
                   lambda c, o, W=W: o["cw"] == W and _all_win(c, o))


def _sparse_pred(c, o):
    cov = o["winner"] >= 0
    bx, by = (o["cw"] + BLK - 1) // BLK, (o["ch"] + BLK - 1) // BLK
    per = [bool(cov[y * BLK:(y + 1) * BLK, x * BLK:(x + 1) * BLK].any()) for y in range(by) for x in range(bx)]
    return o["cw"] > BLK and o["ch"] > BLK and sum(per) >= 3 and not all(per) and cov.mean() < 0.01


def refined_cases() -> List[Refined]:
    out = []
    a = yaw(10, 1.0, 6.5, 2.25)
    out.append(Refined("twins", [noise(32, 24, 1), noise(40, 30, 2), checker(1)(40, 30)], np.stack([shift(0, 0), a, a]),
                       "two frames with the same homography and other content: the later one wins everywhere",
                       lambda c, o: _wins(o, 1) == 0 and _wins(o, 2) > 0 and _wins(o, 0) > 0 and np.array_equal(c.h9s[1], c.h9s[2]), hidden=1))
    out.append(Refined("hidden", [noise(32, 24, 3), noise(10, 8, 4), noise(20, 16, 5)], np.stack([shift(0, 0), shift(5, 5), shift(2, 2)]),
                       "a frame wholly under a later one", lambda c, o: _wins(o, 1) == 0 and _wins(o, 0) > 0 and _wins(o, 2) > 0, hidden=1))
    n = 40
    out.append(Refined("forty", [noise(32, 24, 10 + k) for k in range(n)], np.stack([shift(k % 3, k % 2) for k in range(n)]),
                       "40 frames on one tile: a long candidate list, almost all of it under later frames",
                       lambda c, o: (o["cw"], o["ch"]) == (34, 25) and len(c.imgs) == 40 and _wins(o, 39) > 0 and _wins(o, 0) == 0 and _wins(o, 38) > 0))
    pos = [(0, 0, 5, 4), (300, 10, 3, 3), (10, 290, 2, 2), (790, 290, 9, 2), (259, 257, 4, 5), (253, 254, 6, 5), (511, 100, 3, 2), (640, 17, 2, 7)]
    out.append(Refined("sparse", [noise(w, h, 30 + k) for k, (_, _, w, h) in enumerate(pos)], np.stack([shift(x + 0.25 * (k % 2), y) for k, (x, y, _, _) in enumerate(pos)]),
                       "tiny frames on a canvas of 800 x 300: several list blocks, empty ones, tiles nobody covers", _sparse_pred))
    z = [shift(100, 0), shift(0, 0), shift(7.5, 3.5), shift(0, 100)]
    z[0][8] = 0; z[3][8] = 0
    out.append(Refined("m8_zero_ends", [noise(16, 12, 40 + k) for k in range(4)], np.stack(z), "m8 = 0 on the first and the last frame: neither counts nor renders",
                       lambda c, o: o["cw"] < 100 and o["ch"] < 100 and _wins(o, 0) == 0 and _wins(o, 3) == 0 and _wins(o, 1) > 0 and _wins(o, 2) > 0))
    out.append(Refined("rank_deficient", [noise(24, 20, 50), noise(20, 10, 51), noise(12, 12, 52)],
                       np.stack([shift(0, 0), H(1, 0, 5, 2, 0, 10, 0, 0, 1), shift(3, 30)]),
                       "a homography of rank 2 with m8 = 1: its corners count for the canvas, it gives no pixel",
                       lambda c, o: o["invs"][1] is None and o["ch"] >= 48 and _wins(o, 1) == 0 and _wins(o, 0) > 0 and _wins(o, 2) > 0))
    out.append(Refined("turns", [noise(40, 30, 60), ramp(30, 20), noise(30, 20, 62), white(20, 16), noise(16, 12, 64), noise(12, 10, 65)],
                       np.stack([shift(0, 0), turn(90, 50, 5), turn(270, 5, 40), turn(180, 45, 38), mirror_x(60, 20), times(mirror_y(30, 28), -1)]),
                       "quarter turns and mirrors among upright frames", _all_win))
    out.append(Refined("scaled_matrices", [noise(32, 24, 70), white(30, 20), noise(30, 20, 72)],
                       np.stack([shift(0, 0), times(yaw(17, 1.3, 12, 2), 2), times(yaw(-8, 0.9, 20, 15), -1)]),
                       "affine frames with m8 = 2 and m8 = -1 beside a unit one", lambda c, o: _all_win(c, o) and c.h9s[1, 8] == 2 and c.h9s[2, 8] == -1))
    for W in (1, 2, 3, 4, 5, 7, 8, 127, 128, 129, 255, 256, 257):
        out.append(_refined_width(W))
    return out


# ---- chips and masks ------------------------------------------------------------------------------------------------------------------------
def owned(r):
    return [int((m[:, :int(c["w"])] != 0).sum()) for m, c in zip(r["masks"], r["chips"])]


def valid_counts(r):
    return [int((m[:, :int(c["w"])] != 0).sum()) for m, c in zip(r["valid"], r["chips"])]


def rects(r):
    return [(int(c["x0"]), int(c["y0"]), int(c["w"]), int(c["h"])) for c in r["chips"]]


def block_counts(r):
    """candidates per 256 x 256 canvas block, from the chip rectangles"""
    bx, by = (r["cw"] + BLK - 1) // BLK, (r["ch"] + BLK - 1) // BLK
    cnt = np.zeros((by, bx), np.int64)
    for (x0, y0, w, h) in rects(r):
        cnt[max(0, y0 // BLK):min(by - 1, (y0 + h - 1) // BLK) + 1, max(0, x0 // BLK):min(bx - 1, (x0 + w - 1) // BLK) + 1] += 1
    return cnt


def _seventy_pred(c, r, run):
    o = owned(r)
    b32 = wr.ownership(r["valid"], r["chips"], r["cw"], r["ch"], upto=NE)[1]
    b64 = wr.ownership(r["valid"], r["chips"], r["cw"], r["ch"], upto=2 * NE)[1]
    best = wr.ownership(r["valid"], r["chips"], r["cw"], r["ch"])[1]
    second_beats_first = bool(((b32 >= 0) & (b64 >= NE)).any())
    third_beats_second = bool(((b64 >= NE) & (best >= 2 * NE)).any())
    carried = bool(((b32 >= 0) & (best == b32)).any()) and bool(((b64 >= NE) & (best == b64)).any())      # leaders that survive the later batches
    return (len(c.imgs) == 70 and int(block_counts(r).max()) > 2 * NE and np.array_equal(c.h9s[0], c.h9s[40]) and o[0] > 0 and o[40] == 0 and
            second_beats_first and third_beats_second and carried)


def _outside_is_farther(c, r, run):
    """for chips 1 and 2 the maximum edge distance over all chip pixels exceeds the maximum over the valid ones: a maximum that ignores the
    mask normalises by another number"""
    def tops(k):
        full = np.full_like(r["valid"][k], 255)
        return float(wr.distance_map(full, r["chips"][k])[1]), float(wr.distance_map(r["valid"][k], r["chips"][k])[1])
    return all(tops(k)[0] > tops(k)[1] > 0 for k in (1, 2)) and all(v > 0 for v in owned(r))


def _keep_pred(c, r, run):
    full = run(None)
    return c.keep is not None and int(c.keep[1]) == 0 and owned(full)[1] > 0 and len(r["chips"]) == len(c.imgs) - 1


def chips_cases() -> List[Chips]:
    out = []
    a, b = yaw(5, 1.0, 2.5, 1.5), yaw(5, 1.0, 22.5, 11.5)
    out.append(Chips("duplicates", [noise(48, 40, 1), checker(1)(48, 40), noise(48, 40, 3), white(48, 40)], np.stack([a, a, b, b]), None,
                     "frames 0 = 1 and 2 = 3: exact ties, the first of each pair owns, the second nothing",
                     lambda c, r, run: owned(r)[1] == 0 and owned(r)[3] == 0 and owned(r)[0] > 0 and owned(r)[2] > 0))
    out.append(Chips("thin", [noise(64, 48, 4), white(2, 40), white(40, 2), white(2, 2)], np.stack([shift(0, 0), shift(10, 4), shift(12, 20), shift(30, 30)]), None,
                     "frames of 2 x 40, 40 x 2 and 2 x 2: every valid pixel lies on an edge line, the maximum distance is 0, the map 0 / 0",
                     lambda c, r, run: valid_counts(r)[1:] == [39, 39, 1] and owned(r)[1:] == [0, 0, 0] and owned(r)[0] > 0))
    out.append(Chips("no_valid_pixel", [noise(64, 48, 5), white(2, 2)], np.stack([shift(0, 0), yaw(45, 0.3, 20.3, 20.3)]), None,
                     "a frame scaled down to a diamond between the pixel centres: a chip without any valid pixel",
                     lambda c, r, run: valid_counts(r)[1] == 0 and owned(r)[1] == 0 and owned(r)[0] > 0))
    out.append(Chips("turns", [noise(64, 48, 6), noise(40, 30, 7), noise(30, 20, 8), noise(20, 16, 9), noise(30, 20, 10)],
                     np.stack([shift(0, 0), turn(90, 50, 5), turn(270, 5, 40), turn(180, 40, 30), mirror_x(60, 20)]), None,
                     "quarter turns and a mirror over an upright frame: the vertical-line branch on edges 0 and 2",
                     lambda c, r, run: all(v > 0 for v in owned(r)) and any(abs(float(q["quad"][0] - q["quad"][2])) < 1e-6 for q in r["chips"])))
    out.append(Chips("yaw45", [noise(64, 48, 14), noise(40, 12, 15), noise(37, 11, 16)],
                     np.stack([shift(0, 0), yaw(45, 1.0, 30, 5), yaw(-30, 1.0, 10, 42)]), None,
                     "long frames at yaw 45 and -30: chip pixels WITHOUT a sample lie farther from every edge line than any pixel with one",
                     _outside_is_farther))
    out.append(Chips("turns_negative", [noise(40, 30, 11), noise(30, 20, 12), noise(30, 20, 13)], np.stack([shift(0, 0), turn(90, 10, -8), turn(180, 12, 9)]), None,
                     "turned frames that reach negative coordinates", lambda c, r, run: all(v > 0 for v in owned(r)) and r["dG"][0] > 0 and r["dG"][1] > 0))
    n = 70
    h70 = [yaw((k % 5) - 2, 1.0, 4 + (k * 7) % 41 + 0.25 * (k % 4), 3 + (k * 11) % 29 + 0.5 * (k % 2)) for k in range(n)]
    h70[40] = h70[0].copy()
    out.append(Chips("seventy", [noise(24, 20, 100 + k) for k in range(n)], np.stack(h70), None,
                     "70 chips on one block: three batches of candidates, leaders carried, beaten and tied across the batch boundaries", _seventy_pred))
    out.append(Chips("straddle", [noise(280, 270, 20), noise(40, 30, 21)], np.stack([shift(0, 0), shift(240.5, 245.25)]), None,
                     "a chip across the block boundary at 256 in x and in y",
                     lambda c, r, run: rects(r)[1][0] < BLK <= rects(r)[1][0] + rects(r)[1][2] - 1 and rects(r)[1][1] < BLK <= rects(r)[1][1] + rects(r)[1][3] - 1
                     and owned(r)[1] > 0 and int(block_counts(r).min()) >= 1 and block_counts(r).shape == (2, 2)))
    out.append(Chips("positive", [noise(32, 24, 22), noise(32, 24, 23)], np.stack([shift(20, 15), shift(35.5, 22.25)]), None,
                     "every frame at a positive offset: the canvas still contains the origin, a band of it is empty",
                     lambda c, r, run: min(x for x, _, _, _ in rects(r)) >= 20 and min(y for _, y, _, _ in rects(r)) >= 15 and r["dG"][0] == 0 and r["dG"][1] == 0))
    out.append(Chips("negative", [noise(32, 24, 24), noise(32, 24, 25), noise(20, 20, 26)], np.stack([shift(-30.5, -12.25), shift(0, 0), shift(-10, 5)]), None,
                     "negative offsets", lambda c, r, run: r["dG"][0] == 30.5 and r["dG"][1] == 12.25 and all(v > 0 for v in owned(r))))
    out.append(Chips("keep", [noise(40, 30, 27), noise(40, 30, 28), noise(40, 30, 29)], np.stack([shift(0, 0), shift(15, 5), shift(30, 10)]), np.array([1, 0, 1], np.uint8),
                     "the keep flags drop a frame that would own pixels", _keep_pred))
    out.append(Chips("scaled_matrices", [noise(48, 40, 30), noise(30, 20, 31), noise(30, 20, 32)],
                     np.stack([shift(0, 0), times(yaw(17, 1.3, 12, 2), 2), times(yaw(-8, 0.9, 20, 15), -1)]), None,
                     "affine frames with m8 = 2 and m8 = -1", lambda c, r, run: all(v > 0 for v in owned(r)) and c.h9s[1, 8] == 2 and c.h9s[2, 8] == -1))
    return out


# ---- what the predicates are given: the oracle's output, put together (the oracle is an argument; nothing here loads it) ------------------
def inverse_of(oracle, h9, eps):
    """the numpy restatement's own inverse (tests/test_warp_patterns_oracle.py shows that it has the bits of the oracle's)"""
    return wr.inverse(h9, eps)


def single_out(oracle, case, img):
    """img: case.img or grey(case.img)"""
    rc, res = oracle.image_projection_transform(img, case.h9)
    if rc != 0:
        return dict(rc=rc, inv=inverse_of(oracle, case.h9, 1e-6))
    return dict(rc=0, buf=res[0], dw=res[1], dh=res[2], dws=res[3], inv=inverse_of(oracle, case.h9, 1e-6))


def refined_out(oracle, case):
    rc, res = oracle.mosaic_images_refined(case.imgs, case.h9s)
    assert rc == 0, (case.tag, rc)
    invs = [inverse_of(oracle, m, 1e-12) if m[8] != 0 else None for m in case.h9s]
    ref, winner, nan_seen = wr.mosaic_images_refined(case.imgs, case.h9s, invs)
    return dict(canvas=res[0], cw=res[1], ch=res[2], cws=res[3], invs=invs, winner=winner, nan_seen=nan_seen, numpy=ref)


def chips_out(oracle, case, keep="case", find_masks=True):
    return oracle.chips_and_masks(case.imgs, case.h9s, keep=case.keep if isinstance(keep, str) else keep, find_masks=find_masks)
