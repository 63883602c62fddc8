"""Edge cases of the multiband blend (csrc/blend.hip vs oracle/oracle_blend.c vs tests/blend_ref.py): pure numpy, seeded, no GPU, no oracle.

Every case carries the predicate it exists for -- a function of the geometry (and, where the case is about them, the mask bytes) -- so that
a later edit of a size cannot quietly turn it into an ordinary case.  tests/test_blend_edges_oracle.py asserts the predicates and compares
the oracle with the numpy restatement; tests/test_gpu_blend_edges.py compares the HIP paths with the oracle.

Direct cases feed MultiBandBlend / oracle.multiband_blend: rectangles inside the canvas, chip rows of (3w + 3) & ~3 bytes, mask rows of
(w + 3) & ~3 bytes.  Survey cases are frames + homographies for the warp-fed paths (ChipsAndMasks, MosaicBlended, MosaicBlendedDev).

About `dx`, `dy` of the region geometry (the region "pulled back inside the canvas"): they are zero for every chip that lies inside the
canvas.  The region's left edge is a multiple of 2^bands, its right edge is clipped to the padded canvas width -- a multiple of 2^bands as
well -- before the width is rounded up, so the rounded right edge cannot pass the padded canvas.  `edge_pullback` therefore checks what can
happen at the right / bottom edge: the region ends in the canvas's padding (beyond W / H) and `left` / `top` exceed the gap by the snap; and
tests/test_blend_edges_oracle.py asserts dx == dy == 0 over all cases, so that a geometry change that makes the pull-back live is noticed.
"""
from typing import Callable, List, NamedTuple, Optional

import numpy as np

from tests import blend_ref as br
from tests.synth import texture

MAXB = 32                      # chips per batch in blend_core


class Direct(NamedTuple):
    tag: str
    rects: list                # (x0, y0, w, h) per chip
    chips: list
    masks: list
    W: int
    H: int
    band: int
    why: str
    pred: Callable             # pred(case) -> bool


class Survey(NamedTuple):
    tag: str
    imgs: list
    h9s: np.ndarray
    keep: Optional[np.ndarray]
    why: str
    pred: Callable             # pred(geo) with geo = dict(rects, W, H, owned, n_frames) -> bool


def chip_of(img):
    h, w, _ = img.shape
    c = np.zeros((h, (w * 3 + 3) & ~3), np.uint8)
    c[:, :w * 3] = img.reshape(h, -1)
    return c


def mask_of(m):
    h, w = m.shape
    out = np.zeros((h, (w + 3) & ~3), np.uint8)
    out[:, :w] = m
    return out


def full_mask(w, h, v=255):
    return mask_of(np.full((h, w), v, np.uint8))


def blocks(w, h, seed):
    """0 / 255 blocks of 2, 4, 8 and 16 pixels, xor-ed: large Laplacians at every level"""
    rng = np.random.default_rng(seed)
    out = np.zeros((h, w, 3), np.uint8)
    for s in (2, 4, 8, 16):
        a = rng.integers(0, 2, ((h + s - 1) // s, (w + s - 1) // s, 3), dtype=np.uint8)
        out ^= np.repeat(np.repeat(a, s, 0), s, 1)[:h, :w] * np.uint8(255)
    return out


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def info_array(rects):
    from tests.oracle_lib import CHIPINFO
    a = np.zeros(len(rects), CHIPINFO)
    for k, (x0, y0, w, h) in enumerate(rects):
        a[k]["x0"], a[k]["y0"], a[k]["w"], a[k]["h"], a[k]["img"] = x0, y0, w, h, k
    return a


def nonempty(case):
    """(rects, chips, masks) without the entries of zero size: what the oracle and the numpy reference are given"""
    keep = [k for k, r in enumerate(case.rects) if r[2] > 0 and r[3] > 0]
    return [case.rects[k] for k in keep], [case.chips[k] for k in keep], [case.masks[k] for k in keep]


# ---- geometry, recomputed here -----------------------------------------------------------------------------------------------------------
def bands(W, H, band):
    return br.level_count(W, H, band)


def padded(W, H, nb):
    al = 1 << nb
    return (W + al - 1) // al * al, (H + al - 1) // al * al


def regions(rects, W, H, band):
    nb = bands(W, H, band)
    return [dict(zip(("tlx", "tly", "rw", "rh", "left", "top", "dx", "dy"), br.feed_geometry(x0, y0, w, h, W, H, nb)), cw=w, ch=h)
            for (x0, y0, w, h) in rects if w > 0 and h > 0]


def top_level(W, H, band):
    nb = bands(W, H, band)
    Wp, Hp = padded(W, H, nb)
    return Wp >> nb, Hp >> nb


def batch_offsets(rects, W, H, band):
    """ChipP::tmp as blend_core computes it: inside a batch of up to 32 chips (entries of zero size left out before), the running sum of
    the pixel counts of the levels 1 .. bands of the chips before it (the 2 GB budget is never reached at these sizes)"""
    nb = bands(W, H, band)
    out = []
    for i, g in enumerate(regions(rects, W, H, band)):
        if i % MAXB == 0:
            run = 0
        out.append(run)
        run += sum((g["rw"] >> l) * (g["rh"] >> l) for l in range(1, nb + 1)) if nb > 0 else g["rw"] * g["rh"]
    return out


def _p_levels(n):
    return lambda c: bands(c.W, c.H, c.band) == n


def _p_top(w=None, h=None):
    return lambda c: (w is None or top_level(c.W, c.H, c.band)[0] == w) and (h is None or top_level(c.W, c.H, c.band)[1] == h)


# ---- direct cases --------------------------------------------------------------------------------------------------------------------------
def _narrow():
    out = []
    for tag, (W, H) in (("narrow_w", (20, 300)), ("narrow_h", (300, 20))):
        pred = _p_top(w=1) if W < H else _p_top(h=1)
        why = "canvas narrower than 2^band: the top level is one pixel wide / high"
        base = chip_of(texture(W, H, seed=7))
        out.append(Direct(tag, [(0, 0, W, H)], [base], [full_mask(W, H)], W, H, 5, why, pred))
        if W < H:
            rects = [(0, 0, W, H), (3, 40, 9, 50), (10, 200, 10, 100)]
        else:
            rects = [(0, 0, W, H), (40, 3, 50, 9), (200, 10, 100, 10)]
        chips = [base] + [chip_of(noise(w, h, 70 + k)) for k, (_, _, w, h) in enumerate(rects[1:])]
        masks = [full_mask(w, h) for (_, _, w, h) in rects]
        out.append(Direct(tag + "_3", rects, chips, masks, W, H, 5, why, pred))
    return out


def _level_steps():
    out = []
    for (W, H), n in (((1, 1), 0), ((2, 1), 1), ((1, 2), 1), ((4, 3), 2), ((33, 31), 5), ((32, 32), 5), ((3, 5), 3)):
        rects = [(0, 0, W, H)]
        if W * H > 1:
            rects.append((W // 2, H // 2, W - W // 2, H - H // 2))
        chips = [chip_of(noise(w, h, 11 * W + H + k)) for k, (_, _, w, h) in enumerate(rects)]
        masks = [full_mask(w, h) for (_, _, w, h) in rects]
        out.append(Direct("canvas_%dx%d" % (W, H), rects, chips, masks, W, H, 5, "level count %d set by the canvas" % n, _p_levels(n)))
    return out


def _band_over():
    W, H = 100, 70
    rects = [(0, 0, 70, 70), (40, 10, 60, 60)]
    chips = [chip_of(texture(w, h, seed=20 + k)) for k, (_, _, w, h) in enumerate(rects)]
    m0 = np.full((70, 70), 255, np.uint8); m0[:, 55:] = 0
    m1 = np.full((60, 60), 255, np.uint8); m1[:, :15] = 0
    masks = [mask_of(m0), mask_of(m1)]
    return [Direct("band_over_%d" % b, rects, chips, masks, W, H, b, "level count clipped by the canvas (7), not by band",
                   lambda c: bands(c.W, c.H, c.band) == 7 and c.band > 7) for b in (12, 16)]


def _multi_reflect(c):
    """some chip is at most 9 wide or high (never on the packed fast paths) and some chip is reflected more than twice into its border"""
    g = regions(c.rects, c.W, c.H, c.band)
    return (any(min(r["cw"], r["ch"]) <= 9 for r in g) and
            any(r["left"] > 2 * r["cw"] or r["top"] > 2 * r["ch"] for r in g) and
            any(r["cw"] == 1 and r["ch"] == 1 for r in g))


def _tiny_chips():
    W, H = 300, 200
    rects = [(150, 100, 1, 1), (0, 0, 2, 7), (292, 197, 8, 3), (100, 50, 9, 9), (200, 0, 5, 200), (290, 0, 10, 10), (0, 196, 11, 4), (299, 199, 1, 1),
             (17, 101, 7, 2)]
    chips = [chip_of(noise(w, h, 300 + k)) for k, (_, _, w, h) in enumerate(rects)]
    masks = [full_mask(w, h) for (_, _, w, h) in rects]
    why = "chips of 1 .. 11 pixels: border forms of the first REDUCE and of level 0 only, reflected many times across a 96-pixel gap"
    bg = (0, 0, W, H)
    return [Direct("tiny_chips", rects, chips, masks, W, H, 5, why, _multi_reflect),
            Direct("tiny_chips_on_background", [bg] + rects, [chip_of(texture(W, H, seed=31))] + chips, [full_mask(W, H)] + masks, W, H, 5, why, _multi_reflect),
            Direct("tiny_chips_band2", rects, chips, masks, W, H, 2, why, _multi_reflect)]


def _edge_pred(c):
    nb = bands(c.W, c.H, c.band)
    al = 1 << nb
    g = regions(c.rects, c.W, c.H, c.band)
    rx = [r for r, (x0, y0, w, h) in zip(g, c.rects) if x0 + w == c.W]
    by = [r for r, (x0, y0, w, h) in zip(g, c.rects) if y0 + h == c.H]
    return (c.W % al != 0 and c.H % al != 0 and len(rx) >= 2 and len(by) >= 2 and
            all(r["tlx"] + r["rw"] > c.W for r in rx) and all(r["tly"] + r["rh"] > c.H for r in by) and      # the region ends in the padding
            any(r["left"] > 3 * al for r in g) and any(r["top"] > 3 * al for r in g))                          # the snap: left / top exceed the gap


def _edge_pullback():
    out = []
    for W, H in ((300, 200), (289, 193)):
        rects = [(W - 57, 40, 57, 61), (30, 157, 83, H - 157), (W - 41, H - 37, 41, 37), (W - 130, H - 120, 130, 120), (5, 7, 120, 90)]
        chips = [chip_of(texture(w, h, seed=40 + k)) for k, (_, _, w, h) in enumerate(rects)]
        masks = [full_mask(w, h) for (_, _, w, h) in rects]
        out.append(Direct("edge_pullback_%dx%d" % (W, H), rects, chips, masks, W, H, 5,
                          "chips ending exactly at the right / bottom edge / corner of a canvas that is not a multiple of 32", _edge_pred))
    return out


def _grey_pred(c):
    vals = np.concatenate([m[:, :r[2]].ravel() for m, r in zip(c.masks, c.rects)])
    return bool(((vals > 0) & (vals < 255)).any()) and len(c.rects) == 3


def _grey():
    W, H = 200, 100
    rects = [(0, 0, 140, 100), (50, 10, 150, 80), (20, 30, 120, 70)]
    chips = [chip_of(blocks(w, h, 50 + k)) for k, (_, _, w, h) in enumerate(rects)]
    # the order shows in a few bytes only and not for every draw of the masks (the weight sums differ in their last bit, which must then move
    # a truncation): of the mask seeds 51 .. 1250, the numpy reference gives order-dependent bytes for 213 and 727
    rng = np.random.default_rng(213)
    uni = [mask_of(rng.integers(0, 256, (h, w), dtype=np.uint8)) for (_, _, w, h) in rects]
    ext = [mask_of(rng.choice(np.array([0, 1, 254, 255], np.uint8), (h, w))) for (_, _, w, h) in rects]
    why = "mask bytes other than 0 / 255: truncations, 1 / 255, w + 1e-5 and the > 1e-5 test at every level; the chip order is part of the result"
    order = [2, 0, 1]
    perm = lambda a: [a[k] for k in order]
    return [Direct("grey_masks", rects, chips, uni, W, H, 5, why, _grey_pred),
            Direct("grey_masks_extremes", rects, chips, ext, W, H, 5, why, _grey_pred),
            Direct("grey_masks_permuted", perm(rects), perm(chips), perm(uni), W, H, 5, why, _grey_pred),
            Direct("grey_masks_extremes_permuted", perm(rects), perm(chips), perm(ext), W, H, 5, why, _grey_pred)]


def _wrap():
    W = H = 64
    chip = chip_of(np.full((H, W, 3), 255, np.uint8))
    m = full_mask(W, H)
    out = []
    for n in (150, 129, 128):
        wraps = n * 255 > 32767
        out.append(Direct("wrap_%d" % n, [(0, 0, W, H)] * n, [chip] * n, [m] * n, W, H, 3,
                          "%d white chips with full masks: the top level's sum %d %s int16" % (n, n * 255, "leaves" if wraps else "stays inside"),
                          (lambda c, n=n, wraps=wraps: len(c.rects) == n and (n * 255 > 32767) == wraps and bands(c.W, c.H, c.band) == 3)))
    return out


def _odd_pred(c):
    t = batch_offsets(c.rects, c.W, c.H, c.band)
    return len(t) == 40 and sum(v & 1 for v in t[:MAXB]) >= 3 and sum(v & 1 for v in t[MAXB:]) >= 2


def _odd_offsets():
    W, H = 200, 160
    rects = []
    for k in range(40):
        if k % 3 != 1:
            rects.append((20 + (k % 7), 10 + (k % 3), 120, 100))           # band 5: region = the padded canvas, 224 x 160 -> 7 x 5; band 3: 21 x 17, 22 x 17
        else:
            rects.append((150 - k, 100 - k, 30 + k, 40))
    chips = [chip_of(texture(w, h, seed=60 + k)) for k, (_, _, w, h) in enumerate(rects)]
    rng = np.random.default_rng(61)
    masks = []
    for (_, _, w, h) in rects:
        m = np.zeros((h, w), np.uint8)
        a, b = sorted(rng.integers(0, w + 1, 2)); c_, d = sorted(rng.integers(0, h + 1, 2))
        m[c_:d + 1, a:b + 1] = 255
        masks.append(mask_of(m))
    why = "two batches (32 + 8); regions whose top level is odd x odd put the next chip's pyramid at an odd element offset"
    return [Direct("odd_offsets_band%d" % b, rects, chips, masks, W, H, b, why, _odd_pred) for b in (5, 3)]


def _holes_pred(c):
    cover = np.zeros((c.H, c.W), bool)
    for (x0, y0, w, h), m in zip(c.rects, c.masks):
        cover[y0:y0 + h, x0:x0 + w] |= m[:, :w] != 0
    return bool((~cover).any()) and any(not m[:, :r[2]].any() for m, r in zip(c.masks, c.rects))


def _holes():
    W, H = 120, 90
    rects = [(0, 0, 80, 90), (50, 20, 70, 60), (10, 10, 60, 40)]
    chips = [chip_of(texture(w, h, seed=80 + k)) for k, (_, _, w, h) in enumerate(rects)]
    m0 = np.full((90, 80), 255, np.uint8); m0[30:50, 20:45] = 0; m0[:, 70:] = 0
    m1 = np.full((60, 70), 255, np.uint8); m1[:, :25] = 0; m1[40:, :] = 0
    m2 = np.zeros((40, 60), np.uint8)
    return [Direct("holes", rects, chips, [mask_of(m0), mask_of(m1), mask_of(m2)], W, H, 5,
                   "canvas pixels with no weight at all, and a chip whose mask is all zero", _holes_pred)]


def _content():
    W, H = 160, 120
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = lambda a: np.repeat(a[:, :, None], 3, 2).astype(np.uint8)
    checker = rgb(((xx + yy) & 1) * 255)
    bars = rgb(((xx // 3) & 1) * 255)
    imp = np.zeros((H, W, 3), np.uint8)
    for (x, y, c) in ((0, 0, 0), (W - 1, H - 1, 1), (80, 60, 2), (31, 32, 0), (33, 31, 1), (1, 118, 2)):
        imp[y, x, c] = 255
    black, white = np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8)
    seam = (3 * xx + 4 * yy < 480)
    ma, mb = mask_of(seam.astype(np.uint8) * 255), mask_of((~seam).astype(np.uint8) * 255)
    pred = lambda c: all(set(np.unique(a)) <= {0, 255} for a in c.chips + c.masks)
    out = []
    for tag, a, b in (("checker_bars", checker, bars), ("impulses_white", imp, white), ("black_white", black, white), ("white_checker", white, checker)):
        out.append(Direct("content_" + tag, [(0, 0, W, H)] * 2, [chip_of(a), chip_of(b)], [ma, mb], W, H, 5,
                          "extreme content (only 0 and 255) under a diagonal 0 / 255 mask seam: the largest Laplacians there are", pred))
    return out


def _zero_size():
    W, H = 90, 60
    rects = [(0, 0, 60, 60), (5, 5, 0, 10), (30, 0, 60, 60), (40, 20, 10, 0)]
    dummy = np.zeros((1, 4), np.uint8)
    chips = [chip_of(texture(60, 60, seed=90)), dummy, chip_of(texture(60, 60, seed=91)), dummy]
    masks = [full_mask(60, 60), dummy, full_mask(60, 60), dummy]
    return [Direct("zero_size", rects, chips, masks, W, H, 5, "entries with w = 0 / h = 0 are skipped: the result is the blend of the others",
                   lambda c: any(r[2] == 0 for r in c.rects) and any(r[3] == 0 for r in c.rects) and len(nonempty(c)[0]) == 2)]


def direct_cases() -> List[Direct]:
    out = []
    for f in (_narrow, _level_steps, _band_over, _tiny_chips, _edge_pullback, _grey, _wrap, _odd_offsets, _holes, _content, _zero_size):
        out += f()
    return out


# ---- survey cases ----------------------------------------------------------------------------------------------------------------------------
def _h(sx=1.0, tx=0.0, ty=0.0, yaw=0.0, h31=0.0, h32=0.0):
    c, s = np.cos(np.deg2rad(yaw)), np.sin(np.deg2rad(yaw))
    return np.array([sx * c, -sx * s, tx, sx * s, sx * c, ty, h31, h32, 1.0], np.float32)


def survey_bands(case):
    """pyramid depths a survey case is blended with: 5 (the reference's), 3, 1, and a band of 12 that the canvas cuts to 9 levels (not for
    the strips: their canvas would be padded to 1024 x 1024 and every region with it)"""
    return (5, 3, 1) if case.tag in ("strip", "keep") else (5, 3, 1, 12)


def _owns_few(g):
    return any(1 <= o <= 30 for o in g["owned"])


def survey_cases() -> List[Survey]:
    out = []
    out.append(Survey("narrow", [texture(20, 300, seed=1), texture(6, 5, seed=2), texture(12, 9, seed=3)],
                      np.stack([_h(), _h(tx=9, ty=120), _h(tx=4, ty=250)]), None,
                      "a canvas narrower than 2^band with chips of a few pixels inside it",
                      lambda g: g["W"] < 32 and g["H"] >= 290 and min(min(r[2], r[3]) for r in g["rects"]) <= 9 and _owns_few(g)))
    out.append(Survey("downscaled", [texture(320, 240, seed=4), texture(200, 152, seed=5), texture(64, 48, seed=6)],
                      np.stack([_h(), _h(sx=0.04, tx=140, ty=100), _h(sx=0.1, tx=312, ty=233)]), None,
                      "frames scaled to a few pixels: chips that own 1 .. 30 pixels, one in the canvas's corner",
                      lambda g: len(g["rects"]) == 3 and sum(1 for r in g["rects"] if max(r[2], r[3]) <= 12) == 2 and _owns_few(g)))
    out.append(Survey("projective", [texture(320, 240, seed=7), texture(320, 240, seed=8)],
                      np.stack([_h(), _h(tx=60, ty=30, h31=8e-4, h32=-6e-4)]), None,
                      "projective terms of 8e-4: the chip is not the frame's shape",
                      lambda g: len(g["rects"]) == 2 and tuple(g["rects"][1][2:]) != (320, 240) and tuple(g["rects"][1][2:]) != (321, 241)))
    out.append(Survey("tiny_only", [texture(3, 3, seed=9), texture(2, 2, seed=10)], np.stack([_h(), _h(tx=2, ty=1)]), None,
                      "a whole survey of 3 x 3 and 2 x 2 frames: a canvas of a few pixels, two levels",
                      lambda g: max(g["W"], g["H"]) <= 4 and bands(g["W"], g["H"], 5) == 2))
    n = 12
    strip = [texture(96, 64, seed=20 + k) for k in range(n)]
    strip_h = np.stack([_h(tx=73.0 * k, ty=(0 if k == 0 else float((5 * k) % 7))) for k in range(n)])
    p_strip = lambda g: g["W"] >= 850 and g["H"] <= 96 and top_level(g["W"], g["H"], 5)[1] in (2, 3)
    out.append(Survey("strip", strip, strip_h, None, "twelve frames along a line: a canvas of about 900 x 70, the top level has 2-3 rows",
                      lambda g: p_strip(g) and len(g["rects"]) == n))
    keep = np.ones(n, np.uint8); keep[1] = 0
    out.append(Survey("keep", strip, strip_h, keep, "the strip without the first frame's neighbour",
                      lambda g: p_strip(g) and len(g["rects"]) == n - 1))
    return out
