"""Cases whose canvas or frame coordinates leave 16 bits: pure numpy, seeded, no GPU, no oracle import.

Every other pattern file of the suite stays below a canvas of 45 000 pixels on a side and a frame of 8 200.  Here a coordinate, a list-block
index (x / 256), a seam cell index or a workgroup row passes 65 535.  (float)xD - dGx is exact up to 2^24, so the restatements of the smaller
cases (render_patterns.Restated and what the *_ref modules make of it) remain the definition and nothing new is restated.

Canvas cases are render_patterns.Render objects, so that rp.restate, rp.gain_pairs, rp.fitted_grid and the seamcut and blend restatements apply
as they stand.  Every case carries a tag, one line on why it is there, and a predicate over the RESTATEMENT'S output, so that a later edit of
a size or a shift cannot quietly turn it into an ordinary case; and the mutations (MUTATIONS below) that must change its restatement: a case
whose bytes survive its own mutation does not test what its name says.  tests/test_extent_patterns_ref.py asserts both;
tests/test_gpu_extents.py compares the HIP paths with the restatements.

Frame cases are for the per-frame passes: frames with a side of 65 537 and of 2^20 (the limit include/mi355_mosaic.h names), on the pitches
3 w and 3 w + 5, whose content differs in every 256-column block (a repeating pattern would hide a wrapped column).
"""
from typing import Callable, List, NamedTuple, Optional, Tuple

import numpy as np

from tests import gain_ref as gr
from tests import render_patterns as rp
from tests import sharp_ref as shr
from tests import warp_patterns as wp  # noqa: F401
from tests.synth import texture

BLK = wp.BLK
FAR = 65536
ROWS_PER_WORKGROUP = (1, 4, 16)          # blend.hip's grid2; warp.hip's launches; the owner kernels and the tile renders
# what a 16-bit slip would do to the map step (mutated() below)
MUTATIONS = ("wrap_x", "wrap_y", "wrap_block") + tuple("rows_%d" % r for r in ROWS_PER_WORKGROUP)
GAIN_STEPS = (1, 3, 64)
SHARP_STEP = 1


class Canvas(NamedTuple):
    tag: str
    render: rp.Render                # frames and homographies
    far: Tuple[int, int]             # the pair of frames that overlaps past the threshold
    axis: int                        # 1: the case is about x, 0: about y
    beyond: int                      # the canvas extent along `axis` exceeds this
    mutations: Tuple[str, ...]       # each of them must change the restatement
    why: str
    pred: Callable                   # pred(case, r): r a render_patterns.Restated
    blend: bool = False              # chips, multiband blend and overviews are compared on it
    pairs: Optional[tuple] = None    # the statistics' pair list where render_patterns.gain_pairs' would leave the far frames out


# ---- mutations of the map step ----------------------------------------------------------------------------------------------------------------
def _box_blocks(cover, nby, nbx):
    """[nby, nbx] bool: the list blocks the frame's canvas box meets"""
    ys, xs = np.flatnonzero(cover.any(axis=1)), np.flatnonzero(cover.any(axis=0))
    listed = np.zeros((nby, nbx), bool)
    if len(ys):
        listed[ys[0] // BLK:ys[-1] // BLK + 1, xs[0] // BLK:xs[-1] // BLK + 1] = True
    return listed


def mutated(maps, mutate):
    """gain_ref.frame_sample_maps' result the way a kernel with one 16-bit slip would see it, frame by frame (a generator: a million-row map
    is held once):
      wrap_x, wrap_y  the canvas coordinate is taken modulo 65 536: pixel (x, y) holds what (x & 0xffff, y) holds;
      wrap_block      the index by * nbx + bx of the pixel's 256 x 256 list block is taken modulo 256: the pixel sees the frames listed for
                      that other block, a frame being listed where its canvas box meets the block;
      rows_R          a launch with R canvas rows per workgroup stops at gridDim.y = 65 535: no row from 65 535 R on is rendered."""
    assert mutate in MUTATIONS, mutate
    for m in maps:
        if m is None:
            yield None
            continue
        samp, cover = m
        ch, cw = cover.shape
        if mutate == "wrap_x":
            xs = np.arange(cw) & 0xffff
            yield samp[:, xs], cover[:, xs]
        elif mutate == "wrap_y":
            ys = np.arange(ch) & 0xffff
            yield samp[ys], cover[ys]
        elif mutate == "wrap_block":
            nby, nbx = (ch + BLK - 1) // BLK, (cw + BLK - 1) // BLK
            listed = _box_blocks(cover, nby, nbx).ravel()
            seen = listed[np.arange(nby * nbx) % 256].reshape(nby, nbx)
            seen = np.repeat(np.repeat(seen, BLK, axis=0)[:ch], BLK, axis=1)[:, :cw]
            yield samp * seen[..., None], cover & seen
        else:
            end = min(ch, 65535 * int(mutate[5:]))
            keep = np.zeros((ch, 1), bool)
            keep[:end] = True
            yield samp * keep[..., None], cover & keep


def survives(maps, mutate):
    """True where the mutation changes no frame's cover and no sample"""
    for m, mm in zip(maps, mutated(maps, mutate)):
        if m is not None and not (np.array_equal(m[1], mm[1]) and np.array_equal(m[0], mm[0])):
            return False
    return True


# ---- predicates -------------------------------------------------------------------------------------------------------------------------------
def far_overlap(case, r):
    """the pixels both frames of case.far give a sample, past 65 535 along the case's axis"""
    a, b = case.far
    both = r.maps[a][1] & r.maps[b][1]
    return both[:, FAR:] if case.axis == 1 else both[FAR:]


def pairs_of(case, r, reverse=False):
    if case.pairs is None:
        return rp.gain_pairs(case.render, r, reverse)
    pairs = list(case.pairs)
    if reverse:
        pairs[len(pairs) // 2] = pairs[len(pairs) // 2][::-1]
    return pairs


def records(case, r):
    """what the case's statistics are compared on: {("gain", step): (pair records, frame cover), ("sharp", 1): (pair records, frame records)}
    over pairs_of(case, r)"""
    pairs = pairs_of(case, r)
    out = {("gain", s): gr.stats_ref(r.maps, pairs, s) for s in GAIN_STEPS}
    out[("sharp", SHARP_STEP)] = shr.stats_ref(shr.lap_maps(r.maps), pairs, SHARP_STEP)
    return pairs, out


def _base_pred(case, r):
    """the extent, the far overlap and the far pair's records: gain at steps 1 and 3 and sharpness at step 1 count points there, and at no
    step are a case's records all zero (at step 64 the far overlap of the small frames holds no lattice point: the frames' own cover counts)"""
    if (r.cw, r.ch)[1 - case.axis] <= case.beyond or not far_overlap(case, r).any():
        return False
    pairs, rec = records(case, r)
    i = pairs.index(case.far)
    if not (rec[("gain", 1)][0][i][0] > 0 and rec[("gain", 3)][0][i][0] > 0 and int(rec[("sharp", 1)][0]["n"][i]) > 0):
        return False
    if not all(int(rec[("sharp", 1)][1]["n"][k]) > 0 for k in case.far):
        return False
    return all(any(n > 0 for n, _, _ in rec[("gain", s)][0]) or rec[("gain", s)][1].any() for s in GAIN_STEPS)


def _and(extra):
    return lambda case, r: _base_pred(case, r) and bool(extra(case, r))


def _boundary_pred(case, r):
    """frame 1 starts exactly on a list-block boundary, frame 2 on neither a block nor a cell boundary"""
    t1, t2 = (float(case.render.h9s[k][2 if case.axis == 1 else 5]) for k in (1, 2))
    return t1 == 69120 == 270 * BLK and t2 == 69131.5 and all(t2 % s for s in (4, 8, 16, 32, BLK))


def _turned_pred(case, r):
    h = case.render.h9s
    return h[2][8] == 0 and h[3][8] == 2 and h[3][6] != 0 and h[3][7] != 0 and h[1][1] != 0 and rp.skipped(case.render, r) == [2]


def _ribbon_pred(case, r):
    """the ribbon's own side passes 65 535, it gives samples there, and its box crosses 271 list blocks"""
    img = case.render.imgs[0]
    cover = r.maps[0][1]
    along = cover.any(axis=1 - case.axis)
    return img.shape[case.axis] == 69200 and bool(along[FAR:].any()) and int(np.ptp(np.flatnonzero(along)) // BLK) + 1 == 271


def _many_pred(case, r):
    return len(case.render.imgs) == 71 and int(r.layers[:, FAR:].max()) > 64 and 69000 // BLK > 256


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
def _t(img):
    return np.ascontiguousarray(img.transpose(1, 0, 2))


def _swap(h9):
    """the homography of the transposed frame on the transposed canvas"""
    m = np.asarray(h9, np.float32).reshape(3, 3)
    p = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    return (p @ m @ p).reshape(9).astype(np.float32)


def _render(tag, imgs, h9s, why, tall):
    if tall:                                                                # "swap": the same frames, x and y of the matrices exchanged
        imgs, h9s = imgs if tall == "swap" else [_t(i) for i in imgs], [_swap(h) for h in h9s]
    return rp.Render(tag, imgs, np.stack(h9s), why, lambda c, r: True, new=True)


def _case(tag, imgs, h9s, far, tall, beyond, mutations, why, pred, blend=False, pairs=None):
    return Canvas(tag, _render(tag, imgs, h9s, why, tall), far, 0 if tall else 1, beyond, mutations, why, pred, blend, pairs)


def _rows(upto):
    return tuple("rows_%d" % r for r in ROWS_PER_WORKGROUP if r <= upto)


def canvas_cases() -> List[Canvas]:
    out = []
    tex = lambda w, h, seed: texture(w, h, seed=seed)
    for tall in (False, True):
        d, n = ("tall", "rows") if tall else ("wide", "columns")
        mut = ("wrap_y", "wrap_block", "rows_1") if tall else ("wrap_x", "wrap_block")
        out.append(_case("%s_69k" % d, [tex(40, 24, 1), tex(40, 24, 2), tex(40, 24, 3)], [wp.shift(0, 0), wp.shift(69120, 3), wp.shift(69131.5, 5.25)],
                         (1, 2), tall and "swap", 69000, mut,
                         "two frames that overlap by most of a frame past 69 000 %s: one on the list-block boundary 270 * 256, one on no boundary" % n,
                         _and(_boundary_pred), blend=True))
        proj = wp.yaw(-5, 1.0, 69131.5, 5.25)
        proj[6], proj[7] = 1e-6, -1.5e-6
        gone = wp.shift(69125, 4)
        gone[8] = 0
        out.append(_case("%s_turned_far" % d, [tex(40, 24, 4), tex(40, 24, 5), tex(40, 24, 6), tex(40, 24, 7)],
                         [wp.shift(0, 0), wp.yaw(4, 1.0, 69120, 3), gone, wp.times(proj, 2)], (1, 3), tall and "swap", 69000, mut,
                         "the same distance under a yaw and a projective matrix with m8 = 2, a frame with m8 = 0 between them: the frame map works above 65 536",
                         _and(_turned_pred), blend=True))
        out.append(_case("ribbon_%s" % ("y" if tall else "x"), [wp.noise(69200, 6, 8), tex(40, 6, 9), tex(30, 5, 10)],
                         [wp.shift(0, 0), wp.shift(69150.5, 0.25), wp.shift(69160, 1)], (0, 1), tall, 69000, mut,
                         "a frame 69 200 long with two small ones over its far end: a frame side, a begX..endX span and a source column above 65 535, a box across 271 list blocks",
                         _and(_ribbon_pred)))
    n = 70
    out.append(_case("far_many", [wp.noise(12, 8, 399)] + [wp.noise(12, 8, 400 + k) for k in range(n)],
                     [wp.shift(0, 0)] + [wp.shift(69000 + (k * 7) % 5 + 0.25 * (k % 4), (k * 3) % 4 + 0.5 * (k % 2)) for k in range(n)], (1, 2), False, 69000,
                     ("wrap_x", "wrap_block"),
                     "70 frames on one spot at x = 69 000 and one at the origin: list offsets block * n with a block index above 256 and more than a wave of frames",
                     _and(_many_pred), pairs=((0, 1),) + tuple((k, k + 1) for k in range(1, rp.MAX_PAIRS))))
    out.append(_case("tall_262k", [tex(10, 12, 11), tex(10, 12, 12), tex(10, 12, 13)], [wp.shift(0, 0), wp.shift(262208, 1), wp.shift(262211.25, 2.5)],
                     (1, 2), True, 262140, ("wrap_y", "wrap_block") + _rows(4),
                     "a canvas taller than 4 * 65 535 rows: the launches with 4 rows per workgroup", _base_pred))
    out.append(_case("tall_1m", [tex(10, 12, 14), tex(10, 12, 15), tex(10, 12, 16)], [wp.shift(0, 0), wp.shift(1048640, 1), wp.shift(1048643.25, 2.5)],
                     (1, 2), True, 1048560, ("wrap_y", "wrap_block") + _rows(16),
                     "a canvas taller than 16 * 65 535 rows: the tile renders and the owner kernels", _base_pred))
    return out


def by_tag():
    return {c.tag: c for c in canvas_cases()}


# ---- frame cases ----------------------------------------------------------------------------------------------------------------------------
FRAME_SIZES = ((65537, 3), (3, 65537), (1 << 20, 2), (2, 1 << 20))
FRAME_PADS = (0, 5)


def frame(w, h, seed):
    """[h, w, 3] uint8 whose every 256-pixel block along either side differs from every other one: seeded noise (a wrapped column or row would
    have to meet its own bytes 65 536 pixels on)"""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def blocks_differ(img):
    """every 256-pixel block along the long side is unlike every other one"""
    a = img if img.shape[1] >= img.shape[0] else img.transpose(1, 0, 2)
    n = a.shape[1] // BLK
    rows = np.ascontiguousarray(a[:, :n * BLK].reshape(a.shape[0], n, BLK, 3).transpose(1, 0, 2, 3)).reshape(n, -1)
    return len(np.unique(rows, axis=0)) == n


def padded(img, pad):
    """(buffer [h, 3 w + pad] uint8 with 0xEE in the padding, pitch)"""
    h, w = img.shape[:2]
    buf = np.full((h, 3 * w + pad), 0xEE, np.uint8)
    buf[:, :3 * w] = img.reshape(h, 3 * w)
    return buf, 3 * w + pad
