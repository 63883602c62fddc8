"""The cases of the multiband blend along optimised seams (tests/blend_seam_ref.py): small surveys, each built to hold one thing the candidates
in the blend's geometry or the map-following ownership can get wrong.  tests/test_blend_seam_ref.py asserts on the restatement that each case
holds what its name says, tests/test_gpu_blend_seam.py that the build gives the restatement's bytes on every one.

A case is Case(imgs, h9s, params dict, keep or None, cells or None): cells is a cell map given by the caller ([gh, gw] uint16, or a function of
(gw, gh, n) that makes one); None: the label stage's own.  Frames are at most 128 x 96.
"""
from typing import Callable, NamedTuple, Optional, Union

import numpy as np

from tests import blend_seam_ref as bs
from tests import seamcut_patterns as sp
from tests import warp_patterns as wp
from tests.synth import texture


class Case(NamedTuple):
    imgs: list
    h9s: np.ndarray
    p: dict
    keep: Optional[np.ndarray] = None
    cells: Union[None, np.ndarray, Callable] = None


def _of(case3, **kw):
    """a case of tests/seamcut_patterns.py with its level, depth and costs; ramp has no meaning here"""
    imgs, h9s, p = case3[:3]
    return Case(imgs, h9s, bs.params(**dict({k: v for k, v in p.items() if k != "ramp"}, **kw)))


CRAFTED = {"crafted2": dict(frames=2), "crafted3": dict(frames=3), "relief2": dict(frames=2, relief=True), "relief3": dict(frames=3, relief=True),
           "symmetric2": dict(frames=2, symmetric=True)}
# what the numpy prototype gave on the crafted scenes before anything ran on a GPU: (energy before, after, cells changed, the rectangle's pixels
# owned by frame 0 and by frame 1 before, after, pixels whose owner changed)
CRAFTED_EXPECT = {"crafted2": (3938, 2492, 32, (96, 288), (0, 384), 462), "crafted3": (2798, 2280, 16, (64, 192), (0, 256), 240),
                  "relief2": (3016, 2492, 32, (96, 96), (0, 192), 462), "relief3": (3404, 2487, 21, (96, 96), (0, 192), 310)}


def crafted_rect(name):
    return sp.crafted(**CRAFTED[name])[3]


def keep_drops():
    """three frames in a row, the middle one dropped by keep; the caller's map names it in every cell: nothing may follow it"""
    imgs = [texture(40, 30, seed=600 + k) for k in range(3)]
    h9s = sp._translations([(0, 0), (15, 5), (30, 10)])
    return Case(imgs, h9s, bs.params(level=2), np.array([1, 0, 1], np.uint8), lambda gw, gh, n: np.full((gh, gw), 2, np.uint16))


def random_ids():
    """a caller's map with any of 0 .. n in every cell, whether or not that frame touches the cell"""
    c = _of(sp.skipped())
    return c._replace(cells=lambda gw, gh, n: sp.random_cells(n, gw, gh, seed=610))


def far_ids():
    """a caller's map that names in every cell the frame farthest from it: most cells name a frame that does not cover them"""
    c = _of(sp.holes())

    def cells(gw, gh, n):
        m = np.zeros((gh, gw), np.uint16)
        m[:, :gw // 2] = 2                                                  # frame 1 lies on the right, frame 0 and 2 on the left
        m[:, gw // 2:] = 1
        m[gh // 2:, :] = 2
        return m
    return c._replace(cells=cells)


def above_n():
    """ids above n, 65535 among them, and the skipped frame's id"""
    c = _of(sp.skipped())

    def cells(gw, gh, n):
        m = np.random.default_rng(611).choice(np.array([n + 1, n + 2, 65535, 4, 0], np.uint16), (gh, gw))       # 4: the frame with h9[8] == 0
        return m.astype(np.uint16)
    return c._replace(cells=cells)


def big():
    """twelve 128 x 96 frames on a canvas wider and higher than 256 px: cells in four ownership blocks, chips across the block boundaries"""
    offs = [(100 * i + 3 * j, 70 * j + 2 * i) for j in range(4) for i in range(3)]
    imgs = [texture(128, 96, seed=620 + k) for k in range(len(offs))]
    return Case(imgs, sp._translations(offs), bs.params(level=4, depth=8))


def many(n, seed):
    """n noise frames of 16 x 16 a few pixels apart in one ownership block: past owner_kernel's 32-entry LDS batch, past one chip per lane of
    the candidates kernel, past two"""
    imgs, h9s, p = sp.wave(n, seed, side=(16, 16))
    return Case(imgs, h9s, bs.params(level=2, depth=8))


def warp_chips(tag, frame):
    """a chip survey of tests/warp_patterns.py whose distance map is 0 / 0 or that has no valid pixel, under a map that names `frame` in every
    cell: never a candidate, but able to own through the map wherever it has a valid sample"""
    c = next(c for c in wp.chips_cases() if c.tag == tag)
    return Case(c.imgs, np.asarray(c.h9s, np.float32), bs.params(level=2, depth=8), c.keep, lambda gw, gh, n: np.full((gh, gw), frame + 1, np.uint16))


CASES = dict({name: (lambda kw=kw: _of(sp.crafted(**kw))) for name, kw in CRAFTED.items()})
CASES.update({
    "holes": lambda: _of(sp.holes()),
    "staircase": lambda: _of(sp.staircase()),
    "twins": lambda: _of(sp.twins()),
    "skipped": lambda: _of(sp.skipped()),
    "projective": lambda: _of(sp.projective()),
    "keep_drops": keep_drops,
    "random_ids": random_ids,
    "far_ids": far_ids,
    "above_n": above_n,
    "big": big,
    "many33": lambda: many(33, 630),
    "many65": lambda: many(65, 640),
    "many130": lambda: many(130, 650),
    "thin_named1": lambda: warp_chips("thin", 1),
    "thin_named3": lambda: warp_chips("thin", 3),
    "no_valid_named": lambda: warp_chips("no_valid_pixel", 1),
})
CASES.update({"nine_depth%d" % d: (lambda d=d: _of(sp.nine(d))) for d in range(1, 9)})
# canvases with every remainder of the cell side that moves the probe clamp, at levels 2 .. 5 (tests/seamcut_patterns.py: remainder, rem_pairs)
CASES.update({name: (lambda make=make: _of(make())) for name, make in sp.REM_CASES.items()})

_REF = {}


def cells_of(case, gw, gh):
    if case.cells is None:
        return None
    return np.ascontiguousarray(case.cells(gw, gh, len(case.imgs)) if callable(case.cells) else case.cells, np.uint16)


def reference(orc, name):
    """the restatement's results for a case, computed once and not to be written to: (case, given cells or None, blend_seam_ref dict)"""
    if name not in _REF:
        case = CASES[name]()
        r = bs.chip_set(case.imgs, case.h9s, case.keep)
        gw, gh = bs.sc.grid_of(r["cw"], r["ch"], case.p["level"])
        cells = cells_of(case, gw, gh)
        _REF[name] = (case, cells, bs.blend_seam_ref(orc, case.imgs, case.h9s, case.p, keep=case.keep, cells=cells, chips=r))
    return _REF[name]
