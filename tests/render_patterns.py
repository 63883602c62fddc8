"""Edge cases of the blended one-pass renders and the gain statistics (csrc/feather.hip, seamline.hip, median.hip, gain.hip, overview.hip):
pure numpy, seeded, no GPU, no oracle import.

The cases are those of tests/warp_patterns.py's refined list, reused as they stand (their predicates are asked of the restatement's winner
map), plus what the blended renders add: canvas heights around the tile heights 8 RPL (RPL = 1, 2, 4) and the 256-row list block, and three
frames that overlap across a list-block corner.  Every case carries a tag, one line on why it is there, and a predicate over the
RESTATEMENT'S output (Restated below: gain_ref.frame_sample_maps and what feather_ref, seamline_ref and median_ref make of it), so that a
later edit of a size or a matrix cannot quietly turn it into an ordinary case.  tests/test_render_patterns_oracle.py asserts the predicates
and the restatements' mutual consistency; tests/test_gpu_render_edges.py compares the HIP paths with the restatements.

The oracle is always an argument (restate(oracle, case)); nothing here loads it.
"""
import itertools
from typing import Callable, List, NamedTuple, Optional

import numpy as np

from tests import block_gain_ref as br
from tests import feather_ref as fr
from tests import gain_ref as gr
from tests import median_ref as mr
from tests import seamline_ref as sr
from tests import warp_patterns as wp

BLK = wp.BLK                   # candidate lists are kept per 256 x 256 block of the canvas
HEIGHTS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 256, 257)         # 8 RPL for RPL = 1, 2, 4 and the list block, each -1, +0, +1
RAMPS = (0, 3)
DEPTHS = (1, 2, 3, 5, 9)       # every K instantiation of median_tile_kernel and a depth below its K
MAX_PAIRS = 60


class Render(NamedTuple):
    tag: str
    imgs: list
    h9s: np.ndarray
    why: str
    pred: Callable                   # pred(case, r): r a Restated
    hidden: Optional[int] = None     # warp_patterns.Refined.hidden
    new: bool = False                # not among warp_patterns.refined_cases(): tests/test_gpu_warp_edges.py does not see it


# ---- the restatement of one case, made once -------------------------------------------------------------------------------------------------
class Restated:
    """what the numpy restatements give for a case: maps (gain_ref.frame_sample_maps), cw, ch, cws, layers [ch, cw], refined [ch, cws] (the
    oracle's refined render), top [ch, cw] (the highest covering frame, -1: none), and -- made when first asked for, then kept --
    weights(ramp), feather(ramp) -> (canvas, layers), seamline(ramp) -> (canvas, owner, count, omega_max, ties), median(ramp, depth) ->
    (canvas, spread, count, selected, boundary_tie), coords / block_maps (block_gain_ref.coord_maps / sample_maps)"""
    def __init__(self, orc, case):
        self.orc, self.case = orc, case
        self.maps = gr.frame_sample_maps(orc, case.imgs, case.h9s)
        self.ch, self.cw = next(m for m in self.maps if m is not None)[1].shape
        self.cws = (3 * self.cw + 3) & ~3
        self.layers = sum(m[1].astype(np.int64) for m in self.maps if m is not None)
        rc, res = orc.mosaic_images_refined(case.imgs, case.h9s)
        assert rc == 0 and (res[1], res[2], res[3]) == (self.cw, self.ch, self.cws), (case.tag, rc)
        self.refined = res[0]
        self.top = sr.top_frame(self.maps) - 1
        self.sizes = [(i.shape[1], i.shape[0]) for i in case.imgs]
        self._w, self._f, self._s, self._m, self._c = {}, {}, {}, {}, None

    def weights(self, ramp=0):
        if ramp not in self._w:
            self._w[ramp] = sr.weight_maps(self.orc, self.case.imgs, self.case.h9s, ramp, self.maps)
        return self._w[ramp]

    def feather(self, ramp=0):
        if ramp not in self._f:
            self._f[ramp] = fr.blend(self.maps, self.weights(ramp))
        return self._f[ramp]

    def seamline(self, ramp=0):
        if ramp not in self._s:
            self._s[ramp] = sr.pick(self.maps, self.weights(ramp))
        return self._s[ramp]

    def median(self, ramp=0, depth=0):
        if (ramp, depth) not in self._m:
            self._m[(ramp, depth)] = mr.pick(self.maps, self.weights(ramp), depth)
        return self._m[(ramp, depth)]

    @property
    def coords(self):
        if self._c is None:
            coords, (mw, mh) = br.coord_maps(self.sizes, self.case.h9s)
            assert (mw, mh) == (self.cw, self.ch), self.case.tag
            self._c = (coords, br.sample_maps(self.case.imgs, coords))
        return self._c[0]

    @property
    def block_maps(self):
        self.coords
        return self._c[1]

    @property
    def stats_maps(self):
        """maps in the form block_gain_ref.stats_ref takes: None for every frame without coordinates (the oracle gives a frame without an
        inverse an empty cover; tests/test_render_patterns_oracle.py shows that nothing else differs)"""
        return [None if c is None else m for m, c in zip(self.maps, self.coords)]


_RESTATED = {}


def restate(orc, case) -> Restated:
    if case.tag not in _RESTATED:
        _RESTATED[case.tag] = Restated(orc, case)
    return _RESTATED[case.tag]


# ---- predicates -----------------------------------------------------------------------------------------------------------------------------
def _as_refined_out(case, r):
    """what a warp_patterns.Refined predicate is given, from the restatement: the winner map is the highest covering frame"""
    invs = [wp.inverse_of(None, m, 1e-12) if m[8] != 0 else None for m in case.h9s]
    return dict(canvas=r.refined, cw=r.cw, ch=r.ch, cws=r.cws, winner=r.top, invs=invs)


def _reused(base, extra=None):
    def pred(case, r):
        return bool(base.pred(base, _as_refined_out(case, r))) and (extra is None or bool(extra(case, r)))
    return pred


def _forty_extra(case, r):
    """the layer count reaches 40, and the median's selected set at depth 9 is more than the set at depth 5 somewhere (whose frames are
    depth 9's first five: the list is sorted)"""
    s5, s9 = r.median(0, 5)[3], r.median(0, 9)[3]
    return int(r.layers.max()) == 40 and bool((s9[5:] > 0).any()) and np.array_equal(s9[:5], s5)


def _twins_extra(case, r):
    """frames 1 and 2 have equal weight everywhere they overlap -- and they overlap wherever either covers --, so that the index alone decides
    the seamline owner (never frame 1) and the median's selection order (frame 2 before frame 1)"""
    w, (c1, c2) = r.weights(0), (r.maps[1][1], r.maps[2][1])
    owner, ties = r.seamline(0)[1], r.seamline(0)[4]
    sel = r.median(0, 2)[3]
    both = c1 & c2
    return (both.sum() > 100 and np.array_equal(c1, c2) and np.array_equal(w[1][0][..., 0][both], w[2][0][..., 0][both]) and not (owner == 2).any()
            and bool(((owner == 3) & ties).any()) and bool(((sel[0] == 3) & (sel[1] == 2)).any()) and not ((sel[0] == 2) & (sel[1] == 3)).any())


def _height_pred(H):
    def pred(case, r):
        return r.ch == H and all(m is not None and m[1].any() for m in r.maps) and int(r.layers.max()) == 2
    return pred


def _straddle_pred(case, r):
    if (r.cw, r.ch) != (291, 281):
        return False
    for by in range(2):
        for bx in range(2):
            blk = r.layers[by * BLK:(by + 1) * BLK, bx * BLK:(bx + 1) * BLK]
            if not ((blk == 3).any() and int((blk >= 2).sum()) > 500):
                return False
    return True


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def _height_case(H):
    if H == 1:
        imgs = [wp.noise(5, 2, 800), wp.noise(3, 2, 801)]
        h9s = np.stack([wp.scale(1.0, 0.4), wp.scale(1.0, 0.4, 1.5, 0)])
    else:
        imgs = [wp.noise(5, H, 800 + H), wp.noise(3, H, 801 + H)]
        h9s = np.stack([wp.shift(0, 0), wp.shift(1.5, 0)])
    return Render("canvas_h%d" % H, imgs, h9s, "canvas height %d: the last tile row of 8, 16 and 32 rows and the 256-row list block at their edges" % H,
                  _height_pred(H), new=True)


def cases() -> List[Render]:
    out = []
    extra = {"forty": _forty_extra, "twins": _twins_extra}
    for c in wp.refined_cases():
        out.append(Render(c.tag, c.imgs, c.h9s, c.why, _reused(c, extra.get(c.tag)), hidden=c.hidden))
    for H in HEIGHTS:
        out.append(_height_case(H))
    out.append(Render("straddle_overlap", [wp.noise(280, 270, 90), wp.noise(60, 50, 91), wp.ramp(50, 60)],
                      np.stack([wp.shift(0, 0), wp.shift(226.5, 231.25), wp.turn(90, 290, 226)]),
                      "three frames that overlap across the list-block corner at (256, 256): every block holds pixels with 3 layers", _straddle_pred, new=True))
    return out


def by_tag():
    return {c.tag: c for c in cases()}


def skipped(case, r):
    """the frames the renders skip: m8 == 0, or no inverse (block_gain_ref.coord_maps gives them no coordinates)"""
    return [k for k, c in enumerate(r.coords) if c is None]


def gain_pairs(case, r, reverse):
    """all pairs i < j, the first MAX_PAIRS of them; reverse: one of them the other way round (a listed pair must not repeat, so it is
    turned in place, or -- where the list was cut -- an unlisted one is added).  Where the case has a skipped frame the list names it."""
    n = len(case.imgs)
    every = list(itertools.combinations(range(n), 2))
    pairs = every[:MAX_PAIRS]
    if reverse:
        if len(every) > MAX_PAIRS:
            pairs.append((n - 1, n - 2))
        else:
            a, b = pairs[len(pairs) // 2]
            pairs[len(pairs) // 2] = (b, a)
    sk = skipped(case, r)
    assert not sk or any(a in sk or b in sk for a, b in pairs), case.tag
    return pairs


def fitted_grid(case, r, gx, gy):
    """(gx, gy) cut down to the smallest frame that takes part: mi355_block_gain_stats_dev refuses a grid finer than a frame"""
    part = [s for s, c in zip(r.sizes, r.coords) if c is not None]
    return min([gx] + [w for w, h in part]), min([gy] + [h for w, h in part])
