"""Cases of cover depth (include/mi355_mosaic.h, "cover depth"; csrc/cover.hip, csrc/cover_select.cpp): pure numpy, seeded, no GPU, no oracle
import.

Statistics cases: tests/render_patterns.py's cases reused as they stand (their cover is the oracle's, through rp.restate), one case of
tests/extent_patterns.py with a side past 65 535 (step 64 only), and what the cover walk adds: depths 7, 8 and 9 at neighbouring lattice
points, 65 / 257 / 600 frames meeting one list block, and a canvas with lattice points at pixels 255 and 256 of both axes.  The cover of the
added cases is cover_ref.geometry's (numpy; hundreds of oracle renders of hundreds of frames would take minutes), which
tests/test_cover_patterns_ref.py holds against the oracle's on the reused cases.  Pitch is irrelevant here: the stage takes no image pointer
and reads no pixel, so no case pads its rows.

Selection layouts: integer translations of small frames, each with what must happen under the reference.  A w x h frame at canvas offset
(X, Y) covers columns X .. X + w - 2 and rows Y .. Y + h - 2 (the map's bounds test is xs < w - 1); its clipped box is X - 1 .. X + w - 1,
Y - 1 .. Y + h - 1, cut at the canvas.

Every case carries a tag, one line on why it is there, and a predicate over the restatement's output, so that a later edit of a size or a
shift cannot quietly turn it into an ordinary case.  tests/test_cover_patterns_ref.py asserts the predicates; tests/test_cover_host.py and
tests/test_gpu_cover.py compare the library with the restatement.
"""
from typing import Callable, List, NamedTuple, Optional

import numpy as np

from tests import cover_ref as cr
from tests import extent_patterns as ep
from tests import render_patterns as rp
from tests import warp_patterns as wp

BLK = wp.BLK
ALL_STEPS = (1, 3, 7, 8, 37, 64)
KEEPS = ("null", "ones", "zeros", "one_off", "alternate")


class Stats(NamedTuple):
    tag: str
    sizes: list                      # [(w, h)]
    h9s: np.ndarray
    steps: tuple
    why: str
    pred: Callable                   # pred(case, r): r a Restated
    render: Optional[rp.Render] = None   # reused from render_patterns / extent_patterns: the cover is the oracle's


def keep_mask(name, n):
    """NULL, all ones (the same bytes as NULL), all zeros (everything in hist[0]), one frame off, every second frame off"""
    if name == "null":
        return None
    k = np.ones(n, np.uint8)
    if name == "zeros":
        k[:] = 0
    elif name == "one_off":
        k[min(1, n - 1)] = 0
    elif name == "alternate":
        k[1::2] = 0
    return k


class Restated:
    """covers (per frame None or [ch, cw] bool), boxes, cw, ch; stats(step, keep name) -> (FRAME_STATS [n], hist [9]), made once"""
    def __init__(self, orc, case):
        self.case = case
        self.n = len(case.sizes)
        if case.render is not None:
            r = self.rp = rp.restate(orc, case.render)
            self.maps = r.maps
            self.covers, self.cw, self.ch = cr.covers_of(r.maps), r.cw, r.ch
            _, self.boxes, _ = cr.geometry(case.sizes, case.h9s, want_covers=False)
        else:
            self.maps = None
            self.covers, self.boxes, (self.cw, self.ch) = cr.geometry(case.sizes, case.h9s)
        self._s = {}

    @property
    def shape(self):
        return (self.ch, self.cw)

    def depth(self, keep=None):
        return cr.depth_map(self.covers, keep, self.shape)

    def stats(self, step, keep="null"):
        if (step, keep) not in self._s:
            self._s[(step, keep)] = cr.stats_ref(self.covers, keep_mask(keep, self.n), step, self.shape)
        return self._s[(step, keep)]


_RESTATED = {}


def restate(orc, case) -> Restated:
    if case.tag not in _RESTATED:
        _RESTATED[case.tag] = Restated(orc, case)
    return _RESTATED[case.tag]


# ---- statistics cases ---------------------------------------------------------------------------------------------------------------------
def _reused_pred(case, r):
    """render_patterns' own predicate, asked of its own restatement"""
    return bool(case.render.pred(case.render, r.rp))


def _forty_pred(case, r):
    """depth 40: the >= 8 bucket and bins below it hold lattice points, per frame as well"""
    fs, hist = r.stats(1)
    at = fs["at_depth"].sum(axis=0)
    return _reused_pred(case, r) and int(r.depth().max()) == 40 and hist[8] > 0 and bool((hist[1:8] > 0).any()) and at[7] > 0 and bool((at[:7] > 0).any())


def _stack_pred(case, r):
    d = r.depth()[2]
    return d[6:9].tolist() == [7, 8, 9] and int(d.max()) == 9 and r.stats(1)[1][7] > 0 and r.stats(1)[1][8] > 0


def _list_pred(n):
    def pred(case, r):
        one_block = r.cw <= BLK and r.ch <= BLK and all(b is not None for b in r.boxes)
        return len(case.sizes) == n and one_block and int(r.depth().max()) > 8 and bool((r.stats(1)[1][1:8] > 0).any())
    return pred


def _edge_pred(case, r):
    """lattice points at pixel 255 and at pixel 256 of both axes exist at some step and are covered; at steps 7 and 37 the lattice points either
    side of the block edge are covered too"""
    d = r.depth()
    if not (r.cw > 260 and r.ch > 260 and 255 % 3 == 0 and 256 % 8 == 0 and 256 % 64 == 0):
        return False
    at = lambda p: d[p, p] > 0 and d[p, 0] > 0 and d[0, p] > 0
    straddle = all(at((255 // s) * s) and at((255 // s + 1) * s) and (255 // s + 1) * s < min(r.cw, r.ch) for s in (7, 37))
    return bool(at(255) and at(256) and straddle and int(d[250:262, 250:262].max()) >= 3)


def _far_pred(case, r):
    far = [b for b in r.boxes if b is not None and b[0] > ep.FAR]
    fs, hist = r.stats(64)
    return r.cw > 69000 and len(far) >= 2 and int(fs["at_depth"].sum()) > 0 and int(hist.sum()) == ((r.cw - 1) // 64 + 1) * ((r.ch - 1) // 64 + 1)


def _horizon_pred(case, r):
    """frame 0's horizon crosses the frame itself: its image is all but the span between its corners, so it takes part and covers nothing in
    its clipped box, while canvas pixels outside the box map back into it: only the box test keeps them out"""
    loose = cr.geometry(case.sizes, case.h9s, box_test=False)[0][0]
    x0, x1, y0, y1 = r.boxes[0]
    outside = loose.copy()
    outside[y0:y1 + 1, x0:x1 + 1] = False
    return r.boxes[0] is not None and bool(outside.any()) and not r.covers[0].any() and bool((r.covers[1] & outside).any())


def _sizes(imgs):
    return [(i.shape[1], i.shape[0]) for i in imgs]


def _tiny_frames(n, seed):
    """n frames of 2 - 6 pixels a side under integer translations of 0 .. 9: all of them meet the one list block"""
    rng = np.random.default_rng(seed)
    sizes = [(int(w), int(h)) for w, h in rng.integers(2, 7, (n, 2))]
    offs = rng.integers(0, 10, (n, 2))
    offs[0] = (0, 0)
    return sizes, np.stack([wp.shift(float(x), float(y)) for x, y in offs])


def stats_cases() -> List[Stats]:
    out = []
    for c in rp.cases():
        steps = ALL_STEPS if c.tag in ("forty", "straddle_overlap") else (1, 8) if not c.tag.startswith("canvas_") else (1, 3)
        pred = _forty_pred if c.tag == "forty" else _reused_pred
        out.append(Stats(c.tag, _sizes(c.imgs), c.h9s, steps, c.why, pred, render=c))
    far = ep.by_tag()["wide_69k"]
    out.append(Stats("wide_69k", _sizes(far.render.imgs), far.render.h9s, (64,), far.why + " (a list-block index above 256 in the cover walk)", _far_pred,
                     render=far.render))
    out.append(Stats("stack_789", [(12, 6)] * 9, np.stack([wp.shift(float(k), 0.0) for k in range(9)]), (1, 2),
                     "nine frames stacked a pixel apart: depth exactly 7, 8 and 9 at neighbouring lattice points, either side of the saturation", _stack_pred))
    for n in (65, 257, 600):
        sizes, h9s = _tiny_frames(n, 1000 + n)
        out.append(Stats("list%d" % n, sizes, h9s, (1, 3),
                         "%d frames meet one list block: past the 64 cover bits of a point, past a workgroup's lanes, past every chunk of list entries" % n, _list_pred(n)))
    out.append(Stats("horizon_inside", [(40, 10), (60, 10)], np.stack([wp.H(1, 0, 0, 0, 1, 0, -0.05, 0, 1), wp.shift(0, 0)]), (1, 3),
                     "a frame whose horizon (x = 20) crosses the frame: the map alone would let it cover pixels far outside its box", _horizon_pred))
    out.append(Stats("edge_255_256", [(300, 290), (40, 30), (30, 40)], np.stack([wp.shift(0, 0), wp.shift(236.0, 240.0), wp.shift(244.5, 232.25)]), ALL_STEPS,
                     "lattice points at pixels 255 and 256 of both axes, three frames across the list-block corner: tiles are cut at the block edge at every step",
                     _edge_pred))
    return out


def by_tag():
    return {c.tag: c for c in stats_cases()}


# ---- selection layouts ----------------------------------------------------------------------------------------------------------------------
class Select(NamedTuple):
    tag: str
    sizes: list
    h9s: np.ndarray
    step: int
    min_depth: int
    max_loss: int
    order: Optional[tuple]
    pairs: Optional[tuple]
    keep: Optional[tuple]
    why: str
    pred: Callable                   # pred(case, res): res = Result


class Result(NamedTuple):
    status: np.ndarray
    keep_out: np.ndarray
    rounds: int
    lost: int


def _shifts(offs):
    return np.stack([wp.shift(float(x), float(y)) for x, y in offs])


def geometry_of(case):
    return cr.geometry(case.sizes, case.h9s)


def stats_fn_of(case, covers, shape):
    return lambda keep: cr.stats_ref(covers, keep, case.step, shape)[0]


_RESULTS = {}


def reference(case, **mut) -> Result:
    """the round rule on the case (mut: cover_ref.select_rounds' mutations; only the plain result is kept)"""
    key = case.tag if not mut else None
    if key is None or key not in _RESULTS:
        covers, boxes, (cw, ch) = geometry_of(case)
        res = Result(*cr.select_rounds(len(case.sizes), boxes, stats_fn_of(case, covers, (ch, cw)), order=case.order, pairs=case.pairs, keep=case.keep,
                                       min_depth=case.min_depth, max_loss=case.max_loss, **mut))
        if key is None:
            return res
        _RESULTS[key] = res
    return _RESULTS[key]


def sequential(case):
    covers, boxes, (cw, ch) = geometry_of(case)
    return cr.select_sequential(len(case.sizes), boxes, stats_fn_of(case, covers, (ch, cw)), order=case.order, pairs=case.pairs, keep=case.keep,
                                min_depth=case.min_depth, max_loss=case.max_loss)


def _status(*want):
    return lambda case, res: tuple(int(s) for s in res.status) == want


def _and(*preds):
    return lambda case, res: all(p(case, res) for p in preds)


STRIP5 = ([(21, 11)] * 5, [(8 * k, 0) for k in range(5)])                  # covers 20 columns each, 8 apart: 60 % overlap


def select_cases() -> List[Select]:
    out = []
    s5, o5 = STRIP5
    out.append(Select("strip5_waits", s5, _shifts(o5), 1, 1, 40, (1, 2, 3), None, None,
                      "a five-frame strip at 60 % overlap: the drop of frame 1 makes 2 wait, 2 makes 3 wait; 2 goes at a loss of 4 x 10 points, 3 would cost 80",
                      _and(_status(0, 1, 1, 2, 0), lambda c, r: r.rounds >= 3 and r.rounds == 3 and r.lost == 40)))
    out.append(Select("waiting_blocks", [(21, 11)] * 5, _shifts([(12 * k, 0) for k in range(5)]), 1, 1, 120, (1, 2, 3), None, None,
                      "frames 12 apart: 3's box meets the waiting 2's but not the dropped 1's.  Settled a round early, 3 would go at 40 points and 2, alone over 200, would stay",
                      _and(_status(0, 1, 1, 1, 0), lambda c, r: r.rounds == 3 and r.lost == 280)))
    out.append(Select("two_clusters", [(20, 12)] * 6, _shifts([(0, 0), (1, 0), (2, 0), (200, 0), (201, 0), (202, 0)]), 1, 1, 0, (1, 4), None, None,
                      "two clusters far apart: one candidate in each, their boxes do not meet, both settle in one round",
                      _and(_status(0, 1, 0, 0, 1, 0), lambda c, r: r.rounds == 1 and r.lost == 0)))
    out.append(Select("crit_at_max_loss", [(20, 6), (20, 6), (20, 12), (20, 12)], _shifts([(0, 0), (2, 0), (100, 0), (101, 0)]), 1, 1, 10, (1, 3), None, None,
                      "frame 1 alone holds 2 x 5 = 10 points = max_loss and goes; frame 3 alone holds 1 x 11 = max_loss + 1 and stays",
                      _and(_status(0, 1, 0, 2), lambda c, r: r.lost == 10 and r.rounds == 1)))
    out.append(Select("fails_both", [(20, 10)] * 3, _shifts([(0, 0), (15, 0), (30, 0)]), 1, 1, 0, (1,), ((0, 1), (1, 2)), None,
                      "the middle of a chain is the sole cover of a band and a cut vertex: coverage is asked first, status 2 and not 3", _status(0, 2, 0)))
    out.append(Select("leaf_frees_cut_vertex", [(20, 10)] * 3 + [(40, 14)], _shifts([(2, 1), (4, 1), (6, 1), (0, 0)]), 1, 1, 0, (1, 2), ((0, 1), (1, 2)), None,
                      "chain 0 - 1 - 2 under a frame that covers all three: 1 is settled first as a cut vertex, then the leaf 2 goes; 1 would now be a leaf but a settled candidate stays settled",
                      _and(_status(0, 3, 1, 0), lambda c, r: r.rounds == 1)))
    out.append(Select("block3x3_depth2", [(21, 21)] * 9, _shifts([(10 * i, 10 * j) for j in range(3) for i in range(3)]), 1, 2, 0, tuple(range(9)), None, None,
                      "min_depth = 2 on a 3 x 3 block at 50 % overlap: only the centre lies 4 deep everywhere; its drop makes the frames after it wait a round",
                      _and(_status(2, 2, 2, 2, 1, 2, 2, 2, 2), lambda c, r: r.rounds == 2 and r.lost == 0)))
    out.append(Select("order_null", s5, _shifts(o5), 1, 1, 0, None, None, None,
                      "order = NULL on the strip: the candidates are every kept frame by ascending crit of the first round (1, 2, 3, 0, 4)",
                      _and(_status(2, 1, 2, 1, 2), lambda c, r: r.rounds == 3)))
    gone = _shifts([(0, 0), (1, 0), (2, 0), (0, 0)])
    gone[1][8] = 0
    out.append(Select("not_examined", [(20, 10)] * 3 + [(30, 14)], gone, 1, 1, 0, (0, 1, 2), None, (0, 1, 1, 1),
                      "a candidate with keep = 0 and a skipped one (m8 = 0) get status 4 and are never examined; the third goes",
                      _and(_status(4, 4, 1, 0), lambda c, r: tuple(r.keep_out) == (0, 0, 0, 1) and r.rounds == 1)))
    return out


def by_select():
    return {c.tag: c for c in select_cases()}


def random_layout(seed, with_pairs=False) -> Select:
    """3 .. 12 small frames thrown on a spot, random step, depth, loss, order (a permutation of a subset, or NULL) and keep"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(3, 13))
    sizes = [(int(w), int(h)) for w, h in rng.integers(6, 21, (n, 2))]
    offs = rng.integers(0, 36, (n, 2))
    offs[0] = (0, 0)
    h9s = _shifts(offs.tolist())
    if rng.random() < 0.3:
        h9s[int(rng.integers(1, n))][8] = 0
    keep = tuple(int(v) for v in (rng.random(n) < 0.85)) if rng.random() < 0.5 else None
    order = None if rng.random() < 0.3 else tuple(int(k) for k in rng.permutation(n)[:int(rng.integers(1, n + 1))])
    pairs = None
    if with_pairs:
        every = [(a, b) for a in range(n) for b in range(a + 1, n)]
        pick = rng.permutation(len(every))[:int(rng.integers(n - 1, 2 * n))]
        pairs = tuple(every[i] if rng.random() < 0.5 else every[i][::-1] for i in pick)
    return Select("random_%d%s" % (seed, "_pairs" if with_pairs else ""), sizes, h9s, int(rng.choice([1, 2, 3])), int(rng.integers(1, 4)),
                  int(rng.choice([0, 5, 30])), order, pairs, keep, "seeded random boxes", lambda c, r: True)


RANDOM_SEEDS = range(200)
