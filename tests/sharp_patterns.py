"""Cases of frame sharpness (csrc/sharp.hip, csrc/sharp_solve.cpp): pure numpy, seeded, no GPU, no oracle import.

Stats cases: a subset of tests/render_patterns.py's cases reused as they stand (pair lists from render_patterns.gain_pairs), plus what the
five-point rule adds.  Every case carries a tag, a kind, one line on why it is there and a predicate over the RESTATEMENT'S output (Restated
below: render_patterns.restate and what sharp_ref makes of it), so that a later edit of a size or a matrix cannot quietly turn it into an
ordinary case.  tests/test_sharp_patterns_ref.py asserts the predicates; tests/test_gpu_sharp.py compares sharp_stats_kernel with the
restatement on every case at each of its steps.

render_patterns' height cases hold frames 5 and 3 pixels wide: at no height can both frames have a Laplacian at one point, so their pair
records are all zero.  Heights 1, 2 and 3 are reused as they stand (all-zero is their point; 3 is render_patterns._height_case(3), the
list there has no 3); heights 8, 9, 17 and 257 are rebuilt here the same way from frames 9 and 7 pixels wide, or they would only add
all-zero cases (the cap on those is asserted in tests/test_sharp_patterns_ref.py).

Graph cases: records made by hand for the host code (solve, flag, select).
"""
import itertools
from typing import Callable, List, NamedTuple, Optional, Tuple

import numpy as np

from tests import render_patterns as rp
from tests import sharp_ref as sr
from tests import warp_patterns as wp
from tests.synth import texture

MAX_PAIRS = rp.MAX_PAIRS
L_MAX2 = 1020 * 1020


class Stats(NamedTuple):
    tag: str
    render: rp.Render                # frames and homographies (for a reused case: render_patterns' own object)
    kind: str                        # "reused" | "height" | "edge" | "new"
    steps: Tuple[int, ...]
    why: str
    pred: Callable                   # pred(case, r): r a Restated
    pads: Optional[Tuple[int, ...]] = None      # row padding in bytes per frame on the device (None: 3 w)


class Restated:
    """the render restatement of a case (render_patterns.Restated: maps, cw, ch, ...) and what sharp_ref makes of it: lm (lap_maps), pairs,
    and stats(step) -> (pair records, frame records), made when first asked for, then kept"""
    def __init__(self, orc, case):
        self.case = case
        self.r = rp.restate(orc, case.render)
        self.maps, self.cw, self.ch = self.r.maps, self.r.cw, self.r.ch
        self.lm = sr.lap_maps(self.maps)
        self.pairs = rp.gain_pairs(case.render, self.r, reverse=False) if case.kind == "reused" else list(itertools.combinations(range(len(case.render.imgs)), 2))[:MAX_PAIRS]
        self._s = {}

    def stats(self, step):
        if step not in self._s:
            self._s[step] = sr.stats_ref(self.lm, self.pairs, step)
        return self._s[step]

    def covered(self, step):
        return sr.covered_both(self.maps, self.pairs, step)


_RESTATED = {}


def restate(orc, case) -> Restated:
    if case.tag not in _RESTATED:
        _RESTATED[case.tag] = Restated(orc, case)
    return _RESTATED[case.tag]


# ---- predicates ---------------------------------------------------------------------------------------------------------------------------------
def _all_zero(case, r):
    return all(not r.stats(s)[0]["n"].any() for s in case.steps)


def _no_laplacian_at_all(case, r):
    """no frame has a Laplacian anywhere: every count is 0, the frames' too"""
    return _all_zero(case, r) and all(not r.stats(s)[1]["n"].any() for s in case.steps) and r.ch <= 3


def _some(case, r):
    return bool(r.stats(case.steps[0])[0]["n"].any())


def _cut_down(case, r, step=None):
    """a pair with 0 < n < the lattice points both frames cover: the five-point rule is exercised"""
    step = case.steps[0] if step is None else step
    return any(0 < int(n) < c for n, c in zip(r.stats(step)[0]["n"], r.covered(step)))


def _height_pred(H):
    return lambda case, r: r.ch == H and _some(case, r) and _cut_down(case, r) and int(r.lm[0][2].any(axis=1).sum()) == H - 3


def _overlap_cols(k, n1):
    def pred(case, r):
        both = r.maps[0][1] & r.maps[1][1]
        return int(both.any(axis=0).sum()) == k and int(r.stats(1)[0]["n"][0]) == n1 and (n1 == 0 or _cut_down(case, r, 1))
    return pred


def _row0_pred(case, r):
    """the frames overlap, every lattice point of the overlap lies on canvas row 0, and without the border rule the wrap would count them"""
    both = r.maps[0][1] & r.maps[1][1]
    wrapped = sr.stats_ref(sr.lap_maps(r.maps, border_rule=False), r.pairs, case.steps[0])[0]
    return r.ch == 1 and both[0].sum() > 20 and _all_zero(case, r) and int(wrapped["n"][0]) > 0


def _east_pred(case, r):
    """at lattice step 2 column 38 is covered by both frames and frame 0 has no sample east of it"""
    c0, c1, has0 = r.maps[0][1], r.maps[1][1], r.lm[0][2]
    return bool((c0[2:28:2, 38] & c1[2:28:2, 38]).all()) and not c0[:, 39].any() and not has0[:, 38].any() and bool(has0[2:28, 36].all()) and _cut_down(case, r, 2)


def _south_pred(case, r):
    """the half-turned frame 1 covers its canvas box's far ends and not its near ends: column 22 has its centre and no west neighbour"""
    c0, c1, has1 = r.maps[0][1], r.maps[1][1], r.lm[1][2]
    return bool((c0[16:30, 22] & c1[16:30, 22]).all()) and not c1[:, 21].any() and not has1[:, 22].any() and _cut_down(case, r, 1) and _cut_down(case, r, 2)


def _flat_pred(case, r):
    s = r.stats(1)[0][0]
    return int(s["n"]) > 100 and int(s["e_a"]) == 0 and int(s["s_a"]) == 128 * int(s["n"]) and int(s["e_b"]) > 0 and not sr.usable(r.stats(1)[0]).any()


def _checker_pred(case, r):
    """every Laplacian is +-1020, and the overlap holds a whole 64 x 16 tile of them counted from the intersection box's corner (3, 1): lattice
    columns 67 .. 130, rows 17 .. 32 at step 1 -- one workgroup's 1024 points all carry 1020^2: 1.07e9, the bound the 32-bit reduction is sized for"""
    ok = True
    for step in case.steps:
        s = r.stats(step)[0][0]
        ok = ok and int(s["n"]) > 0 and int(s["e_a"]) == int(s["n"]) * L_MAX2 and int(s["e_b"]) == int(s["n"]) * L_MAX2
    both = r.lm[0][2] & r.lm[1][2]
    first = both.any(axis=0).argmax(), both.any(axis=1).argmax()
    return ok and first == (5, 3) and bool(both[17:33, 67:131].all()) and 1024 * L_MAX2 < 2 ** 32


def _steps_pred(case, r):
    return case.steps == (1, 3, 8, 64) and all(int(r.stats(s)[0]["n"][0]) > 0 for s in case.steps) and int(r.stats(64)[0]["n"][0]) <= 6


def _pitch_pred(case, r):
    return case.pads is not None and all(p > 0 for p in case.pads) and any(p % 4 for p in case.pads) and any(p >= 8 for p in case.pads) and all(int(n) > 0 for n in r.stats(1)[0]["n"])


def _seventy_pred(case, r):
    st = r.stats(1)[0]
    return len(case.render.imgs) == 70 and len(r.pairs) == 60 and bool((st["n"] > 0).all()) and r.cw < 64 and r.ch < 64


def _reused_pred(extra=None):
    def pred(case, r):
        return bool(case.render.pred(case.render, r.r)) and (extra is None or bool(extra(case, r)))
    return pred


def _skipped_pred(which):
    def pred(case, r):
        sk = rp.skipped(case.render, r.r)
        st = r.stats(1)[0]
        return sk == which and all(int(s["n"]) == 0 for s, (a, b) in zip(st, r.pairs) if a in sk or b in sk) and all(r.lm[k] is None or not r.lm[k][2].any() for k in sk)
    return pred


def _twins_pred(case, r):
    """frames 1 and 2 share a homography: their pair has a Laplacian wherever either has one"""
    i = r.pairs.index((1, 2))
    fs = r.stats(1)[1]
    return int(r.stats(1)[0]["n"][i]) == int(fs["n"][1]) == int(fs["n"][2]) > 100


# ---- cases --------------------------------------------------------------------------------------------------------------------------------------
def _render(tag, imgs, h9s, why):
    return rp.Render(tag, imgs, np.stack(h9s), why, lambda c, r: True, new=True)


def _own_height(H):
    imgs = [wp.noise(9, H, 880 + H), wp.noise(7, H, 881 + H)]
    why = "canvas height %d with frames wide enough for a common Laplacian: the last tile row of 16 lattice rows and the last lattice row at its edge" % H
    return Stats("sharp_h%d" % H, _render("sharp_h%d" % H, imgs, [wp.shift(0, 0), wp.shift(1.5, 0)], why), "height", (1, 3), why, _height_pred(H))


def _two(tag, kind, imgs, h9s, steps, why, pred, pads=None):
    return Stats(tag, _render(tag, imgs, h9s, why), kind, steps, why, pred, pads)


def stats_cases() -> List[Stats]:
    base = rp.by_tag()
    out = []
    for H in (1, 2):
        out.append(Stats("canvas_h%d" % H, base["canvas_h%d" % H], "reused", (1, 3), "canvas height %d: no pixel has four neighbours" % H, _reused_pred(_no_laplacian_at_all)))
    out.append(Stats("canvas_h3", rp._height_case(3), "reused", (1, 3), "canvas height 3: row 1 has both neighbours, and the frames' [0, h-1) cover ends at row 1",
                     _reused_pred(_no_laplacian_at_all)))
    for H in (8, 9, 17, 257):
        out.append(_own_height(H))
    out.append(Stats("straddle_overlap", base["straddle_overlap"], "reused", (1, 3, 8), base["straddle_overlap"].why, _reused_pred(lambda c, r: _some(c, r) and _cut_down(c, r))))
    out.append(Stats("twins", base["twins"], "reused", (1, 3), base["twins"].why, _reused_pred(_twins_pred)))
    out.append(Stats("m8_zero_ends", base["m8_zero_ends"], "reused", (1, 3), base["m8_zero_ends"].why, _reused_pred(lambda c, r: _skipped_pred([0, 3])(c, r) and _some(c, r))))
    out.append(Stats("rank_deficient", base["rank_deficient"], "reused", (1, 3), base["rank_deficient"].why, _reused_pred(_skipped_pred([1]))))
    for tag in ("hidden", "forty", "turns", "scaled_matrices"):
        out.append(Stats(tag, base[tag], "reused", (1, 3), base[tag].why, _reused_pred(lambda c, r: _some(c, r) and _cut_down(c, r))))
    tex = lambda w, h, seed: texture(w, h, seed=seed)
    out.append(_two("sharp_overlap3", "edge", [tex(40, 32, 1), tex(40, 32, 2)], [wp.shift(0, 0), wp.shift(36, 0)], (1,),
                    "two 40 x 32 frames whose overlap is exactly 3 canvas columns wide: only the middle one can hold a Laplacian", _overlap_cols(3, 29)))
    out.append(_two("sharp_overlap2", "edge", [tex(40, 32, 3), tex(40, 32, 4)], [wp.shift(0, 0), wp.shift(37, 0)], (1,),
                    "the same with 2 columns: none can", _overlap_cols(2, 0)))
    out.append(_two("sharp_row0", "edge", [tex(48, 2, 5), tex(48, 2, 6)], [wp.scale(1.0, 0.4), wp.scale(1.0, 0.4, 3.0, 0)], (1, 8),
                    "an overlap whose lattice points all lie on canvas row 0: excluded by 1 <= y, counted by a walk that wraps", _row0_pred))
    out.append(_two("sharp_east_edge", "edge", [tex(40, 32, 7), tex(40, 32, 8)], [wp.shift(0, 0), wp.shift(30, 0)], (2, 1),
                    "a lattice point whose centre both frames sample but whose east neighbour frame 0 does not: the frame's [0, w-1) edge", _east_pred))
    out.append(_two("sharp_west_edge_turned", "edge", [tex(40, 32, 9), tex(40, 32, 10)], [wp.shift(0, 0), wp.turn(180, 60, 45)], (1, 2),
                    "the same edge on a half-turned frame, where it is the west and north neighbours that go missing", _south_pred))
    out.append(_two("sharp_flat", "new", [np.full((32, 40, 3), 128, np.uint8), tex(40, 32, 11)], [wp.shift(0, 0), wp.shift(6.5, 3.25)], (1, 3),
                    "a flat frame: e = 0 with n > 0, an unusable pair", _flat_pred))
    out.append(_two("sharp_checker1020", "new", [wp.checker(1)(200, 40), wp.checker(1)(200, 40)], [wp.shift(0, 0), wp.shift(4, 2)], (1, 2),
                    "all-255 against all-0 checker at integer offsets: every L is +-1020 and one workgroup's 1024 points all carry 1020^2, the 32-bit reduction bound",
                    _checker_pred))
    out.append(_two("sharp_steps", "new", [tex(200, 150, 12), tex(200, 150, 13)], [wp.shift(0, 0), wp.yaw(3, 1.0, 60.5, 20.25)], (1, 3, 8, 64),
                    "steps 1, 3, 8 and 64 on one overlap: at 64 a handful of points", _steps_pred))
    out.append(_two("sharp_pitch", "new", [tex(37, 23, 14), tex(37, 23, 15), tex(30, 20, 16)],
                    [wp.shift(0, 0), wp.times(wp.yaw(7, 1.1, 5.5, 3.25), 2), wp.shift(9.75, 4.5)], (1, 3),
                    "padded pitches 3 w + 1, + 7, + 16: the 8-byte and the 4 + 2 byte loads at a row's end", _pitch_pred, pads=(1, 7, 16)))
    n = 70
    out.append(_two("sharp_seventy", "new", [wp.noise(24, 20, 300 + k) for k in range(n)], [wp.shift((k * 7) % 5 + 0.25 * (k % 4), (k * 3) % 4 + 0.5 * (k % 2)) for k in range(n)], (1, 3),
                    "70 frames on one spot: 60 pairs on one tile region, every record's atomics land beside the others'", _seventy_pred))
    return out


def by_tag():
    return {c.tag: c for c in stats_cases()}


# ---- graph cases: records made by hand ------------------------------------------------------------------------------------------------------------
class Graph(NamedTuple):
    tag: str
    n: int
    records: np.ndarray              # sharp_ref.PAIR
    blur_ratio: float
    status: Tuple[int, ...]          # what the definition gives, worked out by hand
    why: str


def records(edges, amp, n_pts=None, e0=10 ** 8, s0=10 ** 6):
    """records of frames with Laplacian amplitude amp[k] over equal brightness: pair (a, b) gets e = e0 amp^2, s = s0, n = n_pts[i] or 1000"""
    st = np.zeros(len(edges), sr.PAIR)
    for i, (a, b) in enumerate(edges):
        st[i] = (a, b, 1000 if n_pts is None else n_pts[i], int(round(e0 * amp[a] ** 2)), int(round(e0 * amp[b] ** 2)), s0, s0)
    return st


def graph_cases() -> List[Graph]:
    out = []
    one = lambda n, **kw: [kw.get("k%d" % k, 1.0) for k in range(n)]
    chain = [(k, k + 1) for k in range(4)]
    out.append(Graph("chain5_middle", 5, records(chain, one(5, k2=0.5)), 0.58, (0, 0, 2, 0, 0), "a chain of 5 with the middle frame blurred: a cut vertex, kept"))
    grid = [(3 * y + x, 3 * y + x + 1) for y in range(3) for x in range(2)] + [(3 * y + x, 3 * y + x + 3) for y in range(2) for x in range(3)]
    out.append(Graph("grid3x3_centre", 9, records(grid, one(9, k4=0.5)), 0.58, (0, 0, 0, 0, 1, 0, 0, 0, 0), "a 3 x 3 grid with the centre blurred: dropped"))
    ring = [(k, (k + 1) % 6) for k in range(6)]
    out.append(Graph("ring6_opposite", 6, records(ring, one(6, k1=0.5, k4=0.4)), 0.58, (0, 2, 0, 0, 1, 0),
                     "two blurred frames in a ring of 6, not adjacent: the blurrier (4) goes first and leaves a chain in which the other is a cut vertex -- "
                     "in index order it would be 1 that goes and 4 that stays"))
    out.append(Graph("ring6_neighbours", 6, records(ring, one(6, k1=0.09, k2=0.165)), 0.58, (0, 1, 0, 0, 0, 0),
                     "two blurred NEIGHBOURS in a ring of 6: frame 2 is measured against the lower median of its partners, which is frame 1, and is not "
                     "flagged; frame 1 is dropped (removing two neighbours of a ring would leave a chain, not a split: the split is ring6_opposite's)"))
    out.append(Graph("ring6_tie", 6, records(ring, one(6, k1=0.5, k4=0.5)), 0.58, (0, 1, 0, 0, 2, 0),
                     "equal rel by symmetry: the lower index goes first (where the two rel differ in a last bit, the order is the solve's, see the test)"))
    lone = records([(0, 1), (0, 3)], one(4, k1=0.5))
    lone[1]["e_b"] = 0
    out.append(Graph("component_of_one", 4, lone, 0.58, (0, 1, 3, 3), "frame 2 in no pair, frame 3 only in an unusable one: status 3; frames 0 and 1 a component of two"))
    dead = records(chain, one(5))
    dead["e_a"] = 0
    out.append(Graph("unusable_only", 5, dead, 0.58, (3, 3, 3, 3, 3), "unusable pairs only: status 3 and sharp exactly 1 everywhere"))
    return out


def random_records(seed, n_max=40):
    """a random connected-ish pair graph with n <= n_max frames, a few blurred, a few unusable pairs, n over three orders of magnitude"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, n_max + 1))
    every = list(itertools.combinations(range(n), 2))
    keep = sorted(set([(k, k + 1) for k in range(n - 1) if rng.random() < 0.9] + [every[i] for i in rng.choice(len(every), min(len(every), 2 * n), replace=False)]))
    edges = [(b, a) if rng.random() < 0.3 else (a, b) for a, b in keep]
    amp = np.exp(rng.normal(0, 0.08, n))
    amp[rng.random(n) < 0.15] *= rng.uniform(0.2, 0.7)
    gain = np.exp(rng.normal(0, 0.05, n))
    st = np.zeros(len(edges), sr.PAIR)
    for i, (a, b) in enumerate(edges):
        npts = int(10 ** rng.uniform(0, 4))
        ground = 10 ** rng.uniform(1, 4) * np.exp(rng.normal(0, 0.02, 2))
        st[i] = (a, b, npts, int(npts * ground[0] * (amp[a] * gain[a]) ** 2) + 1, int(npts * ground[1] * (amp[b] * gain[b]) ** 2) + 1,
                 int(npts * 100 * gain[a]) + 1, int(npts * 100 * gain[b]) + 1)
        if rng.random() < 0.08:
            st[i][str(rng.choice(["n", "e_a", "e_b", "s_a", "s_b"]))] = 0
    return n, st


# ---- the blur-ratio measurement: seeded strips with one blurred frame ------------------------------------------------------------------------
QUALITY_SIGMAS = (0.7, 1.0, 1.5, 2.0, 3.0)
QUALITY_SEEDS = (1, 2, 3)
QUALITY_STEP = 4


def gaussian_blur(a, sigma):
    """separable Gaussian on a float [h, w, 3] array, radius ceil(3 sigma), edges replicated"""
    r = int(np.ceil(3 * sigma))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    for axis in (0, 1):
        pad = [(r, r) if ax == axis else (0, 0) for ax in range(3)]
        p = np.pad(a, pad, mode="edge")
        a = sum(k[i] * np.take(p, np.arange(i, i + a.shape[axis]), axis=axis) for i in range(2 * r + 1))
    return a


def blur_strip(seed, sigma, blurred=3, n=8, w=160, h=120):
    """(imgs, h9s, pairs): n frames of w x h cut from one tests/synth texture along a strip (about 60 % forward overlap, whole-pixel
    offsets: the cut is the frame), each with its own gain in [0.95, 1.05] and N(0, 2) noise; frame `blurred` is blurred by a Gaussian of sigma pixels
    before gain and noise (sigma None: no frame is).  Pairs: every frame with its next two."""
    rng = np.random.default_rng(1000 + seed)
    dx = 0.4 * w
    ox = [int(round(k * dx + rng.uniform(-4, 4))) + 16 for k in range(n)]
    oy = [int(rng.integers(0, 9)) + 8 for k in range(n)]
    big = texture(max(ox) + w + 16, h + 32, seed=seed).astype(np.float64)
    imgs, h9s = [], []
    for k in range(n):
        cut = big[oy[k] - 8:oy[k] + h + 8, ox[k] - 8:ox[k] + w + 8]
        if sigma is not None and k == blurred:
            cut = gaussian_blur(cut, sigma)
        cut = cut[8:-8, 8:-8] * rng.uniform(0.95, 1.05) + rng.normal(0, 2, (h, w, 3))
        imgs.append(np.ascontiguousarray(np.clip(np.floor(cut + 0.5), 0, 255).astype(np.uint8)))
        h9s.append(wp.shift(ox[k] - ox[0], oy[k] - min(oy)))
    pairs = [(k, k + d) for k in range(n) for d in (1, 2) if k + d < n]
    return imgs, np.stack(h9s), pairs


def measure_strip(orc, seed, sigma, step=QUALITY_STEP, blurred=3):
    """(exp(rel) of every frame, the pair records) of blur_strip(seed, sigma) by the numpy restatement"""
    from tests import gain_ref as gr
    imgs, h9s, pairs = blur_strip(seed, sigma, blurred)
    st = sr.stats_ref(sr.lap_maps(gr.frame_sample_maps(orc, imgs, h9s)), pairs, step)[0]
    l = sr.solve_ref(st, len(imgs))
    return np.exp(sr.rel_ref(l, st, len(imgs))), st
