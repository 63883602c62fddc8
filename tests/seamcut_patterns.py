"""The cases of the optimised seamlines (tests/seamcut_ref.py): small surveys under integer translations (every clean sample is the scene's
byte), each built to hold one thing the label stage can get wrong.  A case is (imgs, h9s, params dict); tests/test_seamcut_ref.py asserts on
the reference that each case holds what its name says, tests/test_gpu_seamcut.py that the build gives the reference's bytes on every one.

The edge cases live in dicts of their own (WAVE_CASES, REM_CASES, RECORD_EDGE_CASES; CASES and RECORD_CASES and the tests parametrised over
them stay as they were): surveys with more frames in one list block than a wave has lanes, canvases with every remainder of the cell side
that matters to the probe clamp, and records with up to 8 filled slots.  tests/test_seamcut_edges_ref.py asserts what they hold,
tests/test_gpu_seamcut_edges.py runs them and the cases of tests/render_patterns.py (edge_reference) through the build.
"""
import numpy as np

from tests import seamcut_ref as sc
from tests.synth import texture


def _translations(offs):
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (len(offs), 1))
    for k, (ox, oy) in enumerate(offs):
        h9s[k, 2], h9s[k, 5] = ox, oy
    return h9s


def _cuts(scene, offs, w, h):
    return [np.ascontiguousarray(scene[oy:oy + h, ox:ox + w]) for ox, oy in offs]


SEAM_X = 43.5                                                               # the mid-seam of two 64-wide frames 24 apart: canvas x <= 43 lies deeper in frame 0
CRAFTED = {                                                                 # (frames, relief): canvas rectangle (x, y, width, height) of frame 1's copy
    (2, False): (40, 36, 16, 24), (3, False): (40, 40, 16, 16),             # moved object: columns 40 .. 43, a quarter of it, on frame 0's side
    (2, True): (46, 36, 8, 24), (3, True): (46, 36, 8, 24),                 # relief: frame 0's copy is x = 40 .. 47, half of it on either side
    "symmetric": (40, 36, 8, 24),                                           # moved object, half on either side: the known limit (stays cut)
}


def crafted(frames=2, relief=False, symmetric=False, **kw):
    """two or three 64 x 96 looks at one planar scene: frame 1 is 24 px right of frame 0 (62 % overlap, the geometric mid-seam between canvas
    x = 43 and 44, on a cell boundary at level 2), the third 12 right and 40 down.  A white rectangle that only frame 1 has (a moved object)
    or, relief, that frame 0 has 6 px further left.  The rectangle the tests ask about is the one the mid-seam runs through: frame 1's copy
    for the moved object -- placed asymmetrically, a quarter of its columns on frame 0's side -- and frame 0's copy in the relief cases, which
    the seam halves.  symmetric: a moved object with half its columns on either side, which the aggregation leaves cut (its rows have two
    equal optima and every cell keeps slot 0).  The placements come from scratch/seamcut_quality.py's search on the reference.
    (imgs, h9s, params, rect of the rectangle asked about)"""
    w, h, dx = 64, 96, 24
    x, y, rw, rh = CRAFTED["symmetric" if symmetric else (frames, relief)]
    offs = [(0, 0), (dx, 0), (12, 40)][:frames]
    scene = texture(w + 40, h + 60, seed=301)
    imgs = _cuts(scene, offs, w, h)
    imgs[1][y:y + rh, x - dx:x - dx + rw] = 255
    if relief:
        imgs[0][y:y + rh, x - 6:x - 6 + rw] = 255
    return imgs, _translations(offs), sc.params(level=2, **kw), ((x - 6 if relief else x), y, rw, rh)


def strip(cells, vertical=False, level=2, **kw):
    """a strip one cell row wide and `cells` cells long: frames 96 long every 64 px along it, alternating textures"""
    s = 1 << level
    length, step, flen = cells * s, 64, 96
    starts = list(range(0, max(length - flen, 0) + 1, step))
    if starts[-1] + flen < length:
        starts.append(length - flen)
    if length < flen:
        starts, flen = [0], length
    imgs = []
    for k, _ in enumerate(starts):
        t = texture(flen, s, seed=320 + k)
        imgs.append(np.ascontiguousarray(t.transpose(1, 0, 2)) if vertical else t)
    offs = [(0, a) if vertical else (a, 0) for a in starts]
    return imgs, _translations(offs), sc.params(level=level, **kw)


def holes():
    """three 40 x 32 frames in an L with gaps: cells nothing covers between the frames, on horizontal and on vertical paths"""
    offs = [(0, 0), (64, 0), (0, 56)]
    imgs = [texture(40, 32, seed=330 + k) for k in range(3)]
    return imgs, _translations(offs), sc.params(level=2)


def staircase(depth=4):
    """seven 64 x 24 frames each 8 px right of the last, behind a gap: along a row the number of candidates climbs from 0 to depth"""
    offs = [(0, 0)] + [(80 + 8 * k, 0) for k in range(6)]
    imgs = [texture(64, 24, seed=340 + k) for k in range(7)]
    imgs[0] = texture(16, 24, seed=339)
    return imgs, _translations(offs), sc.params(level=2, depth=depth)


def nine(depth):
    """nine 40 x 40 frames a pixel or two apart: nine contributors in every central cell"""
    offs = [(k % 3, k // 3) for k in range(9)]
    imgs = [texture(40, 40, seed=350 + k) for k in range(9)]
    return imgs, _translations(offs), sc.params(level=3, depth=depth)


def twins(same_image=True):
    """two frames under the same transform (equal omega everywhere: the index orders the slots) beside a third; with the same image in
    both, the twins' slots cost the same everywhere: an argmin tie"""
    a = texture(64, 48, seed=360)
    imgs = [a, a.copy() if same_image else texture(64, 48, seed=361), texture(64, 48, seed=362)]
    return imgs, _translations([(0, 0), (0, 0), (30, 6)]), sc.params(level=2)


def skipped(level=3):
    """four frames, one with h9[8] == 0: it takes part in the layout and in nothing else"""
    offs = [(0, 0), (50, 10), (25, 40), (300, 0)]
    imgs = [texture(96, 64, seed=370 + k) for k in range(4)]
    h9s = _translations(offs)
    h9s[3, 8] = 0.0
    return imgs, h9s, sc.params(level=level)


def projective():
    """the 10-frame case of tests/test_gpu_gain.py cut down: scaled, rotated and projective frames, a skipped one"""
    from tests.synth import warp_cases
    Hs = warp_cases()
    imgs = [texture(128, 96, 380 + k) for k in range(5)]
    h9s = np.zeros((5, 9), np.float32)
    off = [(0, 0), (70, 10), (140, -20), (40, 60), (100, 70)]
    for k in range(5):
        h9s[k] = Hs[[0, 2, 1, 3, 4][k]]
        h9s[k, 2] += off[k][0]
        h9s[k, 5] += off[k][1]
    return imgs, h9s, sc.params(level=3, ramp=16)


CASES = {
    "crafted2": lambda: crafted(2)[:3],
    "crafted3": lambda: crafted(3)[:3],
    "relief2": lambda: crafted(2, relief=True)[:3],
    "relief3": lambda: crafted(3, relief=True)[:3],
    "symmetric2": lambda: crafted(2, symmetric=True)[:3],
    "crafted2_depth1": lambda: crafted(2, depth=1)[:3],
    "crafted3_free": lambda: crafted(3, diff_weight=0, seam_penalty=0)[:3],
    "grid_1x1": lambda: strip(1, level=5),
    "grid_1xN": lambda: strip(7, level=4),
    "grid_Nx1": lambda: strip(7, vertical=True, level=4),
    "holes": holes,
    "staircase": staircase,
    "nine_depth4": lambda: nine(4),
    "nine_depth8": lambda: nine(8),
    "twins": twins,
    "twins_differ": lambda: twins(False),
    "strip_63": lambda: strip(63),
    "strip_64": lambda: strip(64),
    "strip_65": lambda: strip(65),
    "strip_255": lambda: strip(255),
    "strip_256": lambda: strip(256),
    "strip_257": lambda: strip(257),
    "strip_65_v": lambda: strip(65, vertical=True),
    "strip_257_v": lambda: strip(257, vertical=True),
    "skipped_level3": skipped,
    "level5": lambda: skipped(5),
    "projective": projective,
}



def random_records(gw, gh, seed, frames=5, holes=0.15, slots=4, ids=None, **kw):
    """cell records that come from no survey: per cell 0 .. `slots` distinct frames out of `frames`, weights descending, any gray.  The label
    stage takes records as they are, and only here can one frame stand on both sides of an empty cell (frames on a canvas are convex).
    ids: the frame id (frame + 1) each of the `frames` frames goes by, 1 .. frames when None."""
    rng = np.random.default_rng(seed)
    ids = np.arange(1, frames + 1) if ids is None else np.asarray(ids)
    assert len(ids) == frames and len(set(ids.tolist())) == frames and ids.min() >= 1 and ids.max() <= 65535
    frame = np.zeros((gh, gw, sc.SLOTS), np.uint16); omega = np.zeros((gh, gw, sc.SLOTS), np.uint8); gray = np.zeros((gh, gw, sc.SLOTS), np.uint8)
    for y in range(gh):
        for x in range(gw):
            m = 0 if rng.random() < holes else int(rng.integers(1, slots + 1))
            frame[y, x, :m] = ids[rng.permutation(frames)[:m]]
            omega[y, x, :m] = np.sort(rng.integers(1, 256, m))[::-1]
            gray[y, x, :m] = rng.integers(0, 256, m)
    return frame, omega, gray, sc.params(**kw)


RECORD_CASES = {
    "records_holes": lambda: random_records(9, 7, seed=0),
    "records_dear": lambda: random_records(300, 1, seed=0, frames=40, holes=0.0, data_weight=16, diff_weight=16, seam_penalty=255, miss_cost=255),
    "records_dear_v": lambda: tuple(a.swapaxes(0, 1) if isinstance(a, np.ndarray) else a for a in RECORD_CASES["records_dear"]()),
}

# ---- more frames in one list block than a wave has lanes ----------------------------------------------------------------------------
# seam_candidates_kernel shares the list positions of a cell's list block out to the 64 lanes of a wave (position e to lane e % 64), each lane
# keeps a sorted top 8, and the wave draws the cell's `depth` winners from the lanes' heads.  mosaic_lists_kernel lists a block's frames
# highest index first: with all N frames of a survey in block 0 (a canvas below 256 a side, no frame skipped), frame k is at list position
# N - 1 - k.
WAVE = 64


def lane_of(n, k):
    """the lane of seam_candidates_kernel that is handed frame k of an n-frame survey whose frames all lie in list block 0"""
    return (n - 1 - k) % WAVE


def _noise_frames(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]


STACK_PROBE = 18                                                            # wave130: the probe pixel (x = y) of cell (4, 4) at level 2
STACK = {129: 6, 65: 8, 1: 7, 128: 7, 64: 6, 0: 8}                          # wave130: frame -> offset in both axes of a 16 x 16 frame; lanes 0 and 1
STACK_ORDER = (65, 0, 128, 1, 129, 64)                                      # the order (omega, k) puts them in at that probe: omega 159, 159, 128, 128, 96, 96


def _omega_at(p, off, size):
    """omega of a translated frame (ramp 0: the full tent) at canvas pixel (p, p), 0 where it gives no sample (tests/feather_ref.py: wk_image)"""
    (ox, oy), (w, h) = off, size
    d = min(p - ox, ox + w - 1 - p, p - oy, oy + h - 1 - p)
    if d < 0 or p > ox + w - 2 or p > oy + h - 2:
        return 0
    R = (min(w, h) + 1) // 2
    return 1 + 254 * min(d, R) // R


def wave(n, seed, level=2, side=(12, 16), reach=8, stack=None):
    """n tiny noise frames under integer translations drawn at random from 0 .. reach in both axes (not monotone in k: keys reach a lane in
    mixed order), sides drawn from side[0] .. side[1]; a frame at (0, 0) and one of the largest side at (reach, reach), so that the canvas
    is reach + side[1] a side whatever was drawn.  stack: frames that are put, 16 x 16, at the given offsets, where their omega at
    (STACK_PROBE, STACK_PROBE) is above every other frame's (those are drawn again until it is): that cell's first winners are the stacked
    frames, three from each of two lanes, and each lane is handed its three in an order that is neither ascending nor descending"""
    rng = np.random.default_rng(seed)
    offs = rng.integers(0, reach + 1, (n, 2))
    sizes = rng.integers(side[0], side[1] + 1, (n, 2))
    if stack is None:
        offs[0], offs[-1], sizes[-1] = (0, 0), (reach, reach), (side[1], side[1])
    else:
        low = min(_omega_at(STACK_PROBE, (o, o), (16, 16)) for o in stack.values())
        for k in range(n):
            while _omega_at(STACK_PROBE, offs[k], sizes[k]) >= low:
                offs[k], sizes[k] = rng.integers(0, reach + 1, 2), rng.integers(side[0], side[1] + 1, 2)
        offs[2] = (0, 0)
        for k, o in stack.items():
            offs[k], sizes[k] = (o, o), (16, 16)
        assert 2 not in stack and reach in stack.values() and side[1] == 16
    return _noise_frames(sizes.tolist(), seed + 1), _translations(offs.tolist()), sc.params(level=level, depth=8)


ONE_LANE, ONE_LANE_PROBE = 5, 12                                            # wave600_one_lane: the lane, the probe pixel (x = y) of cell (1, 1) at level 3


def wave_one_lane(n=600, seed=77):
    """n 16 x 16 noise frames on a 24 x 24 canvas at level 3.  The frames at list positions = ONE_LANE (mod 64) sit at (4, 4): the probe
    (12, 12) of the middle cell is source pixel (8, 8), border distance 7, the largest a 16 x 16 frame has, and they share it, so the index
    alone orders them.  Every other frame sits where its border distance at that probe is below 7 (an offset of 4 or 5 in both axes gives 7).
    The middle cell's eight winners then all come out of lane ONE_LANE, which was handed more than eight covering frames."""
    rng = np.random.default_rng(seed)
    offs = rng.integers(0, 9, (n, 2))
    for k in range(n):
        while 4 <= offs[k, 0] <= 5 and 4 <= offs[k, 1] <= 5:
            offs[k] = rng.integers(0, 9, 2)
    offs[0], offs[n - 1] = (0, 0), (8, 8)
    for k in range(n):
        if lane_of(n, k) == ONE_LANE:
            offs[k] = (4, 4)
    assert lane_of(n, 0) != ONE_LANE and lane_of(n, n - 1) != ONE_LANE
    return _noise_frames([(16, 16)] * n, seed + 1), _translations(offs.tolist()), sc.params(level=3, depth=8)


WAVE_CASES = {
    "wave65": lambda: wave(65, seed=400),
    "wave130": lambda: wave(130, seed=410, stack=STACK),
    "wave600": lambda: wave(600, seed=420, side=(12, 12), reach=4),
    "wave600_one_lane": wave_one_lane,
}


# ---- level x remainder: the probe clamp min(x0 + s / 2, cw - 1) in the partial cells ---------------------------------------------------------
def remainder(level, rx, ry, turned=False, cells=2):
    """a canvas of `cells` whole cells and a partial one of rx x ry pixels at its right and lower edge: frame 0 is the whole canvas, frame 1
    its lower right part from a third of the way in (an odd offset).  A frame gives samples up to its last column and row but one, so under
    translations the canvas's last column and row have no sample: a probe clamped to them finds no candidate, and the partial cells stay
    empty although both frames cover part of them.  turned: the same two frames each under a half turn about its own place; then the
    canvas's first column and row are the ones without a sample, and every partial cell has a candidate at its clamped probe."""
    s = 1 << level
    assert 0 < rx < s and 0 < ry < s
    cw, ch = cells * s + rx, cells * s + ry
    ox, oy = (cw // 3) | 1, (ch // 3) | 1
    imgs = _noise_frames([(cw, ch), (cw - ox, ch - oy)], 500 + 16 * level + rx)
    h9s = _translations([(0, 0), (ox, oy)])
    if turned:
        h9s[:, 0] = h9s[:, 4] = -1                                          # (x, y) -> (cw - 1 - x, ch - 1 - y): both frames end at the canvas's corner
        h9s[:, 2], h9s[:, 5] = cw - 1, ch - 1
    return imgs, h9s, sc.params(level=level, depth=8)


def rem_pairs(level):
    """(cw mod s, ch mod s) of the four cases of a level: each axis sees 1, s / 2 (the probe of the partial cell is clamped), s / 2 + 1 and
    s - 1 (it is not); within a case one axis is clamped and the other is not"""
    s = 1 << level
    r = (1, s // 2, s // 2 + 1, s - 1)
    return [(r[0], r[2]), (r[1], r[3]), (r[2], r[0]), (r[3], r[1])]


REM_CASES = {"rem_L%d_%dx%d%s" % (level, rx, ry, "_turned" * t): (lambda level=level, rx=rx, ry=ry, t=t: remainder(level, rx, ry, turned=bool(t)))
             for level in (2, 3, 4, 5) for rx, ry in rem_pairs(level) for t in (0, 1)}

SURVEY_EDGE_CASES = dict(WAVE_CASES, **REM_CASES)

# ---- records with up to 8 filled slots --------------------------------------------------------------------------------------------------------
DEAR = dict(depth=8, data_weight=16, diff_weight=16, seam_penalty=255, miss_cost=255)
RECORD_EDGE_CASES = {
    "records8_wide": lambda: random_records(70, 5, seed=11, frames=12, slots=8, depth=8),
    "records8_tall": lambda: random_records(5, 70, seed=12, frames=12, slots=8, depth=8),
    "records8_dear": lambda: random_records(33, 9, seed=13, frames=12, holes=0.0, slots=8, **DEAR),
    "records8_holes_free": lambda: random_records(9, 7, seed=14, frames=12, holes=0.3, slots=8, depth=8, miss_cost=0),
    "records8_ties": lambda: random_records(12, 9, seed=16, frames=12, slots=8, depth=8, data_weight=0, diff_weight=0),    # the seam penalty alone: slots tie
    "records8_ids": lambda: random_records(21, 6, seed=15, frames=12, slots=8, depth=8, ids=[65535, 65534, 32768, 256, 255, 1, 2, 257, 32767, 4096, 511, 9]),
}

_REF = {}


def reference(orc, name):
    """the reference's results for a case, computed once and not to be written to: (imgs, h9s, params, seamcut_ref dict)"""
    if name not in _REF:
        imgs, h9s, p = (CASES[name] if name in CASES else SURVEY_EDGE_CASES[name])()
        _REF[name] = (imgs, h9s, p, sc.seamcut_ref(orc, imgs, h9s, p))
    return _REF[name]


EDGE_SETTINGS = ((2, 8, 0), (5, 8, 0), (3, 4, 3))                           # (level, depth, ramp) the cases of tests/render_patterns.py are run at


def edge_params(level):
    return next(sc.params(level=l, depth=d, ramp=r) for l, d, r in EDGE_SETTINGS if l == level)


def edge_reference(orc, case, level):
    """the reference's results for a case of tests/render_patterns.py at one of EDGE_SETTINGS, from the maps and weights its Restated already
    holds, computed once: (params, seamcut_ref dict)"""
    from tests import render_patterns as rp
    key = ("edge", case.tag, level)
    if key not in _REF:
        R = rp.restate(orc, case)
        p = edge_params(level)
        _REF[key] = (p, sc.seamcut_ref(orc, case.imgs, case.h9s, p, maps=R.maps, wmaps=R.weights(p["ramp"])))
    return _REF[key]


def random_cells(n, gw, gh, seed):
    """a cell map that stage 2 did not make: each cell names nobody (0) or any of the frames 1 .. n, whether or not that frame touches the
    cell, takes part in the render or exists on the canvas at all"""
    return np.random.default_rng(seed).integers(0, n + 1, (gh, gw)).astype(np.uint16)


def shallower(r, p, depth):
    """the reference's records, cell map and report of a case at a smaller depth: the candidates are a prefix"""
    assert 1 <= depth <= p["depth"]
    frame, omega, gray = (a.copy() for a in (r["frame"], r["omega"], r["gray"]))
    for a in (frame, omega, gray):
        a[..., depth:] = 0
    q = dict(p, depth=depth)
    cells, report = sc.labels(frame, omega, gray, q)
    return q, dict(frame=frame, omega=omega, gray=gray, records=sc.record_bytes(frame, omega, gray), cells=cells, report=report)


def record_reference(name):
    """(frame, omega, gray, params, cells, report, slot) of a record case, computed once"""
    if name not in _REF:
        frame, omega, gray, p = (RECORD_CASES[name] if name in RECORD_CASES else RECORD_EDGE_CASES[name])()
        cells, report, slot, _ = sc.labels(frame, omega, gray, p, full=True)
        _REF[name] = (frame, omega, gray, p, cells, report, slot)
    return _REF[name]
