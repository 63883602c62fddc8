"""The cases of the optimised seamlines (tests/seamcut_ref.py): small surveys under integer translations (every clean sample is the scene's
byte), each built to hold one thing the label stage can get wrong.  A case is (imgs, h9s, params dict); tests/test_seamcut_ref.py asserts on
the reference that each case holds what its name says, tests/test_gpu_seamcut.py that the build gives the reference's bytes on every one.
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



def random_records(gw, gh, seed, frames=5, holes=0.15, **kw):
    """cell records that come from no survey: per cell 0 .. 4 distinct frames out of `frames`, weights descending, any gray.  The label stage
    takes records as they are, and only here can one frame stand on both sides of an empty cell (frames on a canvas are convex)."""
    rng = np.random.default_rng(seed)
    frame = np.zeros((gh, gw, sc.SLOTS), np.uint16); omega = np.zeros((gh, gw, sc.SLOTS), np.uint8); gray = np.zeros((gh, gw, sc.SLOTS), np.uint8)
    for y in range(gh):
        for x in range(gw):
            m = 0 if rng.random() < holes else int(rng.integers(1, 5))
            frame[y, x, :m] = rng.permutation(frames)[:m] + 1
            omega[y, x, :m] = np.sort(rng.integers(1, 256, m))[::-1]
            gray[y, x, :m] = rng.integers(0, 256, m)
    return frame, omega, gray, sc.params(**kw)


RECORD_CASES = {
    "records_holes": lambda: random_records(9, 7, seed=0),
    "records_dear": lambda: random_records(300, 1, seed=0, frames=40, holes=0.0, data_weight=16, diff_weight=16, seam_penalty=255, miss_cost=255),
    "records_dear_v": lambda: tuple(a.swapaxes(0, 1) if isinstance(a, np.ndarray) else a for a in RECORD_CASES["records_dear"]()),
}

_REF = {}


def reference(orc, name):
    """the reference's results for a case, computed once and not to be written to: (imgs, h9s, params, seamcut_ref dict)"""
    if name not in _REF:
        imgs, h9s, p = CASES[name]()
        _REF[name] = (imgs, h9s, p, sc.seamcut_ref(orc, imgs, h9s, p))
    return _REF[name]


def record_reference(name):
    """(frame, omega, gray, params, cells, report, slot) of a record case, computed once"""
    if name not in _REF:
        frame, omega, gray, p = RECORD_CASES[name]()
        cells, report, slot, _ = sc.labels(frame, omega, gray, p, full=True)
        _REF[name] = (frame, omega, gray, p, cells, report, slot)
    return _REF[name]
