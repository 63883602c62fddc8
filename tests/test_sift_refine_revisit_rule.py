"""refine_kernel drops a candidate as soon as a move lands on a location it was fitted at before.  The rule behind it: one Newton step is a
function of its location alone, so "revisit => the unshortened loop also ends in a drop".  Checked without a GPU on every move table over
five locations (each location converges and is accepted, converges and is rejected, diverges, leaves the level, or moves to one of the
five, itself included): the shortened loop -- with the kernel's three comparisons, and with all four earlier locations -- ends as the
unshortened one does and never fits more often.  The tables hold cycles of length 1 to 4 and tails that lead into a cycle.

The second test ties tests/sift_moves_ref.py, the numpy restatement the GPU test takes its expectations from, to the oracle."""
import itertools

import numpy as np

from tests import sift_moves_ref as mr

MAX_INTERP = mr.MAX_INTERP
LOCS = [(1, 100, 200), (2, 100, 200), (1, 101, 200), (1, 100, 201), (3, 16383, 16383)]        # differ in one axis each; the last one fills the packing
ACCEPT, REJECT, DIVERGE, LEAVE = "accept", "reject", "diverge", "leave"


def _pack(loc):
    return (loc[0] << 28) | (loc[1] << 14) | loc[2]          # as refine_kernel packs `start`


def _loop(table, rule):
    """the kernel's loop from location 0.  rule None: unshortened; 3: the comparisons the kernel makes; 4: all earlier locations.
    Returns (result, fits): result is the index of the location a record is stored for, or None for no record."""
    at, hist = 0, []
    for it in range(MAX_INTERP):
        what = table[at]
        if what == ACCEPT:
            return at, it + 1
        if what in (REJECT, DIVERGE, LEAVE):
            return None, it + 1
        new = what
        if rule and it + 1 < MAX_INTERP:
            earlier = hist + [at]
            if rule == 3:
                earlier = [earlier[0]] + earlier[-2:]
            if _pack(LOCS[new]) in [_pack(LOCS[j]) for j in earlier]:
                return None, it + 1
        hist.append(at)
        at = new
    return None, MAX_INTERP


def test_revisit_means_drop_on_every_move_table():
    n = len(LOCS)
    assert len({_pack(l) for l in LOCS}) == n and max(_pack(l) for l in LOCS) < 0xffffffff
    cycles, tails, saved, missed = set(), 0, 0, 0
    for table in itertools.product([ACCEPT, REJECT, DIVERGE, LEAVE] + list(range(n)), repeat=n):
        want, fits = _loop(table, None)
        got3, fits3 = _loop(table, 3)
        got4, fits4 = _loop(table, 4)
        assert got3 == want and got4 == want, table
        assert fits4 <= fits3 <= fits, table
        saved += fits - fits3
        missed += fits3 - fits4
        # what this table is, from the walk itself
        walk, at = [], 0
        while isinstance(table[at], int) and at not in walk:
            walk.append(at)
            at = table[at]
        if at in walk:
            assert want is None, table                                       # a cycle never stores a record
            cycles.add(len(walk) - walk.index(at))
            tails += walk.index(at) > 0
            if len(walk) < MAX_INTERP:
                assert fits4 == len(walk), table                             # dropped at the first revisit: one fit per distinct location
                assert fits3 == fits4 or (walk.index(at) == 1 and len(walk) == 4), table      # only a 3-cycle after one step escapes the three comparisons
    assert cycles == {1, 2, 3, 4, 5} and tails > 0 and saved > 0 and missed > 0


def test_restatement_accepts_the_oracles_locations(oracle):
    """the numpy restatement's accepted locations are the oracle's keep-all keypoint locations, on the smallest frame of the GPU test and
    on its odd-width one; summary() itself asserts that no candidate that came back to a location of its own ended otherwise than dropped"""
    for w, h in ((128, 96), (250, 187)):
        img = mr.half_pixel_blobs(w, h)
        s = mr.summary(img)
        kp, _ = oracle.sift(img, 0, 32768)
        o, layer = kp["octave"] & 255, (kp["octave"] >> 8) & 255
        x, y = kp["x"] / 2.0 ** o, kp["y"] / 2.0 ** o
        assert len(s["records"]) >= 40
        assert len(np.unique(np.stack([o, layer, kp["x"].view(np.int32), kp["y"].view(np.int32)], 1), axis=0)) == len(s["records"])
        near = set()
        for a, b, u, v in zip(o, layer, x, y):                               # an offset of almost half a pixel rounds either way
            near |= {(int(a), int(b), int(r), int(c)) for r in (np.floor(v + 0.5), np.ceil(v - 0.5)) for c in (np.floor(u + 0.5), np.ceil(u - 0.5))}
        assert s["records"] <= near
        assert s["early_exits"] > 0 and s["ran_out"] >= s["early_exits_full"] >= s["early_exits"]
