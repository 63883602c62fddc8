"""Named, seeded correspondence sets for Ransac2D, each chosen for what the sequential loop (mosaicimage.h:1785-1918) DOES on it -- where
it stops, which slot wins, how many draws it spends -- as recorded by the oracle's trace (oracle.h orc_ransac2d_trace).  ransac.hip does not
run that loop: it classifies draws in chunks of 256, evaluates the accepted ones in groups of 64 handed to waves at run time, and replays the
loop's bookkeeping afterwards over stored supports in blocks of 256.  The patterns put the loop's events on those seams.

tests/test_ransac_patterns_oracle.py (CPU) asserts each pattern's property on the trace; tests/test_gpu_ransac_edges.py compares the HIP
path with the oracle on all of them.  Test infrastructure only.

Traced values that qualify each pattern (dist 2.5 unless said; "slots" = hypothesis slots filled, the stopper's included; "draws" = draws
consumed; both for the loop as the reference runs it, i.e. ending at the stop):

  name                   n     sample_times  seed  stop slot  stopper's support  slots  draws  remark
  late_stop_wave_1       396   1000          16    91         393                92     145    wave 1 of block 0
  late_stop_wave_3       396   1000          18    195        393                196    323    wave 3 of block 0
  late_stop_block_1      396   1000          17    501        393                502    759    block 1 (list index 256..511)
  late_stop_block_2      396   1000          2     598        393                599    894    block 2
  late_stop_block_3      396   1000          15    783        393                784    1217   block 3
  stop_then_larger       396   4999          3     1          393                2      3      behind the stop (loop run on): 3318 slots, 942 larger
                                                                                               supports, 16 of the 51 entries of column 1 mod 64 (31 %);
                                                                                               list in HBM: ransac_listg_kernel at every ransac_split
  stop_then_larger_lds_4920, _4000   the same points and seed at sample_times 4920 and 4000: the same trace (the list ends at 3318 slots),
                                                                                               list in LDS: ransac_kernel at split 0, else the split form
  float_threshold_500    500   1000          11    3          495 (= 0.99 n)     4      4      96 larger supports behind the stop (1000 slots)
  float_threshold_1000   1000  1000          27    44         990 (= 0.99 n)     45     76     41 larger supports behind the stop
  float_threshold_8000   8000  1000          843   13         7920 (= 0.99 n)    14     29     20 larger supports behind the stop (found in a
                                                                                               search of seeds 1..1499 at noise 0.65: 13 s of CPU)
  fallback_1000          396   1000          2     -          -                  1000   2090   976 slots in the first 2048 draws (8 chunks classified)
  fallback_2400          396   2400          2     -          -                  2400   4911   2380 slots in the first 4864 draws (19 of 20 chunks)
  never_fills            396   3000          2     -          -                  2445   4999   the same points: the list ends short of sample_times
  never_fills_4999       396   4999          2     -          -                  2445   4999
  no_slot                60    1000          9     -          -                  0      4999   every source point on one line: no draw takes a slot
  sizes_<n>              n in 5, 8, 63, 64, 65, 255, 256, 257, 397, 398, 399, 400; half outliers; none stops, all fill 1000 slots
  inliers_<k>            final inlier count k in 3, 4, 30, 31, 256, 257 and 400 of 400 (the oracle's count, asserted by the CPU test)
  dist_<d>               123 points at dist 0, 1e-3, 2.5, 1e4 and -2.5 (0: no support is ever positive; 1e4: slot 0 stops with support n;
                         the other three claim nothing)
  nan_coordinate, inf_coordinate   57 points, one coordinate not finite: the oracle decides

(tests/test_ransac_patterns_oracle.py::test_every_pattern_shows_its_property prints these figures from the trace before it asserts.)
"""
import functools
from collections import namedtuple

import numpy as np

from tests.oracle_lib import SFPOINT
from tests.synth import synth_pairs

SIZE = (4000, 3000)
MAX_DRAWS = 4999          # realSamTimes >= 5000 breaks before drawing (mosaicimage.h:1787-1792)

# check(trace, result): raises AssertionError unless the trace -- taken with keep_going, at the pattern's own sample_times -- shows the
# property the pattern is there for; result = (ok, in1, in2, H) of the loop that stops
Pattern = namedtuple("Pattern", "name p1 p2 dist sample_times seed check")


def _degenerate_case(rng, kind, m):
    w, h = 4000.0, 3000.0
    p1 = np.zeros(m, SFPOINT); p2 = np.zeros(m, SFPOINT)
    p2["x"] = rng.uniform(0, w, m); p2["y"] = rng.uniform(0, h, m)
    A = np.array([[1 + rng.normal(0, .02), rng.normal(0, .02), rng.uniform(-800, 800)], [rng.normal(0, .02), 1 + rng.normal(0, .02), rng.uniform(-600, 600)], [0, 0, 1]])
    q = A @ np.stack([p2["x"], p2["y"], np.ones(m)])
    p1["x"] = q[0] + rng.normal(0, 0.4, m); p1["y"] = q[1] + rng.normal(0, 0.4, m)
    out = rng.random(m) < 0.5
    p1["x"][out] = rng.uniform(0, w, out.sum()); p1["y"][out] = rng.uniform(0, h, out.sum())
    if kind == 0:      # one source point matched by several targets: singular 4-point systems, failed inversions
        k = rng.integers(0, m, m // 2); p2["x"][: m // 2] = p2["x"][k]; p2["y"][: m // 2] = p2["y"][k]
    elif kind == 1:    # duplicated pairs
        k = rng.integers(0, m, m // 3); p2[: m // 3] = p2[k]; p1[: m // 3] = p1[k]
    elif kind == 2:    # integer lattice: collinear quadruples, exact zeros in the eliminations (pivot search below the diagonal)
        p2["x"] = np.round(p2["x"] / 50) * 50; p2["y"] = np.round(p2["y"] / 50) * 50; p1["x"] = np.round(p1["x"]); p1["y"] = np.round(p1["y"])
    elif kind == 3:    # every source point on one line
        p2["y"] = 0.5 * p2["x"] + 10
    elif kind == 4:    # coordinates whose products overflow binary32: non-finite design matrices (the generic routines)
        p1["x"] *= 1e18; p1["y"] *= 1e18; p2["x"] *= 1e18; p2["y"] *= 1e18
    return p1, p2


def float_stops(support, n):
    """the loop's stop test as the reference writes it (mosaicimage.h:1763, 1908): float product with the float reciprocal of n"""
    invn = np.float32(1.0) / np.float32(n)
    return bool(np.float32(support) * invn > np.float32(0.99))


def exact_stops(support, n):
    """support / n > 0.99 in exact arithmetic"""
    return 100 * int(support) > 99 * int(n)


def classified_draws(sample_times):
    """draws the split form's classify pass covers (mi_ransac_batch: twice the slot limit, rounded up to whole chunks of 256 draws)"""
    cap = min(max(sample_times, 1), MAX_DRAWS)
    return min((2 * cap + 255) // 256 * 256, 20 * 256)


# ---- the properties ---------------------------------------------------------------------------------------------------------------------
def _stops_in(lo, hi):
    def check(t, r):
        assert lo <= t["stop_slot"] < hi, (t["stop_slot"], lo, hi)
        assert t["win_slot"] == t["stop_slot"]
    return check


def _stop_then_larger(t, r):
    s, sup = t["stop_slot"], t["supports"]
    assert s >= 0 and t["win_slot"] == s
    col = sup[s + 64::64]                                 # the list entries one lane of a wave can meet after the stopper
    assert len(col) >= 8 and 4 * int((col > sup[s]).sum()) >= len(col), (s, int(sup[s]), len(col), int((col > sup[s]).sum()))


def _stopper_below(n):
    def check(t, r):
        _stop_then_larger(t, r)
        assert t["supports"][t["stop_slot"]] < n
    return check


def _float_threshold(n):
    def check(t, r):
        s, sup = t["stop_slot"], t["supports"]
        assert s >= 0 and 100 * int(sup[s]) == 99 * n, (s, sup[s] if s >= 0 else None)
        assert float_stops(sup[s], n) and not exact_stops(sup[s], n)
        assert (sup[s + 1:] > sup[s]).any()               # a loop that did not stop here would return another winner
    return check


def _fallback(st):
    def check(t, r):
        c = classified_draws(st)
        assert t["stop_slot"] < 0
        assert t["n_slots"] == st and t["draws"] > c, (t["n_slots"], t["draws"], c)   # the list fills, but only behind the classified draws
        assert int(t["took"][:c].sum()) < st
    return check


def _never_fills(st):
    def check(t, r):
        assert t["stop_slot"] < 0 and t["draws"] == MAX_DRAWS and 0 < t["n_slots"] < min(st, MAX_DRAWS), (t["draws"], t["n_slots"])
    return check


def _no_slot(t, r):
    assert t["draws"] == MAX_DRAWS and t["n_slots"] == 0 and not t["took"].any() and t["win_slot"] < 0
    assert r[0] == 0 and len(r[1]) == 0


def _fills_without_stop(st):
    def check(t, r):
        assert t["stop_slot"] < 0 and t["n_slots"] == st, (t["stop_slot"], t["n_slots"])
    return check


def _no_support(t, r):
    assert t["n_slots"] >= 1 and not t["supports"].any() and t["stop_slot"] < 0 and t["win_slot"] < 0 and t["win_support"] == 0
    assert r[0] == 0 and len(r[1]) == 0


def _first_slot_stops(n):
    def check(t, r):
        assert t["stop_slot"] == 0 and t["win_slot"] == 0 and int(t["supports"][0]) == n
        assert r[0] == 1 and len(r[1]) == n
    return check


def _inlier_count(k):
    def check(t, r):
        assert len(r[1]) == k == len(r[2]), (len(r[1]), k)
        assert r[0] == (1 if k >= 4 else 0)
    return check


def _oracle_decides(t, r):
    """no property of the loop is claimed: the input is there for its content, and the oracle's result is the expectation"""


# ---- the generators ---------------------------------------------------------------------------------------------------------------------
def _synth(name, n, out_frac, seed, noise, st, check, dist=2.5):
    p1, p2 = synth_pairs(n, out_frac, seed=seed, size=SIZE, noise=noise)
    return Pattern(name, p1, p2, dist, st, seed, check)


def _exact_plus_far(n, k, seed):
    """k exact correspondences (noise 0: only the rounding to binary32 is left) among n, the other n - k targets moved 500..2500 px away;
    the outliers lie scattered through the list, so that the inlier compaction has gaps in every wave"""
    p1, p2 = synth_pairs(n, 0.0, seed=seed, size=SIZE, noise=0.0)
    rng = np.random.default_rng(1000 + seed)
    out = rng.permutation(n)[: n - k]
    ang = rng.uniform(0, 2 * np.pi, n - k); r = rng.uniform(500, 2500, n - k)
    p1["x"][out] += (r * np.cos(ang)).astype(np.float32); p1["y"][out] += (r * np.sin(ang)).astype(np.float32)
    return p1, p2


@functools.lru_cache(maxsize=None)
def patterns():
    """every pattern, in a fixed order"""
    P = []
    P.append(_synth("late_stop_wave_1", 396, 3 / 396, 16, 0.6, 1000, _stops_in(64, 128)))
    P.append(_synth("late_stop_wave_3", 396, 3 / 396, 18, 0.6, 1000, _stops_in(192, 256)))
    P.append(_synth("late_stop_block_1", 396, 3 / 396, 17, 0.6, 1000, _stops_in(256, 512)))
    P.append(_synth("late_stop_block_2", 396, 3 / 396, 2, 0.6, 1000, _stops_in(512, 768)))
    P.append(_synth("late_stop_block_3", 396, 0, 15, 0.7, 1000, _stops_in(768, 1000)))
    # the same points and seed three times: at 4999 slots list + body pass 80 KB of LDS, so every ransac_split value runs the one-workgroup
    # ransac_listg_kernel (mi_ransac_batch); at 4920 (the last value with the list in LDS for 396 points) and at 4000 the split form applies
    # and the winner's record is looked up in ransac_split_finish.  The list ends at 3318 slots in all three, so the trace is the same
    P.append(_synth("stop_then_larger", 396, 0, 3, 0.3, 4999, _stopper_below(396)))
    P.append(_synth("stop_then_larger_lds_4920", 396, 0, 3, 0.3, 4920, _stopper_below(396)))
    P.append(_synth("stop_then_larger_lds_4000", 396, 0, 3, 0.3, 4000, _stopper_below(396)))
    P.append(_synth("float_threshold_500", 500, 0, 11, 0.5, 1000, _float_threshold(500)))
    P.append(_synth("float_threshold_1000", 1000, 0, 27, 0.6, 1000, _float_threshold(1000)))
    P.append(_synth("float_threshold_8000", 8000, 0, 843, 0.65, 1000, _float_threshold(8000)))
    P.append(_synth("fallback_1000", 396, 0.8, 2, 0.3, 1000, _fallback(1000)))
    P.append(_synth("fallback_2400", 396, 0.8, 2, 0.3, 2400, _fallback(2400)))
    P.append(_synth("never_fills", 396, 0.8, 2, 0.3, 3000, _never_fills(3000)))
    P.append(_synth("never_fills_4999", 396, 0.8, 2, 0.3, 4999, _never_fills(4999)))
    p1, p2 = _degenerate_case(np.random.default_rng(9), 3, 60)
    P.append(Pattern("no_slot", p1, p2, 2.5, 1000, 9, _no_slot))
    for n in (5, 8, 63, 64, 65, 255, 256, 257, 397, 398, 399, 400):
        P.append(_synth("sizes_%d" % n, n, 0.5, 100 + n, 0.3, 1000, _fills_without_stop(1000)))
    # 3 inliers cannot be built from exact ones (a hypothesis fits its own four points): five exact pairs at a distance bound below the
    # rounding error of the 4-point solve, where the oracle counts three
    p1, p2 = synth_pairs(5, 0.0, seed=18, size=SIZE, noise=0.0)
    P.append(Pattern("inliers_3", p1, p2, 3e-4, 1000, 18, _inlier_count(3)))
    for n, k, seed in ((9, 4, 41), (60, 30, 42), (60, 31, 43), (400, 256, 44), (400, 257, 45), (400, 400, 46)):
        p1, p2 = _exact_plus_far(n, k, seed)
        P.append(Pattern("inliers_%d" % k, p1, p2, 2.5, 1000, seed, _inlier_count(k)))
    p1, p2 = synth_pairs(123, 0.4, seed=77, size=SIZE, noise=0.3)
    for d in (0.0, 1e-3, 2.5, 1e4, -2.5):
        P.append(Pattern("dist_%g" % d, p1, p2, d, 1000, 77, {0.0: _no_support, 1e4: _first_slot_stops(123)}.get(d, _oracle_decides)))
    p1, p2 = synth_pairs(57, 0.3, seed=78, size=SIZE, noise=0.3)
    p1 = p1.copy(); p1["x"][10] = np.nan
    P.append(Pattern("nan_coordinate", p1, p2, 2.5, 1000, 78, _oracle_decides))
    p1, p2 = synth_pairs(57, 0.3, seed=79, size=SIZE, noise=0.3)
    p2 = p2.copy(); p2["y"][20] = np.inf
    P.append(Pattern("inf_coordinate", p1, p2, 2.5, 1000, 79, _oracle_decides))
    names = [p.name for p in P]
    assert len(set(names)) == len(names)
    return tuple(P)


def by_name(name):
    return next(p for p in patterns() if p.name == name)
