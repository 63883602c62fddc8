"""The adversarial SURF inputs of tests/surf_patterns.py do what they are for -- checked on the CPU oracle alone (its counters:
oracle.h orc_surf_stats), so that a GPU pass on them (tests/test_gpu_surf_edges.py) means something and none of these conditions is ever
"checked" by the code under test.

Zero keypoints are allowed for the flat frame, for the shape-matrix sizes where no middle layer can hold a maximum
(surf_patterns.octaves_possible() empty: min(w, h) < 23) and for the frames of surf_patterns.ZERO_BY_CONTENT (min(w, h) <= 41) -- nothing else."""
import time

import numpy as np
import pytest

from tests import oracle_lib as ol
from tests import sift_patterns as sp
from tests import surf_patterns as su


@pytest.fixture(scope="module")
def orc():
    return ol.load_oracle_fast()


def _groups(kp):
    """(first position, length) of every run of bit-equal responses in the sorted list"""
    r = kp["response"].view(np.uint32)
    cut = np.flatnonzero(np.diff(r) != 0) + 1
    start = np.concatenate([[0], cut])
    return start, np.diff(np.concatenate([start, [len(r)]]))


def _tie_order_ok(kp):
    """inside a tie group the oracle orders by (octave, layer, row, column): octave never decreases"""
    start, n = _groups(kp)
    return all((np.diff(kp["octave"][s:s + c]) >= 0).all() for s, c in zip(start, n) if c > 1)


@pytest.mark.parametrize("size", [(320, 240), (333, 257)])
def test_content_matrix_ties_and_zero_list(orc, size):
    m = su.content_matrix(*size)
    res = ol.parallel_map(lambda img: orc.surf_with_stats(img, su.THR, su.KEEP_ALL), list(m.values()))
    zero = [n for n, (kp, _, _) in zip(m, res) if len(kp) == 0]
    assert zero == list(su.ZERO_KEYPOINT_PATTERNS), zero
    for n, (kp, d, st) in zip(m, res):
        assert st["maxima"] == st["kept"] == len(kp) and st["dropped"] == 0, (n, st)
        assert _tie_order_ok(kp), n
        if n in su.TIE_PATTERNS:
            assert _groups(kp)[1].max() >= 8, (n, _groups(kp)[1].max())
    assert sum(st["short_ori"] for _, _, st in res) >= 100 and sum(st["clamped"] for _, _, st in res) >= 100


def test_max_kp_cuts_inside_a_tie_group(orc):
    """tiled(640, 480, 6, 48): 3120 keypoints; positions 2564 .. 2680 of the sorted list share one response, max_kp = 2600 keeps 36 of the 117"""
    w, h, seed, P, mk = su.TIE_CUT
    img = su.tie_cut_frame()
    kp, d, st = orc.surf_with_stats(img, su.THR, su.KEEP_ALL)
    start, n = _groups(kp)
    g = int(np.searchsorted(start, mk, side="right")) - 1
    assert (int(start[g]), int(start[g] + n[g] - 1)) == su.TIE_CUT_GROUP and start[g] < mk < start[g] + n[g] - 1 and n[g] >= 8
    assert len(kp) == 3120 and n.max() >= 117
    kc, dc, stc = orc.surf_with_stats(img, su.THR, mk)
    assert len(kc) == mk and stc["maxima"] == 3120 and stc["kept"] == mk
    assert np.array_equal(kc.view(np.uint8), kp[:mk].view(np.uint8)) and np.array_equal(dc.view(np.uint32), d[:mk].view(np.uint32))
    _, cnt = np.unique(d.view(np.uint32), axis=0, return_counts=True)
    assert (cnt > 1).sum() >= 50 and cnt.max() >= 100            # repeated descriptor rows: the matcher's tie rule has something to decide


def test_limit_shapes_reach_past_8191(orc):
    res = {}
    for (w, h, c, thr, mk) in su.LIMIT_SHAPES:
        kp, d, st = orc.surf_with_stats(su.limit_frame(w, h, c), thr, mk)
        res[(w, h)] = (kp, st)
        assert st["dropped"] == 0 and st["layer_mask"] == su.layer_mask(w, h)
        if min(w, h) == 16:
            assert len(kp) == 0 and su.octaves_possible(w, h) == ()
    assert (res[(16383, 40)][0]["x"] > 8191).sum() >= 1000 and res[(16383, 40)][0]["x"].max() > 16350
    assert (res[(40, 16383)][0]["y"] > 8191).sum() >= 1000 and res[(40, 16383)][0]["y"].max() > 16350
    kp, st = res[(16383, 300)]
    assert st["maxima"] > st["kept"] == len(kp) == 20000 and set(np.unique(kp["octave"])) == {0, 1} and (kp["x"] > 8191).sum() >= 1000
    assert res[(16383, 40)][1]["short_ori"] > 1000 and res[(16383, 40)][1]["clamped"] > 1000


def test_bright_frame_wraps_the_integral_image(orc):
    img = su.bright()
    g = img[..., 0].astype(np.int64)                             # B = G = R: gray = the level
    rows = np.cumsum(g.sum(1))
    assert rows[-1] > 1.15 * 2 ** 32
    wrap = int(np.searchsorted(rows, 1 << 32))                    # first row at which the running sum has passed 2^32
    kp, d, st = orc.surf_with_stats(img, su.THR, su.KEEP_ALL)
    assert len(kp) > 3000 and st["dropped"] == 0
    assert (kp["y"] > wrap + 30).sum() >= 300 and kp["y"].max() > img.shape[0] - 32


def test_shape_matrix_masks_octaves_and_zero_list(orc):
    items = [(w, h, c, img) for (w, h) in su.SHAPES for c, img in su.shape_frames(w, h).items()]
    res = ol.parallel_map(lambda it: orc.surf_with_stats(it[3], su.THR_SHAPE, su.KEEP_ALL), items)
    zero, seen, dropped, by_possible = set(), set(), 0, {}
    for (w, h, c, _), (kp, d, st) in zip(items, res):
        assert st["layer_mask"] == su.layer_mask(w, h), (w, h, st)
        seen.add(st["layer_mask"])
        dropped += st["dropped"]
        poss = su.octaves_possible(w, h)
        if len(kp) == 0:
            if poss:
                zero.add((c, w, h))
        else:
            got = set(kp["octave"].tolist())
            assert got <= set(poss), (w, h, got, poss)
            by_possible.setdefault(len(poss), set()).update(got)
    assert zero == su.ZERO_BY_CONTENT, (zero ^ su.ZERO_BY_CONTENT)
    assert all(min(w, h) <= 41 for (_, w, h) in su.ZERO_BY_CONTENT)
    # every step from "no middle layer fits" to all sixteen filters
    for want in [(3, 0, 0, 0), (7, 1, 0, 0), (15, 1, 0, 0), (15, 3, 0, 0), (15, 7, 1, 0), (15, 15, 1, 0), (15, 15, 7, 1), (15, 15, 15, 1),
                 (15, 15, 15, 7), (15, 15, 15, 15)]:
        assert want in seen, (want, sorted(seen))
    # ... and keypoints really come from octave k - 1 where k octaves are possible
    assert sorted(by_possible) == [1, 2, 3, 4] and all(max(by_possible[k]) == k - 1 for k in by_possible), by_possible
    assert dropped == 0


def test_orientation_drop_is_unreachable(orc):
    """the oracle drops a keypoint only when none of its 113 orientation samples lies inside the frame.  The centre sample (0, 0) of the disc
    is at rint(k - (gws - 1) / 2) with gws = 2 rint(2 s) <= 0.54 size: it needs k >= gws / 2 - 1 and k < n - gws / 2, and a maximum sits at
    least (size_above / 2 + step) >= size / 2 from every edge, its interpolated position at most one step from the sample -- so the centre
    sample is always inside.  Searched here: the small and thin shapes, the limit shapes and the largest-scale content (octave 3 at the
    smallest sizes that hold it, blobs at the filter scale)"""
    frames = [(su.limit_frame(w, h, c), thr, mk) for (w, h, c, thr, mk) in su.LIMIT_SHAPES if w * h < 2000000]
    for n in (184, 185, 200, 216, 232, 233, 240):
        for (w, h) in ((n, n), (n, 1000), (1000, n)):
            frames.append((sp.discs(w, h, radii=(30, 45, 60), pitch=n // 2 + 40), 0.0, su.KEEP_ALL))
            frames.append((sp.binary_noise(w, h, n), 0.0, su.KEEP_ALL))
    res = ol.parallel_map(lambda f: orc.surf_with_stats(*f), frames)
    assert sum(st["dropped"] for _, _, st in res) == 0
    assert sum(int((kp["octave"] == 3).sum()) for kp, _, _ in res) >= 20
    assert sum(st["short_ori"] for _, _, st in res) >= 1000


def test_lattice_passes_the_candidate_limit(orc):
    """2.23e6 accepted maxima > 2^21 on a 36 MP frame that needs 1.8 GB of device memory: the refusal case of the GPU test.  max_kp = 1: the
    count is taken before the cut, nothing is described"""
    t = time.time()
    kp, d, st = orc.surf_with_stats(su.lattice(), 0.0, 1)
    print("\nlattice %dx%d: %d maxima, %.1f s" % (su.LATTICE[0], su.LATTICE[1], st["maxima"], time.time() - t))
    assert st["maxima"] > 1.04 * (1 << 21) and st["kept"] == 1
    w, h, _ = su.LATTICE
    assert 50.5 * w * h < 2.0e9


def test_pair_inputs(orc):
    fi, fj = su.dup_pair()
    (k1, d1), (k2, d2) = F = [orc.surf(fi, su.THR, su.KEEP_ALL), orc.surf(fj, su.THR, su.KEEP_ALL)]
    _, inv, cnt = np.unique(d2.view(np.uint32), axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    assert cnt.max() >= len(su.DUP_AT_J)                         # bit-equal train rows
    idx, dist = orc.bf_match_f32(d1, d2)
    tied = np.flatnonzero(cnt[inv[idx]] > 1)                      # queries whose nearest train row has bit-equal twins: the minimum is attained by all of them
    assert len(tied) >= 2
    for q in tied:
        assert idx[q] == np.flatnonzero(inv == inv[idx[q]])[0]   # the first of them wins
    xy1, xy2 = np.stack([k1["x"], k1["y"]], 1), np.stack([k2["x"], k2["y"]], 1)
    s1, _ = orc.select_by_distance(idx, dist, xy1, xy2, 0.5, 200)
    assert len(s1) > 50 and np.isin(tied, s1["id"]).sum() >= 2   # ... in a pair that selects matches, the tied queries among them
    for seed in (1, 4):
        nin, i1, _, _, _ = orc.surf_match_pair(F[0], F[1], 2.5, seed)
        assert nin > 18 and np.isin(tied, i1["id"][:nin]).sum() >= 1      # a tied query is an inlier: which twin the matcher takes decides the record
    assert (dist == 0).sum() == 2 and (dist < 0.05).sum() > 2
    for (md, mf) in su.WALK_TO_EPS:                              # the walk stops at distT = 7.45e-10: exactly the zero distances are below it
        s = orc.select_by_distance(idx, dist, xy1, xy2, md, mf)[0]
        assert len(s) == 2 and (dist[s["id"]] == 0).all()
    assert np.float32(np.float64(np.float32(0.05)) - 0.05) > 0 and np.float32(0.05) - np.float32(0.05) == 0
    for (md, mf) in su.FEW_SELECTED:
        assert 1 <= len(orc.select_by_distance(idx, dist, xy1, xy2, md, mf)[0]) <= 3
    # the walk all the way down: every distance of a self pair is 0, the count stays above max_features until distT <= 0
    nin, _, _, _, ns = orc.surf_match_pair(F[0], F[0], 2.5, 1)
    assert (nin, ns) == (0, 0) and len(k1) > 200
    i0, dd = orc.bf_match_f32(d1, d1)
    assert (dd == 0).all()
    seed, P, dx, dy = su.TILED_PAIR
    T = [orc.surf(sp.tiled(320, 240, seed, P)), orc.surf(sp.tiled_shifted(320, 240, seed, P, dx, dy))]
    assert orc.surf_match_pair(T[0], T[1], 2.5, 1)[4] == 0 and len(T[0][0]) > 200
    # exact feature counts for the matcher's ragged sizes, and pairs that select something at each
    a, b = su.count_frames()
    for n in su.FEATURE_COUNTS:
        A, B = orc.surf(a, su.THR, n), orc.surf(b, su.THR, n)
        assert len(A[0]) == len(B[0]) == n
        if n > 1:
            assert orc.surf_match_pair(A, B, 2.5, 1)[4] > 10


def test_ring_inputs(orc):
    R = su.ring_frames()
    n = [len(kp) for kp, _ in ol.parallel_map(lambda it: orc.surf(*it), R)]
    assert len(R) == su.RING_N and n.count(0) == 2 and n.count(1) >= 2 and max(n) >= 100 and {63, 64, 65} <= set(n), n
