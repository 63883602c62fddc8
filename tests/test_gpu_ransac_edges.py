"""GPU: the bookkeeping around RANSAC's arithmetic (csrc/ransac.hip) -- the 0.99 stop, the replay of the sequential loop over stored supports,
the draw tables and the batched launch -- on the patterns of tests/ransac_patterns.py (tests/test_ransac_patterns_oracle.py shows on the CPU
that each pattern puts the loop's events where its name says).  Every comparison is of bits or bytes against the oracle; there is no tolerance.

  * every pattern through Ransac2D in the one-workgroup and the split forms;
  * sample_times at the wave, block and clamp edges and on either side of the draw list's move from LDS to HBM;
  * mi_ransac_batch (through mi355_debug_ransac_batch) pair by pair against the oracle, with and without min_keep, device-built against
    host-built tables, at the pair counts where the default split width changes;
  * the device-built draw tables of every n (mi355_debug_draw_tables) against a numpy restatement on the oracle's rand() stream;
  * the four seed slots of the table cache driven through eviction, rebuild and return without a synchronise.
"""
import ctypes as C

import numpy as np
import pytest

from tests.golden_util import bits
from tests import ransac_patterns as rp
from tests.oracle_lib import SFPOINT

pytestmark = pytest.mark.gpu

MAX_N = 400            # MI355_MAX_SELECTED: the batched kernels' point limit and the records' list length


@pytest.fixture(scope="module")
def ctx():
    import imagemosaicing_amd as im
    c = im.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected(oracle):
    """the oracle's result on every pattern, computed once"""
    return {p.name: oracle.ransac2d(p.p1, p.p2, p.dist, p.sample_times, p.seed) for p in rp.patterns()}


def _assert_same(a, b, what):
    """ok, both inlier lists and the bits of H, always: with fewer than 4 inliers the oracle leaves H zero, and so must the HIP path"""
    assert a[0] == b[0] and len(a[1]) == len(b[1]), (what, a[0], b[0], len(a[1]), len(b[1]))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), what
    assert np.array_equal(bits(a[3]), bits(b[3])), (what, a[3], b[3])


# ---------------------------------------------------------------------------------------------- patterns through Ransac2D
@pytest.mark.parametrize("split", [0, 1, 3, 8, -1])
def test_patterns_through_ransac2d(ctx, expected, split):
    """Every pattern with at most 400 points in the one-workgroup form (0), as 1, 3 and 8 workgroups per pair and at the default width.
    Which kernel a case runs in follows mi_ransac_batch: where list + body pass 80 KB of LDS (396 points from sample_times 4921 on: the
    patterns stop_then_larger and never_fills_4999, both at 4999) EVERY ransac_split value runs the one-workgroup ransac_listg_kernel; all
    other patterns run ransac_kernel at 0 and classify / evaluate / finish at 1, 3, 8 and -1 (4 workgroups for a single pair).
    The three stop_then_larger patterns are there for recompute_hypothesis.  The stopper (slot 1, support 393) is evaluated by lane 1 of the
    wave that takes group 0; when that lane meets a larger support in a later group of its wave, its kept hypothesis is no longer the
    winner's and the winner is formed again: in ransac_body (stop_then_larger: 4 waves share 52 groups) and, for the two _lds cases in the
    split forms, in ransac_split_finish, whose lookup then finds no record for the winner (4, 12, 32 and 16 waves share the 52 groups).
    Which wave takes which group is decided at run time, and 31 % of the stopper's column is larger: with 13 groups per wave the path is
    taken almost surely, with 32 waves (1 or 2 groups each) in roughly a third to a half of the runs -- with high probability over the four
    split widths, not with certainty.  The expected result is the same either way."""
    try:
        ctx.set_option("ransac_split", split)
        for p in rp.patterns():
            if len(p.p1) > MAX_N:
                continue
            got = ctx.Ransac2D(p.p1, p.p2, p.dist, p.sample_times, p.seed)
            _assert_same(expected[p.name], got, (p.name, split))
    finally:
        ctx.set_option("ransac_split", -1)


def test_patterns_beyond_400_points(ctx, expected):
    """the float_threshold patterns: ransac_big_kernel (n = 500, 1000) and ransac_huge_kernel (n = 8000) stop at a support of exactly 0.99 n,
    where the exact ratio would not; a larger support follows, so a loop that went on returns another winner"""
    big = [p for p in rp.patterns() if len(p.p1) > MAX_N]
    assert sorted(len(p.p1) for p in big) == [500, 1000, 8000]
    for p in big:
        got = ctx.Ransac2D(p.p1, p.p2, p.dist, p.sample_times, p.seed)
        _assert_same(expected[p.name], got, p.name)


# ---------------------------------------------------------------------------------------------- sample_times
def _list_in_hbm(nmax, sample_times):
    """mi_ransac_batch's arithmetic: the draw list (2 uint16 per slot, slots rounded up to 8) leaves LDS when list + body + 2 KB of static
    LDS pass 80 KB; body = 38 nmax floats (or points + the lanes' 9 x 256 hypotheses, if that is more)"""
    list_floats = (min(max(sample_times, 1), rp.MAX_DRAWS) + 7) // 8 * 8
    body = max(38 * nmax, 8 * nmax + 9 * 256)
    return (body + list_floats) * 4 + 2048 > 80 * 1024


@pytest.mark.parametrize("split", [0, 4])
def test_sample_times_edges(ctx, oracle, split):
    from tests.synth import synth_pairs
    # derived from the code (see _list_in_hbm): with 400 points the list is in LDS up to sample_times 4768 and in HBM from 4769 on; with
    # 396 points the step is at 4920 / 4921
    first_hbm = {n: next(st for st in range(1, 5001) if _list_in_hbm(n, st)) for n in (396, 400)}
    assert first_hbm == {396: 4921, 400: 4769}
    try:
        ctx.set_option("ransac_split", split)
        for n, seed in ((396, 61), (400, 62)):
            p1, p2 = synth_pairs(n, 0.5, seed=seed, size=rp.SIZE)
            for st in (0, -1, 1, 63, 64, 65, 255, 256, 257, 4998, 4999, 5000, 5001, 100000, first_hbm[n] - 1, first_hbm[n]):
                want = oracle.ransac2d(p1, p2, 2.5, st, seed)
                got = ctx.Ransac2D(p1, p2, 2.5, st, seed)
                _assert_same(want, got, (n, st, split))
                if st < 1:
                    assert got[0] == 0 and len(got[1]) == 0 and not got[3].any()
    finally:
        ctx.set_option("ransac_split", -1)


# ---------------------------------------------------------------------------------------------- the batched launch
def _ransac_batch(ctx, sets, dist, sample_times, seed, min_keep, host_tables):
    """mi355_debug_ransac_batch on a list of (p1, p2): PAIR_RESULT records"""
    import imagemosaicing_amd as im
    k = len(sets)
    P1 = np.zeros((k, MAX_N), SFPOINT); P2 = np.zeros((k, MAX_N), SFPOINT)
    n = np.zeros(k, np.int32)
    for i, (a, b) in enumerate(sets):
        n[i] = len(a); P1[i, :len(a)] = a; P2[i, :len(b)] = b
    out = np.zeros(k, im.PAIR_RESULT)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ctx.L.mi355_debug_ransac_batch(ctx._h, p(P1), p(P2), p(n), k, C.c_float(dist), int(sample_times), C.c_uint32(seed), int(min_keep), int(bool(host_tables)), p(out))
    assert rc == 0, rc
    return out


def _batch_sets():
    """the point sets of every pattern with at most 400 points, and pairs of 0, 3, 4 and 400 points, ordered so that neighbours differ in n.
    A batch has ONE dist, sample_times and seed, so only the POINTS of the patterns are reused here, not the events they are named for (at
    seed 7 and 1000 slots late_stop_wave_1 stops at slot 540, the stop_then_larger points stop with support 396, and the five dist_* sets and
    the three stop_then_larger sets are equal inputs): the batch is about many pairs of differing n in one launch, record by record"""
    from tests.synth import synth_pairs
    sets = [(p.p1, p.p2) for p in rp.patterns() if len(p.p1) <= MAX_N]
    for n in (0, 3, 4, 400):
        a, b = synth_pairs(max(n, 1), 0.25, seed=300 + n, size=rp.SIZE)
        sets.append((a[:n], b[:n]))
    order, rest = [], list(sets)
    while rest:
        last = len(order[-1][0]) if order else -1
        count = lambda s: sum(len(r[0]) == len(s[0]) for r in rest)
        cand = [s for s in rest if len(s[0]) != last]
        assert cand, "no order with differing neighbours"
        pick = max(cand, key=count)                       # the most frequent n first, or it is left over at the end
        order.append(pick)
        rest.pop(next(i for i, r in enumerate(rest) if r is pick))
    assert all(len(a[0]) != len(b[0]) for a, b in zip(order, order[1:]))
    return order


BATCH_DIST, BATCH_ST, BATCH_SEED = 2.5, 1000, 7


@pytest.fixture(scope="module")
def batch(ctx, oracle):
    sets = _batch_sets()
    want = [oracle.ransac2d(a, b, BATCH_DIST, BATCH_ST, BATCH_SEED) for a, b in sets]
    base = _ransac_batch(ctx, sets, BATCH_DIST, BATCH_ST, BATCH_SEED, -1, False)
    return sets, want, base


def _tails_are_zero(recs):
    for r in recs:
        k = int(r["n_in"])
        assert not r["a"][k:].view(np.uint8).any() and not r["b"][k:].view(np.uint8).any()


def test_batch_equals_oracle_pair_by_pair(ctx, batch):
    """ransac_kernel / the split form on many pairs of stride 400 with the tables indexed by n: every record against the oracle"""
    sets, want, base = batch
    assert {0, 3, 4, 5, 63, 64, 65, 255, 256, 257, 396, 397, 398, 399, 400} <= {len(a) for a, _ in sets}
    for k, (r, w) in enumerate(zip(base, want)):
        n_in = int(r["n_in"])
        assert n_in == len(w[1]) and int(r["ok"]) == w[0], (k, len(sets[k][0]), n_in, len(w[1]), int(r["ok"]), w[0])
        assert np.array_equal(r["a"][:n_in], w[1]) and np.array_equal(r["b"][:n_in], w[2]), k
        assert np.array_equal(bits(r["H"]), bits(w[3])), (k, len(sets[k][0]), r["H"], w[3])
    _tails_are_zero(base)
    host = _ransac_batch(ctx, sets, BATCH_DIST, BATCH_ST, BATCH_SEED, -1, True)
    assert host.tobytes() == base.tobytes()               # host-built tables (table_of) against the device-built ones (n - 4)


def test_batch_min_keep(ctx, batch):
    """cnt <= min_keep: ok 0, H zero, the inlier lists kept; every other record unchanged"""
    sets, want, base = batch
    counts = {int(r["n_in"]) for r in base}
    assert {0, 4, 30, 31} <= counts and max(counts) > 31, sorted(counts)
    for host_tables in (False, True):
        kept = _ransac_batch(ctx, sets, BATCH_DIST, BATCH_ST, BATCH_SEED, 30, host_tables)
        for k, (r, b) in enumerate(zip(kept, base)):
            if int(b["n_in"]) <= 30:
                assert int(r["ok"]) == 0 and not r["H"].view(np.uint32).any(), (k, int(b["n_in"]))
                assert int(r["n_in"]) == int(b["n_in"]) and r["a"].tobytes() == b["a"].tobytes() and r["b"].tobytes() == b["b"].tobytes(), k
            else:
                assert r.tobytes() == b.tobytes(), (k, int(b["n_in"]))
        _tails_are_zero(kept)


@pytest.mark.parametrize("n_pairs", [1, 128, 256, 257])
def test_batch_sizes_where_the_default_split_changes(ctx, batch, n_pairs):
    """the default width is 2 x CUs / pairs, capped at 4 and dropped below 2: 1 and 128 pairs run 4 workgroups per pair, 256 pairs 2, 257 the
    one-workgroup form.  The set is repeated to the count; a record depends on its own input alone"""
    sets, want, base = batch
    idx = [k % len(sets) for k in range(n_pairs)]
    recs = _ransac_batch(ctx, [sets[k] for k in idx], BATCH_DIST, BATCH_ST, BATCH_SEED, -1, False)
    for r, k in zip(recs, idx):
        assert r.tobytes() == base[k].tobytes(), (n_pairs, k, len(sets[k][0]))


def test_debug_batch_refuses_more_than_400(ctx):
    import imagemosaicing_amd as im
    P = np.zeros((1, MAX_N), SFPOINT); n = np.array([401], np.int32); out = np.zeros(1, im.PAIR_RESULT)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for host_tables in (0, 1):
        assert ctx.L.mi355_debug_ransac_batch(ctx._h, p(P), p(P), p(n), 1, C.c_float(2.5), 1000, C.c_uint32(1), -1, host_tables, p(out)) < 0


# ---------------------------------------------------------------------------------------------- draw tables
def _tables_restated(stream, n_lo, n_hi):
    """the k-th draw is the k-th aligned group of four stream values that are pairwise distinct mod n (mosaicimage.h:1801-1813)"""
    groups = stream[: len(stream) // 4 * 4].reshape(-1, 4)
    out = np.zeros((n_hi - n_lo + 1, rp.MAX_DRAWS, 4), np.uint16)
    for n in range(n_lo, n_hi + 1):
        g = groups if n < 8 else groups[:20000]              # from n = 8 on more than 40 % of the groups are distinct: 20000 hold 4999 by far
        v = g % n
        ok = np.ones(len(v), bool)
        for i in range(4):
            for j in range(i + 1, 4):
                ok &= v[:, i] != v[:, j]
        keep = v[ok]
        assert len(keep) >= rp.MAX_DRAWS, (n, len(keep))
        out[n - n_lo] = keep[: rp.MAX_DRAWS]
    return out


@pytest.mark.parametrize("seed", [1, 12345, 0xFFFFFFFF])
def test_device_draw_tables_equal_the_restatement(ctx, oracle, seed):
    """draw_tables_kernel for every n in 4..400: what MatchPairs, MatchPairsDev and SURF read (Ransac2D's tables are built on the host)"""
    got = np.zeros((MAX_N - 3, rp.MAX_DRAWS, 4), np.uint16)
    assert ctx.L.mi355_debug_draw_tables(ctx._h, C.c_uint32(seed), 4, MAX_N, got.ctypes.data_as(C.c_void_p)) == 0
    st = (C.c_int32 * 40)()
    oracle.L.orc_srand(st, C.c_uint(seed))
    rnd = oracle.L.orc_rand
    nstream = 404 * 992                                       # the device's stream length (ransac.hip RAW_STREAM)
    stream = np.fromiter((rnd(st) for _ in range(nstream)), np.int64, nstream)
    want = _tables_restated(stream, 4, MAX_N)
    bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
    assert len(bad) == 0, ("n", (bad[:8] + 4).tolist())
    # a sub-range starts at its own n
    sub = np.zeros((3, rp.MAX_DRAWS, 4), np.uint16)
    assert ctx.L.mi355_debug_draw_tables(ctx._h, C.c_uint32(seed), 63, 65, sub.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(sub, want[59:62])
    assert ctx.L.mi355_debug_draw_tables(ctx._h, C.c_uint32(seed), 3, 10, sub.ctypes.data_as(C.c_void_p)) < 0
    assert ctx.L.mi355_debug_draw_tables(ctx._h, C.c_uint32(seed), 399, 401, sub.ctypes.data_as(C.c_void_p)) < 0


# ---------------------------------------------------------------------------------------------- the seed slots
def test_seed_slots_evict_rebuild_and_return_without_synchronise():
    """mi_ransac_tables keeps four seeds' tables and reuses the slot used longest ago.  Seeds 1 2 3 4 fill the slots, 5 takes seed 1's, 1 takes
    seed 2's (the return to an evicted seed), 2 takes seed 3's, 6 takes seed 4's, 1 is found again -- every rebuild is enqueued behind launches
    that still read the slot's old tables, and nothing synchronises between the calls.  Same bytes as on a fresh context that synchronises
    after every call."""
    import torch
    import imagemosaicing_amd as im
    from tests.test_gpu_parity import _synthetic_feature_pair
    seeds = [1, 2, 3, 4, 5, 1, 2, 6, 1]
    rng = np.random.default_rng(12)
    feats = [_synthetic_feature_pair(rng, n=900 + 150 * k) for k in range(3)]
    pairs = [(0, 1), (2, 3), (4, 5), (0, 3)]
    item = im.PAIR_RESULT.itemsize

    def run(sync_each):
        c = im.Context(0)
        try:
            for k, (kp1, d1, kp2, d2) in enumerate(feats):
                c.SetFeatures(2 * k, kp1, d1.astype(np.float32), 4000, 3000)
                c.SetFeatures(2 * k + 1, kp2, d2.astype(np.float32), 4000, 3000)
            bufs = [torch.zeros((len(pairs), item), dtype=torch.uint8, device="cuda") for _ in seeds]
            torch.cuda.synchronize()
            for s, b in zip(seeds, bufs):
                c.MatchPairsDev(pairs, b.data_ptr(), 2.5, s)
                if sync_each:
                    c.synchronize()
            c.synchronize()
            return [b.cpu().numpy().tobytes() for b in bufs]
        finally:
            c.close()

    chained = run(False)
    stepped = run(True)
    assert chained == stepped, [k for k in range(len(seeds)) if chained[k] != stepped[k]]
    by_seed = {}
    for s, b in zip(seeds, stepped):
        assert by_seed.setdefault(s, b) == b, s               # a seed's records do not depend on the slot its tables were rebuilt in
    # the seed matters to these pairs: tables left over from the seed a slot held before would show.  Seed 5 took the slot of 1, the second
    # 1 that of 2, the second 2 that of 3, and 6 that of 4
    for new, old in ((5, 1), (1, 2), (2, 3), (6, 4)):
        assert by_seed[new] != by_seed[old], (new, old)
    r = np.frombuffer(stepped[0], im.PAIR_RESULT)
    assert int(r["accepted"].sum()) >= 2 and int(r["n_selected"].min()) >= 4
