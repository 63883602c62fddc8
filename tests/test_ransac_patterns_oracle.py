"""CPU: the RANSAC patterns of tests/ransac_patterns.py against the oracle's trace of the loop (orc_ransac2d_trace) -- every pattern must
show the property it is named for -- the trace against the plain oracle, and the oracle against the reference's own Ransac2D where
oracle/_ref is built.  The GPU side is tests/test_gpu_ransac_edges.py."""
import numpy as np
import pytest

from tests.golden_util import bits
from tests import ransac_patterns as rp


@pytest.fixture(scope="module")
def traced(oracle):
    return {p.name: oracle.ransac2d_trace(p.p1, p.p2, p.dist, p.sample_times, p.seed, keep_going=True) for p in rp.patterns()}


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(bits(a[3]), bits(b[3]))


def test_every_pattern_shows_its_property(oracle, traced):
    for p in rp.patterns():
        r, t = traced[p.name]
        s = t["stop_slot"]
        stopped_slots = s + 1 if s >= 0 else t["n_slots"]
        stopped_draws = t["stop_draw"] + 1 if s >= 0 else t["draws"]
        print("%-22s n %5d st %4d seed %4d stop %4d support %5s slots %4d draws %4d | run on: slots %4d draws %4d larger behind %4d | n_in %d ok %d" % (
            p.name, len(p.p1), p.sample_times, p.seed, s, int(t["supports"][s]) if s >= 0 else "-", stopped_slots, stopped_draws, t["n_slots"], t["draws"],
            int((t["supports"][s + 1:] > t["supports"][s]).sum()) if s >= 0 else 0, len(r[1]), r[0]))
        p.check(t, r)


def test_trace_equals_plain_oracle(oracle, traced):
    """one loop body serves both entry points: same result, and the trace's winner and slot count are those of the loop that stops"""
    for p in rp.patterns():
        plain = oracle.ransac2d(p.p1, p.p2, p.dist, p.sample_times, p.seed)
        for keep in (False, True):
            r, t = traced[p.name] if keep else oracle.ransac2d_trace(p.p1, p.p2, p.dist, p.sample_times, p.seed, keep_going=False)
            assert _same(plain, r), (p.name, keep)
            sup, s = t["supports"], t["stop_slot"]
            assert len(sup) == t["n_slots"] == int(t["took"].sum()) and len(t["took"]) == t["draws"] <= rp.MAX_DRAWS
            assert t["n_slots"] <= min(p.sample_times, 5000)
            seen = sup[: s + 1] if s >= 0 else sup             # what the loop looks at
            if len(seen) and seen.max() > 0:
                assert t["win_slot"] == int(seen.argmax()) and t["win_support"] == int(seen.max()), p.name      # first strict maximum
            else:
                assert t["win_slot"] == -1 and t["win_support"] == 0
            if s >= 0:
                assert rp.float_stops(sup[s], len(p.p1)) and (s == 0 or sup[s] > sup[:s].max())
                assert int(t["took"][: t["stop_draw"] + 1].sum()) == s + 1 and t["took"][t["stop_draw"]]
                if not keep:
                    assert t["n_slots"] == s + 1 and t["draws"] == t["stop_draw"] + 1
            if keep:
                # the stopper is simply the first slot whose support passes the float test: supports below it pass neither that test nor,
                # the product being monotone, exceed it -- so "strictly larger than every earlier support" is implied at the stop, and the
                # running maximum replay_supports carries from block to block cannot change where the loop stops (only bestkey, the winner
                # so far, has to cross the blocks)
                passing = np.nonzero(sup.astype(np.float32) * (np.float32(1.0) / np.float32(len(p.p1))) > np.float32(0.99))[0]
                assert (s == int(passing[0])) if len(passing) else s < 0, p.name
            # no earlier slot would have stopped the loop
            run = np.maximum.accumulate(np.concatenate([[0], seen[:-1]])) if len(seen) else np.zeros(0, np.int64)
            for i in np.nonzero(seen > run)[0][: -1 if s >= 0 else None]:
                assert not rp.float_stops(seen[i], len(p.p1)), (p.name, int(i))


def test_oracle_equals_reference_on_patterns(oracle):
    """the oracle's result on every pattern against the reference's own Ransac2D (oracle/_ref), where that library is at hand"""
    from tests import oracle_lib
    ref = oracle_lib.load_ref()
    if ref is None:
        pytest.skip("oracle/_ref is not built")
    for p in rp.patterns():
        a = oracle.ransac2d(p.p1, p.p2, p.dist, p.sample_times, p.seed)
        b = ref.ransac2d(p.p1, p.p2, p.dist, p.sample_times, p.seed)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), p.name
        if len(a[1]) >= 4:
            assert np.array_equal(bits(a[3]), bits(b[3])), p.name


def test_float_stop_differs_from_exact_only_at_099n_and_only_for_big_n():
    """(float)support * (1.0f / n) > 0.99f against support / n > 0.99 exactly, for every n up to 65535.  The float product is monotone in the
    support, so the two can only differ next to 0.99 n: the supports within 4 of it are compared.  They differ only where support = 0.99 n
    exactly, and there only for some n (500, 1000, 2000, 4000, 7100, 8000 and further ones above), all beyond the 400 points of the batched
    kernels: hence the float_threshold patterns' n = 500, 1000 and 8000."""
    n = np.arange(4, 65536, dtype=np.int64)
    invn = np.float32(1.0) / n.astype(np.float32)
    differ = set()
    for d in range(-4, 5):
        s = np.clip(99 * n // 100 + d, 0, n)
        f = s.astype(np.float32) * invn > np.float32(0.99)
        e = 100 * s > 99 * n
        for k in np.nonzero(f != e)[0]:
            assert f[k] and not e[k]                          # the float form stops where the exact ratio would not
            differ.add((int(n[k]), int(s[k])))
    assert differ and all(100 * s == 99 * m for m, s in differ), sorted(differ)[:8]          # only at a support of exactly 0.99 n
    assert min(m for m, _ in differ) > 400                                                   # never in the batched kernels' range
    assert sorted(m for m, _ in differ if m <= 8000) == [500, 1000, 2000, 4000, 7100, 8000]
    for m, s in differ:
        assert rp.float_stops(s, m) and not rp.exact_stops(s, m)
