"""CPU: the response threshold of top-k SIFT's selection, restated in numpy two ways.

select_unique_kernel (csrc/sift.hip) orders the refined points by the 16-bit key (resp_bits >> 15) & 0xffff -- the exponent byte and the top
eight mantissa bits of |response| -- and takes T = the lower edge of the first key, from the top, at which the count of points with a key
at or above it reaches `want`.  It finds that key with two 8-bit radix passes (high byte, then the low byte among the points that share
the selected high byte).  One histogram of all 65 536 keys scanned from the top is the other way to the same number; a kernel that took
that route would have to give the same T bit for bit, so the two are set against each other here, on the multisets where they could part:
keys that share one exponent byte (what real responses do), n = want and want +- 1, a tie that spans the threshold.

Duplicates: refine_kernel stores a record per accepted start point, so a location that several start points converged to is counted
several times towards `want`.  The last tests state what that does to T and to the points that remain once each location is kept once."""
import numpy as np
import pytest


def keys_of(resp_bits):
    return (np.asarray(resp_bits, np.uint32) >> 15) & 0xffff


def t_histogram(resp_bits, want):
    """T from the 16-bit key histogram, top down; 0 where everything is taken (n <= want)"""
    k = keys_of(resp_bits)
    if len(k) <= want:
        return 0
    hist = np.bincount(k, minlength=65536)
    cum = np.cumsum(hist[::-1])                       # cum[j]: points with key >= 65535 - j
    j = int(np.searchsorted(cum, want, side="left"))  # first j with cum[j] >= want
    return (65535 - j) << 15


def t_radix(resp_bits, want):
    """the kernel's way: two 8-bit passes, `above` carried from the first into the second"""
    k = keys_of(resp_bits)
    if len(k) <= want:
        return 0

    def scan(hist, cum):
        b = 255
        while b >= 0:
            if cum + hist[b] >= want:
                break
            cum += hist[b]
            b -= 1
        return max(b, 0), cum
    hi, above = scan(np.bincount(k >> 8, minlength=256), 0)
    lo, _ = scan(np.bincount(k[(k >> 8) == hi] & 255, minlength=256), above)
    return ((hi << 8) | lo) << 15


def _resp(rng, n, one_exponent=False):
    """|response| bits: positive floats; one_exponent: all in [2^-5, 2^-4), as a frame's contrasts above the threshold mostly are"""
    if one_exponent:
        v = rng.uniform(2.0 ** -5, 2.0 ** -4, n).astype(np.float32)
        v = np.minimum(v, np.nextafter(np.float32(2.0 ** -4), np.float32(0)))
        bits = v.view(np.uint32)
        assert len(np.unique(bits >> 23)) == 1
        return bits
    return np.exp(rng.uniform(-8, 3, n)).astype(np.float32).view(np.uint32)


def _check(bits, want):
    t = t_histogram(bits, want)
    assert t == t_radix(bits, want), (len(bits), want)
    if len(bits) > want:
        assert t & 0x7fff == 0
        assert np.count_nonzero(bits >= t) >= want                              # enough at or above T
        assert np.count_nonzero(bits >= t + (1 << 15)) < want                   # and T is the highest such key edge
    return t


@pytest.mark.parametrize("one_exponent", [False, True])
def test_random_multisets(one_exponent):
    rng = np.random.default_rng(5 + one_exponent)
    for n in (1, 2, 63, 64, 65, 1000, 4097, 70000):
        bits = _resp(rng, n, one_exponent)
        for want in sorted({1, 2, 17, 256, 2256, 2304, n // 2 + 1, max(n - 1, 1)}):
            _check(bits, want)


@pytest.mark.parametrize("one_exponent", [False, True])
def test_n_at_want(one_exponent):
    """n = want: everything is taken (T = 0); n = want + 1: T is the key of the second weakest point; n = want - 1: T = 0"""
    rng = np.random.default_rng(11 + one_exponent)
    want = 2304
    for n in (want - 1, want, want + 1):
        bits = _resp(rng, n, one_exponent)
        t = _check(bits, want)
        if n <= want:
            assert t == 0
        else:
            assert t == int(keys_of(np.sort(bits)[1])) << 15


def test_tie_spans_threshold():
    """300 points share the key at which the count passes `want`: all of them lie at or above T, however many more than `want` that makes;
    the same with the tie at the very top and at key 0"""
    rng = np.random.default_rng(3)
    base = _resp(rng, 5000, True)
    srt = np.sort(base)[::-1]
    for pos in (0, 100, 2200, 4990):
        tie = np.full(300, srt[pos], np.uint32)
        bits = rng.permutation(np.concatenate([base, tie]))
        for want in (pos + 1, pos + 150, pos + 300, pos + 301):
            if want >= len(bits):
                continue
            t = _check(bits, want)
            if want <= pos + 300:
                assert t == int(keys_of(srt[pos])) << 15
                assert np.count_nonzero(bits >= t) >= pos + 300
    zeros = np.zeros(400, np.uint32)                                            # key 0: the scan ends in its last bin
    bits = np.concatenate([base[:100], zeros])
    assert _check(bits, 300) == 0


def test_all_keys_equal():
    bits = np.full(5000, np.float32(0.04).view(np.uint32), np.uint32)
    assert _check(bits, 2304) == int(keys_of(bits[:1])[0]) << 15


@pytest.mark.parametrize("one_exponent", [False, True])
def test_duplicates_counted_and_not(one_exponent):
    """Records of one location share their response.  T over the records (duplicates counted) is never below T over the locations, the
    locations at or above it are the strongest ones and number at least want - (duplicates among them); selecting again with `want` raised
    by that number lowers T, if anything."""
    rng = np.random.default_rng(21 + one_exponent)
    for n_loc, n_dup, want in ((3000, 0, 2304), (3000, 40, 2304), (3000, 900, 2304), (2400, 300, 2304), (2304, 50, 2304), (500, 100, 64)):
        loc = _resp(rng, n_loc, one_exponent)
        extra = rng.integers(0, n_loc, n_dup)                                  # locations stored once more (some several times)
        owner = np.concatenate([np.arange(n_loc), extra])
        rec = loc[owner]
        t_rec, t_loc = _check(rec, want), _check(loc, want)
        assert t_rec >= t_loc
        kept = np.unique(owner[rec >= t_rec])                                   # what is left when each location is listed once
        dropped = np.count_nonzero(rec >= t_rec) - len(kept)
        assert np.array_equal(kept, np.flatnonzero(loc >= t_rec))
        if len(rec) > want:
            assert len(kept) >= want - dropped
        if n_dup == 0:
            assert t_rec == t_loc and dropped == 0
        t_again = _check(rec, want + dropped)                                  # (new duplicates may enter with the weaker points: no promise of `want`)
        assert t_again <= t_rec
        assert len(np.unique(owner[rec >= t_again])) >= len(kept)
