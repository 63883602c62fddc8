"""The host half of cover depth (csrc/cover_select.cpp: mi355_cover_select) from the built library, driven through its callback with the numpy
restatement (tests/cover_ref.py) supplying every round's statistics: status, keep_out, rounds and lost equal the reference's round rule on
every selection layout of tests/cover_patterns.py and on 200 random ones, with and without a pair list.  The boxes are the library's own
(mi_frame_dev_setup), so the comparison also holds cover_ref.geometry's boxes against them.  Then every refusal and its message, the defaults
and the record sizes, and the same source under AddressSanitizer and UBSan as a stand-alone program (tests/cxx/cover_select_sanitize.cpp:
nothing is loaded into Python under a sanitizer).  No GPU.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import cover_patterns as cp
from tests import cover_ref as cr

SELECTS = cp.select_cases()


@pytest.fixture(scope="module")
def im():
    import imagemosaicing_amd as im
    return im


def _run(im, case, **kw):
    covers, boxes, (cw, ch) = cp.geometry_of(case)
    calls = []

    def stats(keep):
        calls.append(keep.copy())
        fs = cr.stats_ref(covers, keep, case.step, (ch, cw))[0]
        out = np.zeros(len(fs), im.COVER_FRAME_STATS)
        out["at_depth"] = fs["at_depth"]
        return out
    w, h = [s[0] for s in case.sizes], [s[1] for s in case.sizes]
    args = dict(order=case.order, pairs=case.pairs, keep=None if case.keep is None else np.array(case.keep, np.uint8), step=case.step, min_depth=case.min_depth,
                max_loss=case.max_loss)
    args.update(kw)
    return im.cover_select(w, h, case.h9s, stats, **args), calls


def _equal(got, want, what):
    status, keep_out, rounds, lost = got
    assert status.dtype == np.uint8 and keep_out.dtype == np.uint8
    assert status.tolist() == want.status.tolist(), (what, status.tolist(), want.status.tolist())
    assert keep_out.tolist() == want.keep_out.tolist(), what
    assert (rounds, lost) == (want.rounds, want.lost), (what, rounds, lost, want.rounds, want.lost)


def test_sizes_and_defaults(im):
    p = im.cover_params()
    assert im.COVER_FRAME_STATS.itemsize == 64 and im.COVER_BINS == 9
    import ctypes
    assert ctypes.sizeof(im.CoverParams) == 16 and im.CoverParams.max_loss.offset == 8
    assert (p.step, p.min_depth, p.max_loss) == (8, 1, 0)
    assert im.COVER_FRAME_STATS == cr.FRAME_STATS
    assert (im.COVER_NOT_CANDIDATE, im.COVER_DROPPED, im.COVER_KEPT_COVERAGE, im.COVER_CUT_VERTEX, im.COVER_NOT_EXAMINED) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize("case", SELECTS, ids=[s.tag for s in SELECTS])
def test_selection_layouts_equal_the_reference(im, case):
    got, calls = _run(im, case)
    want = cp.reference(case)
    _equal(got, want, case.tag)
    assert len(calls) == want.rounds                                        # one statistics call per round, none after the last
    n = len(case.sizes)
    assert all(len(k) == n and set(k.tolist()) <= {0, 1} for k in calls)
    if calls:                                                               # each round is asked under the kept set of the moment: it only shrinks
        assert all((b <= a).all() for a, b in zip(calls, calls[1:])) and (got[1] <= calls[-1]).all()


def test_random_layouts_equal_the_reference(im):
    for seed in cp.RANDOM_SEEDS:
        for with_pairs in (False, True):
            case = cp.random_layout(seed, with_pairs)
            _equal(_run(im, case)[0], cp.reference(case), case.tag)


def test_no_candidate_takes_no_round(im):
    case = cp.by_select()["strip5_waits"]
    (status, keep_out, rounds, lost), calls = _run(im, case, order=[])
    assert not status.any() and keep_out.all() and (rounds, lost) == (0, 0) and not calls
    (status, keep_out, rounds, lost), calls = _run(im, case, order=None, keep=np.zeros(5, np.uint8))
    assert not status.any() and not keep_out.any() and rounds == 0 and not calls


def test_an_exception_in_the_statistics_function_comes_back(im):
    case = cp.by_select()["strip5_waits"]

    def boom(keep):
        raise KeyError("statistics")
    with pytest.raises(KeyError):
        im.cover_select([21] * 5, [11] * 5, case.h9s, boom, order=[1])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def _refused(im, needle, case=None, sizes=None, h9s=None, **kw):
    case = case or cp.by_select()["strip5_waits"]
    sizes = sizes or case.sizes
    h9s = case.h9s if h9s is None else h9s
    called = []
    with pytest.raises(im.Mi355Error) as e:
        im.cover_select([s[0] for s in sizes], [s[1] for s in sizes], h9s, lambda keep: called.append(1), **kw)
    assert e.value.code == -1 and needle in str(e.value) and "cover_select: " in str(e.value), str(e.value)
    assert not called                                                       # refused before the first round


def test_refusals_name_the_index_or_value(im):
    _refused(im, "step=0 outside [1, 64]", step=0)
    _refused(im, "step=65 outside [1, 64]", step=65)
    _refused(im, "min_depth=0 outside [1, 8]", min_depth=0)
    _refused(im, "min_depth=9 outside [1, 8]", min_depth=9)
    _refused(im, "max_loss=-1 < 0", max_loss=-1)
    _refused(im, "order[1]=5 outside [0, 5)", order=[0, 5])
    _refused(im, "order[0]=-1 outside [0, 5)", order=[-1])
    _refused(im, "order[2]=3 repeats order[0]", order=[3, 1, 3])
    _refused(im, "pair 1 (2, 2): a == b", pairs=[(0, 1), (2, 2)])
    _refused(im, "position outside [0, 5)", pairs=[(0, 5)])
    _refused(im, "repeats pair 0", pairs=[(0, 1), (1, 0)])
    case = cp.by_select()["strip5_waits"]
    _refused(im, "frame 2: bad geometry w=1 h=11", sizes=[(21, 11), (21, 11), (1, 11), (21, 11), (21, 11)])
    _refused(im, "frame 0: bad geometry w=21 h=1", sizes=[(21, 1)] + [(21, 11)] * 4)
    gone = case.h9s.copy()
    gone[2][8] = 0                                                          # a frame that takes no part may have any size
    (status, _, _, _), _ = _run(im, case._replace(sizes=[(21, 11), (21, 11), (1, 1), (21, 11), (21, 11)], h9s=gone))
    assert status[2] == 4


def test_more_than_65535_frames_is_refused(im):
    n = 65536
    with pytest.raises(im.Mi355Error) as e:
        im.cover_select(np.full(n, 4, np.int32), np.full(n, 4, np.int32), np.tile(np.eye(3, dtype=np.float32).reshape(9), (n, 1)), lambda keep: None)
    assert "n=65536 outside [1, 65535]" in str(e.value)


# ---- the same source under AddressSanitizer and UBSan, as a stand-alone program ------------------------------------------------------------------
def test_cover_select_under_asan_ubsan(tmp_path):
    from tests.test_sanitize import CSRC, ROOT, _runner
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    prefix = _runner(tmp_path, flags, "asan")
    exe = str(tmp_path / "cover_select_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + flags + ["-I", os.path.join(ROOT, "include"), "-I", CSRC,
           os.path.join(ROOT, "tests", "cxx", "cover_select_sanitize.cpp"), os.path.join(CSRC, "cover_select.cpp"), os.path.join(CSRC, "gain_solve.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run(prefix + [exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "SANITIZE_OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
