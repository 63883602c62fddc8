"""CPU: the narrow octaves' routes of csrc/sift_plan.cpp (Routes::narrow, option "narrow_routes") without a GPU.  A wrong route gives the
same features more slowly, and a wrong segment list leaves rows unwritten only at some heights; tests/cxx/sift_plan_narrow_check.cpp is
compiled together with the plan by g++ -fsanitize=address,undefined, in the manner of tests/test_sift_plan.py, and run as a program of
its own.

  off   narrow = 0 written out equals a Routes whose narrow member was left at its default, launch by launch (tests/test_sift_plan.py pins
        that default against the loops the plan replaced)
  on    narrow = 1: the segments of a streamed launch cover every row exactly once, L is even and at least STREAM_NARROW_MIN_L, the last
        strip is wider than MAX_R, the grid holds nstrip x nseg x n waves, the ds launch is the R = 8 level of an even-height octave, and
        all five launch kinds occur
Both over w in the new lower width +- 8, 508..520, 996..1004 crossed with h in 62..70 and 372..378, plus 4000x3000, 2000x1500 and
1000x750; 1 / 4 / 21 / 32 frames; both `aligned` values; xstream_min_w 1000 and 1500.
The last test states the 12 MP frames' octaves 2 and 3 at batches of 32 and 21 as numbers, worked out from the rule by hand."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sift_plan_narrow") / "sift_plan_narrow_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "cxx", "sift_plan_narrow_check.cpp"), os.path.join(ROOT, "imagemosaicing_amd", "csrc", "sift_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-300:])
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    return exe


def _run(driver, *args):
    r = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def test_narrow_off_is_the_pinned_plan(driver):
    out = _run(driver, "off")
    print(out)
    assert " 0 failed" in out


def test_narrow_on_invariants(driver):
    out = _run(driver, "on")
    print(out)
    assert " 0 failed" in out
    kinds = [int(v) for v in out.split("kind")[1].split()]
    assert len(kinds) == 5 and all(k > 0 for k in kinds), out


def _blurs(out, narrow, octave):
    """(R, L, nstrip, nseg, gx) of the five blurs of an octave's levels 1 .. 5 and the kind of its extrema launch"""
    rows = [l.split() for l in out.splitlines() if l.startswith(f"narrow {narrow} octave {octave} ")]
    f = [dict(zip(r[0::2], r[1::2])) for r in rows]
    blurs = [(int(d["kind"]), int(d["R"]), int(d["L"]), int(d["nstrip"]), int(d["nseg"]), int(d["grid"])) for d in f if 1 <= int(d["level"]) <= 5]
    ext = [int(d["kind"]) for d in f if int(d["level"]) == -1]
    return blurs, ext


@pytest.mark.parametrize("n", [32, 21])
def test_12mp_octaves_2_and_3(driver, n):
    """4000x3000.  Octave 2 (1000x750, 4 strips): the pinned rule stops at 64 rows, 12 segments: 48 n waves, 1.5 (n = 32) / 1.0 (21) per
    SIMD.  narrow: ceil(2048 / 4 n) = 16 / 25 segments -> 47 / 30 rows -> L = 48 / 30.  Octave 3 (500x375, 2 strips): tiled before; narrow:
    32 / 49 segments -> 12 / 8 rows -> the floor of 16, 24 segments.  Octave 4 (250x187) stays tiled.  The radii of levels 1 .. 5 are
    5, 6, 8, 10, 13.  Octave 2's extrema: streamed at xstream_min_w = 1000 either way."""
    out = _run(driver, "show", 4000, 3000, n)
    radii = [5, 6, 8, 10, 13]
    L2 = {32: 48, 21: 30}[n]
    nseg2 = -(-750 // L2)
    b0, e0 = _blurs(out, 0, 2)
    b1, e1 = _blurs(out, 1, 2)
    assert b0 == [(0, r, 64, 4, 12, (4 * 12 * n + 3) // 4) for r in radii] and e0 == [3]
    assert b1 == [(0, r, L2, 4, nseg2, (4 * nseg2 * n + 3) // 4) for r in radii] and e1 == [3]
    b0, e0 = _blurs(out, 0, 3)
    b1, e1 = _blurs(out, 1, 3)
    assert [b[:2] for b in b0] == [(1, r) for r in radii] and e0 == [4]
    assert b1 == [(0, r, 16, 2, 24, (2 * 24 * n + 3) // 4) for r in radii] and e1 == [4]
    for narrow in (0, 1):
        b, e = _blurs(out, narrow, 4)
        assert [x[:2] for x in b] == [(1, r) for r in radii] and e == [4]
    for o in (0, 1):
        assert _blurs(out, 0, o) == _blurs(out, 1, o)
