"""CPU: what a SIFT batch decides on the host (csrc/sift_plan.cpp: Gaussian taps, work-area layout, batch length, the pyramid and extrema
launches with their routes and grids) without a GPU.  A wrong route gives the same features more slowly, so no parity test sees it; this
one does.  The plan is host code with no HIP in it: tests/cxx/sift_plan_check.cpp is compiled together with it by
g++ -fsanitize=address,undefined, in the manner of tests/test_blend_plan.py, and run as a program of its own.

  print   taps, layout and launch list of every case equal the restatement below, which follows the host code the plan replaced
          (sift.hip's sift_prepare / blur_streams / stream_grid / launch_blur / sift_run_batch before the plan existed), loop by loop
  sweep   the invariants listed at the driver's check_layout / check_launches over w, h in 16..70, 250..262, 508..520, 1020..1030,
          2040..2056 crossed, 1 / 2 / 5 / 32 frames and five route settings
"""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

N_LAYERS, N_LEVELS, IMG_BORDER, MAX_OCT, MAX_R = 3, 6, 5, 16, 16
EW, EH, REG_SHIFT, NREG, XSW, XWAVES, KA_TILE, SEL_STRIDE, T16W, T16H = 64, 16, 0, 64, 248, 3, 4096, 2048, 64, 32
BLUR_STREAM, BLUR_TILE, DOWNSAMPLE, EXTREMA_STREAM, EXTREMA_TILE = range(5)

SIZES = [(16, 16), (64, 64), (129, 200), (333, 257), (320, 240), (640, 480), (1024, 768), (1100, 780), (1101, 700), (2200, 1604), (1920, 1080),
         (3840, 2160), (4000, 3000), (1048575, 16), (16, 1048575)]
KEEPALL = [(16384, 16384, 32768), (16384, 16384, 262144)]
REFUSED = [(40000, 30000, "sift: image too large")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sift_plan") / "sift_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "cxx", "sift_plan_check.cpp"), os.path.join(ROOT, "imagemosaicing_amd", "csrc", "sift_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-300:])
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    return exe


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def gauss_kernel_host(sigma):
    """cv::getGaussianKernel(ksize, sigma, CV_32F): each exp() rounded to float, the floats summed in double, taps (float)(tap / sum)"""
    ksize = int(round(sigma * 8.0 + 1.0)) | 1
    k = np.array([np.float32(math.exp(-0.5 / (sigma * sigma) * (i - (ksize - 1) * 0.5) ** 2)) for i in range(ksize)], np.float32)
    s = 0.0
    for v in k:
        s += float(v)
    s = 1.0 / s
    return ksize // 2, np.array([np.float32(float(v) * s) for v in k], np.float32)


def taps():
    sigma, k = 1.6, 2.0 ** (1.0 / N_LAYERS)
    out = [None] * N_LEVELS
    for i in range(1, N_LEVELS):
        sp = k ** (i - 1) * sigma
        st = sp * k
        out[i] = gauss_kernel_host(math.sqrt(st * st - sp * sp))
    sd = np.sqrt(np.maximum(np.float32(sigma) * np.float32(sigma) - np.float32(0.25), np.float32(0.01)), dtype=np.float32)
    out[0] = gauss_kernel_host(float(sd))
    return out


TAPS = taps()
RADIUS0, RADIUS = TAPS[0][0], [0] + [t[0] for t in TAPS[1:]]


def up64(v):
    return (v + 63) & ~63


def sift_prepare(w, h, keepall, kmax):
    """-> error text, or the sizes and pointers (as offsets) of one frame's work area"""
    if w >= 1 << 20 or h >= 1 << 20:
        return "sift: image too large"
    if w < 16 or h < 16:
        return "sift: image too small"
    n_oct = min(int(round(math.log(min(w, h)) / math.log(2.0) - 2.0)), MAX_OCT)
    fl = cl = no = 0
    for o in range(n_oct):
        ow, oh = w >> o, h >> o
        if ow < 2 * IMG_BORDER + 2 or oh < 2 * IMG_BORDER + 2:
            break
        fl += up64(ow * oh) * N_LEVELS
        cl += ((ow * oh * 4 + 31) // 32 + 63) & ~63
        no = o + 1
    if no == 0:
        return "sift: image too small"
    px0 = w * h
    if 4 * px0 + 1024 > 0xfffffff0:
        return "sift: image too large"
    p = dict(n_oct=no)
    p["cand_cap"] = (4 * px0 + 1024 + NREG - 1) // NREG + ((MAX_OCT * 3 * EW * EH) << REG_SHIFT) + 1024
    p["ref_cap"] = p["kp_cap"] = px0 // 8 + 65536
    p["cube_cap"] = min(px0 // 4 // NREG + 4096, p["cand_cap"])
    ml = sum((w >> o) * (h >> o) * 4 for o in range(no)) if keepall else 0
    p["bs"] = dict(pyr=fl, claimed=cl, cand=p["cand_cap"] * NREG, refined=p["ref_cap"], kps=p["kp_cap"], cube=p["cube_cap"] * NREG * 32,
                   sel=kmax if keepall else SEL_STRIDE, mins=ml)
    p["ksort_stride"] = (kmax + KA_TILE - 1) // KA_TILE * KA_TILE if keepall else 0
    fo = co = mo = 0
    p["oc"] = []
    for o in range(no):
        ow, oh = w >> o, h >> o
        lv = []
        for _ in range(N_LEVELS):
            lv.append(fo)
            fo += up64(ow * oh)
        p["oc"].append(dict(w=ow, h=oh, lv=lv, claimed=co, mins=mo if keepall else None))
        co += ((ow * oh * 4 + 31) // 32 + 63) & ~63
        mo += ow * oh * 4
    return p


def batch_frames(w, h, keepall, sift_batch, slots, total_mem):
    nb = 1 if sift_batch < 1 else min(sift_batch, 32)
    per_frame = 60.0 * w * h
    if total_mem:
        fit = int(0.6 * total_mem / ((1.4 if keepall else 1.0) * per_frame) / slots)
        if fit < nb:
            nb = max(fit, 1)
    if keepall and nb > 8:
        nb = 8
    return nb


def blur_streams(a, bgr, R, stream_mode):
    """a: w, h, ds, and for the base level `aligned`: every frame pointer and pitch a multiple of 4, pitch >= 3 w.  The work area's own
    pointers and frame stride pass their tests (multiples of 64 samples from a 256-byte aligned allocation)."""
    has_r = R == 6 if bgr else R in (5, 6, 8, 10, 13)
    ok = bool(stream_mode) and has_r and a["w"] & 3 == 0 and (a["w"] & 255 == 0 or a["w"] & 255 > MAX_R) and a["w"] >= 512 and a["h"] >= 64
    if bgr:
        ok = ok and a["aligned"]
    if a["ds"]:
        ok = ok and R == 8 and a["h"] & 1 == 0
    return ok


def stream_grid(w, h, nb, waves):
    units_target = 1024 * waves
    nstrip = (w + 255) // 256
    nseg = (units_target + nstrip * nb - 1) // (nstrip * nb)
    L = max((h + nseg - 1) // nseg, 64)
    L = (L + 1) & ~1
    return L, nstrip, (h + L - 1) // L


def launch_blur(a, bgr, R, stream_mode, n, o, level, nbytes):
    rec = dict(octave=o, level=level, radius=R, ds=int(bool(a["ds"])), waves=0, L=0, nstrip=0, nseg=0, xsw=0, bytes=nbytes)
    if blur_streams(a, bgr, R, stream_mode):
        waves = 4 if R <= 8 else 3
        L, nstrip, nseg = stream_grid(a["w"], a["h"], n, waves)
        return dict(rec, kind=BLUR_STREAM, waves=waves, L=L, nstrip=nstrip, nseg=nseg, grid=((nstrip * nseg * n + 3) // 4, 1, 1))
    assert 2 <= R <= 16
    return dict(rec, kind=BLUR_TILE, grid=(((a["w"] + T16W - 1) // T16W) * ((a["h"] + T16H - 1) // T16H), n, 1))


def sift_run_batch(P, n, blur_stream, xstream_min_w, xstream_min_frames, aligned):
    out = []
    ds_fused = False
    for o in range(P["n_oct"]):
        oc = P["oc"][o]
        level_bytes = oc["w"] * oc["h"] * 2 * n
        if o == 0:
            a = dict(w=oc["w"], h=oc["h"], ds=False, aligned=aligned)
            out.append(launch_blur(a, True, RADIUS0, blur_stream, n, 0, 0, level_bytes + oc["w"] * oc["h"] * 3 * n))
        elif not ds_fused:
            out.append(dict(kind=DOWNSAMPLE, octave=o, level=0, radius=0, waves=0, ds=0, grid=((oc["w"] + 63) // 64, (oc["h"] + 3) // 4, n), L=0, nstrip=0, nseg=0, xsw=0,
                            bytes=level_bytes * 2))
        ds_fused = False
        for i in range(1, N_LEVELS):
            a = dict(w=oc["w"], h=oc["h"], ds=False)
            if i == N_LAYERS and o + 1 < P["n_oct"] and oc["w"] & 3 == 0 and P["oc"][o + 1]["w"] == oc["w"] >> 1 and P["oc"][o + 1]["h"] == oc["h"] >> 1:
                a["ds"] = True
                ds_fused = True
                if not blur_streams(a, False, RADIUS[i], blur_stream):
                    b = dict(a, ds=False)
                    if blur_streams(b, False, RADIUS[i], blur_stream):
                        a["ds"] = False
                        ds_fused = False
            out.append(launch_blur(a, False, RADIUS[i], blur_stream, n, o, i, level_bytes * 2))
        rec = dict(octave=o, level=-1, radius=0, waves=0, ds=0, L=0, nstrip=0, nseg=0, xsw=0, bytes=level_bytes * 6)
        xs = bool(blur_stream) and oc["w"] & 3 == 0 and oc["w"] >= xstream_min_w and oc["h"] >= xstream_min_w * 3 // 4 and n >= xstream_min_frames
        if xs:
            nstrip = (oc["w"] + XSW - 1) // XSW
            xsw = ((oc["w"] + nstrip - 1) // nstrip + 3) & ~3
            L = oc["h"]
            for k in (2, 1):
                ns = (1024 * XWAVES * k) // (nstrip * n)
                if ns < 1:
                    continue
                ll = (oc["h"] + ns - 1) // ns
                if ll >= 64 or k == 1:
                    L = max(ll, 64)
                    break
            nseg = (oc["h"] + L - 1) // L
            out.append(dict(rec, kind=EXTREMA_STREAM, grid=((nstrip * nseg * n + 3) // 4, 1, 1), L=L, nstrip=nstrip, nseg=nseg, xsw=xsw))
        else:
            out.append(dict(rec, kind=EXTREMA_TILE, grid=(((oc["w"] + EW - 1) // EW) * ((oc["h"] + EH - 1) // EH), n, 1)))
    return out


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
def _cases():
    """(tag, w, h, keepall, kmax, n, blur_stream, xstream_min_w, xstream_min_frames, aligned)"""
    frames = [(w, h, 0, 0) for w, h in SIZES] + [(w, h, 1, kmax) for w, h, kmax in KEEPALL] + [(w, h, 0, 0) for w, h, _ in REFUSED]
    out = []
    for (w, h, ka, kmax), n, bs, xw, xf, al in itertools.product(frames, (1, 3, 4, 16, 32), (0, 1), (256, 1000, 1500), (1, 4), (0, 1)):
        out.append(("%dx%d_k%d_n%d_%d_%d_%d_%d" % (w, h, kmax, n, bs, xw, xf, al), w, h, ka, kmax, n, bs, xw, xf, al))
    return out


def test_plans_equal_the_restated_host_code(driver, tmp_path):
    cases = _cases()
    assert len(cases) == 18 * 5 * 2 * 3 * 2 * 2
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        f.write("%d\n" % len(cases))
        f.writelines("%s %d %d %d %d %d %d %d %d %d\n" % c for c in cases)
    r = subprocess.run([driver, "print", str(path)], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    lines = iter(r.stdout.split("\n"))
    for i in range(N_LEVELS):
        t = next(lines).split()
        assert t[0] == "taps" and int(t[1]) == TAPS[i][0], (i, t[:2])
        assert np.array_equal(np.array(t[2:], np.float64).astype(np.float32), TAPS[i][1]), i
    assert (RADIUS0, RADIUS[1:]) == (6, [5, 6, 8, 10, 13])
    kinds, refused = set(), 0
    for tag, w, h, ka, kmax, n, bs, xw, xf, al in cases:
        head = next(lines).split()
        assert head[0] == tag, (head, tag)
        P = sift_prepare(w, h, bool(ka), kmax)
        if isinstance(P, str):
            assert " ".join(head[1:]) == "REFUSED " + P, head
            refused += 1
            continue
        got = list(map(int, head[1:]))
        want = sift_run_batch(P, n, bs, xw, xf, bool(al))
        assert got == [P["n_oct"], P["cand_cap"], P["ref_cap"], P["kp_cap"], P["cube_cap"], P["ksort_stride"]] + \
            [P["bs"][k] for k in ("pyr", "claimed", "cand", "refined", "kps", "cube", "sel", "mins")] + \
            [batch_frames(w, h, bool(ka), n, 3, 288 << 30), batch_frames(w, h, bool(ka), 40, 3, 0), len(want)], tag
        for oc in P["oc"]:
            got = list(map(int, next(lines).split()))
            assert got[:9] == [oc["w"], oc["h"]] + oc["lv"] + [oc["claimed"]] and (oc["mins"] is None or got[9] == oc["mins"]), tag
            assert all(v % 64 == 0 for v in oc["lv"]) and P["bs"]["pyr"] % 64 == 0, tag        # what blur_streams() asked of the pointers
        for k, L in enumerate(want):
            got = list(map(int, next(lines).split()))
            assert got == [L["kind"], L["octave"], L["level"], L["radius"], L["waves"], L["ds"], *L["grid"],
                           L["L"], L["nstrip"], L["nseg"], L["xsw"], L["bytes"]], (tag, k, got, L)
            kinds.add(L["kind"])
    assert refused == len(REFUSED) * len(cases) // 18 and kinds == set(range(5))


def test_invariants_over_the_sweep(driver):
    r = subprocess.run([driver, "sweep"], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0 and "SIFT_PLAN_OK" in r.stdout and not r.stderr.strip(), (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
