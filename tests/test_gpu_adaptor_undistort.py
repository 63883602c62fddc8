"""GPU: mi355::UndistortImage through include/mi355_adaptor.h alone (tests/cxx/adaptor_undistort.cpp, built the way
tests/test_gpu_adaptor_median.py builds its driver) gives the bytes and the count of the C ABI call: with fitted parameters, without
parameters, and in place."""
import os
import subprocess

import numpy as np
import pytest

from tests import undistort_ref as ur

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "imagemosaicing_amd")


def build(out_dir):
    exe = os.path.join(out_dir, "adaptor_undistort")
    cmd = ["g++", "-std=c++11", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "adaptor_undistort.cpp"),
           "-L", PKG, "-lmi355mosaic", "-Wl,-rpath," + PKG, "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def read_image(path):
    raw = np.fromfile(path, np.uint8)
    w, h = raw[:8].view(np.int32)
    return raw[16:].reshape(int(h), int(w), 3), int(raw[8:16].view(np.int64)[0])


def test_adaptor_undistort_equals_the_cabi_call(tmp_path):
    import imagemosaicing_amd as im
    from tests.synth import texture
    w, h = 203, 151                                               # widthStep 612: three bytes of padding per row
    img = texture(w, h, 90)
    cam = ur.cameras_for(w, h)["pincushion"]
    j, out = ur.fit(cam, w, h)
    out = (out[0] * 0.9, out[1] * 0.9, out[2], out[3])            # a little wider than fitted: some rim pixels get the fill
    d = str(tmp_path)
    with open(os.path.join(d, "frame.bin"), "wb") as f:
        f.write(np.array([w, h, 200, 0], np.int32).tobytes())
        f.write(np.array([cam[k] for k in ur.NAMES], np.float64).tobytes())
        f.write(np.array(out, np.float64).tobytes())
        f.write(img.tobytes())
    exe = build(d)
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ADAPTOR UNDISTORT OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    ctx = im.Context(0)
    cc = im.Camera(**cam)
    want, n_want = ctx.UndistortImage(img, cc, out_fx=out[0], out_fy=out[1], out_cx=out[2], out_cy=out[3], fill=200)
    own, _ = ctx.UndistortImage(img, cc)
    ctx.close()
    ref, n_ref = ur.undistort(img, cam, out, 200)
    assert n_want == n_ref > 0 and np.array_equal(want, ref)
    got, n_got = read_image(os.path.join(d, "fitted.out"))
    assert np.array_equal(got, want) and n_got == n_want
    got, n_got = read_image(os.path.join(d, "inplace.out"))
    assert np.array_equal(got, want) and n_got == n_want
    got, _ = read_image(os.path.join(d, "own.out"))
    assert np.array_equal(got, own) and (got != want).any()
