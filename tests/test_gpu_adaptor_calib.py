"""mi355::CalibrateLens through include/mi355_adaptor.h alone (tests/cxx/adaptor_calib.cpp, built the way tests/test_adaptor_projective.py
builds its driver) gives the bits of the flat-list call of the Python binding, on grid16's list.  The call itself is host only; the test
runs with the GPU suite, beside the stage's other tests."""
import os
import subprocess

import numpy as np
import pytest

import imagemosaicing_amd as im
from tests import calib_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "imagemosaicing_amd")


def build(out_dir):
    exe = os.path.join(out_dir, "adaptor_calib")
    cmd = ["g++", "-std=c++11", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "adaptor_calib.cpp"),
           "-L", PKG, "-lmi355mosaic", "-Wl,-rpath," + PKG, "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def read_out(path):
    raw = open(path, "rb").read()
    cam = im.Camera.from_buffer_copy(raw[:72])
    return cam, im.CalibReport.from_buffer_copy(raw[72:]).as_dict()


def test_adaptor_calibration_equals_the_flat_list_call(tmp_path):
    flat = im.results_to_match_pairs(cc.survey("grid16", 0.5))
    start = im.Camera(*cc.CAM_START)
    d = str(tmp_path)
    with open(os.path.join(d, "calib.bin"), "wb") as f:
        f.write(np.array([len(flat), 15, 0, 0], np.int32).tobytes())
        f.write(bytes(start))
        f.write(flat.tobytes())
    exe = build(d)
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ADAPTOR CALIB OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    want, wrep = im.calibrate_lens(flat, start, mask=15)
    got, grep_ = read_out(os.path.join(d, "calib.out"))
    assert bytes(got) == bytes(want) and grep_ == wrep and wrep["accepted"] >= 3 and got.p1 != 0.0
    want2, _ = im.calibrate_lens(flat, start)
    got2, _ = read_out(os.path.join(d, "calib_default.out"))
    assert bytes(got2) == bytes(want2) and got2.p1 == 0.0 and abs(got2.k1 - cc.CAM_TRUE[4]) < 0.01
