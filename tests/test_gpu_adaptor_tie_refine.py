"""GPU: mi355::GetMatchedPairsOneToAllSIFT(..., window, ties) through include/mi355_adaptor.h alone (tests/cxx/adaptor_tie_refine.cpp, built the
way tests/test_gpu_adaptor_undistort.py builds its driver): ties == NULL gives the bytes of the window overload; with ties the list is that of
mi355_match_pairs, mi355_refine_ties on the kept frames and mi355_results_to_match_pairs applied by hand; without kept frames the call is
refused."""
import os
import subprocess

import numpy as np
import pytest

from tests.synth_frames import strip
from tests.test_gpu_cxx import write_images

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "imagemosaicing_amd")


def build(out_dir):
    exe = os.path.join(out_dir, "adaptor_tie_refine")
    cmd = ["g++", "-std=c++11", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "adaptor_tie_refine.cpp"),
           "-L", PKG, "-lmi355mosaic", "-Wl,-rpath," + PKG, "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_adaptor_overload_with_and_without_ties(tmp_path):
    frames, _ = strip(4, 640, 480, seed=21)
    d = str(tmp_path)
    write_images(os.path.join(d, "images.bin"), frames, [np.eye(3, dtype=np.float32).reshape(9)] * len(frames))
    r = subprocess.run([build(d), d], capture_output=True, text=True, timeout=600)
    print(r.stdout[-500:])
    assert r.returncode == 0 and "ADAPTOR TIE REFINE OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
