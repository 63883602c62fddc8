"""GPU: mi355::GetMatchedPairsOneToAllSIFT(..., window, verify, summary) through include/mi355_adaptor.h alone (tests/cxx/adaptor_verify.cpp,
built the way tests/test_gpu_adaptor_tie_refine.py builds its driver): the list is that of mi355_match_pairs, mi355_verify_pairs_results and
mi355_results_to_match_pairs applied by hand and holds the kept records' correspondences alone; a verified pair shifted by a period is no
longer kept."""
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
    exe = os.path.join(out_dir, "adaptor_verify")
    cmd = ["g++", "-std=c++11", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "adaptor_verify.cpp"),
           "-L", PKG, "-lmi355mosaic", "-Wl,-rpath," + PKG, "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_adaptor_overload_with_verification(tmp_path):
    frames, _ = strip(5, 640, 480, seed=21, overlap=0.7)          # frames k and k + 2 overlap by 40 %: the pairs close triangles
    d = str(tmp_path)
    write_images(os.path.join(d, "images.bin"), frames, [np.eye(3, dtype=np.float32).reshape(9)] * len(frames))
    r = subprocess.run([build(d), d], capture_output=True, text=True, timeout=600)
    print(r.stdout[-500:])
    assert r.returncode == 0 and "ADAPTOR VERIFY OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
