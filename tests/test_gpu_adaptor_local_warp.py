"""GPU: mi355::LocalRegistration through include/mi355_adaptor.h alone (tests/cxx/adaptor_local_warp.cpp, built with
MI355_ADAPTOR_KEEP_FRAMES the way tests/test_gpu_adaptor_tie_refine.py builds its driver): refused without kept frames; its grids are those of
mi355_tie_residual_stats_host and mi355_solve_local_warps on records cut by hand; the render after it equals mi355_local_register_results and
mi355_mosaic_refined_into applied by hand to second copies of the frames and differs from the render before it; host images stay unchanged."""
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
    exe = os.path.join(out_dir, "adaptor_local_warp")
    cmd = ["g++", "-std=c++11", "-O1", "-pthread", "-DMI355_ADAPTOR_KEEP_FRAMES", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cxx", "adaptor_local_warp.cpp"), "-L", PKG, "-lmi355mosaic", "-Wl,-rpath," + PKG, "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_adaptor_local_registration(tmp_path):
    frames, _ = strip(4, 640, 480, seed=21)
    d = str(tmp_path)
    write_images(os.path.join(d, "images.bin"), frames, [np.eye(3, dtype=np.float32).reshape(9)] * len(frames))
    r = subprocess.run([build(d), d], capture_output=True, text=True, timeout=600)
    print(r.stdout[-500:])
    assert r.returncode == 0 and "ADAPTOR LOCAL WARP OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
