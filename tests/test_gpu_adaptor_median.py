"""GPU: mi355::MosaicImagesMedian through include/mi355_adaptor.h alone (tests/cxx/adaptor_median.cpp, built the way
tests/test_gpu_adaptor_seamline.py builds its driver) gives the bytes of the C ABI call, with and without kept frames -- and the adaptor's
one-pass helper still gives MosaicImagesSeamline its own canvas."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_cxx import write_images

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "imagemosaicing_amd")


def build(out_dir, keep=False):
    exe = os.path.join(out_dir, "adaptor_median" + ("_keep" if keep else ""))
    cmd = ["g++", "-std=c++11", "-O1", "-pthread"] + (["-DMI355_ADAPTOR_KEEP_FRAMES"] if keep else []) + [
        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "adaptor_median.cpp"),
        "-L", PKG, "-lmi355mosaic", "-Wl,-rpath," + PKG, "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def read_canvas(path):
    raw = np.fromfile(path, np.uint8)
    w, h = raw[:8].view(np.int32)
    return raw[8:].reshape(int(h), int(w), 3)


@pytest.mark.parametrize("keep", [False, True])
def test_adaptor_median_equals_the_cabi_call(tmp_path, keep):
    import imagemosaicing_amd as im
    from tests.test_gpu_gain import _case
    imgs, h9s, _ = _case()
    d = str(tmp_path)
    write_images(os.path.join(d, "images.bin"), imgs, list(h9s))
    exe = build(d, keep)
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ADAPTOR MEDIAN OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    ctx = im.Context(0)
    pix = lambda a: a[:, :3 * cw].reshape(ch, cw, 3)
    want, cw, ch = ctx.MosaicMedianInto(imgs, None, h9s)
    got = read_canvas(os.path.join(d, "median.out"))
    assert got.shape == (ch, cw, 3) and np.array_equal(got, pix(want))
    host, cw2, ch2, cws2 = ctx.MosaicMedian(imgs, h9s)
    assert (cw2, ch2) == (cw, ch) and np.array_equal(got, pix(host))
    seamline, _, _ = ctx.MosaicSeamlineInto(imgs, None, h9s)
    assert np.array_equal(read_canvas(os.path.join(d, "seamline.out")), pix(seamline))
    feathered, _, _ = ctx.MosaicFeatheredInto(imgs, None, h9s)
    # the median is none of the older renders
    assert (got != pix(seamline)).any() and (got != pix(feathered)).any()
    ctx.close()
