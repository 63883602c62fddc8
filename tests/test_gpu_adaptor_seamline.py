"""GPU: mi355::MosaicImagesSeamline through include/mi355_adaptor.h alone (tests/cxx/adaptor_seamline.cpp, built the way
tests/test_gpu_adaptor_frames.py builds its driver) gives the bytes of the C ABI call -- and, generalising the adaptor's one-pass helper
changed nothing for its two older wrappers: MosaicImagesWeighted and MosaicImagesRefined still give the bytes of their C ABI calls."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_cxx import write_images

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "imagemosaicing_amd")


def build(out_dir, keep=False):
    exe = os.path.join(out_dir, "adaptor_seamline" + ("_keep" if keep else ""))
    cmd = ["g++", "-std=c++11", "-O1", "-pthread"] + (["-DMI355_ADAPTOR_KEEP_FRAMES"] if keep else []) + [
        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "adaptor_seamline.cpp"),
        "-L", PKG, "-lmi355mosaic", "-Wl,-rpath," + PKG, "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def read_canvas(path):
    raw = np.fromfile(path, np.uint8)
    w, h = raw[:8].view(np.int32)
    return raw[8:].reshape(int(h), int(w), 3)


@pytest.mark.parametrize("keep", [False, True])
def test_adaptor_seamline_equals_the_cabi_call(tmp_path, keep):
    import imagemosaicing_amd as im
    from tests.test_gpu_gain import _case
    imgs, h9s, _ = _case()
    d = str(tmp_path)
    write_images(os.path.join(d, "images.bin"), imgs, list(h9s))
    exe = build(d, keep)
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ADAPTOR SEAMLINE OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    ctx = im.Context(0)
    want, cw, ch = ctx.MosaicSeamlineInto(imgs, None, h9s)
    got = read_canvas(os.path.join(d, "seamline.out"))
    assert got.shape == (ch, cw, 3) and np.array_equal(got, want[:, :3 * cw].reshape(ch, cw, 3))
    host, cw2, ch2, cws2 = ctx.MosaicSeamline(imgs, h9s)
    assert (cw2, ch2) == (cw, ch) and np.array_equal(got, host[:, :3 * cw].reshape(ch, cw, 3))
    feathered, _, _ = ctx.MosaicFeatheredInto(imgs, None, h9s)
    refined, _, _ = ctx.MosaicImagesRefinedInto(imgs, None, h9s)
    assert np.array_equal(read_canvas(os.path.join(d, "weighted.out")), feathered[:, :3 * cw].reshape(ch, cw, 3))
    assert np.array_equal(read_canvas(os.path.join(d, "refined.out")), refined[:, :3 * cw].reshape(ch, cw, 3))
    # the three renders are three renders
    assert (got != refined[:, :3 * cw].reshape(ch, cw, 3)).any() and (got != feathered[:, :3 * cw].reshape(ch, cw, 3)).any()
    ctx.close()
