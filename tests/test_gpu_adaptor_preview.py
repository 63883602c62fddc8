"""GPU: mi355::MosaicImagesPreview through include/mi355_adaptor.h alone (tests/cxx/adaptor_preview.cpp, built the way
tests/test_gpu_adaptor_seamline.py builds its driver) gives the bytes of mi355_mosaic_preview_into, which are the restatement
(tests/overview_ref.py) of the full-size render under exact coverage."""
import os
import subprocess

import numpy as np
import pytest

from tests import overview_ref as ovr
from tests.test_gpu_cxx import write_images

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "imagemosaicing_amd")


def build(out_dir, keep=False):
    exe = os.path.join(out_dir, "adaptor_preview" + ("_keep" if keep else ""))
    cmd = ["g++", "-std=c++11", "-O1", "-pthread"] + (["-DMI355_ADAPTOR_KEEP_FRAMES"] if keep else []) + [
        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "adaptor_preview.cpp"),
        "-L", PKG, "-lmi355mosaic", "-Wl,-rpath," + PKG, "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def read_canvas(path):
    raw = np.fromfile(path, np.uint8)
    w, h = raw[:8].view(np.int32)
    return raw[8:].reshape(int(h), int(w), 3)


@pytest.mark.parametrize("keep", [False, True])
def test_adaptor_preview_equals_the_cabi_call(tmp_path, keep):
    import imagemosaicing_amd as im
    from tests.test_gpu_gain import _case
    imgs, h9s, _ = _case()
    d = str(tmp_path)
    write_images(os.path.join(d, "images.bin"), imgs, list(h9s))
    exe = build(d, keep)
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ADAPTOR PREVIEW OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    ctx = im.Context(0)
    full = {0: ctx.MosaicImagesRefinedInto(imgs, None, h9s), 1: ctx.MosaicFeatheredInto(imgs, None, h9s), 2: ctx.MosaicSeamlineInto(imgs, None, h9s)}
    _, cw, ch, _, owner = ctx.MosaicSeamline(imgs, h9s, want_owner=True)
    seen = []
    for render, level in ((0, 2), (1, 2), (2, 2), (2, 5)):
        got = read_canvas(os.path.join(d, "preview_r%d_l%d.out" % (render, level)))
        want, ow, oh = ctx.MosaicPreviewInto(imgs, None, h9s, render=render, level=level)
        assert got.shape == (oh, ow, 3) and np.array_equal(got, want[:, :3 * ow].reshape(oh, ow, 3)), (render, level)
        ref = ovr.overview_ref(full[render][0], cw, level, ovr.MAP, owner)[level - 1][0]          # owner > 0 is count > 0
        assert np.array_equal(got, ref[:, :3 * ow].reshape(oh, ow, 3)), (render, level)
        seen.append(got)
    assert np.array_equal(read_canvas(os.path.join(d, "preview_again.out")), seen[2])
    assert (seen[0] != seen[1]).any() and (seen[0] != seen[2]).any()                              # three renders are three previews
    ctx.close()
