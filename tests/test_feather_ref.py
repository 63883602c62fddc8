"""CPU: weighted (feather) blending (include/mi355_mosaic.h, "weighted (feather) blending").

  * the numpy restatement (tests/feather_ref.py, built from the oracle's refined render) on the 10-frame case of tests/test_gpu_gain.py:
    single-cover pixels equal the oracle's refined canvas, every byte lies between its contributing samples, frame order changes nothing,
    two constant frames blend monotonically along a row through their overlap;
  * Wk against a direct double loop;
  * the new symbols are exported and declared, the adaptor's MosaicImagesWeighted compiles in its three modes, and the binding fails loudly
    without a context.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import feather_ref as fr
from tests import gain_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi355_default_feather_params", "mi355_mosaic_feathered_dev", "mi355_mosaic_feathered", "mi355_mosaic_feathered_into")


@pytest.fixture(scope="module")
def case(oracle):
    from tests.test_gpu_gain import _case
    imgs, h9s, _ = _case()
    return imgs, h9s, gr.frame_sample_maps(oracle, imgs, h9s)


@pytest.mark.parametrize("ramp", [0, 16])
def test_restatement_properties(case, oracle, ramp):
    imgs, h9s, maps = case
    out, layers = fr.feather_ref(oracle, imgs, h9s, ramp, maps)
    rc, (canvas, cw, ch, cws) = oracle.mosaic_images_refined(imgs, h9s)
    assert rc == 0 and out.shape == (ch, cw, 3)
    refined = canvas[:, :3 * cw].reshape(ch, cw, 3)
    single, multi = layers == 1, layers > 1
    assert single.sum() > 10000 and multi.sum() > 10000 and layers.max() >= 4
    assert np.array_equal(out[single], refined[single])                     # one frame: the refined render's byte
    assert not out[layers == 0].any()                                       # nobody: zero
    assert (out[multi] != refined[multi]).any(axis=1).mean() > 0.99         # the case does exercise the blend
    lo = np.full(out.shape, 255, np.int64)
    hi = np.zeros(out.shape, np.int64)
    for m in maps:
        if m is None:
            continue
        c = m[1][..., None]
        lo = np.where(c, np.minimum(lo, m[0]), lo)
        hi = np.where(c, np.maximum(hi, m[0]), hi)
    cov = layers > 0
    assert (out[cov] >= lo[cov]).all() and (out[cov] <= hi[cov]).all()


def test_frame_order_changes_nothing(case, oracle):
    imgs, h9s, maps = case
    out, _ = fr.feather_ref(oracle, imgs, h9s, 0, maps)
    perm = [3, 9, 0, 7, 1, 8, 5, 2, 6, 4]
    out2, _ = fr.feather_ref(oracle, [imgs[k] for k in perm], h9s[perm], 0)
    assert np.array_equal(out, out2)


def test_two_constant_frames_blend_monotonically(oracle):
    a, b = (30, 90, 200), (220, 140, 10)
    imgs = [np.empty((60, 100, 3), np.uint8), np.empty((60, 100, 3), np.uint8)]
    imgs[0][:] = a
    imgs[1][:] = b
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    h9s[1, 2] = 40.0                                                        # frame 1 shifted right: columns 40 .. 98 overlap
    out, layers = fr.feather_ref(oracle, imgs, h9s, 0)
    row = out[30].astype(int)
    both = np.flatnonzero(layers[30] == 2)
    assert len(both) > 50 and np.all(np.diff(both) == 1)
    for c in range(3):
        d = np.diff(row[both, c])
        assert (d >= 0).all() if b[c] > a[c] else (d <= 0).all(), (c, row[both, c])
        assert min(a[c], b[c]) < row[both[len(both) // 2], c] < max(a[c], b[c])
    left, right = np.flatnonzero(layers[30] == 1)[0], np.flatnonzero(layers[30] == 1)[-1]
    assert tuple(row[left]) == a and tuple(row[right]) == b


@pytest.mark.parametrize("w,h", [(2, 2), (3, 2), (2, 3), (3, 3), (17, 9), (64, 48)])
@pytest.mark.parametrize("ramp", [1, 7, 0])
def test_wk_equals_the_double_loop(w, h, ramp):
    R = ramp if ramp > 0 else (min(w, h) + 1) // 2
    want = np.zeros((h, w), np.uint8)
    for j in range(h):
        for i in range(w):
            d = min(i, w - 1 - i, j, h - 1 - j)
            want[j, i] = (254 * min(d, R)) // R
    got = fr.wk_image(w, h, ramp)
    assert np.array_equal(got, want)
    assert got.max() <= 254 and fr.ramp_of(w, h, ramp) == R >= 1


# ---- the public surface -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def im():
    from imagemosaicing_amd import build
    build.build()
    import imagemosaicing_amd
    return imagemosaicing_amd


def test_new_symbols_are_exported_and_declared(im):
    L = im.load_library()
    hdr = open(os.path.join(ROOT, "include", "mi355_mosaic.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in hdr, name
    assert "mi355_feather_params" in hdr
    for name in ("FeatherParams", "feather_params"):
        assert hasattr(im, name), name
    for name in ("MosaicFeathered", "MosaicFeatheredDev", "MosaicFeatheredInto"):
        assert hasattr(im.Context, name), name
    p = im.feather_params()
    assert C.sizeof(p) == 16 and p.ramp == 0 and list(p.reserved) == [0, 0, 0]
    assert im.feather_params(ramp=12).ramp == 12


@pytest.mark.parametrize("keep", [False, True])
def test_adaptor_weighted_compiles_as_cxx(tmp_path, keep):
    src = tmp_path / "t.cpp"
    src.write_text('#include "mi355_adaptor.h"\nusing namespace mi355ref;\n'
                   'int f(ImagePoseInfo* p, int n, ImageTransform* t, int blending) {\n'
                   '  IplImage* out = NULL;\n'
                   '  int rc = blending == 1 ? mi355::MosaicImagesWeighted(p, n, t, out) : mi355::MosaicImagesRefined(p, n, t, out);\n'
                   '  cvReleaseImage(&out); return rc; }\n'
                   'int main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-c"] + (["-DMI355_ADAPTOR_KEEP_FRAMES"] if keep else []) +
                       ["-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    syms = subprocess.run(["nm", "-C", str(tmp_path / "t.o")], capture_output=True, text=True).stdout
    assert "mi355_mosaic_feathered_into" in syms and "mi355_mosaic_refined_into" in syms


from tests.test_cabi import REF, REF_CVI  # noqa: E402  (where the reference tree sits, as the plain mode's test reads it)


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference tree")
def test_adaptor_weighted_compiles_against_the_references_own_types(tmp_path):
    """MosaicImagesWeighted with MI355_ADAPTOR_USE_REFERENCE_TYPES (and KEEP_FRAMES), against the reference's own declarations, extracted at
    test time as tests/test_frames_into_cabi.py does; nothing of the reference is kept in the repository"""
    def extract(name, ranges, out):
        txt = subprocess.run(["iconv", "-f", "GB18030", "-t", "UTF-8", os.path.join(REF, name)], capture_output=True, check=True).stdout.decode("utf-8").split("\n")
        with open(tmp_path / out, "w") as f:
            for a, b in ranges:
                f.write("\n".join(txt[a - 1:b]) + "\n")
    extract("Point.h", [(1, 10 ** 6)], "Point.h")
    extract("Bitmap.h", [(42, 45)], "projectmat.inc")
    extract("Bitmap.h", [(105, 128)], "bitmapimage.inc")
    extract("MosaicWithoutPos.h", [(135, 153)], "matchpointpairs.inc")
    extract("MosaicWithoutPos.h", [(224, 228)], "imagetransform.inc")
    extract("MosaicWithoutPos.h", [(268, 297)], "imageposeinfo.inc")
    (tmp_path / "tu.cpp").write_text(r"""
#include <vector>
#include <cstddef>
using namespace std;
#include "Point.h"
using namespace pool;
namespace pool {
#include "bitmapimage.inc"
}
#include "projectmat.inc"
#include "opencv2/core/core_c.h"
#include "opencv2/features2d/features2d.hpp"
using namespace cv;
#include "matchpointpairs.inc"
#include "imagetransform.inc"
#include "imageposeinfo.inc"
#define MI355_ADAPTOR_USE_REFERENCE_TYPES
#define MI355_ADAPTOR_KEEP_FRAMES
#include "mi355_adaptor.h"

int render(ImagePoseInfo* pImgPoses, int nImages, ImageTransform* pRectified, int m_blending) {
    IplImage* pMosaicResult = NULL;
    if (m_blending == 1) return mi355::MosaicImagesWeighted(pImgPoses, nImages, pRectified, pMosaicResult);
    return mi355::MosaicImagesRefined(pImgPoses, nImages, pRectified, pMosaicResult);
}
""")
    r = subprocess.run(["g++", "-std=c++11", "-fpermissive", "-w", "-c", "-I", str(tmp_path), "-I", REF_CVI, "-I", os.path.join(ROOT, "include"),
                        str(tmp_path / "tu.cpp"), "-o", str(tmp_path / "tu.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    syms = subprocess.run(["nm", "-C", str(tmp_path / "tu.o")], capture_output=True, text=True).stdout
    for name in ("mi355::MosaicImagesWeighted<ImagePoseInfo>", "mi355::MosaicImagesRefined<ImagePoseInfo>", "mi355_mosaic_feathered_into"):
        assert name in syms, name


def test_binding_raises_without_a_context(im):
    """a context that does not exist: every new method reaches the C ABI and fails there, loudly (no CPU path answers instead)"""
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(im.Mi355Error):
            im.Context(0)
    ctx = im.Context.__new__(im.Context)
    ctx.L, ctx._h, ctx.device = im.load_library(), C.c_void_p(), 0
    img = np.zeros((32, 32, 3), np.uint8)
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    h9s[1, 2] = 10
    for call in (lambda: ctx.MosaicFeathered([img, img], h9s),
                 lambda: ctx.MosaicFeathered([img, img], h9s, ramp=4),
                 lambda: ctx.MosaicFeatheredDev([0, 0], [32, 32], [32, 32], [96, 96], h9s, 0, 42, 32, 128),
                 lambda: ctx.MosaicFeatheredInto([img, img], None, h9s)):
        with pytest.raises(im.Mi355Error) as e:
            call()
        assert e.value.code == -1
