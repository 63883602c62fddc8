"""CPU: the kept-frame / render-into-caller-memory surface (mi355_drop_frames, mi355_get_frame_dev, mi355_mosaic_refined_into,
mi355_mosaic_blended_into) is exported, the adaptor's MI355_ADAPTOR_KEEP_FRAMES mode compiles on its own types and on the reference's,
and the binding fails loudly without a device."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi355_drop_frames", "mi355_get_frame_dev", "mi355_mosaic_refined_into", "mi355_mosaic_blended_into")


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


@pytest.mark.parametrize("keep", [False, True])
def test_adaptor_keep_frames_compiles_as_cxx(tmp_path, keep):
    src = tmp_path / "t.cpp"
    src.write_text('#include "mi355_adaptor.h"\nusing namespace mi355ref;\n'
                   'int f(ImagePoseInfo* p, int n, ImageTransform* t, IplImage** imgs, ProjectMat* m) {\n'
                   '  std::vector<MatchPointPairs> v; int ns = 0; IplImage* out = NULL;\n'
                   '  int rc = mi355::GetMatchedPairsOneToAllSIFT_MultiThread(p, n, v, ns) + mi355::GetMatchedPairsOneToAllSurf(p, n, v, ns);\n'
                   '  rc += mi355::MosaicImagesRefined(p, n, t, out) + mi355::MergeImagesRefined(p, n, t, 1.0f, out);\n'
                   '  IplImage* b = mi355::LaplacianPyramidBlending(imgs, n, m, 5, 1.0f); cvReleaseImage(&b); return rc; }\n'
                   'int main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only"] + (["-DMI355_ADAPTOR_KEEP_FRAMES"] if keep else []) +
                       ["-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


from tests.test_cabi import REF, REF_CVI  # noqa: E402  (where the reference tree sits, as the plain mode's test reads it)


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference tree")
def test_adaptor_keep_frames_compiles_against_the_references_own_types(tmp_path):
    """MI355_ADAPTOR_KEEP_FRAMES together with MI355_ADAPTOR_USE_REFERENCE_TYPES, against the reference's own declarations (extracted at
    test time, as test_cabi.py's test of the plain mode does; nothing of the reference is kept in the repo)"""
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

int sequence(ImagePoseInfo* pImgPoses, int nImages, ImageTransform* pRectified, IplImage** pImages, ProjectMat* pImgT) {
    vector<MatchPointPairs> vecMatchPairs; int nSuccess = 0;
    int rc = mi355::GetMatchedPairsOneToAllSIFT_MultiThread(pImgPoses, nImages, vecMatchPairs, nSuccess, 2.5f);
    rc += mi355::GetMatchedPairsOneToAllSurf(pImgPoses, nImages, vecMatchPairs, nSuccess);
    IplImage* pMosaicResult = NULL;
    rc += mi355::MosaicImagesRefined(pImgPoses, nImages, pRectified, pMosaicResult);
    rc += mi355::MergeImagesRefined(pImgPoses, nImages, pRectified, 1.0f, pMosaicResult);
    IplImage* blended = mi355::LaplacianPyramidBlending(pImages, nImages, pImgT, 5, 1.0f);
    cvReleaseImage(&blended);
    return rc;
}
""")
    r = subprocess.run(["g++", "-std=c++11", "-fpermissive", "-w", "-c", "-I", str(tmp_path), "-I", REF_CVI, "-I", os.path.join(ROOT, "include"),
                        str(tmp_path / "tu.cpp"), "-o", str(tmp_path / "tu.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    syms = subprocess.run(["nm", "-C", str(tmp_path / "tu.o")], capture_output=True, text=True).stdout
    for name in ("mi355::MosaicImagesRefined<ImagePoseInfo>", "mi355::LaplacianPyramidBlending", "mi355::detail::record_frame", "mi355_mosaic_refined_into",
                 "mi355_mosaic_blended_into", "mi355_drop_frames"):
        assert name in syms, name


def test_binding_raises_without_a_device(im):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(im.Mi355Error):
        im.Context(0)
    # a context that could not be created: every new method reaches the C ABI and fails there, loudly
    ctx = im.Context.__new__(im.Context)
    import ctypes as C
    ctx.L, ctx._h, ctx.device = im.load_library(), C.c_void_p(), 0
    img = np.zeros((32, 32, 3), np.uint8)
    h9s = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    h9s[1, 2] = 10
    for call in (lambda: ctx.DropFrames(-1), lambda: ctx.FrameDev(0),
                 lambda: ctx.MosaicImagesRefinedInto([img, img], None, h9s),
                 lambda: ctx.MosaicBlendedInto([img, img], None, h9s)):
        with pytest.raises(im.Mi355Error) as e:
            call()
        assert e.value.code == -1
