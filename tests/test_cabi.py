"""CPU: the C-ABI library loads and exports every symbol include/mi355_mosaic.h declares; host-only entry
points (formats, schedule, global alignment known answer) work without a GPU."""
import os
import re
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def im():
    from imagemosaicing_amd import build
    build.build()
    import imagemosaicing_amd
    return imagemosaicing_amd


def test_every_declared_symbol_is_exported(im):
    hdr = open(os.path.join(ROOT, "include", "mi355_mosaic.h")).read()
    names = sorted(set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 30
    L = im.load_library()
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


def test_no_device_fails_loudly(im):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(im.Mi355Error) as e:
        im.Context(0)
    assert e.value.code == -4


def test_match_pairs_file_roundtrip_is_byte_identical(im, tmp_path):
    src = os.path.join(GOLD, "matchPairs.match")
    rec = im.load_match_pairs(src)
    assert len(rec) == 5918
    out = str(tmp_path / "mp.match")
    im.write_match_pairs(out, rec)
    assert open(out, "rb").read() == open(src, "rb").read()


def test_match_pairs_txt_matches_reference_file(im, tmp_path):
    """WriteMatchPairs_ASC2 formatting (MosaicWithoutPos.cpp:4751-4772): re-writing the values parsed from
    the reference's own matchPairs.txt reproduces the file (modulo the CRLF of the Windows build)."""
    src = os.path.join(GOLD, "matchPairs.txt")
    txt = np.loadtxt(src)
    mp = np.zeros(len(txt), im.MATCHPAIR)
    for k, f in enumerate(["ai", "ax", "ay", "af", "bi", "bx", "by", "bf"]):
        mp[f] = txt[:, k]
    out = str(tmp_path / "mp.txt")
    im.write_match_pairs_txt(out, mp)
    want = open(src, "rb").read().replace(b"\r\n", b"\n")
    assert open(out, "rb").read() == want


def test_global_affine_align_known_answer(im, tmp_path):
    """matchPairs.txt -> tran0.txt, the one known-answer fixture of the reference."""
    txt = np.loadtxt(os.path.join(GOLD, "matchPairs.txt"))
    mp = np.zeros(len(txt), im.MATCHPAIR)
    for k, f in enumerate(["ai", "ax", "ay", "af", "bi", "bx", "by", "bf"]):
        mp[f] = txt[:, k]
    T = im.global_affine_align(mp, 20)
    want = np.loadtxt(os.path.join(GOLD, "tran0.txt"))
    assert T["fixed"][0] == 1 and np.array_equal(T["m"][0], np.eye(3, dtype=np.float32).reshape(9))
    assert np.abs(T["m"][1:, :6] - want[:, :6]).max() < 6e-3       # 6 significant digits in the text file
    out = str(tmp_path / "tran.txt")
    im.write_transforms(out, T)
    got = np.loadtxt(out)
    assert got.shape == want.shape and np.abs(got[:, :6] - want[:, :6]).max() < 6e-3


def test_keypoint_file_roundtrip(im, tmp_path):
    kp = np.zeros(5, im.KEYPOINT)
    kp["x"] = np.arange(5) + 0.5
    kp["octave"] = 0x01ff00
    p = str(tmp_path / "keypoint_0.key")
    im.write_keypoints(p, kp)
    raw = open(p, "rb").read()
    assert len(raw) == 4 + 5 * 28 and np.frombuffer(raw[:4], np.int32)[0] == 5
    assert np.array_equal(im.load_keypoints(p), kp)


def test_pair_schedule_matches_reference_window(im):
    # MosaicWithoutPos.cpp:5066,5083: i strided by thread, j in (i, min(N, i+182))
    allp = im.pair_schedule(500, 182)
    assert len(allp) == 74029
    parts = [im.pair_schedule(500, 182, r, 8) for r in range(8)]
    assert sum(len(p) for p in parts) == 74029
    merged = np.concatenate(parts)
    assert len({(int(a), int(b)) for a, b in merged}) == 74029
    assert all((p[:, 0] % 8 == r).all() for r, p in enumerate(parts))
    assert len(im.pair_schedule(2000, 182)) == 345529   # C5


def test_mosaic_layout_matches_oracle(im, oracle):
    from tests.synth import mosaic_case
    imgs, h9s = mosaic_case()
    w = [i.shape[1] for i in imgs]; h = [i.shape[0] for i in imgs]
    cw, ch, cws, dG = im.mosaic_layout(w, h, h9s)
    rc, (canvas, ow, oh, ows) = oracle.mosaic_images_refined(imgs, h9s)
    assert (cw, ch, cws) == (ow, oh, ows)


def test_results_to_match_pairs(im):
    r = np.zeros(3, im.PAIR_RESULT)
    r["i"] = [0, 0, 1]; r["j"] = [1, 2, 2]; r["n_in"] = [40, 10, 35]; r["accepted"] = [1, 0, 1]
    r["a"]["x"][0, :40] = np.arange(40); r["b"]["id"][2, :35] = np.arange(35)
    v = im.results_to_match_pairs(r, fixed_flags=[1, 0, 0])
    assert len(v) == 75 and (v["ai"][:40] == 0).all() and (v["af"][:40] == 1).all() and (v["bi"][40:] == 2).all()
    assert np.array_equal(v["ax"][:40], np.arange(40, dtype=np.float32)) and np.array_equal(v["bid"][40:], np.arange(35))


def test_transform_files_roundtrip(im, tmp_path):
    """tran0.txt as OutTransform writes it (MosaicWithoutPos.cpp:2798-2818) reads back, and ImportTransform's own format (:2820-2843)"""
    T = im.load_transforms(os.path.join(GOLD, "tran0.txt"), tran0=True)
    want = np.loadtxt(os.path.join(GOLD, "tran0.txt"))
    assert len(T) == 20 and T["fixed"][0] == 1 and np.array_equal(T["m"][0], np.eye(3, dtype=np.float32).reshape(9))
    assert np.array_equal(T["m"][1:, :8], want[:, :8].astype(np.float32)) and (T["m"][:, 8] == 1).all()
    assert np.array_equal(T["fixed"][1:], want[:, 8].astype(np.int32))
    out = str(tmp_path / "t.txt")
    im.write_transforms(out, T)
    assert np.array_equal(np.loadtxt(out), want)
    p = str(tmp_path / "refine.txt")
    vals = np.arange(27, dtype=np.float32).reshape(3, 9) * 0.5
    open(p, "w").write("3\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in vals) + "\n")
    R = im.load_transforms(p)
    assert len(R) == 3 and R["fixed"].tolist() == [1, 0, 0] and np.array_equal(R["m"], vals)


def test_adaptor_driver_compiles_and_links(tmp_path):
    """tests/cxx/adaptor_driver.cpp (a C++ caller of every adaptor entry point) builds and links against the library here; it is RUN
    on the GPU box by tests/test_gpu_cxx.py"""
    from tests.test_gpu_cxx import build_driver
    exe = build_driver(str(tmp_path))
    import subprocess
    r = subprocess.run([exe, str(tmp_path), "ransac"], capture_output=True, text=True)
    import torch
    if torch.cuda.is_available():
        # a GPU here: the context is created, and the run stops at its first input, which this test does not write
        assert r.returncode == 3 and "cannot open" in r.stderr and "ransac.bin" in r.stderr, (r.returncode, r.stderr[-2000:])
    else:
        assert r.returncode == 5 and "no context" in r.stderr          # no GPU here: fails loudly, no CPU path


def test_adaptor_header_compiles_as_cxx(tmp_path):
    """include/mi355_adaptor.h (the reference's own signatures over the C ABI) is valid stand-alone C++"""
    import subprocess
    src = tmp_path / "t.cpp"
    src.write_text('#include "mi355_adaptor.h"\nint main() { std::vector<mi355ref::SfPoint> a, b, c, d; float H[9];'
                   ' return mi355::Ransac2D(a, b, c, d, H, 2.5f) ? 1 : 0; }\n')
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


REF = "/root/reference/code/MosaicingCode/mosaicing"
REF_CVI = "/root/reference/code/MosaicingCode/3rdparty/opencv240/opencv/build/include"


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs /root/reference (this container only)")
def test_adaptor_compiles_against_the_references_own_types(tmp_path):
    """Row b's proof (VERDICT r05 next #1c): include/mi355_adaptor.h in the mode INTEGRATION.md prescribes,
    MI355_ADAPTOR_USE_REFERENCE_TYPES, compiled against the REFERENCE'S OWN declarations -- Point.h whole, Bitmap.h:42-45 (ProjectMat),
    :105-128 (pool::BitmapImage), MosaicWithoutPos.h:135-153 (MatchPointPairs), :224-228 (ImageTransform), :268-297 (CameraPose64F,
    ImagePoseInfo), ImageIO.cpp:78-93 (ReleaseBitmap8U) and the OpenCV 2.4.0 headers vendored in the reference tree (IplImage,
    cvCreateImage / cvReleaseImage, cv::DMatch, cv::KeyPoint) -- with EVERY adaptor entry point instantiated the way the reference's call
    sites spell them.  The ranges are extracted into tmp_path at test time (the build_ref.sh pattern: nothing of the reference is kept
    in the repo); the TU is compiled to an object (no OpenCV library exists here to link against)."""
    import subprocess
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
    extract("ImageIO.cpp", [(78, 93)], "releasebitmap.inc")
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
#include "opencv2/core/core_c.h"                 // IplImage, cvCreateImage, cvSize, cvReleaseImage, CvPoint3D64f
#include "opencv2/features2d/features2d.hpp"     // cv::DMatch, cv::KeyPoint
using namespace cv;
#include "matchpointpairs.inc"
#include "imagetransform.inc"
#include "imageposeinfo.inc"
#include "releasebitmap.inc"                     // the reference's own ReleaseBitmap8U (delete[] imageData; delete)
#define MI355_ADAPTOR_USE_REFERENCE_TYPES
#include "mi355_adaptor.h"

int every_entry_point(ImagePoseInfo* pImgPoses, int nImages, ImageTransform* pRectified, IplImage** pImages, ProjectMat* pImgT) {
    int rc = 0;
    // mosaicimage.h:1729-1735, called as MosaicWithoutPos.cpp:5168-5169
    vector<SfPoint> vecMatch1, vecMatch2, vecInner1, vecInner2; float aProjectMat[9];
    rc += mi355::Ransac2D(vecMatch1, vecMatch2, vecInner1, vecInner2, aProjectMat, 2.5f, 1000) ? 1 : 0;
    // MosaicWithoutPos.cpp:4977-4983, called as :5146-5153
    vector<DMatch> matches; vector<KeyPoint> keypoints1, keypoints2;
    rc += mi355::SelectMatchPairs(matches, keypoints1, keypoints2, 400, 4000, 3000, 3, 3, vecMatch1, vecMatch2);
    // MosaicImage.cpp:1613, result released the reference's way (ImageIO.cpp:78-93)
    pool::BitmapImage src, *pResult = NULL; float h[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    rc += mi355::ImageProjectionTransform(&src, pResult, h);
    ReleaseBitmap8U(pResult);
    // MosaicWithoutPos.cpp:5244-5295 / :5300-5533
    vector<MatchPointPairs> vecMatchPairs; int nSuccess = 0;
    rc += mi355::GetMatchedPairsOneToAllSIFT_MultiThread(pImgPoses, nImages, vecMatchPairs, nSuccess, 2.5f);
    rc += mi355::GetMatchedPairsOneToAllSurf(pImgPoses, nImages, vecMatchPairs, nSuccess);
    int fixedFlags[1] = {1};
    rc += mi355::GetMatchedPairsOneToAllSIFT(nImages, 2.5f, 1u, fixedFlags, vecMatchPairs);
    // MosaicWithoutPos.cpp:2194 / :2161, MosaicImage.cpp:2205
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
    for name in ("mi355::Ransac2D", "mi355::SelectMatchPairs<cv::DMatch, cv::KeyPoint>", "mi355::ImageProjectionTransform", "ReleaseBitmap8U",
                 "mi355::GetMatchedPairsOneToAllSIFT_MultiThread<ImagePoseInfo>", "mi355::GetMatchedPairsOneToAllSurf<ImagePoseInfo>",
                 "mi355::MosaicImagesRefined<ImagePoseInfo>", "mi355::MergeImagesRefined<ImagePoseInfo>", "mi355::LaplacianPyramidBlending"):
        assert name in syms, name


def test_global_affine_align_recovers_synthetic_surveys(im):
    """exact correspondences of randomly placed images (affine maps into a common plane, random overlap graph, some images
    isolated and therefore fixed): the solver must return the ground-truth maps relative to image 0"""
    rng = np.random.default_rng(12)
    for trial in range(6):
        N = int(rng.integers(3, 60))
        A = []
        for k in range(N):
            th = rng.normal(0, 0.05); s = 1 + rng.normal(0, 0.03)
            A.append(np.array([[s * np.cos(th), -s * np.sin(th) + rng.normal(0, 0.01), rng.uniform(-3000, 3000)],
                               [s * np.sin(th), s * np.cos(th), rng.uniform(-3000, 3000)], [0, 0, 1]]))
        A[0] = np.eye(3)
        edges = [(i, i + 1) for i in range(N - 2)] + [tuple(sorted(rng.choice(N - 1, 2, replace=False))) for _ in range(N)]     # image N-1 stays isolated
        rows = []
        for (i, j) in edges:
            if i == j:
                continue
            m = int(rng.integers(4, 40))
            world = np.stack([rng.uniform(-4000, 4000, m), rng.uniform(-4000, 4000, m), np.ones(m)])
            pa = np.linalg.inv(A[i]) @ world; pb = np.linalg.inv(A[j]) @ world
            for q in range(m):
                rows.append((pa[0, q], pa[1, q], q, i, 0, pb[0, q], pb[1, q], q, j, 0))
        mp = np.array(rows, dtype=im.MATCHPAIR)
        label = im.select_connected(mp, N)
        assert label[N - 1] == 0 and label[:N - 1].all()
        keep = (label[mp["ai"]] > 0) & (label[mp["bi"]] > 0)
        fixed = [1 if (k == 0 or label[k] == 0) else 0 for k in range(N)]
        T = im.global_affine_align(mp[keep], N, fixed=fixed)
        got = T["m"][:, :6].astype(np.float64).reshape(N, 2, 3)
        for k in range(N - 1):
            assert np.abs(got[k] - A[k][:2]).max() < 2e-2 * max(1.0, np.abs(A[k][:2]).max() / 1000), (trial, k, got[k], A[k][:2])
        assert np.array_equal(T["m"][N - 1], np.eye(3, dtype=np.float32).reshape(9))      # a fixed (isolated) image stays at identity


def test_alignment_from_pair_records_equals_the_match_pairs_form(im):
    """mi355_select_connected_results / mi355_global_affine_align_results (straight from PAIR_RESULT records, host threads) give the
    labels and the transforms of the m_vecMatchPairs forms bit for bit: rejected records and a second, smaller component included; a
    survey large enough for the threaded moments and the threaded banded Cholesky (2000 images, band of 90 image blocks)"""
    rng = np.random.default_rng(3)
    for (N, per, K) in [(40, 7, 60), (2000, 45, 110)]:
        pos = np.stack([(np.arange(N) % per) * 400.0, (np.arange(N) // per) * 300.0], 1)
        pairs = [(i, i + d) for i in range(N - 3) for d in (1, per - 1, per, per + 1, 2 * per) if i + d < N - 3 and abs(pos[i, 0] - pos[i + d, 0]) < 1500]
        pairs.append((N - 2, N - 1))                                  # a component of two images: labelled 0, its pair dropped
        r = np.zeros(len(pairs) + 5, im.PAIR_RESULT)
        for p, (a, b) in enumerate(pairs):
            n = int(rng.integers(31, K))
            r["i"][p] = a; r["j"][p] = b; r["accepted"][p] = 1; r["n_in"][p] = n
            xa = rng.uniform(0, 4000, n).astype(np.float32); ya = rng.uniform(0, 3000, n).astype(np.float32)
            r["a"]["x"][p, :n] = xa; r["a"]["y"][p, :n] = ya
            r["b"]["x"][p, :n] = xa + np.float32(pos[a, 0] - pos[b, 0]) + rng.normal(0, 0.3, n).astype(np.float32)
            r["b"]["y"][p, :n] = ya + np.float32(pos[a, 1] - pos[b, 1]) + rng.normal(0, 0.3, n).astype(np.float32)
        r["i"][len(pairs):] = 0; r["j"][len(pairs):] = N - 1; r["n_in"][len(pairs):] = 12          # rejected records: no edge, no equations
        mp = im.results_to_match_pairs(r)
        label = im.select_connected(mp, N)
        assert label[N - 1] == 0 and label[N - 2] == 0 and label[:N - 3].all()
        assert np.array_equal(im.select_connected_results(r, N), label)
        keep = (label[mp["ai"]] > 0) & (label[mp["bi"]] > 0)
        fixed = [1 if (k == 0 or label[k] == 0) else 0 for k in range(N)]
        T = im.global_affine_align(mp[keep], N, fixed=fixed)
        T2 = im.global_affine_align_results(r, N, fixed=fixed, label=label)
        assert np.array_equal(T.view(np.uint8), T2.view(np.uint8))
        assert np.abs(T["m"][N // 2, [2, 5]] - pos[N // 2]).max() < 5.0          # noisy correspondences, a chain of ~20 rows of images


def test_alignment_bits_do_not_depend_on_the_thread_count(tmp_path):
    """the banded Cholesky of mi355_global_affine_align_results works in panels of 64 columns on a team of host threads; every entry still
    receives its products one by one in ascending order, so the transforms have the same bits on 1, 3 and 7 threads (fresh processes:
    the thread count is read once).  Two systems: a window-120 survey (half bandwidth 362 > panel) and an adjacent-pair strip (5 < panel)."""
    import hashlib
    import subprocess
    import sys
    script = tmp_path / "align_threads.py"
    script.write_text(
        "import sys, hashlib, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import imagemosaicing_amd as im\n"
        "out = []\n"
        "for (N, win, frac) in [(260, 120, 0.06), (300, 2, 1.0)]:\n"
        "    rng = np.random.default_rng(N)\n"
        "    pairs = [(i, j) for i in range(N) for j in range(i + 1, min(N, i + win)) if (j == i + 1 or rng.random() < frac)]\n"
        "    r = np.zeros(len(pairs), im.PAIR_RESULT)\n"
        "    pos = np.cumsum(rng.uniform(300, 900, (N, 2)), axis=0)\n"
        "    for k, (i, j) in enumerate(pairs):\n"
        "        n = 400 if win > 2 else 60\n"
        "        xy = rng.uniform(0, 4000, (n, 2)).astype(np.float32)\n"
        "        r['i'][k] = i; r['j'][k] = j; r['n_in'][k] = n; r['accepted'][k] = 1\n"
        "        r['a']['x'][k, :n] = xy[:, 0] + (pos[j, 0] - pos[i, 0]); r['a']['y'][k, :n] = xy[:, 1] + (pos[j, 1] - pos[i, 1])\n"
        "        r['b']['x'][k, :n] = xy[:, 0] + rng.normal(0, .3, n); r['b']['y'][k, :n] = xy[:, 1] + rng.normal(0, .3, n)\n"
        "    T = im.global_affine_align_results(r, N)\n"
        "    assert np.isfinite(T['m']).all() and (win == 2 or np.abs(T['m'][:, 2] - (pos[:, 0] - pos[0, 0])).max() < 2.0)   # (a 300-link chain of free affines drifts)\n"
        "    out.append(hashlib.sha1(T['m'].tobytes()).hexdigest())\n"
        "print(' '.join(out))\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    seen = set()
    for th in ("1", "3", "7"):
        r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, MI355_HOST_THREADS=th), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        seen.add(r.stdout.strip().splitlines()[-1])
    assert len(seen) == 1, seen


def test_descriptor_xml_layout_and_round_trip(tmp_path):
    """discriptor_%d.xml, the cv::FileStorage half of WriteSurfKeyPoints / LoadSurfKeyPoints (MosaicWithoutPos.cpp:4685-4688, 4710-4711).  The
    reference commits no such file: the layout is OpenCV 2.4's XML emitter as restated in host_io.cpp (UNPINNED) -- integers as "12.", other
    floats "%.8e", data lines of at most 72 characters indented by 4, closing tags behind the last number -- and the reader takes any
    white-space-separated numbers, so a file cv::FileStorage wrote reads whatever its wrapping."""
    import imagemosaicing_amd as im
    small = np.array([[0, 12, 255, 0.5], [3, -7, 1e-3, 16777216]], np.float32)
    p = str(tmp_path / "discriptor_0.xml")
    im.write_descriptors_xml(p, small)
    text = open(p).read()
    assert text == ('<?xml version="1.0"?>\n<opencv_storage>\n<descriptor type_id="opencv-matrix">\n  <rows>2</rows>\n  <cols>4</cols>\n  <dt>f</dt>\n  <data>\n'
                    '    0. 12. 255. 5.00000000e-01 3. -7. 1.00000005e-03 16777216.</data></descriptor>\n</opencv_storage>\n')
    assert np.array_equal(im.load_descriptors_xml(p), small)
    rng = np.random.default_rng(2)
    d = rng.integers(0, 256, (300, 128)).astype(np.float32)                 # SIFT: byte-valued floats
    d[7, 5] = np.float32(1.0) / 3; d[9, 0] = np.inf; d[9, 1] = -np.inf
    im.write_descriptors_xml(p, d)
    lines = open(p).read().split("\n")
    data = lines[7:-2]
    assert all(l.startswith("    ") and not l.startswith("     ") for l in data) and max(len(l) for l in data[:-1]) <= 72 and min(len(l) for l in data[:-1]) >= 60
    back = im.load_descriptors_xml(p)
    assert back.shape == d.shape and np.array_equal(back.view(np.uint32), d.view(np.uint32))
    # a file wrapped differently (and with OpenCV's header comment) reads the same
    with open(p, "w") as f:
        f.write('<?xml version="1.0"?>\n<opencv_storage>\n<descriptor type_id="opencv-matrix">\n<rows>2</rows><cols>4</cols><dt>f</dt>\n<data>\n0. 12.\n 255.\t5.00000000e-01 3. -7. 1.00000005e-03\n16777216.\n</data></descriptor></opencv_storage>\n')
    assert np.array_equal(im.load_descriptors_xml(p), small)
    im.write_descriptors_xml(p, np.zeros((0, 128), np.float32))
    assert im.load_descriptors_xml(p).shape == (0, 128)
    with pytest.raises(im.Mi355Error):
        im.load_descriptors_xml(str(tmp_path / "missing.xml"))
