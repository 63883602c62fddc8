// include/mi355_adaptor.h -- header-only C++ adaptor: the reference's OWN per-pair function signatures,
// forwarded to libmi355mosaic.so (include/mi355_mosaic.h).  A maintainer of YuhuaXu/ImageMosaicing includes
// this header instead of calling the CPU implementations; the driver code (CMosaicByPose::MosaicWithoutPose,
// MosaicWithoutPos.cpp:4430-4679) stays as it is.  See INTEGRATION.md for the exact edit.
//
// The adaptor is written against the reference's POD layouts (Point.h:27-47 SfPoint, Bitmap.h:42-45 ProjectMat,
// Bitmap.h:105-128 BitmapImage, MosaicWithoutPos.h:135-153 MatchPointPairs, :224-228 ImageTransform).  When it
// is compiled INSIDE the reference tree those types already exist: define MI355_ADAPTOR_USE_REFERENCE_TYPES
// before including it.  Stand-alone (this repo's tests) it declares layout-identical types in namespace
// mi355ref.
#pragma once
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>
#include "mi355_mosaic.h"
// Needs a C++11 compiler (std::call_once guards the process-wide context; the reference's VS2008 project moves to VS2012+).

#ifndef MI355_ADAPTOR_USE_REFERENCE_TYPES
namespace mi355ref {
struct SfPoint { float x, y; int id; SfPoint() {} SfPoint(float x_, float y_) : x(x_), y(y_), id(0) {} };   // Point.h:27-47
struct ProjectMat { float m[9]; };                                                                           // Bitmap.h:42-45
struct BitmapImage {                                                                                         // Bitmap.h:105-128
    unsigned char* imageData; int width, height, widthStep, nChannels;
    BitmapImage() : imageData(NULL), width(0), height(0), widthStep(0), nChannels(0) {}
};
inline void ReleaseBitmap8U(BitmapImage*& p) { if (!p) return; delete[] p->imageData; p->imageData = NULL; delete p; p = NULL; }      // ImageIO.cpp:78-93
struct MatchPointPairs { SfPoint ptA; int ptA_i, ptA_Fixed; SfPoint ptB; int ptB_i, ptB_Fixed; };            // MosaicWithoutPos.h:135-153
struct ImageTransform { ProjectMat h; int fixed; };                                                          // MosaicWithoutPos.h:224-228
// IplImage, OpenCV 2.4.0 core/types_c.h (field for field); stand-alone images own imageData through malloc
struct IplImage {
    int nSize, ID, nChannels, alphaChannel, depth; char colorModel[4], channelSeq[4];
    int dataOrder, origin, align, width, height; void* roi; void* maskROI; void* imageId; void* tileInfo;
    int imageSize; char* imageData; int widthStep; int BorderMode[4], BorderConst[4]; char* imageDataOrigin;
};
inline IplImage* cvCreateImage8U(int w, int h, int ch) {              // cvCreateImage(cvSize(w, h), 8, ch): rows aligned to 4 bytes
    IplImage* im = (IplImage*)std::calloc(1, sizeof(IplImage));
    if (!im) return NULL;
    im->nSize = (int)sizeof(IplImage); im->nChannels = ch; im->depth = 8; im->width = w; im->height = h; im->align = 4;
    im->widthStep = (w * ch + 3) & ~3; im->imageSize = im->widthStep * h;
    im->imageData = im->imageDataOrigin = (char*)std::malloc((size_t)im->imageSize > 0 ? (size_t)im->imageSize : 1);
    if (!im->imageData) { std::free(im); return NULL; }
    return im;
}
inline void cvReleaseImage(IplImage** p) { if (p && *p) { std::free((*p)->imageDataOrigin); std::free(*p); *p = NULL; } }
struct ImagePoseInfo { IplImage* pImg; int fixed; ImagePoseInfo() : pImg(NULL), fixed(0) {} };              // MosaicWithoutPos.h:283-297 (camPose omitted)
}  // namespace mi355ref
#define MI355_NS mi355ref::
#define MI355_CREATE_IMAGE_8U(w, h, ch) mi355ref::cvCreateImage8U((w), (h), (ch))
#else
#define MI355_NS
#define MI355_CREATE_IMAGE_8U(w, h, ch) cvCreateImage(cvSize((w), (h)), 8, (ch))
#endif

namespace mi355 {

static_assert(sizeof(MI355_NS SfPoint) == sizeof(mi355_sfpoint), "SfPoint layout");
static_assert(sizeof(MI355_NS MatchPointPairs) == sizeof(mi355_match_point_pairs), "MatchPointPairs layout");
static_assert(sizeof(MI355_NS ImageTransform) == sizeof(mi355_image_transform), "ImageTransform layout");

// MI355_ADAPTOR_KEEP_FRAMES (opt-in): the SIFT and SURF front-ends set "keep_frames" on the context, so that every frame
// they extract stays in HBM under its image index, and record per index the imageData pointer and geometry they extracted.  The render
// functions then take image k from its kept frame wherever pImgs[k] still has that pointer and geometry, and upload it otherwise.  This
// assumes what the reference's driver does (MosaicWithoutPos.cpp:4430-4679): the frames are rendered with the indices they were extracted
// under and no pixel changes in between.  Without the macro no frame is kept.
namespace detail {
struct FrameRecord { const void* data; int w, h, ws; };
inline std::mutex& frames_mu() { static std::mutex m; return m; }
inline std::vector<FrameRecord>& frame_records() { static std::vector<FrameRecord> v; return v; }
inline void record_frame(int i, const void* data, int w, int h, int ws) {
    std::lock_guard<std::mutex> lk(frames_mu());
    std::vector<FrameRecord>& v = frame_records();
    if ((int)v.size() <= i) { FrameRecord none = {NULL, 0, 0, 0}; v.resize((size_t)i + 1, none); }
    FrameRecord r = {data, w, h, ws};
    v[(size_t)i] = r;
}
// the id to render image k from: k where its kept frame is this very image, -1 (upload) otherwise
inline int32_t kept_id(int k, const void* data, int w, int h, int ws) {
    std::lock_guard<std::mutex> lk(frames_mu());
    const std::vector<FrameRecord>& v = frame_records();
    if (!data || k >= (int)v.size()) return -1;
    const FrameRecord& r = v[(size_t)k];
    return (r.data == data && r.w == w && r.h == h && r.ws == ws) ? k : -1;
}
// image k is released (ownership passed to the adaptor): its kept frame goes too, before its address can be reused
inline void forget_frame(mi355_ctx* c, int k) {
    std::lock_guard<std::mutex> lk(frames_mu());
    std::vector<FrameRecord>& v = frame_records();
    if (k < (int)v.size() && v[(size_t)k].data) { v[(size_t)k].data = NULL; mi355_drop_frames(c, k); }
}
}  // namespace detail

// One process-wide context per device (the reference is a single-process program).  Creation is guarded: the reference calls the
// per-pair code from up to 8 worker threads at once (MosaicWithoutPos.cpp:5246-5292); the ctx itself is thread-safe per the C ABI.
inline mi355_ctx* context(int device = 0) {
    struct Slot { std::once_flag once; mi355_ctx* ctx; Slot() : ctx(NULL) {} };
    static Slot slots[16];
    if (device < 0 || device >= 16) return NULL;
    Slot& s = slots[device];
    std::call_once(s.once, [&s, device]() { if (mi355_create(&s.ctx, NULL, device) != MI355_OK) s.ctx = NULL; });
    return s.ctx;
}

// bool Ransac2D(const vector<PointType>&, const vector<PointType>&, vector<PointType>&, vector<PointType>&,
//               float aProjectMat[9], float fRansacDist = 1, int sampleTimes = 1000)          mosaicimage.h:1729-1735
// `seed` stands for the reference's srand((unsigned)time(0)) (mosaicimage.h:1777).  Up to 65535 correspondences (the live path passes
// <= 396: maxNum, MosaicWithoutPos.cpp:5146; above 400 a second kernel keeps the work arrays in HBM, above 4096 a third the points too);
// larger inputs return false with aProjectMat zeroed, where the reference would run on any n.
inline bool Ransac2D(const std::vector<MI355_NS SfPoint>& p1, const std::vector<MI355_NS SfPoint>& p2,
                     std::vector<MI355_NS SfPoint>& in1, std::vector<MI355_NS SfPoint>& in2, float aProjectMat[9],
                     float fRansacDist = 1.0f, int sampleTimes = 1000, unsigned seed = 1) {
    in1.clear(); in2.clear();
    if (p1.empty() || p1.size() != p2.size()) return false;
    mi355_ctx* c = context();
    if (!c) return false;
    const size_t cap = p1.size() > MI355_MAX_SELECTED ? p1.size() : MI355_MAX_SELECTED;
    std::vector<mi355_sfpoint> a(cap), b(cap);
    int n_in = 0;
    const int ok = mi355_ransac2d(c, reinterpret_cast<const mi355_sfpoint*>(&p1[0]), reinterpret_cast<const mi355_sfpoint*>(&p2[0]), (int)p1.size(),
                                  fRansacDist, sampleTimes, seed, &a[0], &b[0], &n_in, aProjectMat);
    if (ok < 0) return false;
    in1.resize(n_in); in2.resize(n_in);
    if (n_in) { std::memcpy(&in1[0], &a[0], sizeof(mi355_sfpoint) * n_in); std::memcpy(&in2[0], &b[0], sizeof(mi355_sfpoint) * n_in); }
    return ok == 1;
}

// int SelectMatchPairs(const vector<DMatch>&, const vector<KeyPoint>&, const vector<KeyPoint>&, int nMatch, int width, int height,
//                      int gridX, int gridY, vector<SfPoint>&, vector<SfPoint>&)                    MosaicWithoutPos.cpp:4977-4983
// One body for both spellings of the element types: cv::DMatch / cv::KeyPoint (OpenCV 2.4.0 features2d.hpp: the reference's own call,
// MosaicWithoutPos.cpp:5146-5153, compiles unchanged against this) and the C-ABI PODs mi355_dmatch / mi355_keypoint.  Nothing of OpenCV
// is included here: the element types are template parameters and only .queryIdx/.trainIdx/.imgIdx/.distance and the point are read.
namespace detail {
inline float kp_x(const mi355_keypoint& k) { return k.x; }
inline float kp_y(const mi355_keypoint& k) { return k.y; }
template <class KP> inline float kp_x(const KP& k) { return k.pt.x; }      // cv::KeyPoint
template <class KP> inline float kp_y(const KP& k) { return k.pt.y; }
}  // namespace detail
template <class DMatchT, class KeyPointT>
inline int SelectMatchPairs(const std::vector<DMatchT>& matches, const std::vector<KeyPointT>& kp1, const std::vector<KeyPointT>& kp2,
                            int nMatch, int width, int height, int gridX, int gridY,
                            std::vector<MI355_NS SfPoint>& v1, std::vector<MI355_NS SfPoint>& v2) {
    v1.clear(); v2.clear();
    mi355_ctx* c = context();
    if (!c) return -1;
    std::vector<mi355_dmatch> dm(matches.size());
    for (size_t i = 0; i < matches.size(); i++) {
        dm[i].queryIdx = matches[i].queryIdx; dm[i].trainIdx = matches[i].trainIdx; dm[i].imgIdx = matches[i].imgIdx; dm[i].distance = matches[i].distance;
    }
    std::vector<float> xy1(kp1.size() * 2), xy2(kp2.size() * 2);
    for (size_t i = 0; i < kp1.size(); i++) { xy1[2 * i] = detail::kp_x(kp1[i]); xy1[2 * i + 1] = detail::kp_y(kp1[i]); }
    for (size_t i = 0; i < kp2.size(); i++) { xy2[2 * i] = detail::kp_x(kp2[i]); xy2[2 * i + 1] = detail::kp_y(kp2[i]); }
    std::vector<mi355_sfpoint> a(MI355_MAX_SELECTED), b(MI355_MAX_SELECTED);
    int n = 0;
    const int rc = mi355_select_grid(c, dm.empty() ? NULL : &dm[0], (int)dm.size(), xy1.empty() ? NULL : &xy1[0], (int)kp1.size(),
                                     xy2.empty() ? NULL : &xy2[0], (int)kp2.size(), nMatch, width, height, gridX, gridY, &a[0], &b[0], &n);
    if (rc != MI355_OK) return rc;
    v1.resize(n); v2.resize(n);
    if (n) { std::memcpy(&v1[0], &a[0], sizeof(mi355_sfpoint) * n); std::memcpy(&v2[0], &b[0], sizeof(mi355_sfpoint) * n); }
    return 0;
}

// int ImageProjectionTransform(BitmapImage* pImage, BitmapImage*& pResult, float h[9])             MosaicImage.cpp:1613
// pResult is allocated the way CreateBitmap8U does (ImageIO.cpp:58-76: new BitmapImage, new unsigned char[widthStep * height]), so the
// reference's callers go on releasing it with ReleaseBitmap8U (ImageIO.cpp:78-93: delete[] imageData, delete) -- stand-alone,
// mi355ref::ReleaseBitmap8U is that function.  The library's own buffer (malloc) never leaves this function.
inline int ImageProjectionTransform(MI355_NS BitmapImage* pImage, MI355_NS BitmapImage*& pResult, float h[9]) {
    if (pImage == NULL) return -1;
    mi355_ctx* c = context();
    if (!c) return -1;
    uint8_t* dst = NULL; int dw = 0, dh = 0, dws = 0;
    const int rc = mi355_warp_image(c, pImage->imageData, pImage->width, pImage->height, pImage->widthStep, pImage->nChannels, h, &dst, &dw, &dh, &dws);
    if (rc != MI355_OK) return rc;
    pResult = new MI355_NS BitmapImage();
    pResult->width = dw; pResult->height = dh; pResult->widthStep = dws; pResult->nChannels = pImage->nChannels;
    pResult->imageData = new unsigned char[(size_t)dws * dh];
    std::memcpy(pResult->imageData, dst, (size_t)dws * dh);
    mi355_free(dst);
    return 0;
}

// The per-pair loop body of GetMatchedPairsOneToAllSIFTThread (MosaicWithoutPos.cpp:5084-5232) for every pair of the
// reference's schedule, appending MatchPointPairs exactly like :5201-5221.  Features must have been extracted with
// mi355_sift_extract(ctx, image_index, ...).
inline int GetMatchedPairsOneToAllSIFT(int nImages, float ransacDist, unsigned seed, const int* fixedFlags,
                                       std::vector<MI355_NS MatchPointPairs>& vecMatchPairs, int window = 182) {
    mi355_ctx* c = context();
    if (!c) return -1;
    int n_pairs = 0;
    mi355_pair_schedule(nImages, window, 0, 1, NULL, 0, &n_pairs);
    if (n_pairs == 0) return 0;
    std::vector<int32_t> pairs((size_t)n_pairs * 2);
    mi355_pair_schedule(nImages, window, 0, 1, &pairs[0], n_pairs, &n_pairs);
    mi355_pair_result* res = (mi355_pair_result*)std::malloc(sizeof(mi355_pair_result) * (size_t)n_pairs);
    if (!res) return -1;
    int rc = mi355_match_pairs(c, &pairs[0], n_pairs, ransacDist, seed, res);
    if (rc == MI355_OK) {
        mi355_match_point_pairs* v = NULL; int n = 0;
        rc = mi355_results_to_match_pairs(res, n_pairs, fixedFlags, &v, &n);
        if (rc == MI355_OK) {
            const size_t old = vecMatchPairs.size();
            vecMatchPairs.resize(old + n);
            if (n) std::memcpy(&vecMatchPairs[old], v, sizeof(mi355_match_point_pairs) * n);
            mi355_free(v);
        }
    }
    std::free(res);
    return rc;
}

// The window form with the tie-point refinement (mi355_refine_ties, "tie-point refinement by patch correlation" in mi355_mosaic.h) between the
// pair stage and the flattening: every accepted pair's inliers in image i are moved to the correlation peak of the patch around their
// partners in image j, read from the frames KEPT at extraction under ids 0 .. nImages - 1 (option "keep_frames"; an id without a kept
// frame is MI355_ERR_ARG), and ties->drop_mask may drop the ties that fail.  ties == NULL: the bytes of the window form above.
inline int GetMatchedPairsOneToAllSIFT(int nImages, float ransacDist, unsigned seed, const int* fixedFlags,
                                       std::vector<MI355_NS MatchPointPairs>& vecMatchPairs, int window, const mi355_tie_params* ties) {
    if (!ties) return GetMatchedPairsOneToAllSIFT(nImages, ransacDist, seed, fixedFlags, vecMatchPairs, window);
    mi355_ctx* c = context();
    if (!c) return -1;
    int n_pairs = 0;
    mi355_pair_schedule(nImages, window, 0, 1, NULL, 0, &n_pairs);
    if (n_pairs == 0) return 0;
    std::vector<int32_t> pairs((size_t)n_pairs * 2), ids((size_t)nImages);
    std::vector<int> w((size_t)nImages), h((size_t)nImages), ws((size_t)nImages);
    for (int k = 0; k < nImages; k++) {
        const uint8_t* d = NULL;
        ids[k] = k;
        const int rc = mi355_get_frame_dev(c, k, &d, &w[k], &h[k], &ws[k]);
        if (rc != MI355_OK) return rc;
    }
    mi355_pair_schedule(nImages, window, 0, 1, &pairs[0], n_pairs, &n_pairs);
    mi355_pair_result* res = (mi355_pair_result*)std::malloc(sizeof(mi355_pair_result) * (size_t)n_pairs);
    if (!res) return -1;
    int rc = mi355_match_pairs(c, &pairs[0], n_pairs, ransacDist, seed, res);
    if (rc == MI355_OK) rc = mi355_refine_ties(c, res, n_pairs, NULL, &ids[0], &w[0], &h[0], &ws[0], nImages, ties, res, NULL, NULL, NULL);
    if (rc == MI355_OK) {
        mi355_match_point_pairs* v = NULL; int n = 0;
        rc = mi355_results_to_match_pairs(res, n_pairs, fixedFlags, &v, &n);
        if (rc == MI355_OK) {
            const size_t old = vecMatchPairs.size();
            vecMatchPairs.resize(old + n);
            if (n) std::memcpy(&vecMatchPairs[old], v, sizeof(mi355_match_point_pairs) * n);
            mi355_free(v);
        }
    }
    std::free(res);
    return rc;
}

// The window form with pair verification (mi355_verify_pairs_results, "pair verification" in mi355_mosaic.h) between the pair stage and the
// flattening: the accepted pairs whose homographies contradict their neighbours are demoted, so the list holds the kept pairs'
// correspondences only.  The flat list carries no homographies, so there is no flat form of the verification: it runs here, on the records.
// verify == NULL: the library's defaults.  summary (may be NULL) receives the counts per verdict.  An error of the verification (for
// example MI355_ERR_FAILED, "no pair could be verified": mi355_last_error(NULL)) leaves vecMatchPairs as it was.
inline int GetMatchedPairsOneToAllSIFT(int nImages, float ransacDist, unsigned seed, const int* fixedFlags,
                                       std::vector<MI355_NS MatchPointPairs>& vecMatchPairs, int window, const mi355_verify_params* verify,
                                       mi355_verify_summary* summary) {
    mi355_ctx* c = context();
    if (!c) return -1;
    int n_pairs = 0;
    mi355_pair_schedule(nImages, window, 0, 1, NULL, 0, &n_pairs);
    if (n_pairs == 0) return 0;
    std::vector<int32_t> pairs((size_t)n_pairs * 2), label((size_t)nImages);
    std::vector<mi355_image_transform> tr((size_t)nImages);
    mi355_pair_schedule(nImages, window, 0, 1, &pairs[0], n_pairs, &n_pairs);
    mi355_pair_result* res = (mi355_pair_result*)std::malloc(sizeof(mi355_pair_result) * (size_t)n_pairs);
    if (!res) return -1;
    int rc = mi355_match_pairs(c, &pairs[0], n_pairs, ransacDist, seed, res);
    if (rc == MI355_OK) rc = mi355_verify_pairs_results(res, n_pairs, nImages, fixedFlags, verify, res, &label[0], &tr[0], NULL, summary);
    if (rc == MI355_OK) {
        mi355_match_point_pairs* v = NULL; int n = 0;
        rc = mi355_results_to_match_pairs(res, n_pairs, fixedFlags, &v, &n);
        if (rc == MI355_OK) {
            const size_t old = vecMatchPairs.size();
            vecMatchPairs.resize(old + n);
            if (n) std::memcpy(&vecMatchPairs[old], v, sizeof(mi355_match_point_pairs) * n);
            mi355_free(v);
        }
    }
    std::free(res);
    return rc;
}

// The same with the descriptor-screened schedule (mi355_screen_pairs) in place of the window: the pairs of images 0 .. nImages - 1 that the
// screen keeps are matched, and vecMatchPairs is filled exactly as the window form fills it.  screen NULL: mi355_default_screen_params
// (all pairs in scope); screen->window >= 2 screens the window's pairs only.
inline int GetMatchedPairsOneToAllSIFT(int nImages, float ransacDist, unsigned seed, const int* fixedFlags,
                                       std::vector<MI355_NS MatchPointPairs>& vecMatchPairs, const mi355_screen_params* screen) {
    mi355_ctx* c = context();
    if (!c || nImages < 0) return -1;
    mi355_screen_params sp;
    if (screen) sp = *screen; else mi355_default_screen_params(&sp);
    if (nImages < 2) return 0;
    std::vector<int32_t> ids((size_t)nImages);
    for (int i = 0; i < nImages; i++) ids[i] = i;
    int cap = sp.partners > 0 ? nImages * sp.partners : 0, n_pairs = 0;
    std::vector<int32_t> pairs((size_t)(cap > 0 ? cap : 1) * 2);
    int rc = mi355_screen_pairs(c, &ids[0], nImages, &sp, 0, 1, &pairs[0], NULL, cap, &n_pairs);
    if (rc == MI355_ERR_ARG && n_pairs > cap) {                  // partners == 0: the count is known now
        cap = n_pairs;
        pairs.resize((size_t)cap * 2);
        rc = mi355_screen_pairs(c, &ids[0], nImages, &sp, 0, 1, &pairs[0], NULL, cap, &n_pairs);
    }
    if (rc != MI355_OK) return rc;
    if (n_pairs == 0) return 0;
    mi355_pair_result* res = (mi355_pair_result*)std::malloc(sizeof(mi355_pair_result) * (size_t)n_pairs);
    if (!res) return -1;
    rc = mi355_match_pairs(c, &pairs[0], n_pairs, ransacDist, seed, res);
    if (rc == MI355_OK) {
        mi355_match_point_pairs* v = NULL; int n = 0;
        rc = mi355_results_to_match_pairs(res, n_pairs, fixedFlags, &v, &n);
        if (rc == MI355_OK) {
            const size_t old = vecMatchPairs.size();
            vecMatchPairs.resize(old + n);
            if (n) std::memcpy(&vecMatchPairs[old], v, sizeof(mi355_match_point_pairs) * n);
            mi355_free(v);
        }
    }
    std::free(res);
    return rc;
}

// int CMosaicByPose::GetMatchedPairsOneToAllSIFT_MultiThread()                                MosaicWithoutPos.cpp:5244-5295
// The reference's member reads m_pImgPoses / m_nImages / m_ransacDist and fills m_vecMatchPairs / m_nSuccess through its threads
// (extraction :4832-4887, matching :5031-5241, results pushed under a mutex :10137-10145; the caller sets
// m_pImgPoses / m_nImages at :4484-4486).  This is that whole call in one: SIFT(2000,3,0.01,20) of every image (parked as batches,
// no keypoint_%d.key / discriptor_%d.xml round trip), then every pair of the window j in (i, i + 182) (:5083-5084), MatchPointPairs
// appended like :5201-5221, nSuccess = accepted pairs.  PoseT is the reference's ImagePoseInfo (.pImg and .fixed are read; the images
// must stay valid until the call returns).  `seed` stands for srand((unsigned)time(0)) (:5061).  Returns 0 like the reference, < 0 on error.
template <class PoseT>
inline int GetMatchedPairsOneToAllSIFT_MultiThread(const PoseT* pImgPoses, const int nImages, std::vector<MI355_NS MatchPointPairs>& vecMatchPairs,
                                                   int& nSuccess, float ransacDist = 2.5f, unsigned seed = 1, int window = 182) {
    nSuccess = 0;
    mi355_ctx* c = context();
    if (!c || !pImgPoses || nImages < 0) return -1;
    std::vector<int32_t> fixed(nImages > 0 ? nImages : 1, 0);
#ifdef MI355_ADAPTOR_KEEP_FRAMES
    mi355_set_option(c, "keep_frames", 1);
#endif
    for (int i = 0; i < nImages; i++) {
        const MI355_NS IplImage* im = pImgPoses[i].pImg;
        if (!im) return -1;
        fixed[i] = pImgPoses[i].fixed;
        // deferred form (no output pointers): the frame is staged in HBM and joins a batch; the match call below waits for the features
        const int rc = mi355_sift_extract(c, i, (const uint8_t*)im->imageData, im->width, im->height, im->widthStep, NULL, NULL, 0, NULL);
        if (rc != MI355_OK) return rc;
#ifdef MI355_ADAPTOR_KEEP_FRAMES
        detail::record_frame(i, im->imageData, im->width, im->height, im->widthStep);
#endif
    }
    int n_pairs = 0;
    mi355_pair_schedule(nImages, window, 0, 1, NULL, 0, &n_pairs);
    if (n_pairs == 0) return 0;
    std::vector<int32_t> pairs((size_t)n_pairs * 2);
    mi355_pair_schedule(nImages, window, 0, 1, &pairs[0], n_pairs, &n_pairs);
    mi355_pair_result* res = (mi355_pair_result*)std::malloc(sizeof(mi355_pair_result) * (size_t)n_pairs);
    if (!res) return -1;
    int rc = mi355_match_pairs(c, &pairs[0], n_pairs, ransacDist, seed, res);
    if (rc == MI355_OK) {
        for (int p = 0; p < n_pairs; p++) nSuccess += res[p].accepted ? 1 : 0;
        mi355_match_point_pairs* v = NULL; int n = 0;
        rc = mi355_results_to_match_pairs(res, n_pairs, &fixed[0], &v, &n);
        if (rc == MI355_OK) {
            const size_t old = vecMatchPairs.size();
            vecMatchPairs.resize(old + n);
            if (n) std::memcpy(&vecMatchPairs[old], v, sizeof(mi355_match_point_pairs) * n);
            mi355_free(v);
        }
    }
    std::free(res);
    return rc;
}

// int CMosaicByPose::GetMatchedPairsOneToAllSurf(const ImagePoseInfo* pImgPoses, const int nImages, vector<MatchPointPairs>& vecMatchPairs,
//                                                int& nSuccess)                                  MosaicWithoutPos.cpp:5300-5533
// (m_minHessian, m_matchDist, m_maxFeatureNum, m_ransacDist are members there: UavMatchParam defaults 50 / 0.5 / 200 / 2.5.)
// SURF features of every image, the ring schedule, exact float matching + distance selection + RANSAC; MatchPointPairs appended
// like :5497-5517; nSuccess = 1 + accepted pairs (:5320, :5516).  `seed` stands for srand((unsigned)time(0)).
template <class PoseT>
inline int GetMatchedPairsOneToAllSurf(const PoseT* pImgPoses, const int nImages, std::vector<MI355_NS MatchPointPairs>& vecMatchPairs, int& nSuccess,
                                       int minHessian = 50, float matchDist = 0.5f, int maxFeatureNum = 200, float ransacDist = 2.5f, unsigned seed = 1) {
    nSuccess = 1;
    mi355_ctx* c = context();
    if (!c || !pImgPoses) return -1;
    std::vector<int32_t> fixed(nImages > 0 ? nImages : 1, 0);
#ifdef MI355_ADAPTOR_KEEP_FRAMES
    mi355_set_option(c, "keep_frames", 1);
#endif
    for (int i = 0; i < nImages; i++) {
        const MI355_NS IplImage* im = pImgPoses[i].pImg;
        if (!im) return -1;
        fixed[i] = pImgPoses[i].fixed;
        int n = 0;
        const int rc = mi355_surf_extract(c, i, (const uint8_t*)im->imageData, im->width, im->height, im->widthStep, (float)minHessian, 1 << 21 /* every keypoint, like the reference */, NULL, NULL, &n);
        if (rc != MI355_OK) return rc;
#ifdef MI355_ADAPTOR_KEEP_FRAMES
        detail::record_frame(i, im->imageData, im->width, im->height, im->widthStep);
#endif
    }
    int np = 0;
    mi355_surf_pair_schedule(nImages, NULL, 0, &np);
    if (np == 0) return 0;
    std::vector<int32_t> pairs((size_t)2 * np);
    mi355_surf_pair_schedule(nImages, &pairs[0], np, &np);
    mi355_pair_result* res = (mi355_pair_result*)std::malloc(sizeof(mi355_pair_result) * (size_t)np);
    if (!res) return -1;
    int rc = mi355_surf_match_pairs(c, &pairs[0], np, ransacDist, seed, matchDist, maxFeatureNum, 18, res);
    if (rc == MI355_OK) {
        for (int p = 0; p < np; p++) nSuccess += res[p].accepted ? 1 : 0;
        mi355_match_point_pairs* v = NULL; int n = 0;
        rc = mi355_results_to_match_pairs(res, np, &fixed[0], &v, &n);
        if (rc == MI355_OK) {
            const size_t old = vecMatchPairs.size();
            vecMatchPairs.resize(old + n);
            if (n) std::memcpy(&vecMatchPairs[old], v, sizeof(mi355_match_point_pairs) * n);
            mi355_free(v);
        }
    }
    std::free(res);
    return rc;
}

namespace detail {
// the one-pass renders into a fresh IplImage: unblended (mi355_mosaic_refined_into), weighted (mi355_mosaic_feathered_into, default ramp),
// seamline (mi355_mosaic_seamline_into, default ramp) or median (mi355_mosaic_median_into, default ramp and depth); with level >= 1 the image
// is that level of the render `render` instead
// (mi355_mosaic_preview_into, exact coverage, default ramp): the full-size canvas is never made
enum OnePass { ONE_PASS_UNBLENDED, ONE_PASS_WEIGHTED, ONE_PASS_SEAMLINE, ONE_PASS_MEDIAN };
template <class PoseT>
inline int render_one_pass(const PoseT* pImgPoses, const int nImages, const MI355_NS ImageTransform* pRectified, MI355_NS IplImage*& pMosaicResult, OnePass mode,
                           int level = 0, int render = 0) {
    if (NULL == pImgPoses || NULL == pRectified || nImages <= 0) return -1;
    mi355_ctx* c = context();
    if (!c) return -2;
    std::vector<const uint8_t*> imgs(nImages); std::vector<int32_t> ids(nImages, -1);
    std::vector<int> w(nImages), h(nImages), ws(nImages); std::vector<float> h9((size_t)9 * nImages);
    for (int n = 0; n < nImages; n++) {
        const MI355_NS IplImage* im = pImgPoses[n].pImg;
        std::memcpy(&h9[(size_t)9 * n], pRectified[n].h.m, 9 * sizeof(float));
        if (!im) { imgs[n] = NULL; w[n] = h[n] = ws[n] = 0; h9[(size_t)9 * n + 8] = 0.0f; continue; }     // no image: skipped like h.m[8] == 0 (:2256)
        imgs[n] = (const uint8_t*)im->imageData; w[n] = im->width; h[n] = im->height; ws[n] = im->widthStep;
#ifdef MI355_ADAPTOR_KEEP_FRAMES
        ids[n] = detail::kept_id(n, im->imageData, w[n], h[n], ws[n]);
#endif
    }
    if (nImages <= 1) return -2;                                         // mi355_mosaic_refined's convention (MergeImagesRefined, :2164-2167)
    int cw = 0, ch = 0, cws = 0;
    int rc = mi355_mosaic_layout(&w[0], &h[0], nImages, &h9[0], &cw, &ch, &cws, NULL);
    if (rc != MI355_OK) return rc == MI355_ERR_ARG ? -1 : -2;
    mi355_preview_params pp;
    mi355_default_preview_params(&pp);
    if (level != 0) {
        if (level < 1 || level > 7 || render < 0 || render > 2) return -1;
        int ow[7], oh[7];
        if (mi355_overview_layout(cw, ch, level, ow, oh, NULL) != MI355_OK) return -1;
        cw = ow[level - 1]; ch = oh[level - 1];
        pp.level = level; pp.render = render;
    }
    MI355_NS IplImage* out = MI355_CREATE_IMAGE_8U(cw, ch, 3);          // :2246-2248; the library renders straight into its rows
    if (!out) return -2;
    rc = level != 0 ? mi355_mosaic_preview_into(c, &imgs[0], &ids[0], &w[0], &h[0], &ws[0], nImages, &h9[0], &pp, (uint8_t*)out->imageData, out->widthStep, NULL, cw, ch)
       : mode == ONE_PASS_WEIGHTED ? mi355_mosaic_feathered_into(c, &imgs[0], &ids[0], &w[0], &h[0], &ws[0], nImages, &h9[0], NULL, (uint8_t*)out->imageData, out->widthStep, cw, ch)
       : mode == ONE_PASS_SEAMLINE ? mi355_mosaic_seamline_into(c, &imgs[0], &ids[0], &w[0], &h[0], &ws[0], nImages, &h9[0], NULL, (uint8_t*)out->imageData, out->widthStep, cw, ch)
       : mode == ONE_PASS_MEDIAN   ? mi355_mosaic_median_into(c, &imgs[0], &ids[0], &w[0], &h[0], &ws[0], nImages, &h9[0], NULL, (uint8_t*)out->imageData, out->widthStep, cw, ch)
                                   : mi355_mosaic_refined_into(c, &imgs[0], &ids[0], &w[0], &h[0], &ws[0], nImages, &h9[0], (uint8_t*)out->imageData, out->widthStep, cw, ch);
    if (rc != MI355_OK) { cvReleaseImage(&out); return rc == MI355_ERR_ARG ? -1 : -2; }
    if (pMosaicResult) cvReleaseImage(&pMosaicResult);
    pMosaicResult = out;
    return 0;
}
}  // namespace detail

// int CMosaicByPose::MosaicImagesRefined(const ImagePoseInfo* pImgPoses, const int nImages, const ImageTransform* pRectified)
//                                                                                              MosaicWithoutPos.cpp:2194-2352
// The member writes m_pMosaicResult; here it is the last argument (released first when not NULL, like a second call would leak in
// the reference).  PoseT is the reference's ImagePoseInfo (only .pImg is read).  Returns 0 / -1 / -2 like the reference.
template <class PoseT>
inline int MosaicImagesRefined(const PoseT* pImgPoses, const int nImages, const MI355_NS ImageTransform* pRectified, MI355_NS IplImage*& pMosaicResult) {
    return detail::render_one_pass(pImgPoses, nImages, pRectified, pMosaicResult, detail::ONE_PASS_UNBLENDED);
}

// UavMatchParam.blending == 1, "weighted blending" (MosaicWithoutPos.h:65): the mode the reference's driver sends down the unblended branch
// (MosaicWithoutPos.cpp:4666-4672).  MosaicImagesRefined's signature, ownership and return values; the canvas is mi355_mosaic_feathered's
// (include/mi355_mosaic.h, "weighted (feather) blending") with the default ramp.  Kept frames are used under MI355_ADAPTOR_KEEP_FRAMES.
template <class PoseT>
inline int MosaicImagesWeighted(const PoseT* pImgPoses, const int nImages, const MI355_NS ImageTransform* pRectified, MI355_NS IplImage*& pMosaicResult) {
    return detail::render_one_pass(pImgPoses, nImages, pRectified, pMosaicResult, detail::ONE_PASS_WEIGHTED);
}

// The seamline render (include/mi355_mosaic.h, "seamline render") with the default ramp: every canvas pixel from the one frame in which it lies
// deepest -- as sharp as MosaicImagesRefined, with the seams in the middle of the overlaps.  The reference has no such mode; the signature,
// ownership and return values are MosaicImagesRefined's.  Kept frames are used under MI355_ADAPTOR_KEEP_FRAMES.
template <class PoseT>
inline int MosaicImagesSeamline(const PoseT* pImgPoses, const int nImages, const MI355_NS ImageTransform* pRectified, MI355_NS IplImage*& pMosaicResult) {
    return detail::render_one_pass(pImgPoses, nImages, pRectified, pMosaicResult, detail::ONE_PASS_SEAMLINE);
}

// The median render (include/mi355_mosaic.h, "median render") with the default ramp and depth (5): every canvas pixel the per-channel median
// of its deepest frames, so that what moved between exposures -- cars, people, shadows -- drops out of the overlaps instead of ghosting or
// being cut at a seam.  The reference has no such mode; the signature, ownership and return values are MosaicImagesSeamline's.  Kept frames
// are used under MI355_ADAPTOR_KEEP_FRAMES.
template <class PoseT>
inline int MosaicImagesMedian(const PoseT* pImgPoses, const int nImages, const MI355_NS ImageTransform* pRectified, MI355_NS IplImage*& pMosaicResult) {
    return detail::render_one_pass(pImgPoses, nImages, pRectified, pMosaicResult, detail::ONE_PASS_MEDIAN);
}

// BundleAdjustmentNonlinear, MosaicWithoutPos.cpp:9750-10081, the step the driver keeps switched off (nonlinearAdjustment, :4628-4637): here
// the damped, Jacobi-scaled projective refinement anchored to its input (include/mi355_mosaic.h, "projective refinement of the global
// alignment"; mi355_global_projective_refine on the flat list).  Host only: no context, no device.  pImagesTransform0 is the affine result
// (vecTransformAffineRefined); an image is fixed iff its own `fixed` member is set, as the reference's function reads it (nFixedImages is kept
// for the signature).  The reference's signature carries no frame sizes, which the prior's control points need: pass the frames' widths and
// heights where the caller has them (the driver does: pImgPoses[k].pImg); WITHOUT them each image's control points span the bounding box of
// its own tie points, w = floor(max x) + 2, h = floor(max y) + 2 (at least 2) -- the region the data speaks about.  Returns 0, the reference's
// -2 (nImages <= 1) and -3 (nPairs <= 4), else the C call's error (mi355_last_error(0)).  Unlike the reference, the input is left unchanged.
inline int BundleAdjustmentNonlinear(MI355_NS MatchPointPairs* pMatchPairs, int nPairs, MI355_NS ImageTransform* pImagesTransform0, int nImages, int nFixedImages,
                                     std::vector<MI355_NS ImageTransform>& vecTransformRefined, const int* pWidths = 0, const int* pHeights = 0,
                                     const mi355_projective_params* params = 0, mi355_projective_report* report = 0) {
    (void)nFixedImages;
    if (nImages <= 1) return -2;
    if (nPairs <= 4) return -3;
    if (!pMatchPairs || !pImagesTransform0) return -1;
    std::vector<int32_t> w((size_t)nImages, 2), h((size_t)nImages, 2), fixed((size_t)nImages, 0);
    for (int k = 0; k < nImages; k++) fixed[k] = pImagesTransform0[k].fixed ? 1 : 0;
    if (pWidths && pHeights) {
        for (int k = 0; k < nImages; k++) { w[k] = pWidths[k]; h[k] = pHeights[k]; }
    } else {
        for (int p = 0; p < nPairs; p++) {
            const MI355_NS MatchPointPairs& m = pMatchPairs[p];
            const int idx[2] = {m.ptA_i, m.ptB_i};
            const MI355_NS SfPoint* pt[2] = {&m.ptA, &m.ptB};
            for (int s = 0; s < 2; s++) {
                if (idx[s] < 0 || idx[s] >= nImages || !(pt[s]->x >= 0.0f && pt[s]->x < 1e9f && pt[s]->y >= 0.0f && pt[s]->y < 1e9f)) continue;
                const int bx = (int)pt[s]->x + 2, by = (int)pt[s]->y + 2;
                if (bx > w[idx[s]]) w[idx[s]] = bx;
                if (by > h[idx[s]]) h[idx[s]] = by;
            }
        }
    }
    vecTransformRefined.resize((size_t)nImages);
    return mi355_global_projective_refine(reinterpret_cast<const mi355_match_point_pairs*>(pMatchPairs), nPairs, nImages, w.data(), h.data(), fixed.data(), 0,
                                          reinterpret_cast<const mi355_image_transform*>(pImagesTransform0), params,
                                          reinterpret_cast<mi355_image_transform*>(vecTransformRefined.data()), report);
}

// Lens undistortion (include/mi355_mosaic.h, "lens undistortion"): src, a frame of the distorted camera `cam`, resampled into dst for the
// pinhole camera of `params` (0: the camera's own intrinsics; mi355_undistort_fit gives the widest one without empty rim pixels).  The
// reference has no such step: its caller, which holds host IplImages, calls this just before SiftExtraction; dst may be
// src.  Both images are 3-channel 8-bit of one size.  0 on success, -1 for bad arguments, else the C call's error; n_outside (may be 0)
// receives the number of output pixels without a sample.
inline int UndistortImage(const MI355_NS IplImage* src, MI355_NS IplImage* dst, const mi355_camera& cam, const mi355_undistort_params* params = 0,
                          long long* n_outside = 0) {
    if (!src || !dst || !src->imageData || !dst->imageData || src->nChannels != 3 || dst->nChannels != 3 || src->depth != 8 || dst->depth != 8 ||
        src->width != dst->width || src->height != dst->height)
        return -1;
    mi355_ctx* ctx = context();
    if (!ctx) return MI355_ERR_DEVICE;
    int64_t cnt = 0;
    const int rc = mi355_undistort_image(ctx, (const uint8_t*)src->imageData, src->width, src->height, src->widthStep, (uint8_t*)dst->imageData,
                                         dst->widthStep, &cam, params, &cnt);
    if (rc == MI355_OK && n_outside) *n_outside = (long long)cnt;
    return rc;
}

// Lens self-calibration (include/mi355_mosaic.h, "lens self-calibration"): the Brown-Conrady coefficients of the camera from the match list
// of the ORIGINAL frames (the SIFT or SURF front-end's vecMatchPairs; a run of equal (ptA_i, ptB_i) is one pair, cut at 400).  `start` gives
// fx, fy, cx, cy, which are held fixed, and the coefficients to start from (usually 0); `out` is `start` with the free coefficients (params->mask,
// default k1 | k2) replaced.  The reference has no such step; its caller puts it between the front-end and UndistortImage, and runs the
// front-end again on the undistorted frames.  Host only: no context, no device.  0 on success, -1 for bad arguments, else
// the C call's error (mi355_last_error(0)).
inline int CalibrateLens(const MI355_NS MatchPointPairs* pMatchPairs, int nPairs, const mi355_camera& start, mi355_camera& out,
                         const mi355_calib_params* params = 0, mi355_calib_report* report = 0) {
    if (nPairs < 0 || (nPairs > 0 && !pMatchPairs)) return -1;
    return mi355_calibrate_lens(reinterpret_cast<const mi355_match_point_pairs*>(pMatchPairs), nPairs, &start, params, &out, report);
}

// Local registration (include/mi355_mosaic.h, "local registration"): what the aligned ties still disagree by on the canvas -- relief, residual
// lens error, rolling shutter -- becomes a smooth, bounded displacement grid per frame, and the frames KEPT at extraction under ids
// 0 .. nImages - 1 (option "keep_frames"; an id without a kept frame is MI355_ERR_ARG) are resampled by it in place, so that every render that
// reads the kept frames (MI355_ADAPTOR_KEEP_FRAMES) shows the corrected pixels.  The reference has no such step: its caller puts it between
// the global alignment and the render.  pMatchPairs is the list of the SIFT or SURF front-end (a run of equal (ptA_i, ptB_i) is one pair, a
// run longer than 400 is cut into blocks of 400, the flat alignment forms' rule), pRectified the alignment's result.  params 0: the defaults;
// grids (nImages x (grid_y+1) x (grid_x+1) x 2 floats) and report (nImages records) may be 0.  0 on success, -1 for bad arguments, else the
// C call's error.  The caller's host images are not changed.
inline int LocalRegistration(const MI355_NS MatchPointPairs* pMatchPairs, int nPairs, const MI355_NS ImageTransform* pRectified, int nImages,
                             const mi355_local_warp_params* params = 0, float* grids = 0, mi355_local_warp_report* report = 0) {
    if (!pRectified || nImages < 1 || nPairs < 0 || (nPairs > 0 && !pMatchPairs)) return -1;
    mi355_ctx* c = context();
    if (!c) return -1;
    std::vector<uint8_t*> frames((size_t)nImages);
    std::vector<int> w((size_t)nImages), h((size_t)nImages), ws((size_t)nImages);
    std::vector<float> h9((size_t)9 * nImages);
    for (int k = 0; k < nImages; k++) {
        const uint8_t* d = NULL;
        const int rc = mi355_get_frame_dev(c, k, &d, &w[k], &h[k], &ws[k]);
        if (rc != MI355_OK) return rc;
        frames[k] = const_cast<uint8_t*>(d);                             // the kept frame itself: the step is in place
        std::memcpy(&h9[(size_t)9 * k], pRectified[k].h.m, 9 * sizeof(float));
    }
    std::vector<mi355_pair_result> rec;
    for (int p = 0; p < nPairs; p++) {
        const MI355_NS MatchPointPairs& m = pMatchPairs[p];
        if (rec.empty() || rec.back().i != m.ptA_i || rec.back().j != m.ptB_i || rec.back().n_in == MI355_MAX_SELECTED) {
            mi355_pair_result r;
            std::memset(&r, 0, sizeof(r));
            r.i = m.ptA_i; r.j = m.ptB_i; r.ok = 1; r.accepted = 1;
            rec.push_back(r);
        }
        mi355_pair_result& r = rec.back();
        r.a[r.n_in].x = m.ptA.x; r.a[r.n_in].y = m.ptA.y; r.a[r.n_in].id = m.ptA.id;
        r.b[r.n_in].x = m.ptB.x; r.b[r.n_in].y = m.ptB.y; r.b[r.n_in].id = m.ptB.id;
        r.n_in++; r.n_selected = r.n_in;
    }
    return mi355_local_register_results(c, rec.empty() ? NULL : &rec[0], (int)rec.size(), &frames[0], &w[0], &h[0], &ws[0], nImages, &h9[0], params, grids, report);
}

// A reduced-size mosaic (include/mi355_mosaic.h, "overview levels" / the preview): level `level` in 1..7 -- 1 / 2^level of the size -- of the
// render `render` (0 MosaicImagesRefined's, 1 MosaicImagesWeighted's, 2 MosaicImagesSeamline's canvas), averaged over the pixels the survey
// covers only, so that the empty surround does not darken the edge.  The survey is rendered in stripes on the device and only the small image
// comes back.  The reference has no such mode; allocation, ownership and return values are MosaicImagesSeamline's (-1 also for a level or a
// render outside its range).  Kept frames are used under MI355_ADAPTOR_KEEP_FRAMES.
template <class PoseT>
inline int MosaicImagesPreview(const PoseT* pImgPoses, const int nImages, const MI355_NS ImageTransform* pRectified, int level, int render,
                               MI355_NS IplImage*& pMosaicResult) {
    if (level < 1 || level > 7 || render < 0 || render > 2) return -1;
    return detail::render_one_pass(pImgPoses, nImages, pRectified, pMosaicResult, detail::ONE_PASS_UNBLENDED, level, render);
}

// IplImage* LaplacianPyramidBlending(IplImage** pImages, int imagesNum, ProjectMat* pImgT, int band, float resScale)
//                                                                                              MosaicImage.cpp:2205-2510
// Same contract as the reference: pImgT[i].m[0..5] are multiplied by resScale IN PLACE (:2216-2223), images overlapping a kept
// earlier one by more than 0.7 are dropped (ResampleByOverlap, :2227-2230), EVERY input image is released and its pointer set
// to NULL (:2464-2467) -- ownership passes to this function -- and the returned image belongs to the caller (cvReleaseImage).
inline MI355_NS IplImage* LaplacianPyramidBlending(MI355_NS IplImage** pImages, int imagesNum, MI355_NS ProjectMat* pImgT, int band, float resScale) {
    if (NULL == pImages || NULL == pImgT || imagesNum <= 0) return NULL;
    mi355_ctx* c = context();
    if (!c) return NULL;
    for (int i = 0; i < imagesNum; i++) for (int j = 0; j < 6; j++) pImgT[i].m[j] *= resScale;
    std::vector<const uint8_t*> imgs(imagesNum); std::vector<int32_t> ids(imagesNum, -1);
    std::vector<int> w(imagesNum), h(imagesNum), ws(imagesNum); std::vector<float> h9((size_t)9 * imagesNum);
    for (int n = 0; n < imagesNum; n++) {
        std::memcpy(&h9[(size_t)9 * n], pImgT[n].m, 9 * sizeof(float));
        if (!pImages[n]) { imgs[n] = NULL; w[n] = h[n] = 2; ws[n] = 8; h9[(size_t)9 * n + 8] = 0.0f; continue; }
        imgs[n] = (const uint8_t*)pImages[n]->imageData; w[n] = pImages[n]->width; h[n] = pImages[n]->height; ws[n] = pImages[n]->widthStep;
#ifdef MI355_ADAPTOR_KEEP_FRAMES
        ids[n] = detail::kept_id(n, pImages[n]->imageData, w[n], h[n], ws[n]);
#endif
    }
    std::vector<uint8_t> keep(imagesNum, 1);
    MI355_NS IplImage* result = NULL;
    int ow = 0, oh = 0;
    if (mi355_resample_by_overlap(&w[0], &h[0], imagesNum, &h9[0], 0.7f, &keep[0]) == MI355_OK &&
        mi355_blend_layout(&w[0], &h[0], imagesNum, &h9[0], &keep[0], &ow, &oh, NULL) == MI355_OK) {
        result = MI355_CREATE_IMAGE_8U(ow, oh, 3);                        // the library renders straight into its rows
        if (result && mi355_mosaic_blended_into(c, &imgs[0], &ids[0], &w[0], &h[0], &ws[0], imagesNum, &h9[0], &keep[0], band,
                                                (uint8_t*)result->imageData, result->widthStep, ow, oh) != MI355_OK) cvReleaseImage(&result);
    }
#ifdef MI355_ADAPTOR_KEEP_FRAMES
    for (int n = 0; n < imagesNum; n++) if (pImages[n]) detail::forget_frame(c, n);
#endif
    for (int n = 0; n < imagesNum; n++) cvReleaseImage(&pImages[n]);     // :2464-2467: the sources are gone whatever happened
    return result;
}

// int CMosaicByPose::MergeImagesRefined(ImagePoseInfo* pImgPoses, const int nImages, const ImageTransform* pRectified)
//                                                                                              MosaicWithoutPos.cpp:2161-2188
// (m_scale and m_pMosaicResult are members there.)  The images are consumed: pImgPoses[i].pImg = NULL on return (:2182-2185).
template <class PoseT>
inline int MergeImagesRefined(PoseT* pImgPoses, const int nImages, const MI355_NS ImageTransform* pRectified, float m_scale, MI355_NS IplImage*& pMosaicResult) {
    if (nImages <= 1) return -2;                                         // :2164-2167
    std::vector<MI355_NS IplImage*> vecImages(nImages); std::vector<MI355_NS ProjectMat> vecHomo(nImages);
    for (int i = 0; i < nImages; i++) { vecImages[i] = pImgPoses[i].pImg; vecHomo[i] = pRectified[i].h; }
    const int band = 5;                                                  // :2179
    pMosaicResult = LaplacianPyramidBlending(&vecImages[0], nImages, &vecHomo[0], band, m_scale);
    for (int i = 0; i < nImages; i++) pImgPoses[i].pImg = NULL;           // :2182-2185
    return 0;
}

}  // namespace mi355
