/* include/mi355_mosaic.h -- C ABI of libmi355mosaic.so
 *
 * MI355X-native (gfx950 / CDNA4, HIP) replacement for ONE hot path of YuhuaXu/ImageMosaicing:
 *   detect+describe -> descriptor match + selection -> RANSAC homography -> inverse-warp into the canvas.
 * Every entry point names the reference interface it replaces; paths are relative to
 * code/MosaicingCode/mosaicing/ of the reference.  INTEGRATION.md shows the binding a maintainer adds
 * on the reference side (mi355_adaptor.h re-exports the reference's own C++ signatures on top of this ABI).
 *
 * Conventions
 *  - plain pointers and sizes, no C++/torch types, no exceptions across the boundary;
 *  - return 0 on success, <0 on error (MosaicVavImages convention, MosaicWithoutPos.h:631:
 *    -1 bad arguments, -2 operation failed); mi355_last_error() gives the text;
 *    bool-like reference functions (Ransac2D) return 1/0;
 *  - images are caller-owned, BGR u8, rows padded to widthStep bytes (IplImage / BitmapImage layout);
 *  - homographies are row-major float[9]; pair homographies map image-j points onto image-i points and
 *    carry H[8] = max residual (matrix.h:866, LeastSquare.h:519), exactly like the reference;
 *  - there is NO CPU fallback: every compute entry point runs HIP kernels on the ctx's device and
 *    fails with MI355_ERR_DEVICE when no gfx950 device is usable;
 *  - a ctx is thread-safe (one internal lock + one HIP stream); results do not depend on call order.
 */
#ifndef MI355_MOSAIC_H
#define MI355_MOSAIC_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_OK            0
#define MI355_ERR_ARG      (-1)   /* bad arguments            (MosaicVavImages: -1) */
#define MI355_ERR_FAILED   (-2)   /* operation failed         (MosaicVavImages: -2) */
#define MI355_ERR_SINGULAR (-3)   /* homography not invertible (reference: undefined behaviour) */
#define MI355_ERR_DEVICE   (-4)   /* no usable gfx950 device / HIP error */
#define MI355_ERR_NOMEM    (-5)

#define MI355_MAX_SELECTED 400    /* maxNum, MosaicWithoutPos.cpp:5146 */
#define MI355_RANSAC_BIG_MAX 65535 /* largest n mi355_ransac2d accepts: what a 16-bit draw table addresses (Ransac2D itself accepts any n, mosaicimage.h:1729-1761) */
#define MI355_DESC_DIM     128

typedef struct mi355_ctx mi355_ctx;

/* Point.h:27-47 SfPoint */
typedef struct { float x, y; int32_t id; } mi355_sfpoint;
/* MosaicWithoutPos.h:135-153 MatchPointPairs (40 bytes; the record of matchPairs.match) */
typedef struct { mi355_sfpoint ptA; int32_t ptA_i, ptA_Fixed; mi355_sfpoint ptB; int32_t ptB_i, ptB_Fixed; } mi355_match_point_pairs;
/* cv::KeyPoint, OpenCV 2.4.0 features2d.hpp (28 bytes; the record of keypoint_%d.key, MosaicWithoutPos.cpp:4691-4700) */
typedef struct { float x, y, size, angle, response; int32_t octave, class_id; } mi355_keypoint;
/* cv::DMatch */
typedef struct { int32_t queryIdx, trainIdx, imgIdx; float distance; } mi355_dmatch;
/* MosaicWithoutPos.h:224-228 ImageTransform {ProjectMat h; int fixed;} */
typedef struct { float m[9]; int32_t fixed; } mi355_image_transform;

/* Result of one image pair (i,j): what GetMatchedPairsOneToAllSIFTThread appends (MosaicWithoutPos.cpp:5201-5221)
 * plus the homography Ransac2D returned.  Fixed size (9664 B) so that ranks can all-gather arrays of it.
 * A pair that is not accepted (n_in <= min_inliers) still carries its real n_in and the inliers of the winning hypothesis in a[0 .. n_in) and
 * b[0 .. n_in); match_pairs skips Ransac2D's closing refinement for it, so its H is all zero and its ok is 0.  The list entries from n_in on
 * are zero in every record. */
typedef struct {
    int32_t i, j;            /* image indices (ptA_i, ptB_i) */
    int32_t n_in;            /* inlier count; the reference accepts the pair iff n_in > min_inliers (30) */
    int32_t n_selected;      /* correspondences after grid selection (<= 396) */
    int32_t ok;              /* Ransac2D's bool; 0 for a pair that is not accepted: match_pairs skips Ransac2D's closing refinement for it */
    int32_t accepted;        /* n_in > min_inliers */
    float   H[9];            /* image j -> image i, H[8] = max residual (accepted pairs; zero otherwise) */
    int32_t _pad;            /* diagnostic: RANSAC draws that took the generic solve path (0 in the common case) */
    mi355_sfpoint a[MI355_MAX_SELECTED];   /* inliers in image i (id = keypoint index) */
    mi355_sfpoint b[MI355_MAX_SELECTED];   /* inliers in image j */
} mi355_pair_result;

/* Literals of the live path; mi355_default_params() fills the reference's values. */
typedef struct {
    int32_t nfeatures;         /* 2000   SIFT(2000,3,0.01,20)            MosaicWithoutPos.cpp:4852; 1 .. 2048, or <= 0 = cv::SIFT's keep-all
                                  (CVI/nonfree/features2d.hpp:61: every keypoint, OpenCV's generation order, <= the ctx's keepall_max per
                                  frame: 32768 unless mi355_set_option(ctx, "keepall_max", n) raised it, up to 262144; what the
                                  reference's committed run used; the matcher takes such frames through its large-pair path, and the
                                  multi-GPU feature exchange carries them as chunk records, mi355_allgather_feature_chunks) */
    int32_t n_octave_layers;   /* 3 */
    float   contrast_threshold;/* 0.01 */
    float   edge_threshold;    /* 20 */
    float   sigma;             /* 1.6    cv::SIFT default */
    int32_t max_selected;      /* 400    maxNum                           MosaicWithoutPos.cpp:5146 */
    double  select_fraction;   /* 0.3 (double literal: Min(400, 0.3*M))   MosaicWithoutPos.cpp:5147 */
    int32_t grid_x, grid_y;    /* 3,3                                     MosaicWithoutPos.cpp:5041-5042 */
    int32_t min_inliers;       /* 30     MIN_INNER_POINTS                 MosaicWithoutPos.cpp:5049 */
    float   ransac_dist;       /* 2.5    UavMatchParam.ransacDist         MosaicWithoutPos.h:74 */
    int32_t sample_times;      /* 1000                                    mosaicimage.h:1735 */
    int32_t pair_window;       /* 182    j in (i, min(N, i+182))          MosaicWithoutPos.cpp:5083 */
    float   ratio;             /* 0 = reference-compatible sort+grid selection; >0: Lowe ratio test on
                                  squared distances (d1 < ratio^2 * d2) before the grid walk (north_star option) */
} mi355_params;

void mi355_default_params(mi355_params* p);

/* ---- context -------------------------------------------------------------------------------------- */
int  mi355_create(mi355_ctx** out, const mi355_params* params /* NULL = defaults */, int device_ordinal);
void mi355_destroy(mi355_ctx* ctx);
const char* mi355_last_error(mi355_ctx* ctx);          /* ctx may be NULL: last creation error */
/* Run on a caller-provided hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = ctx-owned stream. */
int  mi355_set_stream(mi355_ctx* ctx, void* hip_stream);
int  mi355_synchronize(mi355_ctx* ctx);
/* Tunables: "sift_batch" = frames per detect+describe batch (1..32, default 16): frames handed to mi355_sift_extract_dev
 * collect until the batch is full (or until a call needs their features) and are then enqueued together, every pyramid
 * level and every keypoint stage of all frames of the batch in one launch each; batches of very large frames are shortened
 * so that the work areas stay under 60 % of the device memory, keep-all batches (nfeatures <= 0) hold at most 8;
 * "sift_slots" = batch work areas that may be in flight at once, each on its own stream (1..4, default 3; a work area
 * holds the pyramids and candidate lists of one batch); "blur_stream" = 1 (default) runs pyramid levels of at least 384
 * columns (512 with "narrow_routes" = 0) and 64 rows whose width is a multiple of 4 (with a last 256-column strip that is full or wider than 16) through the barrier-free streaming Gaussian and lets big octaves
 * take the streamed extrema kernel, 0 forces the tiled kernels everywhere (same bits either way);
 * "xstream_min_w" (>= 256, default 1000) / "xstream_min_frames" (>= 1, default 4): octaves at least that wide and 3/4 as
 * high, in batches of at least that many frames, take the streamed extrema kernel instead of the tiled one (same candidates
 * either way); "narrow_routes" = 1 (default): the streaming Gaussian also takes levels of 384 to 508 columns, and a launch of
 * it that 64-row segments would leave with fewer waves than the chip has slots for runs in shorter segments (16 to 64 rows,
 * about two waves per SIMD), 0: the routes as they were before the option (same bits either way); "serial_heavy" = 1 (measurement only, default 0): the pyramid + extrema phase of a batch waits for the previous
 * batch's, so that the chip-filling kernels of different batches never overlap and their event-bracketed durations are
 * exclusive (the whole job loses ~10 %); "sift_cascade" and "keepall_order" are accepted and ignored (the kernels they chose
 * between are gone); "profile_every:<class>" = n (measurement only, default 1): with
 * mi355_profile_enable only every n-th launch of that kernel class is bracketed by events (the average duration is then a sample);
 * "keep_frames" = 1 (default 0): host-frame extractions keep their HBM copy (see mi355_get_frame_dev); "download_chunk_mb" (default 64):
 * bytes per chunk, in MB, of the _into calls' canvas download; "download_threads" (1..16, default 4): host threads that copy a downloaded
 * chunk into the caller's rows; "download_mode" (measurement only, default 0): 1 copies with hipMemcpy2DAsync straight into dst,
 * 2 page-locks dst with hipHostRegister for that copy (the same bytes in every mode); "keepall_max" (a multiple of 2048 in
 * [32768, 262144], default 32768): the most keypoints a keep-all frame (nfeatures <= 0) may hold -- a frame with more fails its
 * extraction ("... more than keepall_max=N"), mi355_set_features / mi355_select_grid / the pair stage / the chunk install and pack refuse
 * more rows; resolves pending extractions first; any other value, or one below the keypoint count of a resident image (named in the
 * error), returns MI355_ERR_ARG and leaves the ceiling as it was.  Every rank of a multi-GPU run sets the same value: a rank whose ceiling
 * is below a frame it receives fails its install (MI355_ERR_ARG, its features unchanged) while the other ranks return normally;
 * "big_subpairs_max" (debug, default 65536): sub-pairs of <= 2048 x 2048 per run of the matcher's large-pair path (the same
 * results at any value >= 1); "select_margin" (0 .. 65536, default 256): top-k SIFT orients the strongest nfeatures + margin refined
 * points first and the rest only if fewer than nfeatures keypoints came of them -- the same keypoints at any value, a small margin makes
 * that second pass likely (mi355_last_sift_counters: out8[5] = 1 where it ran); resolves pending extractions first;
 * "nfeatures" (<= 2048; <= 0: keep-all): mi355_params.nfeatures for the extractions that follow, frames already extracted keep their
 * features; resolves pending extractions first. */
int  mi355_set_option(mi355_ctx* ctx, const char* name, int value);
void mi355_free(void* p);                               /* frees host buffers returned by this library */

/* ---- features: replaces the body of SiftExtraction_Thread, MosaicWithoutPos.cpp:4861-4881 ----------- */
/* BGR u8 host image in, keypoints + 128-D descriptors out (desc128: n x 128 floats holding the integers
 * 0..255 like OpenCV's SIFT; either output may be NULL).  Features stay device-resident under img_id for
 * mi355_match_pairs (the reference round-trips them through d:/feature_temp files instead).  With kp, desc128 and n_kp all
 * NULL nothing is waited for: the frame is copied into a staging ring in HBM (bgr may be reused on return) and joins a
 * batch like a device frame -- the fast way to feed host images.
 * Sizes: w and h are at least 16 (smaller: MI355_ERR_ARG, decided on the host before any launch; the ctx stays usable) and below 2^20,
 * keep-all frames at most 16384 x 16384.  Octave 0 is the image itself; cv::SIFT's count is cvRound(log2(min(w, h)) - 2), and octaves are
 * built while both sides have at least 12 samples (no keypoint fits a smaller one: 5 border samples a side) -- for every size the 12-sample
 * stop comes first, so octave o exists exactly when min(w, h) >> o >= 12.
 * Ties at the cut: like KeyPointsFilter::retainBest, every keypoint whose |response| equals the nfeatures-th is kept; a feature record
 * holds 2048 rows, and a frame whose tie group reaches past them (periodic content: identical structures by the hundred) fails with
 * MI355_ERR_FAILED ("... overflow ...") instead of being cut short -- nothing is stored under img_id, the ctx stays usable, and keep-all
 * mode (nfeatures <= 0) takes such frames. */
int  mi355_sift_extract(mi355_ctx* ctx, int img_id, const uint8_t* bgr, int w, int h, int width_step,
                        mi355_keypoint* kp, float* desc128, int max_kp, int* n_kp);
/* Same, image already in HBM (device pointer); nothing is copied back.  With n_kp == NULL the call returns at once and
 * the frame joins the current batch (see "sift_batch"): d_bgr must stay valid and unchanged until a call that needs the
 * features (match, get_features, synchronize) has returned. */
int  mi355_sift_extract_dev(mi355_ctx* ctx, int img_id, const uint8_t* d_bgr, int w, int h, int width_step, int* n_kp);
/* Fetch / install device-resident features (LoadSurfKeyPoints / WriteSurfKeyPoints counterparts,
 * MosaicWithoutPos.cpp:4682-4734).  desc128 holds integer-valued floats. */
int  mi355_get_features(mi355_ctx* ctx, int img_id, mi355_keypoint* kp, float* desc128, int max_kp, int* n_kp);
int  mi355_set_features(mi355_ctx* ctx, int img_id, const mi355_keypoint* kp, const float* desc128, int n_kp, int w, int h);
int  mi355_drop_features(mi355_ctx* ctx, int img_id);   /* img_id < 0: all */

/* ---- match + select + RANSAC for a batch of pairs ------------------------------------------------------
 * replaces the j-loop body MosaicWithoutPos.cpp:5084-5232 (FLANN match -> sort -> SelectMatchPairs ->
 * Ransac2D -> accept).  pairs: n_pairs x {i,j} image ids with features resident.  seed plays the role of
 * time(0) in srand((unsigned)time(0)), mosaicimage.h:1777 (every pair of the batch uses it, as all pairs the
 * reference processes within one second do).  out: host array of n_pairs results. */
int  mi355_match_pairs(mi355_ctx* ctx, const int32_t* pairs_ij, int n_pairs, float ransac_dist, uint32_t seed,
                       mi355_pair_result* out);
/* Same, results left in HBM at d_out (device pointer to n_pairs records), e.g. as the RCCL all-gather input. */
int  mi355_match_pairs_dev(mi355_ctx* ctx, const int32_t* pairs_ij, int n_pairs, float ransac_dist, uint32_t seed,
                           mi355_pair_result* d_out);
/* Exact brute-force 1-NN / 2-NN (replaces cv::FlannBasedMatcher().match, MosaicWithoutPos.cpp:5108-5110,
 * with the exact answer): squared L2 distances as int32, sorted=1 orders the output by (distance, queryIdx)
 * like std::sort(matches) at :5111.  second_d2 may be NULL. Returns number of matches in *n_matches (= K_i). */
int  mi355_bf_match(mi355_ctx* ctx, int img_i, int img_j, int sorted, mi355_dmatch* matches, int32_t* d2, int32_t* second_d2,
                    int max_matches, int* n_matches);

/* ---- stand-alone pieces with the reference's semantics ------------------------------------------------ */
/* SelectMatchPairs (grid form), MosaicWithoutPos.cpp:4977-5028. sorted: matches already ordered. */
int  mi355_select_grid(mi355_ctx* ctx, const mi355_dmatch* sorted, int n, const float* kp1_xy, int n_kp1,
                       const float* kp2_xy, int n_kp2, int nMatch, int width, int height, int gridX, int gridY,
                       mi355_sfpoint* v1, mi355_sfpoint* v2, int* n_out);
/* Ransac2D<SfPoint>, mosaicimage.h:1729-2035.  Returns 1/0 like the bool (or <0 on error). */
int  mi355_ransac2d(mi355_ctx* ctx, const mi355_sfpoint* p1, const mi355_sfpoint* p2, int n, float dist, int sample_times,
                    uint32_t seed, mi355_sfpoint* in1, mi355_sfpoint* in2, int* n_in, float H[9]);
/* ImageProjectionTransform(BitmapImage*, BitmapImage*&, float h[9]), MosaicImage.cpp:1613-1758.
 * *dst is allocated by the library (rows padded to (w*ch+3)/4*4 like CreateBitmap8U) -> mi355_free. */
int  mi355_warp_image(mi355_ctx* ctx, const uint8_t* src, int w, int h, int ws, int ch, const float h9[9],
                      uint8_t** dst, int* dw, int* dh, int* dws);
/* CMosaicByPose::MosaicImagesRefined (float), MosaicWithoutPos.cpp:2194-2352: bbox of all images with
 * h[8]!=0, zeroed 3-channel canvas, per-image inverse bilinear warp, later images overwrite earlier ones.
 * *canvas allocated by the library -> mi355_free. */
int  mi355_mosaic_refined(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n,
                          const float* h9s /* n x 9 */, uint8_t** canvas, int* cw, int* ch, int* cws);
/* Canvas geometry only (MosaicWithoutPos.cpp:2199-2249): size and the (dGX,dGY) shift. */
int  mi355_mosaic_layout(const int* w, const int* h, int n, const float* h9s, int* cw, int* ch, int* cws, float* dGxy);
/* Device-resident form: d_imgs[k] and d_canvas are device pointers; canvas must hold cws*ch bytes and is
 * zeroed by the call.  Only canvas rows [row0, row0+rows) are rendered (canvas stripes for multi-GPU,
 * SURVEY 8e); pass 0, ch for the whole canvas. */
/* d_imgs[k] == NULL: the caller holds no copy of image k and thereby states that these rows do not read it (owner-only frames: the pointers
 * mi355_exchange_frames returns; true of an image that lies under later ones wherever its box meets the rows, MI355_COVER_REFINED_EXACT); the
 * image is left out of the walk.  mi355_set_option("strict_frames", 1) checks the statement first (one extra pass) and names an image that is
 * read after all (MI355_ERR_ARG). */
int  mi355_mosaic_refined_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n,
                              const float* h9s, uint8_t* d_canvas, int cw, int ch, int cws, int row0, int rows);

/* ---- weighted (feather) blending: the third one-pass render (csrc/feather.hip) -----------------------------------------------------
 * UavMatchParam.blending = 1 (MosaicWithoutPos.h:65: 0 none, 1 weighted, 2 multiband).  The reference declares the mode and renders it
 * unblended (MosaicWithoutPos.cpp:4666-4672); its MergeMultiImages2 is unreachable and order-dependent and is NOT what is computed here.
 * Definition (exact integers; the bytes do not depend on frame order, tile shape or stripe cut):
 *   Canvas geometry, frames and skipping are mi355_mosaic_refined_dev's: canvas = mi355_mosaic_layout; frames with h9[8] == 0 or without an
 *   inverse are skipped.  "Frame k gives canvas pixel (x, y) a sample" is the refined render's own statement: the pixel lies in k's clipped
 *   canvas box, the source coordinate (xs, ys) (unit_den / two-division choice as there) lies in [0, w-1) x [0, h-1), and the sample s_k[c],
 *   c = B, G, R, is hm::bilin of the 2 x 2 texels at xi = (int)xs, yi = (int)ys with p = ys - yi, q = xs - xi.
 *   Weight of a w x h frame with ramp R >= 1 (source pixels), for texel (i, j):
 *     d(i, j)  = min(i, w-1-i, j, h-1-j)                       integer border distance
 *     Wk(i, j) = (254 * min(d, R)) / R                         integer division, in [0, 254]
 *     omega_k  = 1 + hm::bilin(Wk(xi,yi), Wk(xi+1,yi), Wk(xi,yi+1), Wk(xi+1,yi+1), p, q)          in [1, 255]
 *   i.e. omega_k - 1 is the byte the refined render would take from a frame whose pixels are Wk.  Wk is evaluated arithmetically; no weight
 *   image is stored.  params.ramp > 0: R = ramp for every frame; ramp == 0 (default): per frame R = (min(w, h) + 1) / 2, a full tent.
 *   out[c] = (sum_k omega_k * s_k[c] + (sum_k omega_k) / 2) / sum_k omega_k                        integer division
 *   over every frame k that gives the pixel a sample; a pixel no frame covers is 0; row padding [3 cw, cws) is 0.  With n <= 65535 every sum
 *   fits 32 unsigned bits (255 * 255 * 65535 + 255 * 65535 / 2 < 2^32).
 * Consequences: where exactly one frame covers a pixel the byte is the refined render's; every byte lies between the smallest and the
 *   largest contributing sample; after mi355_gain_compensate_dev the canvas is the feathered render of the compensated frames.
 * Cost: one launch over canvas tiles, no chips, masks or pyramids; every covering frame is sampled (C5: ~60 per pixel).  No cap on layers.
 * Stripes: row0, rows, and the whole canvas's cw, ch, cws, as mi355_mosaic_refined_dev; a canvas row depends only on the frames whose box
 *   meets it, so MI355_COVER_REFINED is exactly the set of frames a stripe reads.  d_imgs[k] == NULL for such a frame is MI355_ERR_ARG
 *   whatever "strict_frames" says (there is no "lies under later frames" case); NULL for a frame outside the cover is fine.
 * Errors: as the refined twins (argument checks, n <= 1 -> MI355_ERR_FAILED in the host forms, n > 65535, canvas geometry); params NULL =
 *   defaults; ramp < 0 -> MI355_ERR_ARG; a contributing frame wider or higher than 2^20 -> MI355_ERR_ARG. */
typedef struct { int32_t ramp; int32_t reserved[3]; } mi355_feather_params;
void mi355_default_feather_params(mi355_feather_params* p);          /* ramp = 0, reserved = 0 */
int  mi355_mosaic_feathered_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n,
                                const float* h9s, const mi355_feather_params* params, uint8_t* d_canvas, int cw, int ch, int cws, int row0, int rows);
/* host images in, *canvas allocated by the library -> mi355_free (mi355_mosaic_refined's form) */
int  mi355_mosaic_feathered(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n,
                            const float* h9s, const mi355_feather_params* params, uint8_t** canvas, int* cw, int* ch, int* cws);

/* ---- seamline render: the fourth one-pass render, each canvas pixel from its deepest frame (csrc/seamline.hip) -----------------------
 * What orthomosaic tools call a Voronoi seamline: every canvas pixel is taken from exactly ONE frame, the frame in which it lies deepest, so
 * the canvas is as sharp as the unblended render while its seams run through the middle of the overlaps, not along the outlines of late frames.
 * Definition (exact integers; bytes, owner and count do not depend on walk order, tile shape or stripe cut):
 *   Canvas geometry, frame skipping, "frame k gives canvas pixel (x, y) a sample", the sample s_k[c] and the weight omega_k in [1, 255] are
 *   exactly the feathered render's (above), including params.ramp, the default R = (min(w, h) + 1) / 2 and the 2^20 side limit.
 *   owner   = argmax over the contributing frames k of (omega_k, k): the largest weight wins, among equal weights the largest index k (the
 *             position in the caller's arrays) -- the direction of "later frames overwrite" in the refined render;
 *   out[c]  = s_owner[c]; a pixel no frame covers is 0; row padding [3 cw, cws) is 0;
 *   d_owner (optional): uint16_t, the whole canvas's ch x cw at a pitch of cw elements: owner + 1, or 0 where nothing covers the pixel;
 *   d_count (optional): same layout: the number of contributing frames (count > 0 is the no-data mask of all three one-pass renders).
 *   n <= 65535.  Only rows [row0, row0 + rows) of the canvas and of either map are written.
 * Consequences: where count == 1 the bytes are those of the refined render and of the feathered render; count > 0 is exactly the set of pixels
 *   the refined and feathered renders cover; after mi355_gain_compensate_dev the canvas is the seamline render of the compensated frames.
 * Cost: one launch over canvas tiles; the ownership walk maps, tests and weighs every covering frame and loads no texel, then ONE frame is
 *   sampled per pixel.
 * Pointers: d_canvas, d_owner, d_count may each be NULL, at least one must not be.  d_canvas == NULL: nothing is sampled, d_imgs (and ws) may be
 *   NULL altogether.  d_canvas != NULL: a frame that owns no pixel of the rows may have d_imgs[k] == NULL; NULL for a frame that does own one is
 *   MI355_ERR_ARG naming the frame, found before any sample is taken (one extra ownership pass, paid only when some pointer is NULL); no
 *   invalid pointer is dereferenced and the ctx stays usable.
 * mi355_mosaic_seamline_cover: need[k] = 1 exactly for the frames that own at least one pixel of the rows -- the ownership walk with nothing
 *   sampled; what a rank must hold to render the stripe (feeds mi355_exchange_frames with MI355_EXCHANGE_NEED_IS_LOCAL, as
 *   MI355_COVER_REFINED_EXACT does for the refined render).  mi355_mosaic_stripe_cover is unchanged.
 *   A frame the render skips -- h9[8] == 0, or no inverse (a homography of rank 2, say) -- follows the refined render's rule here as in the
 *   render: it owns no pixel, so need[k] = 0 and d_imgs[k] may be NULL, while the corners of a frame with h9[8] != 0 still count for the
 *   layout (mi355_mosaic_layout).  The same holds for mi355_mosaic_median_cover and for the feathered render's box cover.
 * Errors: as the feathered twins (argument checks, n <= 1 -> MI355_ERR_FAILED in the host forms, n > 65535, canvas geometry, ramp < 0, frame
 *   geometry); params NULL = defaults. */
typedef struct { int32_t ramp; int32_t reserved[3]; } mi355_seamline_params;   /* ramp as in mi355_feather_params */
void mi355_default_seamline_params(mi355_seamline_params* p);        /* ramp = 0, reserved = 0 */
int  mi355_mosaic_seamline_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n,
                               const float* h9s, const mi355_seamline_params* params, uint8_t* d_canvas, int cw, int ch, int cws,
                               uint16_t* d_owner, uint16_t* d_count, int row0, int rows);
/* host images in; *canvas and, when owner != NULL, *owner (ch x cw) are allocated by the library -> mi355_free */
int  mi355_mosaic_seamline(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n,
                           const float* h9s, const mi355_seamline_params* params, uint8_t** canvas, int* cw, int* ch, int* cws, uint16_t** owner);
int  mi355_mosaic_seamline_cover(mi355_ctx* ctx, const int* w, const int* h, int n, const float* h9s, const mi355_seamline_params* params,
                                 int row0, int rows, uint8_t* need);

/* ---- median render: the fifth one-pass render, each canvas pixel the median of its deepest frames (csrc/median.hip) ------------------
 * What moves between exposures -- a car on a road, a person, a drifting shadow -- shows in a minority of the looks a deep survey has at a piece
 * of ground.  The feathered mean leaves a ghost of it, the seamline and refined renders cut it at a seam or print it once, multiband smears
 * it over the low bands; a per-pixel median across the looks makes it drop out.  The reference has no such mode.
 * Definition (exact integers; bytes and maps do not depend on walk order, tile shape or stripe cut):
 *   Canvas geometry, frame skipping, "frame k gives canvas pixel (x, y) a sample", the sample s_k[c] and the weight omega_k in [1, 255] are
 *   exactly the feathered render's (above), including params.ramp, the default R = (min(w, h) + 1) / 2, the 2^20 side limit and n <= 65535.
 *   params.depth: 0 = the default, 5; 1 .. MI355_MEDIAN_MAX_DEPTH as given.
 *   Per pixel: C = the set of contributing frames, m = min(|C|, depth), S = the m frames of C that are largest in the lexicographic order
 *   (omega_k, k) -- the seamline order: the deepest frames first, equal weights by the larger caller index.  For each channel c the m values
 *   s_k[c], k in S, sorted ascending are v_0 .. v_{m-1}.
 *   out[c]   = (v[(m-1) >> 1] + v[m >> 1] + 1) >> 1: the median for odd m, the rounded mean of the two middle values for even m; a pixel no
 *              frame covers is 0; row padding [3 cw, cws) is 0;
 *   d_count  (optional): uint16_t, the whole canvas's ch x cw at a pitch of cw elements: |C| -- the seamline render's count map;
 *   d_spread (optional): uint8_t, ch x cw at a pitch of cw bytes: max over c of (v_{m-1} - v_0), 0 where m <= 1: where the selected looks
 *              disagree -- moving objects, misregistration, exposure.  The samples are in registers anyway.
 *   Only rows [row0, row0 + rows) of the canvas and of either map are written.
 * Consequences: with depth = 1 the canvas bytes are the seamline render's at the same ramp; where count == 1 the bytes are the refined
 *   render's; every byte lies between the smallest and the largest selected sample; after mi355_gain_compensate_dev the canvas is the median
 *   render of the compensated frames.
 * Cost: one launch over canvas tiles; the selection walk maps, tests and weighs every covering frame and loads no texel, keeping a sorted
 *   top-`depth` per pixel in registers; then at most `depth` frames are sampled per pixel.
 * Pointers: d_canvas, d_spread, d_count may each be NULL, at least one must not be.  d_canvas == NULL and d_spread == NULL: nothing is sampled,
 *   d_imgs (and ws) may be NULL altogether.  Otherwise a frame that is in S for no pixel of the rows may have d_imgs[k] == NULL; NULL for a frame
 *   that is in S somewhere is MI355_ERR_ARG naming the frame, found before any sample is taken and before anything is written (one extra
 *   selection pass, paid only when some pointer is NULL); no invalid pointer is dereferenced and the ctx stays usable.
 * mi355_mosaic_median_cover: need[k] = 1 exactly for the frames that are in S for at least one pixel of the rows -- the selection walk with
 *   nothing sampled; what a rank must hold to render the stripe (as mi355_mosaic_seamline_cover).
 * Errors: as the seamline twins (argument checks, n <= 1 -> MI355_ERR_FAILED in the host forms, n > 65535, canvas geometry, ramp < 0, frame
 *   geometry); depth < 0 or depth > MI355_MEDIAN_MAX_DEPTH -> MI355_ERR_ARG; params NULL = defaults. */
#define MI355_MEDIAN_MAX_DEPTH 9
typedef struct { int32_t ramp; int32_t depth; int32_t reserved[2]; } mi355_median_params;   /* ramp as in mi355_feather_params */
void mi355_default_median_params(mi355_median_params* p);            /* ramp = 0, depth = 0 (5), reserved = 0 */
int  mi355_mosaic_median_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n,
                             const float* h9s, const mi355_median_params* params, uint8_t* d_canvas, int cw, int ch, int cws,
                             uint8_t* d_spread, uint16_t* d_count, int row0, int rows);
/* host images in; *canvas and, when spread != NULL, *spread (ch x cw bytes) are allocated by the library -> mi355_free */
int  mi355_mosaic_median(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n,
                         const float* h9s, const mi355_median_params* params, uint8_t** canvas, int* cw, int* ch, int* cws, uint8_t** spread);
int  mi355_mosaic_median_cover(mi355_ctx* ctx, const int* w, const int* h, int n, const float* h9s, const mi355_median_params* params,
                               int row0, int rows, uint8_t* need);

/* ---- optimised seamlines: a cost-aware owner map on a grid of canvas cells, and the render that follows it (csrc/seamcut.hip) ----------
 * The seamline render cuts every overlap down its geometric middle, whatever is there.  Here the seam is moved, cell by cell, to where the two
 * frames agree: three stages, integers throughout, restated in numpy by tests/seamcut_ref.py.  The reference has no such mode.
 * Grid: cells of s x s canvas pixels, s = 1 << level, gw = ceil(cw / s) by gh = ceil(ch / s) over the canvas of mi355_mosaic_layout; the probe
 *   of cell (cx, cy) is canvas pixel (min(cx s + s / 2, cw - 1), min(cy s + s / 2, ch - 1)).
 * 1. Candidates (mi355_seam_candidates_dev).  Which frames give the probe a sample, and their weight omega, are the seamline render's own
 *   statement (frame skipping, params.ramp, the 2^20 side limit, n <= 65535 included).  The cell's candidates are the m = min(|C|, depth)
 *   contributing frames that are largest in the seamline order (omega, k): slot 0 is the seamline owner of the probe, slots m .. 7 are empty
 *   (all fields 0).  A slot holds frame + 1, omega, and the gray signature: (sum + num / 2) / num over the num >= 1 pixels of the cell, clipped
 *   to the canvas, at which that frame gives a sample, of the gray (1868 B + 9617 G + 4899 R + 8192) >> 14 of the sample bytes.  A cell mean, not
 *   the probe's one sample: one bilinear sample carries the texture's sub-pixel disagreement, and every seam would look expensive.
 * 2. Labels (mi355_seam_labels_dev; mi355_seam_labels_host gives the same bits without a GPU).  32-bit integers:
 *     D(p, a)  = data_weight (omega_0(p) - omega_a(p))                                     slot a of cell p
 *     V        = 0 where 4-neighbour cells p, q carry the same frame, else seam_penalty + diff_weight (d(p) + d(q)), with
 *     d(x)     = |g_k(x) - g_l(x)| where the two frames k, l are both candidates of cell x, else miss_cost
 *     L_r(p, a) = D(p, a) + min_b [L_r(p - r, b) + V] - min_b L_r(p - r, b)                for each of the four axis directions r,
 *                 = D(p, a) at the start of a path and behind a cell without candidates
 *     S(p, a)  = sum_r L_r(p, a); the label of p is the argmin over its filled slots of (S, a): the lower slot -- the deeper frame -- wins a tie.
 *   L_r <= 16 * 254 + 255 + 16 * 510 = 12479, S < 2^16.  The energy of a labelling is sum_p D + sum V over the 4-neighbour pairs whose cells both
 *   have a candidate (64-bit).  energy_before is that of the all-slot-0 labelling, which is the seamline render's; energy_after that of the
 *   argmin labelling.  If energy_after > energy_before the all-slot-0 labelling is returned and `fallback` set: by its own measure the result
 *   is never worse than the seamline render.  `changed` counts the cells of the RETURNED labelling whose label is not slot 0.
 *   Cell map: uint16_t [gh][gw]: frame + 1 where the returned label is not slot 0, and 0 elsewhere -- a cell without candidates, and a cell that
 *   keeps its slot 0: there the render keeps the seamline rule pixel by pixel, so that a labelling which moves nothing IS the seamline render
 *   (a cell that named its probe's owner would pull the whole cell to that frame and turn every untouched seam into a staircase).
 * 3. Render (mi355_mosaic_seamcut_dev): the seamline render with one more input.  For pixel (x, y), f = cells[y >> level][x >> level] - 1: if
 *   f >= 0 and frame f gives the pixel a sample the owner is f, else the seamline owner; out = s_owner; d_owner, d_count, stripes (row0, rows),
 *   row padding as the seamline render.  d_cells == NULL: stages 1 and 2 run first, over the whole canvas, into a map the ctx keeps -- on every
 *   call, and stage 1 needs every frame it does not skip, so no pointer may be withheld in this form: render stripes, and withhold frames
 *   by mi355_mosaic_seamcut_cover, with a map made once by mi355_seam_cells_dev.
 * Consequences: an all-zero cell map, depth = 1, and diff_weight = seam_penalty = 0 each give the seamline render's bytes, owner and count;
 *   energy_after <= energy_before or the fallback is set; the count map does not depend on the cell map.
 * Cost: stage 1 samples what a depth-`depth` median render samples (each candidate over its cell) in one launch of one wave per cell; stage 2
 *   is four launches of one wave per scanline, a sequential chain of 8 x 8 slot pairs per step, plus three per-cell passes over 32 + 16 + 3
 *   bytes a cell; stage 3 is the seamline render plus one map load per lane and row.
 * Pointers: stage 1 reads every frame the renders do not skip: d_imgs[k] == NULL for one of them is MI355_ERR_ARG naming it.  Stage 3 follows
 *   the seamline render: a frame that owns no pixel of the rows under the rule above may be NULL; NULL for one that does is MI355_ERR_ARG before
 *   anything is written.  mi355_mosaic_seamcut_cover: need[k] = 1 exactly for the frames that own a pixel of the rows under that rule.
 * Errors: every field of the parameters is range-checked -- ramp >= 0, level 2..5, depth 1..8, data_weight and diff_weight 0..16, seam_penalty
 *   and miss_cost 0..255 -- MI355_ERR_ARG outside; gw, gh must be the layout's at params.level; otherwise as the seamline twins.
 * The cost defaults are data_weight 1, diff_weight 2, seam_penalty 2, miss_cost 32.  diff_weight was raised from the first value 1 after the
 *   quality measurement: on small frames, where omega falls by 8 a pixel, no rectangle placed astride the seam was given to one owner at 1, 57
 *   of the 355 searched two- and three-frame placements were at 2 and 85 at 4; a larger seam_penalty changed nothing (scratch/seamcut_quality.py,
 *   profiles/seamcut_quality.json).  A rectangle placed symmetrically on the seam stays cut at any of them: DESIGN 5 says why. */
#define MI355_SEAMCUT_MAX_DEPTH 8
typedef struct { int32_t ramp, level, depth, data_weight, diff_weight, seam_penalty, miss_cost, reserved; } mi355_seamcut_params;
typedef struct { uint16_t frame[MI355_SEAMCUT_MAX_DEPTH]; uint8_t omega[MI355_SEAMCUT_MAX_DEPTH]; uint8_t gray[MI355_SEAMCUT_MAX_DEPTH]; } mi355_seam_cell;   /* 32 bytes */
typedef struct { int64_t energy_before, energy_after; int32_t changed, fallback; } mi355_seam_report;
void mi355_default_seamcut_params(mi355_seamcut_params* p);          /* ramp 0, level 3, depth 4, data_weight 1, diff_weight 2, seam_penalty 2, miss_cost 32 */
int  mi355_seam_candidates_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                               const mi355_seamcut_params* params, mi355_seam_cell* d_cand /* DEVICE, gh x gw */, int gw, int gh);
int  mi355_seam_labels_dev(mi355_ctx* ctx, const mi355_seam_cell* d_cand, int gw, int gh, const mi355_seamcut_params* params,
                           uint16_t* d_cells /* DEVICE, gh x gw */, mi355_seam_report* report /* HOST, may be NULL */);
int  mi355_seam_labels_host(const mi355_seam_cell* cand, int gw, int gh, const mi355_seamcut_params* params, uint16_t* cells, mi355_seam_report* report);
/* stages 1 and 2, the records in a buffer of the ctx */
int  mi355_seam_cells_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                          const mi355_seamcut_params* params, uint16_t* d_cells, int gw, int gh, mi355_seam_report* report);
int  mi355_mosaic_seamcut_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                              const mi355_seamcut_params* params, const uint16_t* d_cells, uint8_t* d_canvas, int cw, int ch, int cws,
                              uint16_t* d_owner, uint16_t* d_count, int row0, int rows);
/* host images in, all three stages; *canvas and, when owner != NULL, *owner (ch x cw) are allocated by the library -> mi355_free */
int  mi355_mosaic_seamcut(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                          const mi355_seamcut_params* params, uint8_t** canvas, int* cw, int* ch, int* cws, uint16_t** owner);
int  mi355_mosaic_seamcut_cover(mi355_ctx* ctx, const int* w, const int* h, int n, const float* h9s, const mi355_seamcut_params* params,
                                const uint16_t* d_cells /* DEVICE */, int row0, int rows, uint8_t* need);

/* LaplacianPyramidBlending warp stage (MosaicImage.cpp:2233-2460) + FindMasksByDistMap (:1761-1881):
 * per kept image a tight chip (3ch u8; the reference then converts to CV_16S), its validity mask and, with
 * find_masks!=0, the exclusive distance-map ownership masks.  h9s must carry the resScale multiplication of
 * m[0..5] (:2216-2223); keep[k] = vecAbandonInd (NULL = keep all). Outputs are library-allocated arrays of
 * n_chips buffers (free each and the arrays with mi355_free). */
typedef struct { int32_t x0, y0, w, h, img; float sx, sy; float quad[8]; } mi355_chip_info;
int  mi355_chips_and_masks(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n,
                           const float* h9s, const uint8_t* keep, int find_masks,
                           int* n_chips, mi355_chip_info** chips, uint8_t*** chip_imgs, uint8_t*** masks,
                           int* canvas_w, int* canvas_h);

/* ResampleByOverlap(pImages, n, overlapT, pImgT, vecAbandonInd), MosaicImage.cpp:2069-2201 (LaplacianPyramidBlending calls it with
 * overlapT = 0.7f, :2227-2230): keep[k] = vecAbandonInd[k] -- image k is dropped (0) when the quadrilateral it covers overlaps an
 * earlier KEPT image's by more than overlapT of its own area; image 0 and image n-1 are always kept.  Host geometry (no ctx): the
 * result is the keep[] argument of the two calls around it.  h9s must already carry the resScale multiplication (:2216-2223). */
int  mi355_resample_by_overlap(const int* w, const int* h, int n, const float* h9s, float overlapT, uint8_t* keep);

/* Multiband blend of those chips ("next" row f3 of SURVEY 8f): replaces detail::MultiBandBlender blender(false, band) --
 * prepare(Rect(0,0,canvas_w,canvas_h)), feed(chip as CV_16S, mask, corner) per chip, blend, convertTo(CV_8U)
 * (MosaicImage.cpp:2296-2299, 2451-2486; the reference passes band = 5).  chips / masks / info exactly as
 * mi355_chips_and_masks returns them (BGR u8 rows padded to 4 bytes, masks after FindMasksByDistMap).  The arithmetic of
 * OpenCV 2.4.0's blender is not available: the definition is the one in oracle/oracle_blend.c (parity unpinned).
 * *out: BGR u8 canvas, rows padded to 4 bytes, library-allocated (mi355_free). */
int  mi355_multiband_blend(mi355_ctx* ctx, const uint8_t* const* chips, const uint8_t* const* masks, const mi355_chip_info* info, int n,
                           int canvas_w, int canvas_h, int band, uint8_t** out, int* out_w, int* out_h, int* out_ws);

/* Both stages in one call, chips and masks never leaving HBM: the whole of LaplacianPyramidBlending(pImages, n, pImgT, band, ...)
 * (MosaicImage.cpp:2205-2510) except that the inputs are NOT released (the adaptor does that, :2464-2467).  Same bytes as
 * mi355_chips_and_masks(find_masks = 1) followed by mi355_multiband_blend. */
int  mi355_mosaic_blended(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                          const uint8_t* keep, int band, uint8_t** out, int* out_w, int* out_h, int* out_ws);

/* Device form for surveys that live in HBM (C5: 2000 frames + chips + masks + distance maps + the blender's pyramids co-resident):
 * d_imgs are DEVICE pointers (no staging copy), the finished canvas is written to the caller's DEVICE buffer d_canvas whose
 * geometry (cw, ch, cws = rows padded to 4 bytes) must be what mi355_blend_layout returns for the same arguments.  Same bytes as
 * mi355_mosaic_blended.  Returns when the work is enqueued on the ctx stream (mi355_synchronize). */
int  mi355_mosaic_blended_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                              const uint8_t* keep, int band, uint8_t* d_canvas, int cw, int ch, int cws);
/* One horizontal STRIPE of that canvas: rows row0 .. row0 + rows - 1 go to d_rows (rows x cws bytes; cw, ch, cws are still the WHOLE
 * canvas's, from mi355_blend_layout).  This is a rank's share of the reference's default compositing path (blending = 2,
 * MosaicWithoutPos.h:57-79 -> LaplacianPyramidBlending, MosaicImage.cpp:2205-2510) when the canvas is cut into G stripes like
 * mi355_mosaic_refined_dev's: the rank forms the chips that reach its rows plus the pyramids' reach (3 * 2^band rows of feed gap, the
 * REDUCE / EXPAND taps per level), FindMasksByDistMap's ownership there (MosaicImage.cpp:1842-1872: per canvas pixel) and the rows of
 * every blender level its output depends on (MosaicImage.cpp:2296-2299, 2471-2486).  Stripes put side by side are the bytes of
 * mi355_mosaic_blended_dev, whatever the cut. */
int  mi355_mosaic_blended_rows_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                   const uint8_t* keep, int band, uint8_t* d_rows, int cw, int ch, int cws, int row0, int rows);
/* canvas size of LaplacianPyramidBlending for these transforms (MosaicImage.cpp:2233-2292; host geometry, no ctx) */
int  mi355_blend_layout(const int* w, const int* h, int n, const float* h9s, const uint8_t* keep, int* cw, int* ch, int* cws);

/* ---- multiband blend along optimised seams (csrc/blend_seam.hip) -----------------------------------------------------------------------
 * The multiband blend cuts every overlap where FindMasksByDistMap puts the seam: along the geometric middle, whatever lies there.  Here the
 * seam finder of the optimised seamlines runs in front of the blender: a cell map moves the seam, cell by cell, to where the chips agree, the
 * ownership masks follow the map, and the blender takes those masks as it takes any.  The cell map of mi355_seam_cells_dev cannot be reused: it
 * lives on mi355_mosaic_layout's canvas under the seamline's sample rule and feather weights, while the blend's canvas always contains the
 * origin, its chips carry sub-pixel shifts and its seam is the normalised-distance arg-max.  Integers everywhere except where the ownership's
 * own float expression is reused; restated in numpy by tests/blend_seam_ref.py.  The reference has no such mode.
 * Grid: the canvas is mi355_blend_layout's (cw x ch) for the same w, h, n, h9s, keep; s = 1 << level, gw = ceil(cw / s), gh = ceil(ch / s); the
 *   probe of cell (cx, cy) is pixel (min(cx s + s / 2, cw - 1), min(cy s + s / 2, ch - 1)), as above.  Parameters: mi355_seamcut_params with the
 *   same ranges and defaults; ramp has no meaning here and must be 0 (MI355_ERR_ARG otherwise).  n <= 65535.
 * 1. Candidates.  For a chip v that covers canvas pixel p with validity byte 255, d_v(p) is the value FindMasksByDistMap compares there: the
 *   distance to the nearest of the chip's four edge lines divided by the chip's maximum of it (over the whole chip), the same float bits.  Chip v
 *   is a candidate of a cell iff it has a valid sample at the probe and d_v > 0 there (false for NaN and for 0).  Candidates are ordered by
 *   (d_v descending as float, chip position ascending): slot 0 is exactly the probe's FindMasksByDistMap owner (strictly largest, first wins).
 *   The cell keeps the first m = min(|C|, depth); slots m .. 7 are all-zero.  A slot holds frame = the chip's image index + 1
 *   (mi355_chip_info.img + 1); omega = 1 + (int) min(d_v * 254.0f, 254.0f), one float32 multiply, then truncation -- monotone in d, so
 *   omega_0 >= omega_a and the label stage's data term stays >= 0; gray = (sum + num / 2) / num over the num >= 1 pixels of the cell, clipped
 *   to the canvas, where that chip's validity byte is 255, of (1868 B + 9617 G + 4899 R + 8192) >> 14 of the chip's own bytes.  The records
 *   are mi355_seam_cell, gh x gw.
 * 2. Labels: mi355_seam_labels_dev, unchanged.  The cell map holds frame + 1 where the label left slot 0, and 0 elsewhere.
 * 3. Ownership under a map.  For canvas pixel (x, y), f = cells[y >> level][x >> level] - 1.  If f >= 0 and some kept chip has img == f and
 *   validity byte 255 at the pixel, that chip owns the pixel (validity is enough, d > 0 is not required); otherwise the owner is the
 *   FindMasksByDistMap owner.  A map value that names a dropped frame, a skipped frame, a frame that does not cover the pixel, or an id above n
 *   is not an error: the pixel keeps that rule.  Masks come out as mi355_chips_and_masks': 255 for the owner, 0 for every other covering chip.
 * Consequences: an all-zero map, depth = 1, and diff_weight = seam_penalty = 0 each give the bytes of mi355_chips_and_masks(find_masks = 1) and
 *   of mi355_mosaic_blended; energy_after <= energy_before or `fallback` is set.
 * Cost: the chip stage makes the pixels of whole chips (stage 1 reads every candidate's bytes around the seams), where mi355_mosaic_blended
 *   makes them inside the owned windows only; stage 1 reads chip bytes and takes no bilinear sample; stage 3 is the ownership plus one map
 *   load per thread.  Whole canvas only: there is no stripe form.  Three-channel frames.
 * Errors: every parameter field is range-checked; gw, gh must be the grid of mi355_blend_layout's canvas at params.level; a NULL frame that is
 *   kept and not skipped is MI355_ERR_ARG naming it; the ctx goes on working after every refusal.
 * mi355_blend_seam_cells_dev: stages 1 and 2 from DEVICE frames; the records go to d_cand too when it is given; complete on return.
 * mi355_chips_and_masks_seam: the public two-stage form, host frames; cells = NULL: stages 1 and 2 first.  Outputs as mi355_chips_and_masks,
 *   the masks after stage 3; they feed mi355_multiband_blend.
 * mi355_mosaic_blended_seam_dev: device frames in, device canvas out, as mi355_mosaic_blended_dev; d_cells = NULL: the map is made first.
 * mi355_mosaic_blended_seam / _into: all three stages with the sources and the download of mi355_mosaic_blended_into (declared here, described
 *   with the kept frames below); *out is library-allocated (mi355_free), rows padded to 4 bytes. */
int  mi355_blend_seam_cells_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                const uint8_t* keep, const mi355_seamcut_params* params, uint16_t* d_cells /* DEVICE, gh x gw */, int gw, int gh,
                                mi355_seam_report* report /* HOST, may be NULL */, mi355_seam_cell* d_cand /* DEVICE, may be NULL */);
int  mi355_chips_and_masks_seam(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                const uint8_t* keep, const mi355_seamcut_params* params, const uint16_t* cells /* HOST gh x gw, NULL = stages 1 and 2 first */,
                                int gw, int gh, int* n_chips, mi355_chip_info** chips, uint8_t*** chip_imgs, uint8_t*** masks, int* canvas_w, int* canvas_h);
int  mi355_mosaic_blended_seam_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                   const uint8_t* keep, int band, const mi355_seamcut_params* params, const uint16_t* d_cells /* DEVICE, NULL = make it */,
                                   int gw, int gh, uint8_t* d_canvas, int cw, int ch, int cws);
int  mi355_mosaic_blended_seam(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                               const uint8_t* keep, int band, const mi355_seamcut_params* params, uint8_t** out, int* out_w, int* out_h, int* out_ws);
int  mi355_mosaic_blended_seam_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h, const int* ws,
                                    int n, const float* h9s, const uint8_t* keep, int band, const mi355_seamcut_params* params, uint8_t* dst,
                                    int dst_pitch, int cw, int ch);

/* ---- frames kept in HBM after extraction, renders into caller memory ----------------------------------------------------
 * The reference's driver extracts features from pImgPoses[i].pImg and later renders the same images with the same indices
 * (MosaicWithoutPos.cpp:4430-4679) without changing a pixel in between.  With mi355_set_option(ctx, "keep_frames", 1) every host-frame
 * extraction -- mi355_sift_extract in both forms, mi355_surf_extract -- keeps its HBM copy of the frame under img_id with its w, h and
 * width_step, so that the render needs no second upload.  A later extraction under the same id replaces the frame (after any batch that
 * still reads the old one).  The copy is taken when the extraction is called: changing the caller's pixels afterwards does NOT change
 * what a render through img_ids sees.  No HBM for the copy: the extraction fails with MI355_ERR_NOMEM.  Features are the same bits with
 * the option on or off.  Kept frames live until mi355_drop_frames or mi355_destroy (mi355_drop_features leaves them alone). */
/* releases the kept frame of img_id (img_id < 0: all of them), after any work that still reads it */
int  mi355_drop_frames(mi355_ctx* ctx, int img_id);
/* the device pointer and geometry of a kept frame (MI355_ERR_ARG when img_id holds none), complete on return and valid until the frame
 * is replaced or dropped: device frames for mi355_mosaic_refined_dev, mi355_mosaic_blended_rows_dev, mi355_exchange_frames */
int  mi355_get_frame_dev(mi355_ctx* ctx, int img_id, const uint8_t** d_frame, int* w, int* h, int* ws);
/* mi355_mosaic_refined / mi355_mosaic_blended, written into the caller's host memory.  Image k comes from the kept frame of img_ids[k]
 * when img_ids != NULL and img_ids[k] >= 0 (imgs[k] may then be NULL; MI355_ERR_ARG naming k and the id when the id holds no kept frame
 * or its geometry differs from w, h, ws[k]), from the host image imgs[k] otherwise.  Images the render skips (h9s[9k+8] == 0; for the
 * blended form also keep[k] == 0) are neither read nor checked.  dst: ch rows of dst_pitch >= 3 * cw bytes (pageable memory is fine);
 * cw, ch must be what mi355_mosaic_layout / mi355_blend_layout return for the same arguments (else MI355_ERR_ARG).  Bytes [0, 3 * cw)
 * of every row are written, the rest of each row is left untouched; the bytes are those of mi355_mosaic_refined / mi355_mosaic_blended
 * whatever mix of sources is used.  The canvas is rendered in HBM and comes back in row chunks through pinned buffers of the ctx
 * ("download_chunk_mb"); no host buffer of the canvas's size is allocated.  Returns when dst is complete.  n <= 1 in the refined form:
 * MI355_ERR_FAILED, as mi355_mosaic_refined. */
int  mi355_mosaic_refined_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h, const int* ws,
                               int n, const float* h9s, uint8_t* dst, int dst_pitch, int cw, int ch);
/* mi355_mosaic_feathered with mi355_mosaic_refined_into's sources (kept frames / host images), destination and download */
int  mi355_mosaic_feathered_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h, const int* ws,
                                 int n, const float* h9s, const mi355_feather_params* params, uint8_t* dst, int dst_pitch, int cw, int ch);
/* mi355_mosaic_seamline's canvas with mi355_mosaic_feathered_into's sources, destination and download */
int  mi355_mosaic_seamline_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h, const int* ws,
                                int n, const float* h9s, const mi355_seamline_params* params, uint8_t* dst, int dst_pitch, int cw, int ch);
/* mi355_mosaic_median's canvas with mi355_mosaic_seamline_into's sources, destination and download */
int  mi355_mosaic_median_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h, const int* ws,
                              int n, const float* h9s, const mi355_median_params* params, uint8_t* dst, int dst_pitch, int cw, int ch);
/* mi355_mosaic_seamcut's canvas (all three stages) with mi355_mosaic_seamline_into's sources, destination and download */
int  mi355_mosaic_seamcut_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h, const int* ws,
                               int n, const float* h9s, const mi355_seamcut_params* params, uint8_t* dst, int dst_pitch, int cw, int ch);
int  mi355_mosaic_blended_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h, const int* ws,
                               int n, const float* h9s, const uint8_t* keep, int band, uint8_t* dst, int dst_pitch, int cw, int ch);

/* ---- overview levels of a canvas and the striped preview render (csrc/overview.hip) ------------------------------------------------
 * The reduced-size levels every orthomosaic product carries (GeoTIFF overviews, tile pyramids), made from a rendered canvas -- refined,
 * feathered, seamline or blended -- in ONE pass that knows which pixels hold data, so that the zero surround is not averaged into the
 * survey's edge.  Definition (exact integers; the bytes do not depend on tile shape, walk order or stripe cut):
 *   Input: the level-0 canvas, cw x ch BGR u8 at pitch cws (cws >= 3 cw, a multiple of 4; the row pointer 4-byte aligned).
 *   Valid map V(x, y) by `nodata`: MI355_NODATA_NONE every pixel is valid; MI355_NODATA_ZERO a pixel is invalid when B = G = R = 0 (what
 *   every render leaves where nothing covers); MI355_NODATA_MAP valid where a caller's uint16_t map (pitch cw elements) is non-zero -- the
 *   seamline render's count map and its owner map both qualify.
 *   Levels l = 1 .. levels, 1 <= levels <= 7: ow_l = (cw + 2^l - 1) >> l, oh_l = (ch + 2^l - 1) >> l, ows_l = (3 ow_l + 3) & ~3
 *   (mi355_overview_layout).  Pixel (X, Y) of level l owns the level-0 block [X 2^l, (X+1) 2^l) x [Y 2^l, (Y+1) 2^l) clipped to the canvas;
 *   n = the number of valid level-0 pixels of the block, S[c] = the sum of their channel c;
 *   out[c] = n ? (S[c] + n / 2) / n : 0 (integer division); row padding [3 ow_l, ows_l) is 0;
 *   cover (optional, per level): uint16_t, oh_l x ow_l at pitch ow_l, the value n (n <= 4^7 = 16384; 255 * 16384 + 8192 < 2^32).
 *   Every level is defined on level 0 directly, never as an average of averages.
 * Consequences: a block with n = 4^l under MI355_NODATA_NONE gives the rounded box mean; every byte lies between the smallest and the
 *   largest valid sample of its block; n > 0 at level l is the OR of V over the block; a constant valid region stays constant right up to
 *   the survey's edge.
 * Stripes: d_rows points at canvas row row0 and d_valid_rows at map row row0 (a stripe buffer serves as well as a whole canvas); cw, ch
 *   are the whole canvas's.  row0 must be a multiple of 2^levels, and so must rows unless row0 + rows == ch (rows < 0: the rest of the
 *   canvas).  Level l receives exactly its rows [row0 >> l, (row0 + rows + 2^l - 1) >> l); other rows of the outputs are left untouched.
 *   Stripes put side by side give the bytes of the whole call.
 * Cost: one launch makes all levels; canvas and map are read once; the higher levels come from sums carried in registers and LDS; no atomics.
 * d_levels[l - 1] / d_covers[l - 1]: the WHOLE buffer of level l (oh_l x ows_l bytes / oh_l x ow_l uint16_t).  d_covers may be NULL, and so may
 *   single entries of it.  Enqueued on the ctx stream like the other _dev forms.
 * MI355_ERR_ARG: levels outside 1..7, nodata outside 0..2, MI355_NODATA_MAP without a map, a misaligned row0 / rows, rows outside the canvas,
 *   NULL d_levels or a NULL entry in it, cw or ch < 1, cws < 3 cw or not a multiple of 4, a row pointer that is not 4-byte aligned. */
#define MI355_NODATA_NONE 0
#define MI355_NODATA_ZERO 1
#define MI355_NODATA_MAP  2
/* host geometry (no ctx): ow, oh, ows each hold `levels` entries (any of the three may be NULL) */
int  mi355_overview_layout(int cw, int ch, int levels, int* ow, int* oh, int* ows);
int  mi355_mosaic_overview_dev(mi355_ctx* ctx, const uint8_t* d_rows, int cw, int ch, int cws, const uint16_t* d_valid_rows, int nodata, int levels,
                               uint8_t* const* d_levels, uint16_t* const* d_covers, int row0, int rows);
/* host form: canvas (and valid, for MI355_NODATA_MAP) in host memory; *out_levels and, when out_covers != NULL, *out_covers are arrays of
 * `levels` buffers, all library-allocated: free each buffer and the arrays with mi355_free */
int  mi355_mosaic_overview(mi355_ctx* ctx, const uint8_t* canvas, int cw, int ch, int cws, const uint16_t* valid, int nodata, int levels,
                           uint8_t*** out_levels, uint16_t*** out_covers);
/* The preview: level `level` of the named render's canvas without that canvas.  render: 0 refined, 1 feathered, 2 seamline; ramp as in
 * mi355_feather_params; nodata as above, where 2 stands for exact coverage: the render's count > 0, which the seamline ownership walk yields
 * without a sample.  Sources, img_ids and refusals are those of mi355_mosaic_refined_into and of the render named; n <= 1 is MI355_ERR_FAILED.
 * ow, oh must be what mi355_mosaic_layout followed by mi355_overview_layout give for `level` (else MI355_ERR_ARG).  dst: oh rows of
 * dst_pitch >= 3 ow bytes, bytes [0, 3 ow) of each written; cover (NULL ok): oh x ow uint16_t at pitch ow, the level's n.
 * The survey is rendered stripe by stripe in HBM, every stripe is reduced by the overview kernel, and the one level comes back through the
 * ctx's pinned download buffers.  Stripe height: option "preview_stripe_rows" (default 1024, rounded up to a multiple of 2^level; 0: the
 * whole canvas in one stripe).  Work memory is ONE stripe of canvas (and of map, for nodata 2) plus the one output level: the full-size
 * canvas is never allocated and never crosses to the host.  The bytes are those of level `level` of mi355_mosaic_overview_dev applied to
 * the whole canvas of the render, whatever the stripe height. */
typedef struct { int32_t render; int32_t ramp; int32_t level; int32_t nodata; int32_t reserved[4]; } mi355_preview_params;
void mi355_default_preview_params(mi355_preview_params* p);          /* render 0, ramp 0, level 3, nodata MI355_NODATA_MAP */
int  mi355_mosaic_preview_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h, const int* ws,
                               int n, const float* h9s, const mi355_preview_params* params, uint8_t* dst, int dst_pitch, uint16_t* cover,
                               int ow, int oh);

/* ---- callers / formats either side of the path ("next" rows f1, f2 of SURVEY 8f) ---------------------- */
/* matchPairs.match: int32 n + n x 40-byte records (WriteMatchPairs / LoadMatchPairs, MosaicWithoutPos.cpp:4736-4797) */
int  mi355_write_match_pairs(const char* path, const mi355_match_point_pairs* v, int n);
int  mi355_load_match_pairs(const char* path, mi355_match_point_pairs** v, int* n);          /* *v -> mi355_free */
/* matchPairs.txt (WriteMatchPairs_ASC2, MosaicWithoutPos.cpp:4751-4772) */
int  mi355_write_match_pairs_txt(const char* path, const mi355_match_point_pairs* v, int n);
/* tran0.txt (OutTransform, MosaicWithoutPos.cpp:2798-2818): rows for images 1..n-1: m0..m7 fixed */
int  mi355_write_transforms(const char* path, const mi355_image_transform* t, int n);
/* ImportTransform (MosaicWithoutPos.cpp:2820-2843): "n" then n x 9 floats; fixed = 1 for the first transform.  *t -> mi355_free. */
int  mi355_load_transforms(const char* path, mi355_image_transform** t, int* n);
/* Reads back what OutTransform / mi355_write_transforms wrote (rows "m0..m7 fixed" for images 1..n-1): returns n transforms with the
 * identity of image 0 in front and m8 = 1.  *t -> mi355_free. */
int  mi355_load_tran0(const char* path, mi355_image_transform** t, int* n);
/* keypoint_%d.key (WriteSurfKeyPoints, MosaicWithoutPos.cpp:4691-4700): int32 n + n x 28-byte cv::KeyPoint */
int  mi355_write_keypoints(const char* path, const mi355_keypoint* kp, int n);
int  mi355_load_keypoints(const char* path, mi355_keypoint** kp, int* n);
/* discriptor_%d.xml, the other half of WriteSurfKeyPoints / LoadSurfKeyPoints (MosaicWithoutPos.cpp:4685-4688, 4710-4711):
 * cv::FileStorage fs(path, WRITE); fs << "descriptor" << Mat(n_rows x n_cols, CV_32F).  The text follows OpenCV 2.4's XML emitter
 * (persistence.cpp: icvFloatToString -- integers as "12.", others "%.8e" --, lines of the <data> block wrapped at column 71, indent 4,
 * the closing tags on the last data line).  PARITY UNPINNED: the reference commits no such file; a reader that takes any
 * white-space-separated numbers (as cv::FileStorage does) makes files written by OpenCV readable whatever the wrapping.
 * The live path never needs these files: features stay resident in HBM.  *desc -> mi355_free. */
int  mi355_write_descriptors_xml(const char* path, const float* desc, int n_rows, int n_cols);
int  mi355_load_descriptors_xml(const char* path, float** desc, int* n_rows, int* n_cols);
/* Flatten accepted pair results into the driver's m_vecMatchPairs order (pair order, inlier order). */
int  mi355_results_to_match_pairs(const mi355_pair_result* r, int n_pairs, const int32_t* fixed_flags /* per image or NULL */,
                                  mi355_match_point_pairs** v, int* n);
/* Global affine alignment: Select_Connected_Matched_Images is the caller's; this is BundleAdjustmentSparse's
 * linear system (MosaicWithoutPos.cpp:6971-7202) solved by dense Cholesky of the normal equations.
 * Image 0 (and every image with fixed[k]!=0) is held at identity. out: n_images transforms. */
int  mi355_global_affine_align(const mi355_match_point_pairs* v, int n, int n_images, const int32_t* fixed,
                               mi355_image_transform* out);

/* Select_Connected_Matched_Images (MosaicWithoutPos.cpp:2754-2796, ClusterMatchNode :2673-2752): label[k]=1 for
 * the images of the largest group connected through match pairs, else 0 (the driver then drops the other pairs
 * and flags those images invalid, h.m[8]=0, :4512-4523, 4646-4652).  Ties -> the group holding the lowest index. */
int  mi355_select_connected(const mi355_match_point_pairs* v, int n, int n_images, int32_t* label);
/* The two driver steps above straight from the pair records of mi355_match_pairs (no m_vecMatchPairs copy: at C5 that vector holds
 * 28 M correspondences, 1.1 GB): accepted pairs with at least one inlier are the edges / the equations; with label != NULL the
 * alignment uses only the pairs whose two images carry a non-zero label (the driver drops the others, :4512-4523).  Same sums in
 * the same order as the m_vecMatchPairs forms: the transforms are the same bits. */
int  mi355_select_connected_results(const mi355_pair_result* r, int n_pairs, int n_images, int32_t* label);
int  mi355_global_affine_align_results(const mi355_pair_result* r, int n_pairs, int n_images, const int32_t* fixed,
                                       const int32_t* label, mi355_image_transform* out);

/* ---- SURF variant of the path ("next" row f4 of SURVEY 8f): GetMatchedPairsOneToAllSurf, MosaicWithoutPos.cpp:5300-5533 ----------
 * (every call site of it in the reference is commented out, :4461-4499; named in north_star).  cv::SURF's arithmetic is not
 * available: the definition is oracle/oracle_surf.c (parity unpinned).  SURF features live in their own id space of the ctx. */
/* SurfFeatureDetector detector(minHessian).detect + SurfDescriptorExtractor.compute (:5313-5335): SURF(hessianThreshold, 4 octaves,
 * 2 layers, extended 128-float descriptors, oriented).  The reference keeps every keypoint; here the max_kp strongest by Hessian response
 * are kept (max_kp <= 2^21 = the candidate list: pass that to keep all; an image with more maxima above the threshold than that fails), ordered by (response descending, octave, layer, row, column).  desc128: n x 128 floats, unit norm;
 * kp[].class_id = sign of the Laplacian.  Synchronous. */
int  mi355_surf_extract(mi355_ctx* ctx, int img_id, const uint8_t* bgr, int w, int h, int width_step, float hessian_threshold, int max_kp,
                        mi355_keypoint* kp, float* desc128, int* n_kp);
int  mi355_surf_extract_dev(mi355_ctx* ctx, int img_id, const uint8_t* d_bgr, int w, int h, int width_step, float hessian_threshold, int max_kp, int* n_kp);
int  mi355_surf_get_features(mi355_ctx* ctx, int img_id, mi355_keypoint* kp, float* desc128, int max_kp, int* n_kp);
int  mi355_surf_drop_features(mi355_ctx* ctx, int img_id);   /* img_id < 0: all */
/* the ring schedule of that function: ext = min(15, n/2 - 1), j0 in (i, i + ext] wrapped modulo n (:5370-5377) */
int  mi355_surf_pair_schedule(int n_images, int32_t* pairs_ij, int max_pairs, int* n_pairs);
/* the j-loop body :5379-5527 for a batch of pairs: exact float 1-NN (what FlannBasedMatcher approximates, :5389-5391), sort by
 * (distance, queryIdx) (:5392), every match below matchDist with matchDist lowered by 0.05 until at most max_features remain
 * (:5400-5424; UavMatchParam: matchDist 0.5, maxFeatruesNum 200), CMosaicHarris::Ransac (:5459 -- Ransac2D's arithmetic with the
 * pool allocator, see tests/test_surf.py), accepted when more than min_inliers (18, :5306) inliers. */
int  mi355_surf_match_pairs(mi355_ctx* ctx, const int32_t* pairs_ij, int n_pairs, float ransac_dist, uint32_t seed, float match_dist, int max_features,
                            int min_inliers, mi355_pair_result* out);

/* ---- multi-GPU: one process per GPU ------------------------------------------------------- */
/* Deterministic shard of the reference's pair schedule (i strided by rank like the threads at
 * MosaicWithoutPos.cpp:5066, j in (i, min(N, i+window))): writes pairs of rank `rank` of `world`.
 * Rank r extracts the frames k mod world == r (:4861) and matches the pairs whose i it owns; j may be any frame
 * of the window, so every rank needs every frame's features before matching: mi355_allgather_features. */
int  mi355_pair_schedule(int n_images, int window, int rank, int world, int32_t* pairs_ij, int max_pairs, int* n_pairs);

/* ---- descriptor-screened pair schedule (opt-in; csrc/screen.hip) ------------------------------------------------------------------
 * An exact all-pairs score on the strongest top_k keypoints of every frame proposes the pairs worth matching; mi355_match_pairs(_dev) then
 * matches only those.  For surveys whose capture order is not their spatial order (shuffled sets, several flights, lawnmower strips) and
 * for large surveys whose window pairs are mostly rejected.  SIFT features only (resident through mi355_sift_extract*, mi355_set_features
 * or the feature exchange); SURF features (float descriptors) are out of scope.
 *
 * Score of frames A, B (positions a, b of img_ids):
 *   top-K list of a frame: its min(n, top_k) keypoints in the order (response descending, keypoint index ascending); its position in the
 *     list breaks ties below.  D(q, t) = |q - t|^2 on the u8 descriptors, exact.
 *   nn(q): the argmin of D over the other frame's list (ties: lower position); d1 its minimum; d2 the second smallest over the multiset
 *     (d2 may equal d1; +infinity when the other list has one row).
 *   score = #q in A's list with nn(nn(q)) == q and both q and nn(q) passing 10000 d1 < ratio_pct^2 d2 (int64; ratio_pct == 100: no test).
 *   Symmetric; a frame without keypoints scores 0 with every other.
 * Selection: position a ranks its in-scope candidates by (score descending, position ascending) and nominates the first `partners` of them
 * whose score is >= min_score (partners == 0: every candidate with score >= min_score).  A pair is kept when either side nominates it.
 * Scope: all pairs (window == 0) or the positions with |a - b| < window (mi355_pair_schedule's window); window >= n is all pairs.
 * Edges of the definition (tests/test_gpu_screen_edges.py): top_k is any multiple of 32, a power of two or not, with the same list order;
 * +-0 responses are equal, +infinity is the strongest, negative and denormal responses order as numbers.
 * A score is at most top_k, so min_score > top_k nominates nothing and the schedule is empty; min_score <= 0 acts as 0.  partners above
 * the number of candidates nominates all of them.  world > n is valid: rank r owns the rows a == r (mod world), so the ranks from n - 1
 * on own no pair and return an empty list.  n = 0 and n = 1 give an empty schedule (and an n x n matrix of -1).
 * Limits: n <= 16384 (the n x n score matrix is 1 GB there).  MI355_ERR_ARG, with a message naming the value, for an unknown or duplicate
 * id, top_k outside {32, 64, ..., 512}, partners < 0, ratio_pct outside [1, 100], window == 1 or < 0, and a bad rank / world.
 * Results are identical across contexts and devices for the same features: every rank of a multi-GPU run computes the whole screen after
 * the feature exchange and keeps its own rows (no collective). */
typedef struct {
    int32_t top_k;      /* keypoints per frame used by the screen: multiple of 32 in [32, 512]; default 256 */
    int32_t partners;   /* per frame: nominate its best `partners` candidates; 0 = every candidate with score >= min_score */
    int32_t min_score;  /* a nomination needs at least this score */
    int32_t ratio_pct;  /* Lowe ratio in percent, 1..100 (100 = test off); default 80 */
    int32_t window;     /* 0 = all pairs of the id list; >= 2 = only positions b - a < window (mi355_pair_schedule's window) */
} mi355_screen_params;
/* defaults measured on the C4 survey ("Screened pair schedule") */
#define MI355_SCREEN_DEFAULT_PARTNERS  12
#define MI355_SCREEN_DEFAULT_MIN_SCORE 6
void mi355_default_screen_params(mi355_screen_params* p);

/* n x n int32 scores, row-major, device memory (ctx's stream, complete on return); diagonal and out-of-window entries = -1.  p NULL: defaults. */
int  mi355_screen_scores_dev(mi355_ctx* ctx, const int32_t* img_ids, int n, const mi355_screen_params* p, int32_t* d_scores);

/* the screened schedule: pairs {img_ids[a], img_ids[b]}, a < b, sorted by (a, b), only a mod world == rank; scores (the pairs' scores) may
 * be NULL; same count / max_pairs convention as mi355_pair_schedule: *n_pairs = the count; pairs_ij == scores == NULL counts only; more
 * pairs than max_pairs writes the first max_pairs and returns MI355_ERR_ARG.  With partners > 0, n * partners is always enough. */
int  mi355_screen_pairs(mi355_ctx* ctx, const int32_t* img_ids, int n, const mi355_screen_params* p, int rank, int world,
                        int32_t* pairs_ij, int32_t* scores, int max_pairs, int* n_pairs);

/* Fixed-size feature record of one frame (what the reference keeps in keypoint_%d.key + discriptor_%d.xml,
 * MosaicWithoutPos.cpp:4682-4734): bytes [0, 57344) 2048 x cv::KeyPoint, [57344, 319488) 2048 x 128 u8 descriptors,
 * zero beyond the frame's n_kp.  The header travels separately (host-readable). */
#define MI355_FEATURE_RECORD_BYTES 319488
typedef struct { int32_t img_id /* < 0: padding record */, n_kp, w, h; } mi355_feature_header;
/* Transport-agnostic halves: pack resident features into records at d_payload (device, n x MI355_FEATURE_RECORD_BYTES; headers to
 * the HOST array hdr) / install records as resident features (as if extracted here).  Used by callers that bring their own
 * transport (MPI, the gloo CPU tests); mi355_allgather_features does both around one RCCL all-gather.  A record is the one-chunk
 * case of the chunk records below ({chunk 0, n_chunks 1, row0 0, rows n_kp}; this header is the chunk header's first four fields), and
 * the install checks the whole table like theirs: a bad header (n_kp outside [0, 2048], w or h <= 0) or an image named twice returns
 * MI355_ERR_ARG and leaves the ctx's features as they were. */
int  mi355_pack_features_dev(mi355_ctx* ctx, const int32_t* img_ids, int n, mi355_feature_header* hdr, void* d_payload);
int  mi355_install_features_dev(mi355_ctx* ctx, const mi355_feature_header* hdr, const void* d_payload, int n);

/* Chunk records: the feature exchange of frames of any keypoint count (keep-all frames, nfeatures <= 0, hold up to keepall_max).  A frame of n_kp
 * keypoints travels as max(1, ceil(n_kp / 2048)) records of the layout above; chunk c holds rows [row0, row0 + rows) of the frame (the
 * packer writes row0 = 2048 c): keypoints at [0, rows * 28), descriptors at 57344 + [0, rows * 128), zeros elsewhere.  A frame of <= 2048
 * keypoints is one chunk, byte for byte the record mi355_pack_features_dev writes. */
typedef struct { int32_t img_id /* < 0: padding record */, n_kp /* whole frame */, w, h, chunk, n_chunks, row0, rows; } mi355_feature_chunk_header;  /* 32 B */
#define MI355_FEATURE_CHUNK_ROWS 2048
/* the records the frames take (sum of max(1, ceil(n_kp / 2048))); resolves pending extractions */
int  mi355_feature_chunk_count(mi355_ctx* ctx, const int32_t* img_ids, int n, int* n_records);
/* resident features -> chunk records at d_payload (device, max_records x MI355_FEATURE_RECORD_BYTES), one header per record to the HOST
 * array hdr (max_records entries); *n_records = the records written.  More records than max_records: MI355_ERR_ARG, nothing written. */
int  mi355_pack_feature_chunks_dev(mi355_ctx* ctx, const int32_t* img_ids, int n, mi355_feature_chunk_header* hdr, void* d_payload,
                                   int max_records, int* n_records);
/* chunk records -> resident features, as if extracted here (records with img_id < 0 are skipped).  Every table is checked before any
 * state changes: each image's chunks 0 .. n_chunks - 1 appear exactly once, agree on n_kp / w / h, their rows tile [0, n_kp) in chunk order
 * with 1 .. 2048 rows each (one chunk of 0 rows for n_kp = 0), n_kp <= the ctx's keepall_max (32768 by default).  A bad table returns MI355_ERR_ARG and leaves the ctx's
 * features as they were. */
int  mi355_install_feature_chunks_dev(mi355_ctx* ctx, const mi355_feature_chunk_header* hdr, const void* d_payload, int n_records);
/* The collective over the chunk records (ncclAllGather of the headers and the payload, in place): no n_max argument, the per-rank record
 * counts travel first.  Every rank gathers {records, status} of every rank, reserves world x R records (R = the largest count), packs its
 * own, and gathers a second status word: a failure on any rank up to there (an unknown id, no memory) makes EVERY rank return the error
 * after one of the two small all-gathers, before any payload moves.  Own frames are not re-installed unless flags has
 * MI355_FEATURES_INSTALL_OWN (a communicator of one rank then exercises the whole path). */
#define MI355_FEATURES_INSTALL_OWN 1
int  mi355_allgather_feature_chunks(mi355_ctx* ctx, const int32_t* img_ids, int n_local, int flags);
/* Accepted pair records to the front of d_out (order kept): what the reference pushes to the driver (:5201-5227). */
int  mi355_compact_accepted_dev(mi355_ctx* ctx, const mi355_pair_result* d_in, int n, mi355_pair_result* d_out, int* n_out);

/* RCCL communicator of the ctx (librccl is bound at run time; a process that already holds one -- PyTorch -- shares it).
 * Rank 0 obtains the id and hands the 128 bytes to the other ranks by any means (the reference has none: file, socket,
 * torch.distributed store); then every rank calls mi355_comm_init.  Collective calls, like every RCCL collective. */
int  mi355_comm_unique_id(uint8_t id128[128]);
int  mi355_comm_init(mi355_ctx* ctx, const uint8_t id128[128], int rank, int world);
int  mi355_comm_destroy(mi355_ctx* ctx);
/* MI355_OK when librccl can be bound in this process (no communicator is touched): lets every rank agree on the transport
 * BEFORE any of them blocks inside ncclCommInitRank. */
int  mi355_comm_available(void);
/* what the communicator itself reports: ncclCommUserRank / ncclCommCount (both 0 ranks -> MI355_ERR_ARG without a communicator) */
int  mi355_comm_info(mi355_ctx* ctx, int* rank, int* n_ranks);
/* ncclAllGather over xGMI of the feature records of this rank's frames (img_ids, n_local <= n_max_per_rank, the same
 * n_max_per_rank on every rank): afterwards the features of every rank's frames are resident on every rank
 * (replaces the d:/feature_temp hand-off between SiftExtraction_Thread and the matcher threads, :4874-4880 / :5100-5103).
 * A rank whose own arguments / features are bad still takes part in the collective (it sends records flagged img_id == -2),
 * so that EVERY rank returns the error together instead of the others hanging in ncclAllGather. */
int  mi355_allgather_features(mi355_ctx* ctx, const int32_t* img_ids, int n_local, int n_max_per_rank);
/* The result exchange (PushMatchPairs, :10137-10145): d_local = this rank's n_local device records (mi355_match_pairs_dev);
 * flags: MI355_GATHER_ACCEPTED_ONLY sends the accepted pairs only (C4: 96 % of the window pairs do not overlap);
 * MI355_GATHER_NO_WAIT (root >= 0 only) returns on the root once the receives and the device-to-host copy are ENQUEUED: *all is complete
 * after the next mi355_synchronize -- the 1.1 GB of C5 then cross PCIe while the host runs the alignment on the moments.
 *   root < 0   ncclAllGather: every rank's host receives the records of all ranks (rank-major);
 *   root >= 0  only rank `root`'s host does -- the rank that runs the reference's unchanged driver on the inlier lists
 *              (Select_Connected_Matched_Images / BundleAdjustmentSparse, MosaicWithoutPos.cpp:4575-4591).  The other ranks ncclSend their
 *              records to it and get *all = NULL; a deployment gives them the moments (mi355_allgather_moments) for the replicated
 *              alignment that places their canvas stripes.  C5: 1.1 GB of records then cross PCIe on one rank instead of on eight.
 * *n_all = the number of records of all ranks, on every rank.  *all points into PINNED host memory owned by the ctx (grown when needed, never
 * shrunk): valid until the next mi355_allgather_results call on this ctx or mi355_destroy -- do NOT free it.  (Until round 5 this was a
 * fresh malloc per call: page faults and a staged copy held the device-to-host leg to 3.7 GB/s.) */
#define MI355_GATHER_ACCEPTED_ONLY 1
#define MI355_GATHER_NO_WAIT       2
int  mi355_allgather_results(mi355_ctx* ctx, const mi355_pair_result* d_local, int n_local, int flags, int root,
                             const mi355_pair_result** all, int* n_all);

/* What the global alignment needs of an accepted pair (round 5): the second moments of its inlier coordinates -- the sums the normal
 * equations of BundleAdjustmentSparse's system are made of (MosaicWithoutPos.cpp:6971-7202) -- instead of the 9664-byte record with its two
 * inlier lists.  ca = (xa, ya, 1) from the record's a[], cb = (xb, yb, 1) from b[]; aa = sum ca ca^T (lower triangle, row-major: 00 10 11 20
 * 21 22), ab = sum ca cb^T (row-major 3 x 3), bb = sum cb cb^T; doubles, summed in inlier order, every product and sum rounded separately:
 * the device forms the very sums mi355_global_affine_align_results forms on the host, so the transforms are the same bits either way. */
typedef struct { int32_t i, j, n_in, _pad; double aa[6], ab[9], bb[6]; } mi355_pair_moments;      /* 184 bytes */
/* one record per pair record, on the device (a wave per pair); pairs that are not accepted get n_in = 0 and zero sums */
int  mi355_pair_moments_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, mi355_pair_moments* d_out);
/* the same sums on the host (callers without a device, tests) */
int  mi355_pair_moments_host(const mi355_pair_result* r, int n, mi355_pair_moments* out);
/* mi355_allgather_results for callers that only align: this rank's ACCEPTED pairs -> their moments (on the device) -> ncclAllGather -> host
 * array, rank-major, the same on every rank; pinned and owned by the ctx like mi355_allgather_results' (valid until the next
 * mi355_allgather_moments call; do NOT free).  52 x fewer bytes over xGMI and PCIe than the records (C5: 117 621 accepted pairs are 1.1 GB of
 * records per rank), and the replicated host step starts from the sums instead of 28 M correspondences. */
int  mi355_allgather_moments(mi355_ctx* ctx, const mi355_pair_result* d_local, int n_local, const mi355_pair_moments** all, int* n_all);
/* Select_Connected_Matched_Images / the global alignment from the moments (entries with n_in <= 0 are skipped): the same labels and, bit
 * for bit, the same transforms as the _results forms give on the records the moments were formed from */
int  mi355_select_connected_moments(const mi355_pair_moments* m, int n, int n_images, int32_t* label);
int  mi355_global_affine_align_moments(const mi355_pair_moments* m, int n, int n_images, const int32_t* fixed, const int32_t* label,
                                       mi355_image_transform* out);

/* ---- projective refinement of the global alignment, anchored to the affine result -----------------------------------------------------------
 * The reference's nonlinearAdjustment (MosaicWithoutPos.cpp:4628-4637 -> BundleAdjustmentNonlinear, :9750-10081: one undamped Gauss-Newton
 * step on 8 parameters per image, switched off there) made usable: Jacobi-scaled, damped (Levenberg-Marquardt), and held to the affine start
 * by a prior.  All arithmetic is double; every product, sum and quotient is rounded separately, in the order written, no contraction.
 *
 * Taking part.  Image k takes part iff start[k].m[8] is finite and non-zero and (label == NULL or label[k] != 0); its parameters are
 *   h[k][j] = (double)m[j] / (double)m[8], j = 0..7.  It is fixed iff (fixed ? fixed[k] != 0 : k == 0), the affine forms' rule.  A pair record
 *   is USED iff it is accepted, 1 <= n_in <= 400, i != j, both images take part and they are not both fixed.  An image is FREE iff it takes
 *   part, is not fixed and occurs in a used pair.
 * Side of a point p = (x, y) (doubles of the record's floats) under parameters h:
 *   w = (h6*x + h7*y) + 1.0;  u = (h0*x + h1*y) + h2;  v = (h3*x + h4*y) + h5;  qx = x / w, qy = y / w, q1 = 1.0 / w;  U = u / w, V = v / w;
 *   Jx = [qx, qy, q1, 0, 0, 0, -(U*qx), -(U*qy)],  Jy = [0, 0, 0, qx, qy, q1, -(V*qx), -(V*qy)]      (:9850-9863, u*x/(w*w) as (u/w)*(x/w)).
 * Block of a pair (i, j), inliers a[k] in image i, b[k] in image j: Rx = [Jx(a) | -Jx(b)], Ry = [Jy(a) | -Jy(b)], rx = U_b - U_a,
 *   ry = V_b - V_a (:9891-9892); for k = 0 .. n_in - 1 in order: N[r][c] = N[r][c] + Rx[r]*Rx[c], then + Ry[r]*Ry[c] (c <= r);
 *   g[r] = g[r] + Rx[r]*rx, then + Ry[r]*ry; cost = cost + rx*rx, then + ry*ry.  Rows 0..7 are image i's h0..h7, rows 8..15 image j's.
 *   A record that is not used gets n_in = 0 and zeros (i, j copied).  The block entry points know the images through part[k]: 0 = takes no
 *   part, 1 = takes part, 2 = takes part and is fixed; an accepted record with n_in > 400 or an index outside [0, n_images) gets a zero
 *   block that KEEPS its n_in (the refine entry points answer MI355_ERR_ARG to it, like the affine forms).
 * The block is a fixed-size POD with i, j, n_in like mi355_pair_moments, so that a later change can all-gather it between ranks (not done
 * here: the refine entry points work on one rank's records). */
typedef struct { int32_t i, j, n_in, _pad; double cost; double g[16]; double N[136]; } mi355_pair_normal_block;   /* 1240 B; N lower triangle, row-major: r(r+1)/2 + c */
/* Prior.  Control points of a free frame k: c_pq = (p*(w_k-1)/2, q*(h_k-1)/2), p, q in {0, 1, 2}, q outer, p inner; targets t_pq = (U, V) of
 *   c_pq under the start parameters; weight omega_k = (prior * n_k) / 9.0, n_k = the sum of n_in over the used pairs that contain k.  Per frame,
 *   over the nine points in order, with the one-sided rows Jx, Jy of c_pq under the current h and rx = t.U - U, ry = t.V - V:
 *   P[r][c] = P[r][c] + Jx[r]*Jx[c], then + Jy[r]*Jy[c]; pg[r] = pg[r] + Jx[r]*rx, then + Jy[r]*ry; pc = pc + rx*rx, then + ry*ry.  Then
 *   N_kk[r][c] = N_kk[r][c] + omega_k*P[r][c], g_k[r] = g_k[r] + omega_k*pg[r], cost_prior = cost_prior + omega_k*pc.  Host arithmetic.
 * System and step.  Unknowns: the free images in index order, 8 each.  Blocks are added in record order, entry by entry (a fixed image's rows
 *   and columns are dropped, :9894-9981; cost_data = cost_data + block.cost), then the prior, frames in index order.  s_i = 1 / sqrt(N_ii)
 *   (1 where N_ii is not positive).  Solve M y = b with M_ij = (s_i*N_ij)*s_j, M_ii = (s_i*N_ii)*s_i + lambda, b_i = s_i*g_i by the envelope
 *   Cholesky of the affine alignment; delta_i = s_i*y_i; the trial is h' = h + delta.  A non-positive pivot is a rejected trial.
 * Loop.  lambda = lambda0, c = data + prior cost at the start (the prior is 0 there).  While trials < max_iters and c != 0 and
 *   lambda <= 1e16: one trial -- blocks and prior at h', c' = data' + prior'; if c' is finite and c' < c: h = h', the trial's system becomes the
 *   system, lambda = lambda / lambda_down, rel = (c - c') / c, c = c', stop if rel < min_rel_decrease; else lambda = lambda * lambda_up.
 *   A non-finite cost at the start is MI355_ERR_FAILED.
 * Output.  Free images get m[j] = (float)h[j], m[8] = 1, fixed = 0; every other image is the input copied bit for bit.  No free image or no
 *   used pair: output = input, MI355_OK, a report of zeros.
 * Errors (MI355_ERR_ARG, the message names the value): max_iters < 0, prior < 0, lambda0 < 0, lambda_up <= 1, lambda_down <= 1,
 *   min_rel_decrease < 0, any of them not finite, n_images < 1, a free image with w < 2 or h < 2, NULL where a pointer is required
 *   (w, h, start, out; fixed, label, params and report may be NULL), an accepted record with n_in > 400 or an index outside the images.
 * Same contract as the affine solver: the same bits from call to call and for every MI355_HOST_THREADS. */
typedef struct { int32_t max_iters, reserved; double prior, lambda0, lambda_up, lambda_down, min_rel_decrease; } mi355_projective_params;
    /* defaults 20, 0, 0.01, 1e-3, 10, 10, 1e-6.  The prior's default comes from a prototype on synthetic planar surveys with 0.5 px of tie noise:
     * without a prior the fit shrinks far frames (the cost lives in canvas space); at 0.01 the data rms falls to the noise level and no
     * corner moved more than 4.3 px from the affine start (CHANGELOG) */
typedef struct { int32_t trials, accepted, n_free, n_pairs_used; int64_t n_points; double cost0, cost_data, cost_prior, lambda; } mi355_projective_report;
    /* rms = sqrt(cost / n_points) */
void mi355_default_projective_params(mi355_projective_params* p);
/* one block per pair record, on the device (a wave per record); h8: n_images x 8 doubles and part: n_images bytes, both on the HOST, uploaded
 * per call; enqueued on the ctx stream like mi355_pair_moments_dev */
int  mi355_pair_normal_blocks_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, const double* h8, const uint8_t* part, int n_images,
                                  mi355_pair_normal_block* d_out);
/* the same bits on the host */
int  mi355_pair_normal_blocks_host(const mi355_pair_result* r, int n, const double* h8, const uint8_t* part, int n_images, mi355_pair_normal_block* out);
/* The refinement on device records: the accepted ones are compacted once (mi355_compact_accepted_dev's path), then every trial is one launch
 * and one copy of the blocks into pinned memory of the ctx; the sparse solve runs on the host.  Errors: mi355_last_error(ctx). */
int  mi355_global_projective_refine_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n_pairs, int n_images, const int32_t* w, const int32_t* h,
                                        const int32_t* fixed, const int32_t* label, const mi355_image_transform* start, const mi355_projective_params* params,
                                        mi355_image_transform* out, mi355_projective_report* report);
/* the same loop on host records with the host blocks: no ctx, no device; errors: mi355_last_error(NULL) */
int  mi355_global_projective_refine_results(const mi355_pair_result* r, int n_pairs, int n_images, const int32_t* w, const int32_t* h,
                                            const int32_t* fixed, const int32_t* label, const mi355_image_transform* start, const mi355_projective_params* params,
                                            mi355_image_transform* out, mi355_projective_report* report);
/* ... and on the flat correspondence list: a run of equal (ptA_i, ptB_i) is one pair, a run longer than 400 is cut into blocks of 400.  Host
 * only.  The three forms give the same bits on the same correspondences. */
int  mi355_global_projective_refine(const mi355_match_point_pairs* v, int n, int n_images, const int32_t* w, const int32_t* h,
                                    const int32_t* fixed, const int32_t* label, const mi355_image_transform* start, const mi355_projective_params* params,
                                    mi355_image_transform* out, mi355_projective_report* report);

/* ---- tie-point refinement by patch correlation in the resident frames (opt-in; csrc/tie_refine.hip) ------------------------------------------
 * The inlier lists of a pair record are SIFT keypoint positions; nothing checks them against the pixels again.  This is the area-based step
 * photogrammetric pipelines put between matching and adjustment: for every inlier (a, b) of every accepted pair the position a in image i is
 * replaced by the peak of the zero-mean normalised cross-correlation of a small gray patch around b in image j, and every tie and pair gets a
 * photometric verdict.  Nothing calls it unless asked.  It is for MEASURED ties: on exact synthetic ties it adds its own floor (DESIGN).
 * Definition.  Every float operation is a separate float32 operation in the order written, likewise every double operation; all correlation
 *   sums are exact integers.  R = radius, S = search, n = (2R+1)^2.
 * Processed records.  A record is processed iff accepted != 0, 1 <= n_in <= 400, 0 <= i, j < n_images, i != j and both frames are present
 *   (pointer not NULL).  Any other record is copied bit for bit; its status and ncc2 entries are 0 and its report carries ONE flag, the first
 *   that applies: 1 not accepted; 4 bad record (n_in or an index out of range, or i == j); 2 a frame is missing.
 * Gray of a texel: (1868 B + 9617 G + 4899 R + 8192) >> 14 (SIFT's and SURF's integer expression).  The gray sample at a float position (x, y)
 *   is hm::bilin of the four texel grays at xi = (int)x, yi = (int)y with q = x - (float)xi, p = y - (float)yi: the renders' pixel expression,
 *   truncating cast included, an integer 0..255.  A position is inside a w x h frame iff x >= 0 && x < w-1 && y >= 0 && y < h-1, tested on the
 *   floats before any cast (NaN is outside).
 * One tie (a, b).  M = the record's H with M[8] replaced by 1.0f (H[8] holds Ransac2D's residual); apply_div9(M, x, y) =
 *   ((M0 x + M1 y + M2) / (M6 x + M7 y + M8), (M3 x + M4 y + M5) / (M6 x + M7 y + M8)), sums left to right.
 *   1 Template: (b.x - R, b.y - R) and (b.x + R, b.y + R) both inside frame j, else EDGE.  T(u, v), u, v in [-R, R], is the gray sample of
 *     frame j at (b.x + (float)u, b.y + (float)v).
 *   2 Window: (X0, Y0) = apply_div9(M, b.x, b.y); for u, v in [-(R+S), R+S]: (X, Y) = apply_div9(M, b.x + (float)u, b.y + (float)v),
 *     xs = (X - X0) + a.x, ys = (Y - Y0) + a.y; every position inside frame i, else EDGE.  W(u, v) is the gray sample of frame i there.
 *   3 St = sum T, Stt = sum T^2 (int64), vt = n Stt - St St; vt == 0: FLAT.
 *   4 For each shift (dx, dy) in [-S, S]^2, over u, v in [-R, R]: Sw = sum W(u+dx, v+dy), Sww = sum W^2, Stw = sum T W;
 *     vw = n Sww - Sw Sw, num = n Stw - St Sw (int64).
 *   5 score = (num > 0 && vw > 0) ? ((double)num * (double)num) / ((double)vt * (double)vw) : 0.0        (ZNCC squared, no square root)
 *   6 Peak: the largest score; among equal scores the smallest index (dy+S)(2S+1) + (dx+S).  peak == 0 or
 *     peak < (double)min_ncc * (double)min_ncc: LOW.  Otherwise |dx| == S or |dy| == S: BORDER.
 *   7 Per axis, with sm, s0, sp the scores at -1, 0, +1 around the peak: den = (sm - s0) + (sp - s0);
 *     off = den < 0 ? (0.5 * (sm - sp)) / den : 0.0;  ex = (float)((double)dx + offx), ey likewise.
 *   8 (X1, Y1) = apply_div9(M, b.x + ex, b.y + ey); a'.x = a.x + (X1 - X0), a'.y = a.y + (Y1 - Y0); REFINED.  Ids and b never change; a tie
 *     that is not REFINED keeps its a.
 * Per tie, at the ORIGINAL index k: status[rec*400 + k]; ncc2[rec*400 + k] = (float)peak (0 for EDGE and FLAT).  Entries k >= n_in are 0.
 * Dropping.  A tie with (1 << status) in drop_mask leaves both lists; the order of the rest is kept.  The output record's n_in is the number
 *   kept (n_out) and its list entries from n_out on are zero.  If ties were dropped (n_out < n_in) and n_out <= the ctx's min_inliers the record
 *   becomes a not-accepted record by the existing convention: accepted = 0, ok = 0, H all zero, lists kept; report flag 8.
 * Report: i, j, n_in (input), n_out, flags, count[s] = ties of status s, ncc_q_sum = the sum over the REFINED ties of
 *   (int64_t)(peak * 1048576.0).  A record that is not processed reports n_out = n_in and zero counts.
 * Errors (MI355_ERR_ARG, the message names the value): radius outside [1, 10], search outside [1, 4], min_ncc not finite or outside [0, 1],
 *   drop_mask with bits other than 2..5, reserved != 0, n < 0, n_images < 1, a NULL array, a present frame with w or h < 2 or > 2^20 or
 *   ws < 3 w.  params NULL = defaults.
 * Out of scope: the multi-GPU path (a rank holds frame i of its pairs but usually not frame j: such records come back with flag 2,
 *   unchanged) and single-channel frames (3-channel BGR only). */
#define MI355_TIE_NONE    0   /* entry at or beyond n_in, or record not processed */
#define MI355_TIE_REFINED 1   /* position was replaced */
#define MI355_TIE_EDGE    2   /* a patch leaves a frame */
#define MI355_TIE_FLAT    3   /* the template has no variance */
#define MI355_TIE_LOW     4   /* the peak is below min_ncc */
#define MI355_TIE_BORDER  5   /* the peak lies on the border of the search range */
#define MI355_TIE_FLAG_NOT_ACCEPTED 1
#define MI355_TIE_FLAG_NO_FRAME     2
#define MI355_TIE_FLAG_BAD_RECORD   4
#define MI355_TIE_FLAG_DEMOTED      8
typedef struct { int32_t radius, search, drop_mask, reserved; float min_ncc; } mi355_tie_params;      /* defaults 7, 3, 0, 0, 0.7f */
typedef struct { int32_t i, j, n_in, n_out, flags, count[8], _pad; int64_t ncc_q_sum; } mi355_tie_report;      /* 64 bytes */
void mi355_default_tie_params(mi355_tie_params* p);
/* device records in, device records out (d_out == d_in is allowed); d_imgs: a HOST array of n_images device pointers, the renders' convention
 * (NULL: the frame is not held); w, h, ws: host arrays.  d_status (n x 400 bytes), d_ncc2 (n x 400 floats) and d_report (n records) may each be
 * NULL.  One launch, a workgroup per record, enqueued on the ctx stream like mi355_pair_moments_dev; n == 0 is MI355_OK with nothing launched.
 * Profile class "tie_refine". */
int  mi355_refine_ties_dev(mi355_ctx* ctx, const mi355_pair_result* d_in, int n, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws,
                           int n_images, const mi355_tie_params* params, mi355_pair_result* d_out, uint8_t* d_status, float* d_ncc2,
                           mi355_tie_report* d_report);
/* host records in and out (out == in is allowed), complete on return.  Image k comes from the kept frame of img_ids[k] or from the host image
 * imgs[k], by mi355_mosaic_refined_into's rule and staging; images that no processed record names are neither read nor uploaded; an image with
 * neither source is a missing frame (flag 2).  Unlike the _dev form an accepted record that would get flag 4 makes the call fail with
 * MI355_ERR_ARG before any launch; the message names the record. */
int  mi355_refine_ties(mi355_ctx* ctx, const mi355_pair_result* in, int n, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h,
                       const int* ws, int n_images, const mi355_tie_params* params, mi355_pair_result* out, uint8_t* status, float* ncc2,
                       mi355_tie_report* report);

/* ---- frame ownership for the compositing phase (primary form) --------------------------------------------------------------
 * A rank uploads and holds only the frames it extracts (k mod G == rank, MosaicWithoutPos.cpp:4861).  After the (replicated) alignment
 * every rank knows every rank's canvas stripe and therefore which frames each stripe reads; a frame a stripe reads and its rank does not
 * hold is sent by its owner over xGMI.  Replaces "every rank holds all N frames" (72 GB per GPU at C5; 8 x the PCIe upload). */
/* need[k] = 1 when rendering canvas rows [row0, row0 + rows) reads frame k.  mode:
 *   MI355_COVER_REFINED        mi355_mosaic_refined_dev, by host geometry alone: every frame whose clipped canvas box meets the rows (a superset
 *                              of what is read: a frame lying entirely under later frames is in it).  For mi355_mosaic_feathered_dev this box
 *                              cover is the cover: every frame in it takes part in the walk, and a NULL pointer for one of them is an error there;
 *   MI355_COVER_BLENDED        mi355_mosaic_blended_rows_dev (keep, band as there): the chips that reach the rows plus the blender pyramids' reach;
 *   MI355_COVER_REFINED_EXACT  mi355_mosaic_refined_dev, exactly: the frames that GIVE at least one pixel of the rows its sample -- the tile
 *                              kernel's own walk (descending image index, first valid sample wins, MosaicWithoutPos.cpp:2254-2348 read backwards)
 *                              with its loads and stores left out, one extra launch and a 4-bytes-per-frame copy back; at C5, where ~60 frames
 *                              cover a canvas pixel, a stripe reads 300-340 frames of the 640 whose boxes meet it.
 * Every mode runs the stripe call's own code path with the pixel work left out, so the list cannot drift from what the call dereferences. */
#define MI355_COVER_REFINED       0
#define MI355_COVER_BLENDED       1
#define MI355_COVER_REFINED_EXACT 2
int  mi355_mosaic_stripe_cover(mi355_ctx* ctx, int mode, const int* w, const int* h, int n, const float* h9s, const uint8_t* keep, int band,
                               int row0, int rows, uint8_t* need);
/* The exchange.  d_frames[k]: this rank's device pointer of frame k where it holds it (owner[k] == its rank; owner == NULL: k mod G), else
 * ignored.  need: G x n bytes, need[r * n + k] != 0 = rank r's stripe reads frame k (mi355_mosaic_stripe_cover with rank r's rows); the SAME
 * table on every rank.  For every (r, k) with need set and r != owner[k] the owner ncclSends the frame (ws[k] * h[k] bytes) and rank r ncclRecvs
 * it into storage owned by the ctx ("frame_exchange", grown when needed); the transfers are grouped by runs of 64 frames, every rank walks the
 * same table in the same order.  d_out[k]: this rank's pointer to frame k afterwards -- its own frame, the received copy, or NULL when its
 * stripe does not read it -- ready to be the d_imgs of the stripe calls.  Received copies stay valid until the next call.
 * flags: MI355_EXCHANGE_OWN_THROUGH_RCCL also routes the rank's own needed frames through ncclSend / ncclRecv to itself (a communicator
 * of one rank then exercises the whole path: tests).  bytes_recv / bytes_sent (NULL allowed): this rank's traffic.  Enqueued on the ctx stream.
 * A rank must hold (d_frames[k] != NULL) every frame it owns.  What can fail on one rank alone (an owned frame without a pointer, bad geometry,
 * no memory for the landing area) is found BEFORE any transfer is posted and its verdict travels with the cover rows (one all-gather): every
 * rank returns the error together, none is left waiting in ncclRecv. */
#define MI355_EXCHANGE_OWN_THROUGH_RCCL 1
/* MI355_EXCHANGE_NEED_IS_LOCAL: `need` holds n bytes, this rank's OWN row (what its stripe reads, e.g. from MI355_COVER_REFINED_EXACT on its
 * own device); the call all-gathers the rows of all ranks first (n bytes per rank). */
#define MI355_EXCHANGE_NEED_IS_LOCAL   2
int  mi355_exchange_frames(mi355_ctx* ctx, const uint8_t* const* d_frames, const int* h, const int* ws, int n, const int32_t* owner,
                           const uint8_t* need, int flags, const uint8_t** d_out, uint64_t* bytes_recv, uint64_t* bytes_sent);

/* ---- exposure gain compensation (opt-in; csrc/gain.hip) ------------------------------------------------------------------------
 * One gain per frame and channel, solved from the frames' overlaps and applied to the frames' texels before a render; the renders
 * themselves are unchanged (GainCompensator's place between alignment and blending, OpenCV detail::GainCompensator).
 *
 * Frames: as mi355_mosaic_refined_dev takes them -- d_imgs (device, BGR8 rows of ws bytes), w, h, ws, n, h9s.  Frame k takes part only if
 * h9s[9k+8] != 0 and its inverse exists, exactly as in the refined render; d_imgs[k] of a frame that takes no part may be NULL.  The canvas
 * is mi355_mosaic_layout's for the same arguments (cw, ch, dGxy).
 * Lattice: the canvas pixels (x, y) with x % step == 0 and y % step == 0, 1 <= step <= 64 (default 8).
 * Cover and sample: frame k covers a lattice point, and has a sample there, exactly when the refined render would give that canvas pixel
 *   frame k's sample if k were the top frame: the point lies inside k's clipped canvas box, the source coordinate (same unit_den /
 *   apply_div9 choice) lies in [0, w-1) x [0, h-1), and the sample is the render's hm::bilin byte per channel.  Samples come from each
 *   frame's own pixels whatever covers the point in the canvas.
 * Statistics (integers: exact, independent of execution order):
 *   frame_cover[k] = N_k, the lattice points frame k covers;
 *   per listed pair (a, b) of positions: n = the lattice points both cover, sum_a[c] / sum_b[c] = frame a's / frame b's samples of channel
 *   c (0 B, 1 G, 2 R) summed over those points.
 * Gains: alpha = 1 / sigma_n^2, beta = 1 / sigma_g^2.  Per channel c (channels == 3), or once on the channel mean (channels == 1:
 *   I = sum_c sum / (3 n)), with I_ab = sum_a / n, I_ba = sum_b / n, in double, for each listed pair with n > 0:
 *     A[a][a] += 2 alpha I_ab^2 n + beta n      A[b][b] += 2 alpha I_ba^2 n + beta n
 *     A[a][b] -= 2 alpha I_ab I_ba n            A[b][a] -= 2 alpha I_ab I_ba n
 *     rhs[a]  += beta n                         rhs[b]  += beta n
 *   and for every frame k: A[k][k] += beta N_k, rhs[k] += beta N_k (GainCompensator::singleFeed restricted to the listed pairs).  g solves
 *   A g = rhs within 1e-9 relative (infinity norm) of the exact solution; a frame without an equation (A[k][k] == 0: skipped, or N_k == 0
 *   and no listed pair with n > 0) gets g = 1 exactly.  gains: float[n][3] (channels == 1: the one gain in all three).  The solve is
 *   single-threaded double arithmetic in a fixed order: bit-identical from call to call, across thread counts and contexts, so every rank of
 *   a multi-GPU run solves the same records to the same bits.
 * Apply: LUT_kc[v] = clamp(floor((double)g[k][c] * v + 0.5), 0, 255); bytes [0, 3w) of every row of dst[k] become LUT(src[k]), the pitch
 *   padding of dst is left untouched.  dst[k] may equal src[k] (in place); a frame whose three gains are 1.0f gives identical bytes.  Gains
 *   act on texels before sampling: a compensated canvas is, byte for byte, the render (refined or blended) of the compensated frames.
 * Errors (MI355_ERR_ARG, the message names the index or value): a == b, a position outside [0, n), an unordered pair listed twice; step
 *   outside [1, 64]; channels not 1 or 3; sigma_n or sigma_g <= 0 (or not finite); n > 65535; a dst range that overlaps a src or dst range
 *   other than its own src range exactly; a taking-part frame with a NULL pointer or w < 2, h < 2, ws < 3 w. */
typedef struct {
    int32_t a, b;               /* positions in the frame list */
    int64_t n;                  /* lattice points both frames cover */
    int64_t sum_a[3], sum_b[3]; /* B, G, R samples of frame a / frame b summed over those points */
} mi355_gain_pair_stats;        /* 64 B */
typedef struct {
    float sigma_n, sigma_g;     /* OpenCV GainCompensator: 10, 0.1 */
    int32_t channels;           /* 3: a gain per channel; 1: one gain on the channel mean, copied to all three */
    int32_t step;               /* lattice step in canvas pixels, 1..64 */
} mi355_gain_params;
#ifdef __cplusplus
static_assert(sizeof(mi355_gain_pair_stats) == 64, "mi355_gain_pair_stats is 64 bytes");
static_assert(sizeof(mi355_gain_params) == 16, "mi355_gain_params is 16 bytes");
#else
_Static_assert(sizeof(mi355_gain_pair_stats) == 64, "mi355_gain_pair_stats is 64 bytes");
_Static_assert(sizeof(mi355_gain_params) == 16, "mi355_gain_params is 16 bytes");
#endif
/* sigma_n = 10, sigma_g = 0.1, channels = 3, step = 8 */
void mi355_default_gain_params(mi355_gain_params* p);
/* the statistics (one launch over all pairs and frames; complete on return): pair_stats (HOST, n_pairs records, a / b filled in) and
 * frame_cover (HOST, n values; may be NULL).  pairs_ab: 2 x n_pairs positions. */
int  mi355_gain_stats_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                          const int32_t* pairs_ab, int n_pairs, int step, mi355_gain_pair_stats* pair_stats, int64_t* frame_cover);
/* the gains from the statistics (host only, no ctx, no device); p NULL: defaults (p->step is not used here).  Errors: mi355_last_error(NULL). */
int  mi355_solve_gains(const mi355_gain_pair_stats* pair_stats, int n_pairs, const int64_t* frame_cover, int n, const mi355_gain_params* p,
                       float* gains /* n x 3 */);
/* dst[k] = LUT_k(src[k]) for every k (one launch; enqueued on the ctx stream).  gains: HOST, n x 3.  Kept frames (mi355_get_frame_dev) may
 * be sources; they stay immutable, so their output goes to caller buffers. */
int  mi355_apply_gains_dev(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws, int n,
                           const float* gains);
/* statistics at p->step, solve, apply in place on d_imgs; gains_out (HOST, n x 3; may be NULL) receives the gains.  p NULL: defaults. */
int  mi355_gain_compensate_dev(mi355_ctx* ctx, uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                               const int32_t* pairs_ab, int n_pairs, const mi355_gain_params* p, float* gains_out);

/* ---- block gain compensation (opt-in; csrc/gain.hip) -----------------------------------------------------------------------------
 * A gain MAP per frame and channel on a grid of grid_x x grid_y cells over the frame's own pixels, for what one gain per frame cannot
 * remove: vignetting and uneven light (OpenCV detail::BlocksGainCompensator's place).  Solved from the overlaps like the per-frame gains,
 * smoothed, and applied to the texels with bilinear interpolation between cell centres.  Everything the section above says about frames,
 * taking part, canvas, lattice, cover and sample holds unchanged.
 *
 * Grid: 1 <= grid_x, grid_y <= 16; a taking-part frame needs grid_x <= w and grid_y <= h (and w, h <= 2^20).  cells = grid_x * grid_y, the
 *   cell index is cy * grid_x + cx.
 * Cell of a sample: frame k's sample at a lattice point has the source coordinate (xs, ys) the render maps it to; xi = (int)xs,
 *   yi = (int)ys, cx = (xi * grid_x) / w, cy = (yi * grid_y) / h by integer division.
 * Statistics (integers: exact, independent of tile shape, walk order and launch geometry):
 *   cell_cover[k][cell] = the lattice points frame k covers whose sample falls in that cell;
 *   per listed pair (a, b) and per (cell_a, cell_b) with at least one common lattice point: n, sum_a[3], sum_b[3] as in
 *   mi355_gain_pair_stats, in records sorted by (pair, cell_a, cell_b); only records with n > 0 exist.  pair is the index into pairs_ab.
 *   Summing a pair's records gives mi355_gain_stats_dev's record of that pair at the same step, field for field; summing cell_cover[k]
 *   over the cells gives frame_cover[k].
 * Solve (host, no ctx): the unknowns are the nodes (k, cell), n * cells of them; the equations are those of the section above with every
 *   record a pair between node (a, cell_a) and node (b, cell_b) and N_node = cell_cover; same alpha, beta and channels.  A node without an
 *   equation gets exactly 1.  Within 1e-9 relative (infinity norm) of the exact solution, single-threaded double arithmetic in a fixed
 *   order: the same bits on every call, thread count and context.  (The factorisation of mi355_solve_gains where its envelope is small --
 *   grid 1 x 1 then gives mi355_solve_gains' values --, a diagonally preconditioned conjugate gradient with a proven error bound where it
 *   is not; a system on which that bound cannot be met in double, a weak prior on a very large graph, is MI355_ERR_FAILED.)
 * Smoothing: after the solve, per frame and channel on the grid_y x grid_x map in double: `smooth` passes (0..8) of the separable
 *   [1/4, 1/2, 1/4] filter, x then y, edges replicated.  The smoothed maps cast to float are gains[n][grid_y][grid_x][3].
 * Apply (integers only): q[cy][cx] = clamp((int)floor((double)g * 4096 + 0.5), 0, 32767) per channel (Q12: gains lie in [0, 8)).  For
 *   column x of a frame of width w: num = (2x + 1) grid_x - w clamped to [0, 2w (grid_x - 1)], i0 = num / (2w), rem = num % (2w),
 *   fx = (rem * 256) / (2w), i1 = min(i0 + 1, grid_x - 1); row y gives j0, j1, fy likewise from h and grid_y.  Then in uint32_t:
 *     R_i = (256 - fy) q[j0][i] + fy q[j1][i]  (i = i0, i1),   G = (256 - fx) R_i0 + fx R_i1  (Q28, below 2^31),
 *     Gq = (G + 128) >> 8  (Q20),   out = min(255, (Gq * v + (1 << 19)) >> 20).
 *   A map that is 1.0f everywhere gives identical bytes.  Bytes [0, 3w) of each row are written, the pitch padding is untouched; the
 *   in-place and overlap rules are those of mi355_apply_gains_dev.  With grid 1 x 1 the bytes are NOT promised to equal the per-frame
 *   LUT's: this is a Q12 gain in integers, that one a double product.
 * Errors: as in the section above, plus grid_x, grid_y outside [1, 16], a taking-part frame smaller than the grid (the message names the
 *   frame, its size and the grid), smooth outside [0, 8], w or h above 2^20, a gain that is not finite; in the solve also a record whose
 *   pair or cell index is out of range or whose n < 0, and a cell_cover < 0. */
typedef struct {
    int32_t pair;               /* index into pairs_ab */
    int32_t cell_a, cell_b;     /* cell of frame a's / frame b's sample */
    int32_t reserved;
    int64_t n;                  /* common lattice points with these two cells */
    int64_t sum_a[3], sum_b[3]; /* B, G, R samples of frame a / frame b summed over those points */
} mi355_block_gain_stats;       /* 72 B */
typedef struct {
    float sigma_n, sigma_g;     /* as mi355_gain_params */
    int32_t channels;           /* 3 or 1 */
    int32_t step;               /* lattice step, 1..64 */
    int32_t grid_x, grid_y;     /* cells per frame, 1..16 each */
    int32_t smooth;             /* passes of [1/4, 1/2, 1/4], 0..8 */
    int32_t reserved;
} mi355_block_gain_params;
#ifdef __cplusplus
static_assert(sizeof(mi355_block_gain_stats) == 72, "mi355_block_gain_stats is 72 bytes");
static_assert(sizeof(mi355_block_gain_params) == 32, "mi355_block_gain_params is 32 bytes");
#else
_Static_assert(sizeof(mi355_block_gain_stats) == 72, "mi355_block_gain_stats is 72 bytes");
_Static_assert(sizeof(mi355_block_gain_params) == 32, "mi355_block_gain_params is 32 bytes");
#endif
/* sigma_n = 10, sigma_g = 0.1, channels = 3, step = 8, grid 8 x 6, smooth = 2 */
void mi355_default_block_gain_params(mi355_block_gain_params* p);
/* the statistics (complete on return): *records (HOST, *n_records of them, released with mi355_free; NULL when there are none) and
 * cell_cover (HOST, n x cells values; may be NULL). */
int  mi355_block_gain_stats_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                const int32_t* pairs_ab, int n_pairs, int step, int grid_x, int grid_y,
                                mi355_block_gain_stats** records, int64_t* n_records, int64_t* cell_cover);
/* the smoothed gain maps from the statistics (host only, no ctx, no device); p NULL: defaults (p->step is not used here).  gains: HOST,
 * n x grid_y x grid_x x 3.  Errors: mi355_last_error(NULL). */
int  mi355_solve_block_gains(const mi355_block_gain_stats* records, int64_t n_records, const int32_t* pairs_ab, int n_pairs, const int64_t* cell_cover,
                             int n, const mi355_block_gain_params* p, float* gains);
/* dst[k] = src[k] times its interpolated map, for every k (one launch; complete on return).  gains: HOST, n x grid_y x grid_x x 3. */
int  mi355_apply_block_gains_dev(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws, int n,
                                 int grid_x, int grid_y, const float* gains);
/* statistics at p->step, solve, apply in place on d_imgs; gains_out (HOST, n x grid_y x grid_x x 3; may be NULL) receives the maps.  Frames
 * the render skips are not touched and may be NULL.  p NULL: defaults. */
int  mi355_block_gain_compensate_dev(mi355_ctx* ctx, uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                     const int32_t* pairs_ab, int n_pairs, const mi355_block_gain_params* p, float* gains_out);

/* ---- frame sharpness (opt-in; csrc/sharp.hip, csrc/sharp_solve.cpp, csrc/sharp.h) ---------------------------------------------------------
 * One relative sharpness per frame from the frames' overlaps, and a selection that flags blurred frames (motion blur, missed focus) and
 * drops those the survey can lose without falling apart.  A focus measure of one frame alone measures the ground as much as the lens; here
 * two frames are compared over the SAME ground, on the canvas lattice, through the render's own map and sample.  Its place is the gain
 * stage's, between alignment and render; no render changes.
 *
 * Frames, taking part, canvas, lattice (1 <= step <= 64, default 8), cover and sample: exactly as in "exposure gain compensation" above.
 * Gray of a sample (B, G, R bytes): g = (1868 B + 9617 G + 4899 R + 8192) >> 14.
 * Laplacian: frame k has a Laplacian at lattice point (x, y) when 1 <= x <= cw-2, 1 <= y <= ch-2 and k has a sample at all five canvas pixels
 *   (x, y), (x-1, y), (x+1, y), (x, y-1), (x, y+1); then L = 4 g(x, y) - g(x-1, y) - g(x+1, y) - g(x, y-1) - g(x, y+1), an integer in
 *   [-1020, 1020].  Each of the five source coordinates is the render's map of that integer canvas pixel (nothing is stepped incrementally),
 *   so the five samples are the bytes the refined render would give those pixels from frame k.
 * Statistics (integers: exact, independent of execution order):
 *   per listed pair (a, b): n = the lattice points where both frames have a Laplacian, e_a / e_b = the sum of L^2 of frame a / b over those
 *   points, s_a / s_b = the sum of g(x, y) (the centre sample) of frame a / b over them;
 *   per frame k (optional): n, e, s likewise over all lattice points where k has a Laplacian -- an absolute figure for frames without
 *   partners, for diagnostics only (it measures the ground as much as the lens).
 * Solve (host only, double, single-threaded, fixed order: the same bits from call to call for the same record list; relisting the pairs in
 *   another order changes the order of the sums and may change last bits, never more than the bound below):
 *   a listed pair is usable when n > 0 and e_a, e_b, s_a, s_b are all > 0.  For a usable pair
 *     d = 0.5 (ln e_a - ln e_b) - (ln s_a - ln s_b),
 *   the log ratio of Laplacian amplitude, normalised by mean brightness so that an exposure difference is not read as sharpness.  The
 *   unknowns l_k minimise  sum over usable pairs of n (l_a - l_b - d)^2  +  prior * sum_k W_k l_k^2,  W_k = the sum of n over the usable
 *   pairs that hold k.  prior (default 0.01) fixes the gauge: a lone blurred frame among sharp partners comes out at d / (1 + prior), and
 *   long-wavelength drift along a strip is damped.  l is within 1e-9 absolute of the exact minimiser (the factorisation of
 *   mi355_solve_gains).  sharp[k] = (float)exp(l_k); a frame in no usable pair gets exactly 1.0f.
 * Flag and select (host only): the partners of k are the frames it shares a usable pair with; m_k = the lower median of l over k's
 *   partners; rel_k = l_k - m_k (0 for a frame without partners); k is blurred when rel_k < ln(blur_ratio).  The blurred frames are
 *   visited by ascending rel (ties: lower index first); k is dropped only if the still-kept frames of its connected component stay
 *   connected without it, in the usable-pair graph restricted to kept frames.  status[k]: 0 kept and not blurred, 1 blurred and dropped,
 *   2 blurred but kept because removing it would split the survey, 3 no usable pair.  The caller drops a frame by setting h9s[9k+8] = 0, the
 *   skip convention of every render.
 *   Connectivity is all this rule guarantees.  Coverage is NOT checked: a dropped frame may leave a hole where no other frame covers the
 *   ground.  A caller who needs to know compares the count map of mi355_mosaic_seamline_dev (or the need flags of
 *   mi355_mosaic_seamline_cover) before and after.  "cover depth" below makes that check per candidate: mi355_cover_select_dev with the
 *   blurred frames as its order drops only those whose ground stays covered.
 * blur_ratio default 0.58: measured on synthetic strips (profiles/sharp_quality.json), the geometric mean of the lowest exp(rel) of an
 *   unblurred frame and the exp(rel) of a frame blurred by a Gaussian of sigma 1.5 px.
 * Errors (MI355_ERR_ARG, the message names the index or value): the statistics refuse what mi355_gain_stats_dev refuses (a == b, a
 *   position outside [0, n), an unordered pair listed twice, step outside [1, 64], n > 65535, a taking-part frame with a NULL pointer or
 *   w < 2, h < 2, ws < 3 w); the solve and the selection refuse prior <= 0 or not finite, blur_ratio outside (0, 1], and a record with a
 *   negative n, e_a, e_b, s_a or s_b (and the pair-list errors above, on the records' a and b). */
typedef struct {
    int32_t a, b;               /* positions in the frame list */
    int64_t n;                  /* lattice points where both frames have a Laplacian */
    int64_t e_a, e_b;           /* sum of L^2 of frame a / frame b over those points */
    int64_t s_a, s_b;           /* sum of the centre gray of frame a / frame b over those points */
} mi355_sharp_pair_stats;       /* 48 B */
typedef struct {
    int64_t n, e, s;            /* lattice points where the frame has a Laplacian, sum of L^2, sum of centre gray */
} mi355_sharp_frame_stats;      /* 24 B */
typedef struct {
    float prior;                /* regulariser, > 0 */
    float blur_ratio;           /* a frame is blurred below this sharpness relative to its partners' lower median, in (0, 1] */
    int32_t step;               /* lattice step in canvas pixels, 1..64 */
    int32_t reserved;
} mi355_sharp_params;
#ifdef __cplusplus
static_assert(sizeof(mi355_sharp_pair_stats) == 48, "mi355_sharp_pair_stats is 48 bytes");
static_assert(sizeof(mi355_sharp_frame_stats) == 24 && sizeof(mi355_sharp_params) == 16, "mi355_sharp_frame_stats is 24 bytes, mi355_sharp_params 16");
#else
_Static_assert(sizeof(mi355_sharp_pair_stats) == 48, "mi355_sharp_pair_stats is 48 bytes");
_Static_assert(sizeof(mi355_sharp_frame_stats) == 24 && sizeof(mi355_sharp_params) == 16, "mi355_sharp_frame_stats is 24 bytes, mi355_sharp_params 16");
#endif
#define MI355_SHARP_KEPT       0
#define MI355_SHARP_DROPPED    1
#define MI355_SHARP_CUT_VERTEX 2
#define MI355_SHARP_NO_PAIR    3
/* prior = 0.01, blur_ratio = 0.58, step = 8 */
void mi355_default_sharp_params(mi355_sharp_params* p);
/* the statistics (one launch over all pair tiles and, where frame_stats is given, all cover tiles; complete on return): pair_stats (HOST,
 * n_pairs records, a / b filled in) and frame_stats (HOST, n records; may be NULL, and then no cover tiles are launched). */
int  mi355_sharp_stats_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                           const int32_t* pairs_ab, int n_pairs, int step, mi355_sharp_pair_stats* pair_stats, mi355_sharp_frame_stats* frame_stats);
/* sharp (n floats) and rel (n doubles; may be NULL) from the records (host only, no ctx, no device); p NULL: defaults (p->step is
 * not used here; blur_ratio is checked though only the selection uses it).  Errors: mi355_last_error(NULL). */
int  mi355_solve_sharpness(const mi355_sharp_pair_stats* pair_stats, int n_pairs, int n, const mi355_sharp_params* p, float* sharp, double* rel);
/* status (n bytes) and sharp (n floats; may be NULL) from the records: the solve above, then flag and select (host only). */
int  mi355_select_sharp_frames(const mi355_sharp_pair_stats* pair_stats, int n_pairs, int n, const mi355_sharp_params* p, uint8_t* status, float* sharp);
/* statistics at p->step (no per-frame records), solve, flag and select; sharp (HOST, n floats; may be NULL), status (HOST, n bytes).  The
 * frames are only read.  p NULL: defaults. */
int  mi355_sharpness_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                         const int32_t* pairs_ab, int n_pairs, const mi355_sharp_params* p, float* sharp, uint8_t* status);

/* ---- cover depth (opt-in; csrc/cover.hip, csrc/cover_select.cpp, csrc/cover.h) -------------------------------------------------------------
 * How many kept frames cover each point of the canvas lattice, which frames hold the thinly covered points, and a selection that drops
 * frames only where the ground stays covered: the coverage check the sharpness selection above does not make, and the way to thin a survey
 * flown at a high overlap.  Geometry only: the stage takes w, h, n, h9s and NO image pointers, and loads no pixel.
 *
 * Frames, taking part, canvas, lattice (1 <= step <= 64, default 8) and cover: exactly as in "exposure gain compensation" above.  Frame k
 *   covers lattice point (x, y) when the pixel lies in k's clipped canvas box and the render's map of that integer pixel ((float)x - dGx,
 *   (float)y - dGy through the inverse; nothing is stepped incrementally) falls inside [0, w-1) x [0, h-1).
 * keep (n bytes; NULL: every frame is kept): the KEPT frames are those that take part and have keep[k] != 0.
 * The canvas layout is mi355_mosaic_layout's for h9s AS PASSED; it does not depend on keep.  This is why dropping is expressed by keep and
 *   not by h9s[9k+8] = 0: zeroing m8 may shift or shrink the layout, and with it the lattice, between two calls that are meant to be
 *   compared.  Only once the selection is final does the caller set h9s[9k+8] = 0 for the dropped frames.
 * Depth of a lattice point: d = the number of kept frames that cover it.
 * Statistics (integers: exact, independent of tile shape, walk order and launch geometry):
 *   hist[j], j = 0 .. MI355_COVER_BINS-1 (9 bins): the lattice points of the whole cw x ch canvas with d == j; the last bin takes d >= 8.
 *     The bins sum to the number of lattice points, ((cw-1)/step + 1) * ((ch-1)/step + 1).
 *   per frame k one mi355_cover_frame_stats: at_depth[j] = the lattice points k covers whose depth is j+1; the last entry takes d >= 8.  A
 *     frame that is not kept gets zeros.
 *   With every taking-part frame kept, sum_j at_depth[k][j] equals mi355_gain_stats_dev's frame_cover[k] at the same step; for 1 <= d <= 7,
 *     sum_k at_depth[k][d-1] == d * hist[d].
 *   crit_k(min_depth) = sum over j < min_depth of at_depth[k][j]: the lattice points that fall below min_depth when k alone is removed, plus
 *     the points k covers that already lie below it.
 * Selection (the rule is the definition).  order: n_order distinct frame positions, the candidates in priority order; NULL: every kept frame,
 *   by ascending crit_k of the first round, ties to the lower index.  pairs_ab / n_pairs (optional): the graph whose connectivity must
 *   survive, restricted to the frames kept on entry; the check is the sharpness selection's: the still-kept frames of k's component stay
 *   connected without k (a frame with no still-kept partner is alone in its component and splits nothing).  Without a pair list there is no
 *   connectivity check.
 *   A candidate that does not take part, or is not kept on entry, gets status 4 and is never examined; a frame that is not a candidate gets
 *   status 0.  kept = the kept frames; every other candidate starts WAITING.  Repeat while a candidate waits:
 *     1. take the statistics under the current kept (one ROUND);
 *     2. blocked = the empty list of boxes; walk the waiting candidates in order;
 *     3. for a candidate k take its clipped canvas box (begX..endX, begY..endY, ends included).  If the box meets a box in blocked, k keeps
 *        waiting and its box joins blocked;
 *     4. otherwise k is settled: if crit_k(min_depth) > max_loss, status 2 (kept for coverage); else if removing it would split its
 *        component, status 3 (kept as a cut vertex); else kept[k] = 0, status 1 (dropped), and its box joins blocked.
 *   A settled candidate is never examined again (a cut vertex that a later drop would free stays status 3).  Each round settles the first
 *   waiting candidate at least, so there are at most n_order rounds.  Outputs: status[n], keep_out[n] (1 for a frame still kept, 0
 *   otherwise), rounds, lost = the sum of crit_k over the dropped frames at the time of their drop, and optionally the final frame_stats /
 *   hist under keep_out (one more launch, made only when asked for).
 *   Without a pair list the result equals the sequential greedy that recomputes the statistics after every single drop: a frame's
 *   statistics depend only on frames whose boxes meet its own, and no candidate is settled before an earlier candidate whose box it meets.
 *   With a pair list, connectivity is evaluated on the kept set of the moment; the result may differ from the sequential greedy in that
 *   respect only (within a round, by the drops already made in it, which the sequential order may make later or earlier).
 * Errors (MI355_ERR_ARG, the message names the index or value): step outside [1, 64], min_depth outside [1, 8], max_loss < 0, n > 65535, an
 *   order entry outside [0, n) or listed twice, a taking-part frame with w < 2 or h < 2, and the pair-list errors of mi355_gain_stats_dev
 *   (a == b, a position outside [0, n), an unordered pair listed twice). */
#define MI355_COVER_BINS 9
typedef struct {
    int64_t at_depth[8];        /* lattice points the frame covers whose depth is j+1; [7]: depth >= 8 */
} mi355_cover_frame_stats;      /* 64 B */
typedef struct {
    int32_t step;               /* lattice step in canvas pixels, 1..64 */
    int32_t min_depth;          /* the depth the ground must keep, 1..8 */
    int64_t max_loss;           /* lattice points a single drop may take below min_depth, >= 0 */
} mi355_cover_params;           /* 16 B */
#ifdef __cplusplus
static_assert(sizeof(mi355_cover_frame_stats) == 64 && sizeof(mi355_cover_params) == 16, "mi355_cover_frame_stats is 64 bytes, mi355_cover_params 16");
#else
_Static_assert(sizeof(mi355_cover_frame_stats) == 64 && sizeof(mi355_cover_params) == 16, "mi355_cover_frame_stats is 64 bytes, mi355_cover_params 16");
#endif
#define MI355_COVER_NOT_CANDIDATE 0
#define MI355_COVER_DROPPED       1
#define MI355_COVER_KEPT_COVERAGE 2
#define MI355_COVER_CUT_VERTEX    3
#define MI355_COVER_NOT_EXAMINED  4
/* step = 8, min_depth = 1, max_loss = 0 */
void mi355_default_cover_params(mi355_cover_params* p);
/* the statistics under keep (one launch; complete on return): frame_stats (HOST, n records; may be NULL) and hist (HOST, MI355_COVER_BINS
 * values; may be NULL). */
int  mi355_cover_stats_dev(mi355_ctx* ctx, const int* w, const int* h, int n, const float* h9s, const uint8_t* keep, int step,
                           mi355_cover_frame_stats* frame_stats, int64_t* hist);
/* what the selection asks of its caller once per round: fill frame_stats (n records) with the statistics under keep (n bytes, never NULL);
 * a return other than MI355_OK ends the selection with that code */
typedef int (*mi355_cover_stats_fn)(void* user, const uint8_t* keep, mi355_cover_frame_stats* frame_stats);
/* the selection with the statistics supplied by the caller (host only, no ctx, no device; errors: mi355_last_error(NULL)).  status and
 * keep_out hold n bytes; rounds and lost may be NULL; p NULL: defaults (p->step is checked, the statistics are the caller's). */
int  mi355_cover_select(const int* w, const int* h, int n, const float* h9s, const uint8_t* keep, const int32_t* order, int n_order,
                        const int32_t* pairs_ab, int n_pairs, const mi355_cover_params* p, mi355_cover_stats_fn stats_fn, void* user,
                        uint8_t* status, uint8_t* keep_out, int32_t* rounds, int64_t* lost);
/* that loop with cover_depth_kernel at p->step as stats_fn; frame_stats (n records) / hist (MI355_COVER_BINS values) may be NULL, and where
 * either is given the statistics under keep_out are taken once more at the end. */
int  mi355_cover_select_dev(mi355_ctx* ctx, const int* w, const int* h, int n, const float* h9s, const uint8_t* keep, const int32_t* order,
                            int n_order, const int32_t* pairs_ab, int n_pairs, const mi355_cover_params* p, uint8_t* status, uint8_t* keep_out,
                            int32_t* rounds, int64_t* lost, mi355_cover_frame_stats* frame_stats, int64_t* hist);

/* ---- lens undistortion (opt-in; csrc/undistort.hip, csrc/lens.h) ---------------------------------------------------------------------
 * Every stage of this library relates two frames of flat ground by a homography, which holds for a pinhole camera only.  This pass
 * resamples BGR u8 frames of a camera with Brown-Conrady distortion (OpenCV's model, coefficient order and signs: k1, k2, p1, p2, k3) to an
 * ideal pinhole camera, in front of the extraction; undistorted frames are ordinary frames.  The reference has no such step.
 *
 * Constants, formed once on the host: the nine camera values and out_cx, out_cy cast to float (fx .. k3, ocx, ocy);
 *   ifx = (float)(1.0 / out_fx), ify = (float)(1.0 / out_fy), each quotient taken in double.  out_fx = out_fy = out_cx = out_cy = 0 stands
 *   for the camera's own fx, fy, cx, cy (the doubles).  Nothing is divided per pixel.
 * Map: for output pixel (u, v) of a w x h frame, every operation a separately rounded f32 operation in exactly this order:
 *     x = ((float)u - ocx) * ifx;   y = ((float)v - ocy) * ify;
 *     xx = x*x;  yy = y*y;  xy = x*y;  r2 = xx + yy;  a1 = xy + xy;
 *     t = r2*k3;  t = k2 + t;  t = r2*t;  t = k1 + t;  t = r2*t;  rad = 1.0f + t;
 *     tx = (p1*a1) + (p2*(r2 + (xx + xx)));      ty = (p1*(r2 + (yy + yy))) + (p2*a1);
 *     xd = (x*rad) + tx;   yd = (y*rad) + ty;
 *     xs = (fx*xd) + cx;   ys = (fy*yd) + cy;
 * Inside: the pixel has a sample iff xs >= 0 && xs <= (float)(w-1) && ys >= 0 && ys <= (float)(h-1), which also rejects NaN and
 *   infinities.  The interval is closed -- on purpose not the renders' [0, w-1) --: an undistorted camera gives back its frame, last row
 *   and column included.
 * Sample: xi = min((int)xs, w-2), yi = min((int)ys, h-2), q = xs - (float)xi, p = ys - (float)yi (either may be exactly 1); each channel
 *   is the renders' pixel expression (uchar)(s00 (1-p)(1-q) + s01 (1-p) q + s10 p (1-q) + s11 p q) of the 2 x 2 texels at (xi, yi).
 * Outside: `fill` in all three channels, and the pixel counts towards the frame's n_outside.
 * Sizes: 2 <= w, h <= 2^20.  Bytes [0, 3w) of each destination row are written; the row padding [3w, ws_dst) is not.
 * Consequences: with k1 = k2 = p1 = p2 = k3 = 0, output intrinsics equal to the camera's, fx and fy powers of two and integer cx, cy the
 *   output is the source byte for byte and n_outside = 0.  The bytes of a frame depend on nothing but its own pixels, its size and the
 *   constants: not on its position in the call, the other frames, or the pitches.  In-place output equals out-of-place output.
 * Errors (MI355_ERR_ARG before any launch, the message names the argument, the ctx stays usable): a NULL frame pointer or array; ws < 3w;
 *   w or h below 2 or above 2^20; n < 0 or n > 65535; a camera or output value that is not finite; fx, fy, out_fx or out_fy <= 0 (out_* all
 *   0 excepted); fill outside 0..255; a destination range that meets any source or destination range of the call other than in place. */
typedef struct { double fx, fy, cx, cy, k1, k2, p1, p2, k3; } mi355_camera;            /* pixels; OpenCV's coefficient order and signs */
typedef struct {
    double out_fx, out_fy, out_cx, out_cy;  /* the pinhole camera of the output; all four 0: the camera's own fx, fy, cx, cy */
    int32_t fill;                           /* byte written to all three channels where the source has no sample, 0..255 */
    int32_t reserved[3];
} mi355_undistort_params;
#ifdef __cplusplus
static_assert(sizeof(mi355_camera) == 72, "mi355_camera is 72 bytes");
static_assert(sizeof(mi355_undistort_params) == 48, "mi355_undistort_params is 48 bytes");
#else
_Static_assert(sizeof(mi355_camera) == 72, "mi355_camera is 72 bytes");
_Static_assert(sizeof(mi355_undistort_params) == 48, "mi355_undistort_params is 48 bytes");
#endif
/* out_* = 0 (the camera's own), fill = 0, reserved = 0 */
void mi355_default_undistort_params(mi355_undistort_params* p);
/* The output camera with the widest field of view for which no rim pixel falls outside the source (host only, no ctx; errors:
 * mi355_last_error(NULL)).  *out = the defaults with out_cx = cx, out_cy = cy, out_fx = s * (double)(float)fx, out_fy = s * (double)(float)fy,
 * s = j / 256 for the smallest j in 128..1024 at which all 2 (w + h) - 4 border pixels of the w x h output are inside under the definition
 * above.  The scan ascends, so the result is defined even where validity is not monotone in j.  No such j: MI355_ERR_FAILED.  Only the
 * border is tested: n_outside of the pass itself tells the truth for pathological coefficients. */
int  mi355_undistort_fit(const mi355_camera* cam, int w, int h, mi355_undistort_params* out);
/* The two source-coordinate planes of the definition, xs[v * w + u] and ys[v * w + u] (host only, no ctx; p NULL: defaults): what a caller
 * moves points with. */
int  mi355_undistort_map(const mi355_camera* cam, const mi355_undistort_params* p, int w, int h, float* xs, float* ys);
/* d_dst[k] = frame d_src[k] resampled, for every k: one camera per call, frames of any mix of sizes, one launch, complete on return.
 * n_outside: HOST, n values, may be NULL.  p NULL: defaults.  d_dst[k] == d_src[k] with ws_dst[k] == ws_src[k] is in place: such frames go
 * through a ctx-owned scratch buffer in groups of as many frames as 512 MB hold (at least one; one launch per group) and are copied back 3w
 * bytes per row.  n = 0 is success with nothing done. */
int  mi355_undistort_frames_dev(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h,
                                const int* ws_src, const int* ws_dst, int n, const mi355_camera* cam, const mi355_undistort_params* p,
                                int64_t* n_outside);
/* the host form: upload, the same kernel, download into the caller's rows (3w bytes each, dst_ws apart).  dst == src is allowed. */
int  mi355_undistort_image(mi355_ctx* ctx, const uint8_t* src, int w, int h, int ws, uint8_t* dst, int dst_ws, const mi355_camera* cam,
                           const mi355_undistort_params* p, int64_t* n_outside);

/* ---- lens self-calibration: Brown-Conrady coefficients from the ties (opt-in; csrc/calib.hip, csrc/calib_solve.cpp, csrc/calib.h) ------------
 * The undistortion above needs a mi355_camera.  This stage estimates its coefficients from the pair stage's own records of the ORIGINAL
 * (distorted) frames: a lens error is the part of the ties' disagreement that no per-pair homography explains, the same in every frame.
 * The order of use is pair stage on the original frames -> calibrate -> undistort -> extract and match again.  Nothing calls it unless asked.
 * All arithmetic is double; every product, sum and quotient is rounded separately, in the order written, no contraction.
 *
 * One camera per call.  fx, fy, cx, cy of the start camera are HELD FIXED: planar ties under free pair homographies do not determine them (a
 *   change of the intrinsics is absorbed by the homographies).  theta = (k1, k2, p1, p2, k3) starts at the start camera's values, usually 0;
 *   `mask` selects the free entries (MI355_CALIB_K1 ... _K3, bits 0..4), the default is k1 | k2.
 * Point undistortion U_theta(xo, yo) of an observed pixel:  xd = (xo - cx) / fx, yd = (yo - cy) / fy;  x = xd, y = yd;  then
 *   MI355_CALIB_STEPS (16) times, with lens::distort's terms in double
 *     xx = x*x; yy = y*y; xy = x*y; r2 = xx + yy; a1 = xy + xy;  t = r2*k3; t = k2 + t; t = r2*t; t = k1 + t; t = r2*t;  rad = 1.0 + t;
 *     tx = (p1*a1) + (p2*(r2 + (xx + xx)));   ty = (p1*(r2 + (yy + yy))) + (p2*a1);
 *   the step  inv = 1.0 / rad;  xn = (xd - tx)*inv;  yn = (yd - ty)*inv;  dx = xn - x;  dy = yn - y;  x = xn;  y = yn   (one division).
 *   At the last (x, y), with the terms formed once more:  dr = r2*k3; dr = 3.0*dr; dr = (k2 + k2) + dr; dr = r2*dr; dr = k1 + dr;  d2 = dr + dr;
 *     a11 = (rad + d2*xx) + ((p1*(y + y)) + (p2*(6.0*x)));  a12 = (d2*xy) + ((p1*(x + x)) + (p2*(y + y)));
 *     a22 = (rad + d2*yy) + ((p1*(6.0*y)) + (p2*(x + x)));  idet = 1.0 / (a11*a22 - a12*a12)          (dD/d(x, y), symmetric)
 *     r4 = r2*r2; r6 = r4*r2;  dD/dtheta: ex = [x*r2, x*r4, a1, r2 + (xx + xx), x*r6],  ey = [y*r2, y*r4, r2 + (yy + yy), a1, y*r6];
 *     gx[m] = -((a22*ex[m] - a12*ey[m])*idet),  gy[m] = -((a11*ey[m] - a12*ex[m])*idet)       (dU/dtheta by implicit differentiation).
 *   The point is GOOD iff x, y and idet are finite and |dx|, |dy| <= MI355_CALIB_TOL (1e-7, normalised units: 5e-5 px at f = 520).
 *   Both constants were chosen on tests/calib_ref.py (tests/test_calib_ref.py keeps the sweep): at 640 x 480, f = 520, every camera whose
 *   distort map moves a frame corner by a tenth of the half-diagonal (39.9 px) through k1 of either sign, p1, p2 of either sign or outward
 *   (positive) k2, k3, alone or mixed, is good at every pixel of the frame (the slowest, k3 alone, needs 15 steps, inward k1 13); inward k2
 *   and k3 fold the frame over sooner: good at every pixel only up to 0.06 and 0.04 of the half-diagonal, NOT at the tenth.
 * One tie (a in image i, b in image j) of a record with state h (8 doubles, h8 = 1; normalised coordinates, image j -> image i):
 *   (ua, va) = U(a), (ub, vb) = U(b);  w = (h6*ub + h7*vb) + 1.0;  u = (h0*ub + h1*vb) + h2;  v = (h3*ub + h4*vb) + h5;  q1 = 1.0 / w;
 *   qx = ub*q1; qy = vb*q1; px = u*q1; py = v*q1.  The residual is in pixels: r = (fx (ua - px), fy (va - py)).  The rows hold the residual's
 *   Jacobian and the NEGATED residual (so that g below is minus half the cost's gradient, the step's right-hand side, as in the projective block):
 *     X[0..7] = [-(fx*qx), -(fx*qy), -(fx*q1), 0, 0, 0, fx*(px*qx), fx*(px*qy)],   Y[0..7] = [0, 0, 0, -(fy*qx), -(fy*qy), -(fy*q1), fy*(py*qx), fy*(py*qy)];
 *     dxu = (h0 - px*h6)*q1; dxv = (h1 - px*h7)*q1; dyu = (h3 - py*h6)*q1; dyv = (h4 - py*h7)*q1;
 *     X[8 + m] = fx*(gx_a[m] - (dxu*gx_b[m] + dxv*gy_b[m])),   Y[8 + m] = fy*(gy_a[m] - (dyu*gx_b[m] + dyv*gy_b[m])),   m = k1, k2, p1, p2, k3;
 *     X[13] = fx*(px - ua),   Y[13] = fy*(py - va).
 *   A tie is good iff both its points are good and px, py are finite.
 * Block of a record: over its good ties k = 0 .. n_in - 1 in index order, S[r][c] = S[r][c] + X[r]*X[c], then + Y[r]*Y[c] (c <= r <= 13): N is
 *   rows 0..12 (lower triangle, r(r+1)/2 + c), g row 13, cost S[13][13].  Bad ties add nothing and are counted in n_bad.  The block always
 *   covers all five coefficients; the mask is the host loop's business.
 * Used records.  A record is USED iff it is accepted, min_ties <= n_in <= 400 (default 16), i != j, i, j >= 0 and its eight state values are
 *   finite.  A used record's block carries the record's n_in; any other record gets a zero block with n_in = 0 (i, j copied).  The START STATE
 *   of a record is K^-1 M K scaled to its last entry: M = the record's H as doubles with M[8] = 1 (H[8] carries Ransac2D's residual),
 *   T[r] = [M[r][0]*fx, M[r][1]*fy, (M[r][0]*cx + M[r][1]*cy) + M[r][2]],  G[0][c] = (T[0][c] - cx*T[2][c]) / fx,  G[1][c] = (T[1][c] - cy*T[2][c]) / fy,
 *   G[2][c] = T[2][c],  h[k] = G[k] / G[8].  If any of the eight is not finite the record is unused, and counted.
 * Loop (host; Levenberg-Marquardt with Marquardt's diagonal).  Unknowns: theta's free entries and eight per used record.  lambda = lambda0,
 *   c = the sum of the used blocks' costs in record order.  While trials < max_iters and c != 0 and lambda <= 1e16, one trial: per used record,
 *   A = its N's 8 x 8 part with A_rr = A_rr + lambda*A_rr, factored A = L L^T (Cholesky, row by row, each entry's products subtracted in column
 *   order); W = L^-1 B for B = N's rows of the free coefficients against h; z = L^-1 g_h; its contribution S_mn = C_mn - sum_r W_rm W_rn,
 *   s_m = g_m - sum_r W_rm z_r (r ascending), C its N's free-coefficient part.  The contributions and the diagonals C_mm are summed in record order;
 *   S_mm = S_mm + lambda*(sum C_mm); S dtheta = s by Cholesky; per record dh = L^-T (z - W dtheta).  theta' = theta + dtheta, h' = h + dh, blocks
 *   at (theta', h'), c' = their cost.  The trial FAILS (lambda = lambda*lambda_up) when a pivot is not positive, theta' is not finite, any used
 *   record has a bad tie or is no longer used, or c' is not finite or not below c; else theta, h, c = the trial's, lambda = lambda / lambda_down,
 *   and the loop stops if (c - c') / c < min_rel_decrease.  Bad ties at the start camera are MI355_ERR_FAILED, the message naming the record
 *   and the tie; so is a start cost that is not finite.  The per-record work may run on MI355_HOST_THREADS threads: the sums are taken in
 *   record order afterwards, so the bits are the same for every thread count.
 * Output: the start camera with the free coefficients replaced; the report; rms = sqrt(cost / n_points) in pixels.  n_unused_records counts
 *   the ACCEPTED records that are not used.  No used record: the start camera, a zero report, MI355_OK.
 * Errors (MI355_ERR_ARG before any launch, the message names the value, the ctx stays usable): a camera value that is not finite; fx or
 *   fy <= 0; mask 0 or with bits above 4; min_ties below 8 or above 400; max_iters < 0; lambda0 < 0; lambda_up or lambda_down <= 1;
 *   min_rel_decrease < 0; any of them not finite; NULL where a pointer is required (params and report may be NULL); n < 0.
 * Out of scope: estimating fx, fy, cx, cy; other lens models; a different camera per frame; robust weighting or re-gating of the ties between
 *   trials (the records are RANSAC inliers); priors on the coefficients -- on 16 frames with 60 ties a pair and 0.5 px of tie noise, freeing
 *   p1 and p2 left the data rms unchanged and moved the distort map by 4-10 px: the tangential component is close to what a homography
 *   absorbs, so leave it fixed unless the ties are many and clean --; moving the ties into the undistorted frames (extract again); the
 *   multi-GPU path (the rank that holds the gathered records runs the host form). */
#define MI355_CALIB_K1 1
#define MI355_CALIB_K2 2
#define MI355_CALIB_P1 4
#define MI355_CALIB_P2 8
#define MI355_CALIB_K3 16
#define MI355_CALIB_STEPS 16
#define MI355_CALIB_TOL 1e-7
typedef struct { int32_t i, j, n_in, n_bad; double cost; double g[13]; double N[91]; } mi355_pair_calib_block;   /* 856 B; N lower triangle, row-major: r(r+1)/2 + c */
typedef struct { int32_t max_iters, mask, min_ties, reserved; double lambda0, lambda_up, lambda_down, min_rel_decrease; } mi355_calib_params;
    /* defaults 20, k1 | k2, 16, 0, 1e-3, 10, 10, 1e-6 */
typedef struct { int32_t trials, accepted, n_pairs_used, n_unused_records; int64_t n_points; double cost0, cost, lambda; } mi355_calib_report;
#ifdef __cplusplus
static_assert(sizeof(mi355_pair_calib_block) == 856 && sizeof(mi355_calib_params) == 48 && sizeof(mi355_calib_report) == 48, "calibration records");
#else
_Static_assert(sizeof(mi355_pair_calib_block) == 856 && sizeof(mi355_calib_params) == 48 && sizeof(mi355_calib_report) == 48, "calibration records");
#endif
void mi355_default_calib_params(mi355_calib_params* p);
/* one block per pair record on the device (a wave per record), at the camera `cam` (all nine values: the coefficients are theta) and the
 * states h8: n x 8 doubles, one row per RECORD, on the HOST, uploaded per call; enqueued on the ctx stream like mi355_pair_normal_blocks_dev */
int  mi355_pair_calib_blocks_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, const double* h8, const mi355_camera* cam, int min_ties,
                                 mi355_pair_calib_block* d_out);
/* the same bits on the host (no ctx; errors: mi355_last_error(NULL)) */
int  mi355_pair_calib_blocks_host(const mi355_pair_result* r, int n, const double* h8, const mi355_camera* cam, int min_ties, mi355_pair_calib_block* out);
/* The calibration on device records: the accepted ones are compacted once (mi355_compact_accepted_dev's path) and their 64-byte heads copied
 * for the start states; then every trial is one launch and one copy of the blocks into pinned memory of the ctx; the solve runs on the host.
 * Profile class "calibrate".  n_pairs = 0 or no used record launches nothing more.  Errors: mi355_last_error(ctx). */
int  mi355_calibrate_lens_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n_pairs, const mi355_camera* start, const mi355_calib_params* params,
                              mi355_camera* out, mi355_calib_report* report);
/* the same loop on host records with the host blocks: no ctx, no device; errors: mi355_last_error(NULL) */
int  mi355_calibrate_lens_results(const mi355_pair_result* r, int n_pairs, const mi355_camera* start, const mi355_calib_params* params, mi355_camera* out,
                                  mi355_calib_report* report);
/* The flat correspondence list as accepted pair records: a run of equal (ptA_i, ptB_i) is one record, a run longer than 400 is cut into
 * records of 400 (the projective form's rule).  The list carries no homography, so each record's H is the least-squares homography of its own
 * ties (image j -> image i, H[8] = 1): both sides shifted to their mean and scaled by s = 1 / sqrt((sxx + syy) / n) of the shifted points, the
 * eight unknowns of  (h0 x + h1 y + h2) - x'(h6 x + h7 y) = x',  (h3 x + h4 y + h5) - y'(h6 x + h7 y) = y'  from the normal equations by
 * Cholesky, mapped back and scaled to its last entry; all sums in tie order.  A run it cannot fit gets an H of NaN (such a record is unused
 * by the calibration).  *n_out = the number of records; out may be NULL to ask for the count; cap < the count is MI355_ERR_ARG.  Host only. */
int  mi355_match_pairs_to_results(const mi355_match_point_pairs* v, int n, mi355_pair_result* out, int cap, int* n_out);
/* ... and the calibration on the flat list: mi355_calibrate_lens_results on mi355_match_pairs_to_results' records.  Host only.  The three
 * forms give the same bits on the same correspondences and homographies. */
int  mi355_calibrate_lens(const mi355_match_point_pairs* v, int n, const mi355_camera* start, const mi355_calib_params* params, mi355_camera* out,
                          mi355_calib_report* report);

/* ---- local registration (opt-in; csrc/local_warp.hip) --------------------------------------------------------------------------------
 * What is left after the alignment is what no homography explains: relief and buildings (parallax), residual lens error, rolling shutter.
 * The ties of the accepted pair records measure it: after the alignment their disagreement on the canvas is a sampled displacement field of
 * each frame against its neighbours.  This section turns those residuals into a smooth, bounded displacement grid per frame (statistics, a
 * small regularised solve per frame, as block gain) and resamples the frames by it in front of any render (as undistortion): the renders,
 * the gain passes and the preview see ordinary frames.  Nothing calls it unless asked.
 * Arithmetic.  Every integer expression is the one written; every float and every double operation is rounded separately, in the order
 *   written, no contraction.  (int)v truncates; floor is the mathematical floor.
 * Grid.  1 <= grid_x, grid_y <= 16, and a frame that takes part needs grid_x <= w-1 and grid_y <= h-1.  NX = grid_x + 1, NY = grid_y + 1,
 *   NN = NX * NY nodes per frame; node (u, v), 0 <= u <= grid_x, 0 <= v <= grid_y, has the index v * NX + u and lies at the frame position
 *   (u (w-1) / grid_x, v (h-1) / grid_y).  A grid holds per node the displacement (Dx, Dy) in source pixels: the corrected frame's pixel at a
 *   position reads the source frame at position + D.
 *
 * Stage 1: residual statistics.
 * Taking part.  Frame k takes part iff h9s[9k + 8] != 0 and its double inverse is finite.  With a..i = (double)h9[0..8]:
 *     A0 = e*i - f*h;  A1 = c*h - b*i;  A2 = b*f - c*e;  A3 = f*g - d*i;  A4 = a*i - c*g;  A5 = c*d - a*f;
 *     A6 = d*h - e*g;  A7 = b*g - a*h;  A8 = a*e - b*d;  det = (a*A0 + b*A3) + c*A6;  I[q] = A[q] / det, q = 0..8;
 *   the inverse is finite iff all nine I[q] are.  Formed on the host, once per call.
 * Processed records.  Tie refinement's rule: accepted != 0, 1 <= n_in <= 400, 0 <= i, j < n, i != j; and both frames take part.  Any other
 *   record contributes nothing and counts towards n_skipped.
 * Map.  P(M, x, y), M nine doubles: den = (M6*x + M7*y) + M8;  X = ((M0*x + M1*y) + M2) / den;  Y = ((M3*x + M4*y) + M5) / den
 *   (apply_div9's two divisions and left-to-right sums).
 * One tie (a in frame i, b in frame j; coordinates are the doubles of the record's floats), H_k = the doubles of h9s[9k ..]:
 *   1 ci = P(H_i, a), cj = P(H_j, b).  A den that is not finite or <= 0 rejects the tie: REJ_DEN.
 *   2 rx = cj.x - ci.x, ry = cj.y - ci.y.  rx*rx + ry*ry > max_residual*max_residual rejects the tie: REJ_RESIDUAL (an outlier of the
 *     alignment, not relief).
 *   3 mx = ci.x + 0.5*rx, my = ci.y + 0.5*ry.
 *   4 For each side (k, p) in ((i, a), (j, b)): q = P(I_k, m);  dx = p.x - q.x, dy = p.y - q.y.  The side is kept iff
 *     q.x >= 0 && q.x <= (double)(w_k-1) && q.y >= 0 && q.y <= (double)(h_k-1) && fabs(dx) <= max_shift && fabs(dy) <= max_shift (NaN fails);
 *     else REJ_SIDE.  A kept side says: the corrected frame k reads, at q, the source pixel p.
 *   REJ_DEN and REJ_RESIDUAL count once in frame i and once in frame j; REJ_SIDE counts in the side's frame.
 * Quantisation of a kept side in frame k:
 *     sx = (q.x * (double)grid_x) / (double)(w-1);  cx = min((int)sx, grid_x-1);  fx = (int)floor((sx - (double)cx) * 256.0 + 0.5)  (0..256);
 *     sy, cy, fy likewise from q.y, grid_y, h;  dqx = (int)floor(dx * 256.0 + 0.5), dqy likewise  (Q8).
 *   The side's four nodes and Q16 weights: (cx, cy): (256-fx)(256-fy);  (cx+1, cy): fx (256-fy);  (cx, cy+1): (256-fx) fy;  (cx+1, cy+1): fx fy.
 *   They sum to 65536.
 * Sums per frame, all int64_t, in a block of MI355_LOCAL_WARP_STATS_STRIDE(grid_x, grid_y) = 7 NN + 8 values:
 *     [0, 5 NN)        S[t][node], t = 0..4: the sum of weight(node) * weight(neighbour t of node) over the kept sides, neighbour 0 = the node itself,
 *                      1 = E (u+1, v), 2 = S (u, v+1), 3 = SE (u+1, v+1), 4 = SW (u-1, v+1): the symmetric 9-point stencil;
 *     [5 NN, 6 NN)     bx[node] = sum of weight * dqx;      [6 NN, 7 NN)   by[node] = sum of weight * dqy;
 *     7 NN + 0 .. 7    n_ties (kept sides), sum of dqx dqx + dqy dqy, REJ_DEN, REJ_RESIDUAL, REJ_SIDE, 0, 0, 0.
 *   The n blocks are followed by one tail of 8 values: n_skipped, then zeros: n * stride + 8 values in all.  The sums are exact: they do not
 *   depend on record order, launch geometry or the entry point that formed them.
 * Stage 2: solve (host only, no ctx).  Per frame with n_ties >= max(min_ties, 1), in double, unknowns = the nodes, one system, two
 *   right-hand sides:  A = S / 2^32 + smooth * L + prior * I,  L the Laplacian of the 4-neighbour node lattice (degree on the diagonal, -1
 *   per lattice edge);  rhs = bx / 2^24 and by / 2^24 (source pixels).  Banded Cholesky (envelope_chol.h, half bandwidth NX + 1) in a fixed
 *   single-threaded order per frame, threads across frames only: the same bits for every call and thread count; within 1e-9 relative
 *   (infinity norm) of the exact solution for prior >= 1e-6 of A's largest diagonal entry.  The solution, clamped to [-max_shift, max_shift]
 *   and cast to float, is grids[n][NY][NX][2] (x then y).  Every other frame gets exact zeros.
 *   Report per frame, from the sums and the unclamped solution g alone: n_ties and the reject counts; rms_before =
 *   sqrt((sum dq^2 / 65536) / n_ties); rms_after = sqrt(max(0, dd - 2 g.b + g^T S g) / n_ties) with dd, b, S scaled as above (the fit's
 *   residual at the ties, both components); max_shift = the largest |grid value| after the clamp; solved = 1 iff the frame was solved.
 * Stage 3: apply.  Node values nq = (int)floor((double)g * 256.0 + 0.5) per component (Q8, |nq| <= 16384).  Pixel (x, y) of a w x h frame:
 *     num = x * grid_x;  i0 = min(num / (w-1), grid_x-1);  fx = ((num - i0 (w-1)) * 256) / (w-1)      (integer division; 0..256)
 *     j0, fy likewise from y, grid_y, h-1;
 *     Dx = (256-fy) ((256-fx) nq[j0][i0].x + fx nq[j0][i0+1].x) + fy ((256-fx) nq[j0+1][i0].x + fx nq[j0+1][i0+1].x)   (int32, Q24, below 2^31)
 *     Dy likewise;  then in f32:  xs = (float)x + (float)Dx * 0x1p-24f;  ys = (float)y + (float)Dy * 0x1p-24f;
 *     xs = xs < 0 ? 0 : xs > (float)(w-1) ? (float)(w-1) : xs, ys likewise (edge replication); a pixel with either coordinate changed by
 *     that counts towards the frame's n_clamped;
 *     xi = min((int)xs, w-2), yi = min((int)ys, h-2), q = xs - (float)xi, p = ys - (float)yi; the sample is undistortion's (its "Sample").
 *   Consequences: an all-zero grid returns the source byte for byte, last row and column included, n_clamped = 0.  A frame's bytes depend
 *   only on its own pixels, its size and its grid: not on pitches, its position in the call or the other frames.  In-place output equals
 *   out-of-place output.  Bytes [0, 3w) of each destination row are written, the row padding is not.
 * Errors (MI355_ERR_ARG before any launch, the message names the value, the ctx stays usable): grid_x or grid_y outside 1..16, or
 *   grid_x > w-1 or grid_y > h-1 on a frame that takes part (apply: on any frame); max_residual, max_shift, smooth or prior not finite;
 *   max_residual <= 0, max_shift outside (0, 64], smooth < 0, prior <= 0, min_ties < 0; reserved != 0; a NULL array; w or h outside 2..2^20;
 *   ws < 3w; n < 0 or n > 65535; n_pairs < 0; a grid value that is not finite or outside [-64, 64]; a negative sum in the solve's input; and,
 *   in the apply, mi355_undistort_frames_dev's overlap rules.
 * Out of scope: the multi-GPU path (the sums are integers and would add across ranks; no collective is added); single-channel frames;
 *   iterating the step; moving keypoints or ties into the warped frames (the caller has the grids for that). */
#define MI355_LOCAL_WARP_STATS_STRIDE(grid_x, grid_y) (7 * ((grid_x) + 1) * ((grid_y) + 1) + 8)
typedef struct {
    int32_t grid_x, grid_y;     /* cells per frame, 1..16 each */
    int32_t min_ties;           /* a frame with fewer kept sides keeps a zero grid */
    int32_t reserved;
    double max_residual;        /* canvas pixels: ties that disagree by more are outliers of the alignment */
    double max_shift;           /* source pixels: bound of a side's displacement and of the grid values, (0, 64] */
    double smooth;              /* weight of the lattice Laplacian */
    double prior;               /* weight of the pull towards zero, > 0 */
} mi355_local_warp_params;
typedef struct {
    int64_t n_ties, rej_den, rej_residual, rej_side;
    double rms_before, rms_after, max_shift;      /* source pixels */
    int32_t solved, _pad;
} mi355_local_warp_report;
#ifdef __cplusplus
static_assert(sizeof(mi355_local_warp_params) == 48, "mi355_local_warp_params is 48 bytes");
static_assert(sizeof(mi355_local_warp_report) == 64, "mi355_local_warp_report is 64 bytes");
#else
_Static_assert(sizeof(mi355_local_warp_params) == 48, "mi355_local_warp_params is 48 bytes");
_Static_assert(sizeof(mi355_local_warp_report) == 64, "mi355_local_warp_report is 64 bytes");
#endif
/* grid 8 x 6, min_ties 8, max_residual 8, max_shift 8, smooth 2, prior 0.25 (DESIGN: the sweep behind them) */
void mi355_default_local_warp_params(mi355_local_warp_params* p);
/* the sums of device records into d_stats (DEVICE, n * stride + 8 int64_t, cleared by the call): one launch over the records, a workgroup per
 * record, enqueued on the ctx stream like mi355_pair_moments_dev.  w, h, h9s: host arrays, read before the call returns.  Of p only grid_x,
 * grid_y, max_residual and max_shift are used (NULL: defaults).  Profile class "tie_residuals". */
int  mi355_tie_residual_stats_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n_pairs, const int* w, const int* h, const float* h9s, int n,
                                  const mi355_local_warp_params* p, int64_t* d_stats);
/* the same bits from host records (no ctx, no device; errors: mi355_last_error(NULL)) */
int  mi355_tie_residual_stats_host(const mi355_pair_result* results, int n_pairs, const int* w, const int* h, const float* h9s, int n,
                                   const mi355_local_warp_params* p, int64_t* stats);
/* stage 2 (host only, no ctx): stats as above -> grids (n x NY x NX x 2 floats) and report (n records; may be NULL) */
int  mi355_solve_local_warps(const int64_t* stats, int n, const mi355_local_warp_params* p, float* grids, mi355_local_warp_report* report);
/* stage 3: d_dst[k] = frame d_src[k] resampled by grids[k], for every k: frames of any mix of sizes, one launch, complete on return.
 * grids: HOST, n x NY x NX x 2.  n_clamped: HOST, n values, may be NULL.  In place (d_dst[k] == d_src[k], equal pitches), the scratch
 * groups, the overlap checks and n = 0 are mi355_undistort_frames_dev's, rule for rule.  Profile class "local_warp". */
int  mi355_apply_local_warps_dev(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws_src,
                                 const int* ws_dst, int n, int grid_x, int grid_y, const float* grids, int64_t* n_clamped);
/* stages 1 to 3 in place on d_imgs (frames that take no part are not touched and may be NULL); grids_out (HOST, n x NY x NX x 2) and
 * report_out (HOST, n records) may be NULL.  p NULL: defaults.  Complete on return. */
int  mi355_local_register_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n_pairs, uint8_t* const* d_imgs, const int* w, const int* h,
                              const int* ws, int n, const float* h9s, const mi355_local_warp_params* p, float* grids_out,
                              mi355_local_warp_report* report_out);
/* the same from HOST records (uploaded by the call): for callers that hold the pair stage's records on the host, as the adaptor does */
int  mi355_local_register_results(mi355_ctx* ctx, const mi355_pair_result* results, int n_pairs, uint8_t* const* d_imgs, const int* w, const int* h,
                                  const int* ws, int n, const float* h9s, const mi355_local_warp_params* p, float* grids_out,
                                  mi355_local_warp_report* report_out);

/* ---- pair verification (opt-in; csrc/verify.hip, csrc/verify.h, csrc/verify_loop.cpp) -------------------------------------------------
 * A pair is accepted when RANSAC finds more than min_inliers ties that agree with one homography.  On repetitive ground that also happens
 * for frames that do not overlap, or that overlap and were matched one period off, and ONE such record bends the linear alignment by
 * hundreds of pixels (DESIGN).  This stage sits between the pair stage and the alignment: it keeps the pairs whose homographies close
 * triangles with their neighbours, aligns on them, admits the rest by their residual against that alignment, and demotes what is left.
 * Nothing calls it unless asked; no other entry point changes its bits.
 * Arithmetic.  All of it is double unless it says float; every operation is rounded separately, in the order written, no contraction.
 * Map.  P(M, x, y) is local registration's: den = (M6*x + M7*y) + M8;  X = ((M0*x + M1*y) + M2) / den;  Y = ((M3*x + M4*y) + M5) / den.
 *   A den that is not finite or <= 0 is a DEN FAILURE.
 *
 * Stage 1: edges, one per record (device: a wave per record; the host twin gives the same bytes).
 *   A record is USABLE iff accepted != 0, 1 <= n_in <= 400, 0 <= i, j < n_images and i != j (tie refinement's rule).  Any other record gives
 *   a zero edge with i, j, n_in copied and flags = 0.  For a usable record:
 *   F[q] = (double)H[q], q = 0..7, F[8] = 1.0 (the record's H[8] is Ransac2D's max residual, not a matrix entry): F maps frame j to frame i.
 *   B = the inverse of F by local registration's adjugate formula (A0..A8, det, I[q] = A[q] / det with a..i = F[0..8]).
 *   box = (min x, min y, max x, max y) over b[0 .. n_in): floats, frame j coordinates, the support of F.  Minimum and maximum are those of
 *     the total order of the float bit patterns (-0 below +0, a NaN beyond the infinity of its sign): the box does not depend on the order.
 *   flags: bit 0 USABLE; bit 1 TESTABLE: all 18 of F and B are finite.  A NaN among them is stored as the quiet NaN 0x7ff8000000000000
 *     (so is a NaN sum_r2 below): the sign and payload of an arithmetic NaN differ between processors, the stored bytes do not.
 *   Two usable records of the same unordered frame pair are MI355_ERR_ARG wherever the adjacency is built (the cycle and the verify entry
 *   points; the message names both record indexes): the check runs on the host, on the edges.
 *
 * Stage 2: cycles.  The host builds a CSR adjacency of the testable edges (per frame its neighbours ascending; with each neighbour the edge
 *   index and one bit: the frame is the edge's i) and uploads it.  Device: a wave per edge, four per workgroup; the lanes stride over the
 *   shorter of the two lists (frame i's when they are equally long), find each candidate in the other by binary search, and the counts are
 *   reduced across the wave, no atomics.  For a testable edge e = (i, j) and every frame k adjacent to both:
 *     M_kj = the map j -> k of the edge between j and k: its F if that edge's i is k, else its B;  M_ik = the map k -> i, likewise.
 *     Control points: (x0, y0, x1, y1) = (double)box, xm = (x0 + x1) * 0.5, ym = (y0 + y1) * 0.5; the nine (x, y), y outer over
 *       {y0, ym, y1}, x inner over {x0, xm, x1}.
 *     Per point c: d = P(F_e, c);  t = P(M_kj, c);  l = P(M_ik, t.x, t.y);  e2 = (l.x - d.x)*(l.x - d.x) + (l.y - d.y)*(l.y - d.y).
 *     A den failure in any of the three maps at any point makes the triangle BAD.  Otherwise E = the largest e2 of the nine (a NaN e2
 *     makes E NaN); a non-finite E is BAD; OK iff E <= cycle_tol * cycle_tol.
 *   Per edge: n_ok, n_bad, and min_e2 = the smallest E over the triangles without a den failure (+inf if there are none; a NaN E never
 *   lowers it).  The three do not depend on order, launch geometry or entry point.  Edges that are not testable get 0, 0, +inf.
 *
 * Pair residuals of the records under transforms h9s (n_images x 9 floats) and label (n_images int32, may be NULL): one launch, a wave per
 *   record.  A record is MEASURED iff it is usable, both frames have label != 0 (or label == NULL) and both h9s[9k + 8] != 0.  Per tie in
 *   order, H_k = the doubles of h9s[9k ..]: ci = P(H_i, a), cj = P(H_j, b); a den failure counts in n_den and adds nothing; otherwise
 *   rx = cj.x - ci.x, ry = cj.y - ci.y, r2 = rx*rx + ry*ry, sum_r2 = sum_r2 + r2, max_r2 = r2 > max_r2 ? r2 : max_r2, n_used + 1.
 *   The sum is sequential in tie order (the lanes form the r2 values, one lane adds them).  Records that are not measured get n_used = 0 and
 *   zeros (i, j copied).
 *
 * Stage 3: the loop (host only).  Parameters: cycle_tol, gate_abs, gate_k, max_rounds, bridges; defaults 6.0, 3.0, 4.0, 8, 1 (DESIGN: the
 *   sweep behind them, for 0.5 px of tie noise).
 *   Initial states.  Usable and n_ok >= 1 && n_ok > n_bad: KEPT, verdict VERIFIED.  Other usable records: PENDING.  The rest: NOT_USED.
 *     A pending pair with n_ok == 0 && n_bad == 0 is UNTESTED.
 *   Seed.  If no pair is KEPT, the untested pending pair with the largest n_in (ties: the lowest record index) becomes KEPT / BRIDGE, round 0.
 *     If there is none: MI355_ERR_FAILED, "no pair could be verified".
 *   A round r = 1 .. max_rounds:
 *     1 label = mi355_select_connected_moments over the KEPT pairs' moments (every other entry with n_in = 0).
 *     2 transforms = mi355_global_affine_align_moments on the same moments with that label and the caller's fixed.  The solver needs a
 *       fixed frame among the labelled ones: a round without one (a seed pair far from the fixed frame) also fixes the lowest labelled
 *       frame, for that round only.  The output pass does not: without a fixed frame among its labelled ones it is MI355_ERR_FAILED.
 *     3 The residuals of all records under those transforms and that label.  rms_p = sqrt(sum_r2 / n_used), +inf when n_used == 0.
 *       s = the lower median of rms_p over the KEPT measured pairs (sorted ascending, element (m - 1) / 2; 0 when there are none).
 *       g = gate_k * s;  gate = g > gate_abs ? g : gate_abs.
 *     4 Every PENDING measured pair becomes KEPT / ADMITTED if rms_p <= gate, else REJECTED; its round is r.
 *     5 If step 4 changed nothing and bridges != 0: layers, without re-aligning, until a layer admits none.  A layer looks, with the labels
 *       as they stand at its start, at every frame with label 0 that an untested pending pair joins to a labelled frame, and admits for
 *       each such frame the one such pair with the largest n_in (ties: the lowest record index) as KEPT / BRIDGE, round r; then those
 *       frames get label 1.  A pair that failed every triangle it is in (n_ok == 0, n_bad > 0) never bridges.
 *     6 If steps 4 and 5 changed nothing, stop.
 *   After the loop PENDING pairs become UNDECIDED; label and transforms are formed once more as in 1 and 2 (they are the output), and the
 *   residuals, s and gate under them are the report's.  The output therefore equals, bit for bit, what mi355_select_connected_results and
 *   mi355_global_affine_align_results return for the kept records alone.
 *   Report per record: i, j, n_in, verdict, n_ok, n_bad, round (0 where no round decided it), flags, min_e2, rms (+inf unless measured
 *   with n_used > 0), max_r2.  flags bit 0 = SUSPECT: a kept pair whose final rms exceeds the final gate; reported only.
 *   Summary: count[v] = records of verdict v, rounds used, frames labelled, s and gate of the final pass.
 *
 * Stage 4: apply.  The records are copied to the output (in place is allowed); every usable pair that is not KEPT is demoted as tie
 *   refinement demotes: ok = 0, accepted = 0, H all zero, n_in and both lists kept.  KEPT and NOT_USED records are byte-identical copies.
 *
 * Errors: MI355_ERR_ARG before any kernel of this section runs, the message names the value, the ctx stays usable: cycle_tol, gate_abs or
 *   gate_k not finite or <= 0; max_rounds < 1; n_images < 1 or > 65535; n_pairs < 0; a NULL required pointer (params NULL = defaults;
 *   fixed, report and summary may be NULL); an accepted record with n_in > 400 or an index outside the images (as the affine forms answer
 *   it; the _dev form sees it in the moments); the duplicate pair.
 * Limits (DESIGN): a survey with little redundancy splits instead of bending -- a wrong pair leaves its neighbours without a good
 *   triangle; a survey without any triangle (adjacent pairs only) keeps everything as BRIDGE, and the summary says so: count[VERIFIED] = 0.
 * Out of scope: the multi-GPU path, cycles longer than three, re-fitting homographies, tie-level gating (local registration's
 *   max_residual does that), verification under non-affine transforms (the residual entry point takes any h9s; the loop aligns affinely),
 *   the SURF path. */
#define MI355_EDGE_USABLE   1
#define MI355_EDGE_TESTABLE 2
#define MI355_VERDICT_NOT_USED  0
#define MI355_VERDICT_VERIFIED  1   /* kept: more of its triangles agree than disagree */
#define MI355_VERDICT_ADMITTED  2   /* kept: its residual against the alignment of the kept pairs is inside the gate */
#define MI355_VERDICT_BRIDGE    3   /* kept: in no triangle, and the only way to a frame (or the seed) */
#define MI355_VERDICT_REJECTED  4   /* demoted: its residual is outside the gate */
#define MI355_VERDICT_UNDECIDED 5   /* demoted: never measured (a frame of it stayed outside the kept pairs' component) */
#define MI355_VERIFY_SUSPECT 1
typedef struct { int32_t i, j, n_in, flags; float box[4]; double F[9], B[9]; } mi355_pair_edge;             /* 176 bytes */
typedef struct { int32_t n_ok, n_bad; double min_e2; } mi355_pair_cycle;                                    /* 16 bytes */
typedef struct { int32_t i, j, n_used, n_den; double sum_r2, max_r2; } mi355_pair_residual;                  /* 32 bytes */
typedef struct { double cycle_tol, gate_abs, gate_k; int32_t max_rounds, bridges; } mi355_verify_params;    /* 32 bytes */
typedef struct { int32_t i, j, n_in, verdict, n_ok, n_bad, round, flags; double min_e2, rms, max_r2, reserved; } mi355_verify_report;   /* 64 bytes */
typedef struct { int32_t count[8]; int32_t rounds, n_labelled, reserved[2]; double s, gate; } mi355_verify_summary;                    /* 64 bytes */
#ifdef __cplusplus
static_assert(sizeof(mi355_pair_edge) == 176 && sizeof(mi355_pair_cycle) == 16 && sizeof(mi355_pair_residual) == 32, "pair verification records");
static_assert(sizeof(mi355_verify_params) == 32 && sizeof(mi355_verify_report) == 64 && sizeof(mi355_verify_summary) == 64, "pair verification records");
#else
_Static_assert(sizeof(mi355_pair_edge) == 176 && sizeof(mi355_pair_cycle) == 16 && sizeof(mi355_pair_residual) == 32, "pair verification records");
_Static_assert(sizeof(mi355_verify_params) == 32 && sizeof(mi355_verify_report) == 64 && sizeof(mi355_verify_summary) == 64, "pair verification records");
#endif
void mi355_default_verify_params(mi355_verify_params* p);
/* stage 1: device records -> device edges, one launch, enqueued on the ctx stream like mi355_pair_moments_dev.  Profile class "pair_edges". */
int  mi355_pair_edges_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, int n_images, mi355_pair_edge* d_out);
/* the same bytes on the host (no ctx; errors: mi355_last_error(NULL)) */
int  mi355_pair_edges_host(const mi355_pair_result* r, int n, int n_images, mi355_pair_edge* out);
/* stage 2: edges and out are HOST arrays of n entries; the adjacency is built here, the edges and the adjacency are uploaded, one launch,
 * complete on return.  Profile class "pair_cycles". */
int  mi355_pair_cycles_dev(mi355_ctx* ctx, const mi355_pair_edge* edges, int n, int n_images, double cycle_tol, mi355_pair_cycle* out);
int  mi355_pair_cycles_host(const mi355_pair_edge* edges, int n, int n_images, double cycle_tol, mi355_pair_cycle* out);
/* the residuals: device records -> device residual records; h9s and label are HOST arrays, read before the call returns; one launch on the
 * ctx stream.  Profile class "pair_residuals". */
int  mi355_pair_residuals_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, const float* h9s, const int32_t* label, int n_images,
                              mi355_pair_residual* d_out);
int  mi355_pair_residuals_host(const mi355_pair_result* r, int n, const float* h9s, const int32_t* label, int n_images, mi355_pair_residual* out);
/* Stages 1 to 4 on device records: the moments by mi355_pair_moments_dev's kernel, edges and cycles once, one residual launch per round
 * and one for the report, the apply pass into d_out (n_pairs records; d_out == d_results is allowed).  label_out (n_images), transforms_out
 * (n_images) are HOST arrays; report (n_pairs records) and summary may be NULL.  Complete on return. */
int  mi355_verify_pairs_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n_pairs, int n_images, const int32_t* fixed,
                            const mi355_verify_params* params, mi355_pair_result* d_out, int32_t* label_out, mi355_image_transform* transforms_out,
                            mi355_verify_report* report, mi355_verify_summary* summary);
/* the same on host records with the host twins: no ctx, no device, the same bits (out == r is allowed); errors: mi355_last_error(NULL) */
int  mi355_verify_pairs_results(const mi355_pair_result* r, int n_pairs, int n_images, const int32_t* fixed, const mi355_verify_params* params,
                                mi355_pair_result* out, int32_t* label_out, mi355_image_transform* transforms_out, mi355_verify_report* report,
                                mi355_verify_summary* summary);

/* ---- guided matching (opt-in; csrc/guided.hip, csrc/guided_host.cpp) ------------------------------------------------------------------------
 * The pair stage has one way to find ties: the global 1-NN of every descriptor, the best 30 % by distance, the grid cap.  On frames that
 * overlap by a third or less the true matches are a minority of that list.  Where the caller already knows where frame j lies in frame i -- from
 * the pair's own H, from a chain of neighbouring H's, from the global alignment -- guided matching looks for each keypoint's partner only near
 * its predicted position: what stitchers and SfM pipelines run after a first geometric fit.  Nothing calls it unless asked.
 * Definition.  Every float operation is a separate float32 operation in the order written.
 * Input per pair p: image ids (i, j) with features resident, i != j, each frame with 0 .. 2048 keypoints (keep-all frames, nfeatures <= 0 with
 *   more than 2048 keypoints, are out of scope for this stage: such a frame is refused), and a guide G[9], row-major, mapping image-j
 *   coordinates to image-i coordinates; G[8] is used as given (a caller who passes a record's H sets [8] = 1: H[8] holds Ransac2D's residual).
 * For each keypoint q of frame j, with b = xy_j[q]:
 *   1 (X, Y) = apply_div9(G, b.x, b.y) (the tie-refinement section's expression: sums left to right, two true divisions).
 *   2 Candidates: the keypoints k of frame i with dx = a_k.x - X, dy = a_k.y - Y and dx*dx + dy*dy <= radius*radius.  A NaN on either side
 *     fails (so does an infinite X or Y).
 *   3 For each candidate d = the sum over the 128 dimensions of (d8_i[k][c] - d8_j[q][c])^2 as int32 (at most 8 323 200).
 *   4 (d1, k1) = the smallest (d, k) in lexicographic order; d2 = the smallest d among the other candidates, if there are any.
 *   5 q proposes k1 iff d1 <= max_dist2 and one of: there is no second candidate; ratio <= 0; (float)d1 < (ratio*ratio) * (float)d2
 *     (equality fails).
 * One-to-one: a keypoint k of frame i keeps, among the queries that proposed it, the one with the smallest (d1, q).  The result does not
 *   depend on evaluation order.
 * Cut and order: the surviving ties in ascending (d1, q) order; the first max_selected of them (the ctx parameter, at most 400) form the
 *   selection lists a[t] = {xy_i[k], id k}, b[t] = {xy_j[q], id q} with count n_sel and distances d1[t].
 * Tail: exactly the pair stage's -- Ransac2D on the lists with ransac_dist, the ctx's sample_times and the seed, the closing refinement skipped
 *   for a pair that will not be accepted, then i, j, n_selected = n_sel, accepted = n_in > min_inliers.  A rejected record therefore follows
 *   mi355_pair_result's convention: real n_in, the winning hypothesis's inliers, H zero, ok 0.
 * Radius against guide precision: the radius must cover the guide's error.  A pair's own H is good to about ransac_dist; a guide chained over
 *   many pairs drifts by several pixels per hop and finds FEWER ties at radius 4 than the pair stage did, so a guided record must never
 *   replace a better existing one: mi355_merge_pair_results keeps the record with the larger n_in, which makes a bad guide harmless.
 * Errors (MI355_ERR_ARG, decided on the host before any launch, the message names the value): radius not finite or outside (0, 64]; max_dist2
 *   outside [0, 8323200]; ratio not finite or outside [0, 1]; reserved != 0; n < 0; a NULL array with n > 0; i == j; a frame without resident
 *   features; a frame with more than 2048 keypoints; a ctx whose max_selected is outside [0, 400].  params NULL = defaults.  n == 0 returns
 *   MI355_OK and launches nothing.
 * Out of scope: the C++ adaptor, the multi-GPU path, the SURF path, keep-all frames. */
typedef struct { float radius; int32_t max_dist2; float ratio; int32_t reserved; } mi355_guided_params;      /* defaults 4.0f, 90000, 0.8f, 0 */
void mi355_default_guided_params(mi355_guided_params* p);
/* The selection alone.  pairs_ij (n x {i, j}) and guides (n x 9) are HOST arrays, read before the call returns; d_a, d_b (n x 400 sfpoints),
 * d_nsel (n ints) and d_dist (n x 400 int32, may be NULL) are device pointers; list entries from n_sel on are zero.  One launch, a workgroup per
 * pair, on the ctx stream.  Frames still in flight are waited for like mi355_match_pairs does.  Profile class "guided_select". */
int  mi355_guided_select_dev(mi355_ctx* ctx, const int32_t* pairs_ij, int n, const float* guides, const mi355_guided_params* params,
                             mi355_sfpoint* d_a, mi355_sfpoint* d_b, int32_t* d_nsel, int32_t* d_dist);
/* Selection plus tail: n records at d_out (device pointer), complete on return. */
int  mi355_guided_match_dev(mi355_ctx* ctx, const int32_t* pairs_ij, int n, const float* guides, const mi355_guided_params* params,
                            float ransac_dist, uint32_t seed, mi355_pair_result* d_out);
/* The same into a host array of n records. */
int  mi355_guided_match(mi355_ctx* ctx, const int32_t* pairs_ij, int n, const float* guides, const mi355_guided_params* params,
                        float ransac_dist, uint32_t seed, mi355_pair_result* out);
/* The pairs an alignment says overlap and no record covers (host only, no ctx; errors: mi355_last_error(NULL)).  transforms: n_images x 9,
 * frame -> canvas, m[8] == 0: the frame is not placed.  have_ij: n_have x {i, j} pairs that need no guide, in either orientation.  Every i < j
 * with both frames placed and (i, j) not in have is considered.  Every double operation is a separate operation in the order written:
 *   A = adj(T_i) (A0 = t4 t8 - t5 t7, A1 = t2 t7 - t1 t8, A2 = t1 t5 - t2 t4, A3 = t5 t6 - t3 t8, A4 = t0 t8 - t2 t6, A5 = t2 t3 - t0 t5,
 *   A6 = t3 t7 - t4 t6, A7 = t1 t6 - t0 t7, A8 = t0 t4 - t1 t3), det = t0 A0 + t1 A3 + t2 A6; P[r][c] = (A[r][0] U[0][c] + A[r][1] U[1][c] +
 *   A[r][2] U[2][c]) / det with U = T_j, sums left to right; G[k] = (float)(P[k] / P[8]).  A pair whose det or P[8] is zero or not finite is
 *   skipped.  Control points: the 3 x 3 grid {0, (w-1)/2, w-1} x {0, (h-1)/2, h-1} of frame j through G (the rounded floats, as doubles:
 *   X = (g0 x + g1 y + g2) / (g6 x + g7 y + g8), Y likewise) and the same grid of frame i through adj(G) / det(G) entry by entry; the count
 *   is the number of the 18 points that land in [0, w-1] x [0, h-1] of the other frame (NaN lands nowhere).  The pair is a candidate iff
 *   count >= min_points (default 2; min_points <= 0 selects the default).  Output ascending (i, j): pairs_ij (max_pairs x 2) and guides
 *   (max_pairs x 9, may be NULL).  pairs_ij == NULL: only the count is returned in *n_pairs.  max_pairs below the count: MI355_ERR_ARG,
 *   nothing written but the count in *n_pairs. */
int  mi355_guided_candidates(int w, int h, int n_images, const float* transforms, const int32_t* have_ij, int n_have, int min_points,
                             int32_t* pairs_ij, float* guides, int max_pairs, int* n_pairs);
/* base and extra record sets into out (host only; room for n_base + n_extra records; out may be base).  The base records keep their places.  An
 * extra record whose (i, j), as written, is already in out replaces that record iff its n_in is larger (base wins ties; so does the earlier of
 * two extra records); any other extra record is appended, in order.  *n_out: the records in out. */
int  mi355_merge_pair_results(const mi355_pair_result* base, int n_base, const mi355_pair_result* extra, int n_extra, mi355_pair_result* out,
                              int* n_out);

/* ---- measurement hooks (bench.py) ----------------------------------------------------------------------- */
/* When enabled, every launch of the named kernel class is bracketed by hipEvents on the ctx stream. */
int  mi355_profile_enable(mi355_ctx* ctx, int on);
/* SIFT stage populations of the last extracted frame: [0] DoG extrema, [1] refined points, [2] oriented keypoints,
 * [3] kept (nfeatures + ties with the last one as KeyPointsFilter::retainBest keeps them, <= 2048), [4] overflow flag */
int  mi355_last_sift_counters(mi355_ctx* ctx, int32_t out8[8]);
int  mi355_profile_reset(mi355_ctx* ctx);
int  mi355_profile_only(mi355_ctx* ctx, const char* kernel_class /* NULL or "" = every class */);
/* class: "gauss", "extrema", "orient", "describe", "match", "select", "ransac", "warp", "gray" ...
 * Synchronises the stream. total_ms/launches may be NULL. */
int  mi355_profile_get(mi355_ctx* ctx, const char* kernel_class, double* total_ms, int64_t* launches, double* alg_bytes);

/* Synthetic input (bench / tests only, never timed): BGR frame sampled from a seeded procedural terrain through the
 * affine map (u,v) = A6 (x,y,1), written straight into HBM at d_dst. */
int  mi355_synth_frame_dev(mi355_ctx* ctx, uint8_t* d_dst, int w, int h, int ws, const float A6[6], uint32_t seed, uint32_t frame_seed,
                           float gain, float noise_sigma);

#ifdef __cplusplus
}
#endif
#endif /* MI355_MOSAIC_H */
