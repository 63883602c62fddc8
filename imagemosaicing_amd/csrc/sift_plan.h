// csrc/sift_plan.h -- what a SIFT batch (sift.hip) decides on the host before it touches the device: the Gaussian taps, the layout of a
// frame's work area, the batch length, and the pyramid + extrema launches of a batch with their routes and grids.  Host only, no HIP
// header (sift_plan.cpp is built by g++ as well: tests/test_sift_plan.py runs it under sanitizers); the constants below are shared
// with the kernels.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

namespace sift_plan {

constexpr int N_LAYERS = 3, N_LEVELS = 6, IMG_BORDER = 5, MAX_OCT = 16;
constexpr int MAX_R = 16;
constexpr int BATCH_MAX = 32;               // frames per batch (MI355_SIFT_BATCH_MAX: per-frame pointers travel in kernel arguments)
constexpr int T16W = 64, T16H = 32;         // blur16_tile's tile
#ifndef EXT_EH
#define EXT_EH 16
#endif
constexpr int EW = 64, EH = EXT_EH;         // extrema_kernel's tile
#ifndef REG_SHIFT_V
#define REG_SHIFT_V 0
#endif
constexpr int REG_SHIFT = REG_SHIFT_V;      // 2^REG_SHIFT consecutive tiles append to the same region: refine_kernel then walks spatially coherent runs
constexpr int NREG = 64;                    // candidate list split into 64 regions, one counter per 128-byte line:
                                            // a single counter caps at ~1e8 returning atomics/s (one per tile = 0.5 ms)
#ifndef MI355_XD
#define MI355_XD 2
#endif
constexpr int XD = MI355_XD;                // extrema_stream: rows in flight per wave
#ifndef MI355_XWAVES
#define MI355_XWAVES 3
#endif
constexpr int XWAVES = MI355_XWAVES;        // waves per SIMD the streamed test is compiled for (the launcher sizes its grid to whole rounds of them)
constexpr int XSW = 248;                    // columns a wave is responsible for: lanes 1..62; lanes 0 and 63 carry the neighbours' columns
constexpr int KA_TILE = 4096;               // keep-all: keys per sorted tile (keepall_sort_tiles_kernel)
constexpr size_t CNT_STRIDE = 64, CCNT_STRIDE = (size_t)64 * 32, SEL_STRIDE = 2048;
constexpr int WAVE_SLOTS = 1024;            // SIMDs of the chip: a streamed launch is sized to whole rounds of WAVE_SLOTS x waves per SIMD
constexpr int STREAM_MIN_L = 64;            // blur16_stream: fewest rows per segment (2R halo rows are read again per segment)
// Routes::narrow (option "narrow_routes"): blur16_stream from STREAM_NARROW_MIN_W columns on (two strips, the second at least half full:
// three quarters of the lanes carry pixels; a single partial strip would also ask reflect101 for columns past 2 w - 2 in its right halo
// lanes below 137 columns, and launches that narrow do not fill the chip); and where STREAM_MIN_L leaves a launch short of its `waves`
// per SIMD, segments sized for STREAM_NARROW_WAVES waves on every SIMD, no shorter than STREAM_NARROW_MIN_L rows and no longer than
// STREAM_MIN_L: a lone wave issues at half the SIMD's rate, so two waves of L + 2R + 1 steps finish before one of 64 + 2R + 1
// (profiles/narrow_octaves_kernel_stats.txt has the sweep over L)
constexpr int STREAM_NARROW_MIN_W = 384, STREAM_NARROW_WAVES = 2, STREAM_NARROW_MIN_L = 16;
constexpr int STREAM_W4_MAX_R = 8;         // blur16_stream: 4 waves per SIMD up to this radius (the register ring of the row results, 4 x (2R + 2), fits 128 registers), 3 above (168)
constexpr int REFINE_GX = 2;                // refine_kernel: workgroups per candidate region (32 x 64 regions x frames of mostly empty workgroups cost more to dispatch than the fits)

// cv::getGaussianKernel(ksize, sigma, CV_32F) into k[0 .. 2r]; returns the radius r
int gauss_taps(double sigma, float* k);
// the base level's taps (sqrt(1.6^2 - 0.5^2)) and those of levels 1 .. 5 (sigma_i = sqrt((s k^i)^2 - (s k^(i-1))^2)); lv[0] is not used.
// Positive and normalised: blur16_stream's rounding assumes results in [0, 32767].  Computed once per process.
struct Taps { int r; float k[2 * MAX_R + 1]; };
struct PyramidTaps { Taps base, lv[N_LEVELS]; };
const PyramidTaps& pyramid_taps();

// One frame's work area.  Offsets and strides in elements of the respective buffer; every pyramid level starts on a 128-byte boundary
// (offsets and bs.pyr are multiples of 64 samples: what the streamed kernels' 8-byte loads and the frame stride ask for holds by layout).
struct Strides { size_t pyr, claimed, cand, refined, kps, cube, sel, mins; };      // sel: selected keypoints per frame; mins: keep-all's start-key table
struct Octave { int w, h; size_t lv[N_LEVELS], claimed, mins; };      // claimed: duplicate claim bitmap (4 bits per pixel; numbered, but sift.hip backs it with no memory: duplicates leave in its selection); mins: keep-all, one word per claim bit
struct Layout {
    int w = 0, h = 0; bool keepall = false; int kmax = 0;      // the key: frame size, keep-all and its ceiling (option "keepall_max")
    int n_oct = 0;
    Octave oc[MAX_OCT];
    Strides bs;
    size_t ksort_stride;                                       // keep-all: per frame, its keys sorted tile by tile
    unsigned cand_cap, ref_cap, kp_cap, cube_cap;              // cand_cap per region; cube_cap: 3x3x3 DoG neighbourhoods of the first candidates of every region (128 B each)
    bool same_key(const Layout& o) const { return w == o.w && h == o.h && keepall == o.keepall && kmax == o.kmax; }
};
Layout make_layout(int w, int h, bool keepall, int kmax, std::string& err);      // err set: the frame is refused

// frames per batch: `requested` clamped to 1 .. BATCH_MAX, shortened for very large frames so that slots x batch work areas stay under
// 60 % of the device memory (total_mem 0: unknown, no shortening); keep-all batches hold at most 8
int batch_frames(int w, int h, bool keepall, int requested, int slots, size_t total_mem);

// The pyramid and extrema launches of a batch of n frames, in stream order.  blur_stream / xstream_min_w / xstream_min_frames: the
// options of those names; base_frames_aligned: every caller frame's pointer and pitch a multiple of 4 and its pitch >= 3 w; narrow: the
// option "narrow_routes" (0: the launches as they were before it existed).
struct Routes { int blur_stream, xstream_min_w, xstream_min_frames; bool base_frames_aligned; int narrow = 0; };
enum Kind { BLUR_STREAM, BLUR_TILE, DOWNSAMPLE, EXTREMA_STREAM, EXTREMA_TILE };
struct Launch {
    Kind kind; int octave, level;      // level: the one written (DOWNSAMPLE: 0 of `octave`; extrema: -1)
    int radius, waves; bool ds;        // blurs: taps radius; BLUR_STREAM: waves per SIMD; ds: also writes the next octave's base
    unsigned gx, gy, gz;               // grid (blocks of 256)
    int L, nstrip, nseg, xsw;          // streamed: rows per segment, strips, segments; EXTREMA_STREAM: columns per strip
    double bytes;                      // algorithmic traffic handed to the profile bracket
};
std::vector<Launch> pyramid_launches(const Layout& l, int n, const Routes& r);

}  // namespace sift_plan
