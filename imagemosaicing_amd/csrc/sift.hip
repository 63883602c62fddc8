// csrc/sift.hip -- K1..K5: SIFT detect + describe on gfx950, replacing the body of SiftExtraction_Thread
// (MosaicWithoutPos.cpp:4832-4887: SiftFeatureDetector(2000,3,0.01,20).detect + SiftDescriptorExtractor.compute).
//
// The algorithm is OpenCV 2.4.0's cv::SIFT as the reference's own binary runs it (oracle/oracle_sift.c says how that was
// established and how the reference's committed run pins it): NO image doubling, 16-BIT FIXED-POINT pyramids (gray x 48), Gaussian
// levels filtered 16S -> 32F -> 16S with separately rounded products and sums in the filter engine's tap order, integer DoG,
// |DoG| > 20, Cramer's rule for the 3x3 fit.  This file implements that definition, independently, for the GPU, and the parity
// tests compare keypoints and descriptors bit for bit with the oracle.
//
// Host side (end of this file): frames collect into batches (SiftWork); sift_plan.{h,cpp} decides a batch's layout and its pyramid and
// extrema launches, sift_run_batch enqueues them, and every launch covers all frames of the batch.  Kernels:
//   blur16_stream<R,BGR,DS,W>  separable Gaussian of one level (>= 384 columns; sift_plan's blur_streams()): a wave walks down a strip of 256 columns, rows arrive
//                         once from HBM (8 bytes per lane: four 16-bit samples), the row-filtered rows of the last 2R+1 steps live in
//                         registers (the column pass needs its taps centre first, then symmetric pairs: a gather, not a scatter),
//                         no workgroup barrier; BGR = true forms gray x 48 of the caller's frame on the fly (base level, no gray
//                         image is ever stored); DS = true (level 3) also writes the decimated base of the next octave
//   blur16_tile<R,BGR>    the same filter for small levels: 64x32 tile + halo in LDS, row pass then column pass
//   downsample16          next octave seed = every second pixel of level 3 (when the blur did not write it on the way out)
//   extrema_stream / extrema_kernel   DoG never materialised in HBM: the 6 Gaussian levels are read once, 26-neighbour
//                         test on the 5 DoG planes (extrema_stream: row extremes in registers, the raw rows in a wave-private
//                         LDS ring; extrema_kernel: LDS tiles), candidates leave with their 3x3x3 neighbourhood
//   refine                one lane per candidate: quadratic fit, contrast / edge tests; every accepted point is stored, also those of
//                         several start points that converged to one location
//   select_unique         response threshold above which nfeatures + margin refined points lie; lists the points above it, each
//                         location once (a hash of the few thousand locations in LDS)
//   orient                one wave per refined point above the threshold: 36-bin histogram in order-free fixed point,
//                         smoothing + peaks via lane shuffles
//   topk                  one workgroup per frame: radix select of the nfeatures-th response, bitonic sort of the
//                         survivors by the total order (response desc, octave, layer, row, col, bin)
//   keepall_live / _reset / _sort_tiles / _place   nfeatures <= 0: selection and top-k replaced by "every point, in generation order"
//   describe              one workgroup per keypoint: trilinear contributions quantised to 2^-10 and added with
//                         64-bit LDS atomics (order-free by definition), normalise / clip / renormalise -> u8
#include "common.h"
#include "sift_plan.h"
#include <memory>
#include "detmath.h"
#include <cmath>
#include <type_traits>

namespace {

using namespace sift_plan;                     // the constants the host plan shares with the kernels (N_LEVELS, MAX_R, EW, XSW, ...)
constexpr int MAX_INTERP = 5, ORI_BINS = 36;
constexpr int FIXPT_SCALE = 48;                 // SIFT_FIXPT_SCALE of the reference's OpenCV build: pyramid samples are gray x 48 in 16 bits
constexpr float DOG_THRESHOLD_P1 = 21.0f;       // |DoG| > floor(0.5 * 0.01 / 3 * 255 * 48) = 20, on integers: |DoG| >= 21
constexpr float HIST_Q = 1024.0f;               // order-free histogram accumulation: contributions quantised to 2^-10 (oracle_sift.c)
constexpr int SIFT_BATCH_MAX = MI355_SIFT_BATCH_MAX;
static_assert(SIFT_BATCH_MAX == BATCH_MAX, "sift_plan.h: BATCH_MAX");
typedef int16_t lvl_t;                          // one pyramid sample

__host__ __device__ __forceinline__ int reflect101(int p, int n) {
    if (n == 1) return 0;
    while (p < 0 || p >= n) { if (p < 0) p = -p; else p = 2 * n - 2 - p; }
    return p;
}

typedef float v2f __attribute__((ext_vector_type(2)));
struct __attribute__((aligned(4))) uint2_a4 { unsigned x, y; };     // two dwords at a 4-byte aligned address (global_load_dwordx2 asks for no more)
typedef float v4f __attribute__((ext_vector_type(4)));

// four / one 16-bit samples as floats (exact)
__device__ __forceinline__ v4f ld4(const lvl_t* p) {              // p 8-byte aligned
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    v4f o;
    o.x = (float)(int)(short)(q.x & 0xffffu); o.y = (float)((int)q.x >> 16);
    o.z = (float)(int)(short)(q.y & 0xffffu); o.w = (float)((int)q.y >> 16);
    return o;
}
__device__ __forceinline__ float ld1(const lvl_t* p) { return (float)(int)*p; }
// saturate_cast<short>(float): round half to even, clamp
__device__ __forceinline__ int sat16(float v) {
    int q = (int)rintf(v);
    q = q < -32768 ? -32768 : (q > 32767 ? 32767 : q);
    return q;
}
__device__ __forceinline__ float gray48(const uint8_t* p) {       // 8-bit BGR2GRAY fixed point, x 48 (convertTo(CV_16S, 48))
    return (float)(((1868 * (int)p[0] + 9617 * (int)p[1] + 4899 * (int)p[2] + 8192) >> 14) * FIXPT_SCALE);
}

// XCD-aware remap: hardware places block b on XCD b % 8; give every XCD a contiguous run of tiles
__device__ __forceinline__ int xcd_remap(int bid, int nb) {
    const int q = nb >> 3, r = nb & 7, xcd = bid & 7, local = bid >> 3;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + local;
}

// compile-time row loop (the unrolled body must see its ring slot as a constant; #pragma unroll gives up on bodies this large)
template <int J, int NPP, class F> __device__ __forceinline__ bool static_rows(F& f) {
    if constexpr (J < NPP) { if (!f(std::integral_constant<int, J>{})) return false; return static_rows<J + 1, NPP>(f); }
    else return true;
}

// ---------- K1/K2: separable Gaussian, 16S -> 32F -> 16S ------------------------------------------------------------------------
// Arithmetic (oracle_sift.c gauss_blur16; OpenCV's RowFilter<short,float> + SymmColumnFilter<Cast<float,short>>), products and sums
// rounded separately (this translation unit is compiled with -ffp-contract=off; nothing below may become an fma):
//   row     t(x) = k[0] * S(x - R);  t(x) += k[i] * S(x - R + i)            for i = 1 .. 2R
//   column  s    = k[R] * t(y);      s    += k[R + j] * (t(y + j) + t(y - j)) for j = 1 .. R;   out = round-half-even(s) in 16 bits
// borders reflect-101.
struct Blur16Args {
    const lvl_t* src;                        // source level (w x h), frame f at src + f * fstride
    const uint8_t* bgr[SIFT_BATCH_MAX];      // BGR = true: the caller's frames (w x h, row stride bgr_ws[f] bytes)
    int bgr_ws[SIFT_BATCH_MAX];
    lvl_t* dst;                              // frame f at dst + f * fstride
    lvl_t* ds;                               // not NULL: also write the 2x decimated level (even rows, even columns): the next octave's base
    int w, h;
    int tiles_x, tiles_y;
    float k[2 * MAX_R + 1];
    float kp[2 * (MAX_R + 1)];               // blur16_stream: tap pairs (k[t], k[t-1]) for t = 0 .. R, k[-1] = 0
    size_t fstride;                          // samples between the frames of a batch
    int nb;                                  // frames in the launch
};

template <int R, bool BGR>
__global__ __launch_bounds__(256) void blur16_tile(Blur16Args a) {
    constexpr int ROWS = T16H + 2 * R, COLS = T16W + 2 * R, PIN = COLS | 1, PMID = T16W + 4;
    __shared__ float s_in[ROWS * PIN];
    __shared__ __attribute__((aligned(16))) float s_mid[ROWS * PMID];
    const int tid = threadIdx.x, fr = blockIdx.y;
    const int tile = xcd_remap(blockIdx.x, a.tiles_x * a.tiles_y);
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x0 = tx * T16W, y0 = ty * T16H;
    const lvl_t* src = BGR ? nullptr : a.src + (size_t)fr * a.fstride;
    const uint8_t* bgr = a.bgr[0]; int bws = a.bgr_ws[0];
    if (BGR) {
#pragma unroll
        for (int q = 1; q < SIFT_BATCH_MAX; q++) if (fr == q) { bgr = a.bgr[q]; bws = a.bgr_ws[q]; }
    }
    lvl_t* dst = a.dst + (size_t)fr * a.fstride;
    for (int idx = tid; idx < ROWS * COLS; idx += 256) {
        const int ry = idx / COLS, rx = idx - ry * COLS;
        const int gy = reflect101(y0 - R + ry, a.h), gx = reflect101(x0 - R + rx, a.w);
        s_in[ry * PIN + rx] = BGR ? gray48(bgr + (size_t)gy * bws + 3 * gx) : ld1(src + (size_t)gy * a.w + gx);
    }
    __syncthreads();
    // row pass: 4 adjacent outputs per item from a sliding window
    for (int item = tid; item < ROWS * (T16W / 4); item += 256) {
        const int xg = item / ROWS, row = item - xg * ROWS;
        const float* in = s_in + row * PIN + 4 * xg;
        float e[2 * R + 4];
#pragma unroll
        for (int m = 0; m < 2 * R + 4; m++) e[m] = in[m];
        float acc[4];
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = a.k[0] * e[q];
#pragma unroll
        for (int i = 1; i <= 2 * R; i++) {
#pragma unroll
            for (int q = 0; q < 4; q++) { const float p = a.k[i] * e[q + i]; acc[q] = acc[q] + p; }
        }
        *reinterpret_cast<v4f*>(s_mid + row * PMID + 4 * xg) = (v4f){acc[0], acc[1], acc[2], acc[3]};
    }
    __syncthreads();
    // column pass: centre tap, then the symmetric pairs outwards; one output row x 4 columns per item
    for (int item = tid; item < T16H * (T16W / 4); item += 256) {
        const int yy = item / (T16W / 4), xg = item - yy * (T16W / 4);
        const float* mid = s_mid + (yy + R) * PMID + 4 * xg;
        v4f acc = *reinterpret_cast<const v4f*>(mid) * a.k[R];
#pragma unroll
        for (int j = 1; j <= R; j++) {
            const v4f sm = *reinterpret_cast<const v4f*>(mid + j * PMID) + *reinterpret_cast<const v4f*>(mid - j * PMID);
            const v4f p = sm * a.k[R + j];
            acc = acc + p;
        }
        const int gx = x0 + 4 * xg, gy = y0 + yy;
        if (gy >= a.h) continue;
        const int o0 = sat16(acc.x), o1 = sat16(acc.y), o2 = sat16(acc.z), o3 = sat16(acc.w);
        lvl_t* d = dst + (size_t)gy * a.w + gx;
        if (gx + 3 < a.w && (a.w & 3) == 0) {
            *reinterpret_cast<uint2*>(d) = make_uint2((unsigned)(o0 & 0xffff) | ((unsigned)o1 << 16), (unsigned)(o2 & 0xffff) | ((unsigned)o3 << 16));
        } else {
            if (gx < a.w) d[0] = (lvl_t)o0;
            if (gx + 1 < a.w) d[1] = (lvl_t)o1;
            if (gx + 2 < a.w) d[2] = (lvl_t)o2;
            if (gx + 3 < a.w) d[3] = (lvl_t)o3;
        }
        if (a.ds && !(gy & 1) && (gy >> 1) < (a.h >> 1)) {
            lvl_t* q = a.ds + (size_t)fr * a.fstride + (size_t)(gy >> 1) * (a.w >> 1);
            if ((gx >> 1) < (a.w >> 1)) q[gx >> 1] = (lvl_t)o0;
            if (((gx + 2) >> 1) < (a.w >> 1)) q[(gx + 2) >> 1] = (lvl_t)o2;
        }
    }
}

// ---- blur16_stream: barrier-free streaming variant for the big levels ---------------------------------------------------------------
// Same arithmetic.  One WAVE owns a strip of 256 columns (4 per lane) and walks down L output rows of it: every input row is read
// once from HBM (prefetched two rows ahead into registers), exchanged with the neighbour lanes through a wave-private LDS row (no
// workgroup barrier anywhere: LDS operations of one wave execute in order), filtered horizontally from a rolling register window, and
// kept in a register ring of the last 2R+2 row results; an output row leaves one step after its last row has arrived (its column pass
// covers the LDS round trip of the next row's window), taps centre first, then the pairs (y + j, y - j).
// The row loop itself is hand-scheduled gfx950 assembly (blur16_asm.inc, generated by gen_blur16_asm.py, which says what the hand
// schedule does that hipcc's did not: counted vmcnt waits, tap-staggered packed products without register moves, ...).  The HIP code
// below only works out the wave's geometry.
#include "build/blur16_asm.inc"     // generated next to the objects (build.py generate()); the path is explicit so that a stale copy left in csrc/ by an older checkout can never be picked up
template <int R, bool BGR, bool DS>
__device__ __forceinline__ void blur16_stream_body(const Blur16Args& a, int L, int nstrip, int nseg) {
    constexpr int RA = (R + 3) / 4 * 4, SW = 256, BW = SW + 2 * RA;
    constexpr int BUF = (BW + 8 + 63) & ~63;          // + 8 floats: dump area for lanes that have no halo sample to write
    static_assert(2 * RA + R <= 64, "halo lanes");
    __shared__ __attribute__((aligned(16))) float s_buf[4][2][BUF];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // wave-uniform by construction; readfirstlane tells the compiler, so that segment, strip and row pointers live in scalar registers.
    // Every return below is taken by whole waves (the tests are on `unit`): the assembly body runs with all 64 lanes on and leaves exec = -1
    int unit = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + wave);
    const int per = nstrip * nseg, fr = unit / per;
    if (fr >= a.nb) return;
    unit -= fr * per;
    const int seg = unit / nstrip, strip = unit - seg * nstrip;
    if (seg >= nseg) return;
    const int x0 = strip * SW, y0 = seg * L;          // L is even (launcher): the decimated rows are the even rows of a segment
    const int lact = (a.h - y0 < L) ? a.h - y0 : L;
    const int wv = a.w - x0;                          // valid columns of this strip (> R, checked by the launcher)
    // columns: the lane's own four (clamped into the row for a partial last strip); one more sample for the lanes < 2 RA (the halos,
    // reflect-101) and, in a partial last strip, for the lanes 2 RA .. 2 RA + R - 1: the reflected columns right of the image,
    // written AFTER the main samples (LDS operations of one wave execute in order) over whatever the clamped main loads left there
    const int xm = x0 + 4 * lane;
    const int xl = xm < a.w - 4 ? xm : a.w - 4;
    int hcol, hpos;
    if (lane < RA) { hcol = x0 - RA + lane; hpos = lane; }
    else if (lane < 2 * RA) { hcol = x0 + SW + (lane - RA); hpos = SW + lane; }
    else if (wv < SW && lane < 2 * RA + R) { hcol = x0 + wv + (lane - 2 * RA); hpos = RA + wv + (lane - 2 * RA); }
    else { hcol = x0; hpos = BW + (lane & 7); }
    hcol = reflect101(hcol, a.w);
    const size_t fro = (size_t)fr * a.fstride;
    const uint8_t* bgr = a.bgr[0]; int bws = a.bgr_ws[0];
    if (BGR) {
#pragma unroll
        for (int q = 1; q < SIFT_BATCH_MAX; q++) if (fr == q) { bgr = a.bgr[q]; bws = a.bgr_ws[q]; }
    }
    const int rowb = BGR ? bws : 2 * a.w;             // bytes per source row
    int gy = y0 - R, dir = 1;                         // first source row of the reflect-101 walk
    if (gy < 0) { gy = -gy; dir = -1; }
    const unsigned long long rp = (unsigned long long)(BGR ? reinterpret_cast<uintptr_t>(bgr) : reinterpret_cast<uintptr_t>(a.src + fro)) + (unsigned long long)gy * (unsigned)rowb;
    const unsigned moff = BGR ? 3u * xl : 2u * xl;    // 3 xl is a multiple of 12; rows are 4-byte aligned (launcher)
    unsigned hoff, hsh = 0;
    if (BGR) {                                        // the 8 bytes inside the row that hold the halo pixel's three
        const int b0 = 3 * hcol; int st = b0 & ~3; if (st + 8 > bws) st = bws - 8;
        hoff = (unsigned)st; hsh = 8u * (unsigned)(b0 - st);
    } else hoff = 2u * hcol;
    const unsigned lds0 = (unsigned)reinterpret_cast<uintptr_t>(&s_buf[wave][0][0]);
    const unsigned lds_win = lds0 + 16u * lane, lds_main = lds0 + 4u * (RA + 4 * lane), lds_halo = lds0 + 4u * hpos;
    const unsigned long long dp = (unsigned long long)reinterpret_cast<uintptr_t>(a.dst + fro) + 2ull * (unsigned long long)y0 * a.w;
    const unsigned long long dsp = DS ? (unsigned long long)reinterpret_cast<uintptr_t>(a.ds + fro) + 2ull * (unsigned long long)(y0 >> 1) * (a.w >> 1) : 0ull;
    const unsigned doff = 2u * xm, dsoff = 2u * (xm >> 1);
    const unsigned long long smask = __ballot(xm < a.w);                 // lanes that store (partial last strip)
    const unsigned long long kp = (unsigned long long)reinterpret_cast<uintptr_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(Blur16Args, kp);
    const int n = lact + 2 * R + 1;                   // steps: 2R + 1 rows fill the ring, then one output row per step
    const int hm1 = a.h - 1, dstr = 2 * a.w;
    (void)hsh;
#define BLUR_ASM_CALL(NAME) NAME(lds_win, lds_main, lds_halo, moff, hoff, doff, dsoff, rp, dp, dsp, kp, smask, rowb, gy, dir, hm1, dstr, n)
    if constexpr (BGR) { static_assert(R == 6, "base level"); blur16_asm_r6_bgr(lds_win, lds_main, lds_halo, moff, hoff, doff, dsoff, hsh, rp, dp, dsp, kp, smask, rowb, gy, dir, hm1, dstr, n); }
    else if constexpr (R == 5) BLUR_ASM_CALL(blur16_asm_r5);
    else if constexpr (R == 6) BLUR_ASM_CALL(blur16_asm_r6);
    else if constexpr (R == 8 && DS) BLUR_ASM_CALL(blur16_asm_r8_ds);
    else if constexpr (R == 8) BLUR_ASM_CALL(blur16_asm_r8);
    else if constexpr (R == 10) BLUR_ASM_CALL(blur16_asm_r10);
    else if constexpr (R == 13) BLUR_ASM_CALL(blur16_asm_r13);
#undef BLUR_ASM_CALL
}
// W waves per SIMD: the launcher sizes the grid to exactly W x 1024 waves, and the cap keeps the dispatcher from stacking them unevenly
template <int R, bool BGR, bool DS, int W>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, W))) void blur16_stream(Blur16Args a, int L, int nstrip, int nseg) {
    blur16_stream_body<R, BGR, DS>(a, L, nstrip, nseg);
}

// next octave seed: every second pixel of level 3 (cv::resize INTER_NEAREST to half size)
__global__ __launch_bounds__(256) void downsample16(const lvl_t* src, int sw, lvl_t* dst, int dw, int dh, size_t fstride) {
    src += (size_t)blockIdx.z * fstride; dst += (size_t)blockIdx.z * fstride;      // blockIdx.z = frame of the batch
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x < dw && y < dh) dst[(size_t)y * dw + x] = src[(size_t)(2 * y) * sw + 2 * x];
}

// ---------- K3: DoG extrema -------------------------------------------------------------------------------------
struct OctaveDev { lvl_t* lv[N_LEVELS]; int w, h; };

constexpr int ECAP = 128;
constexpr int REG_STRIDE = 32;              // one counter of the NREG candidate regions per 128-byte line
// batched launches: frame f = blockIdx.y (z for refine) works on its own copy of every buffer, a fixed stride apart
struct BatchStride { size_t pyr, cand, refined, kps, cube, sel, mins; };   // elements of the respective type (sel: selected keypoints per frame; mins: keep-all's start-key table)
struct FrameOuts { mi355_keypoint* kp[SIFT_BATCH_MAX]; uint8_t* d8[SIFT_BATCH_MAX]; };

// ---------- K3b: sub-pixel refinement ---------------------------------------------------------------------------
struct Refined { int o, layer, r, c; float xi, xr, xc, contr, scl; unsigned start; };      // start: keep-all: (layer, row, column) of the extremum the fit started from, packed 2 + 14 + 14 bits

struct PyrDev { OctaveDev oc[MAX_OCT]; unsigned* mins[MAX_OCT]; int n_oct; };      // mins: keep-all only (one word per layer of every pixel)

// DoG[lvl] = G[lvl + 1] - G[lvl]: 16-bit integers (cv::subtract into CV_16S; the samples are 0 .. 12240, nothing saturates), exact as float
__device__ __forceinline__ float dogv(const OctaveDev& oc, size_t foff, int lvl, int r, int c) {
    const size_t o = foff + (size_t)r * oc.w + c;
    return (float)((int)oc.lv[lvl + 1][o] - (int)oc.lv[lvl][o]);
}

// Matx33f::solve(b, DECOMP_LU) = Matx_FastSolveOp<float, 3, 1>: Cramer's rule in float, the expression of the vendored
// core/operations.hpp:742-750, 882-903 (products and sums rounded separately); det == 0 -> x = 0
__device__ __forceinline__ void solve3(const float a[3][3], const float b[3], float x[3]) {
    const float det = (a[0][0] * (a[1][1] * a[2][2] - a[2][1] * a[1][2]) - a[0][1] * (a[1][0] * a[2][2] - a[2][0] * a[1][2])) + a[0][2] * (a[1][0] * a[2][1] - a[2][0] * a[1][1]);
    if (det == 0.0f) { x[0] = x[1] = x[2] = 0.0f; return; }
    const float d = 1.0f / det;
    x[0] = d * ((b[0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (b[1] * a[2][2] - a[1][2] * b[2])) + a[0][2] * (b[1] * a[2][1] - a[1][1] * b[2]));
    x[1] = d * ((a[0][0] * (b[1] * a[2][2] - a[1][2] * b[2]) - b[0] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])) + a[0][2] * (a[1][0] * b[2] - b[1] * a[2][0]));
    x[2] = d * ((a[0][0] * (a[1][1] * b[2] - b[1] * a[2][1]) - a[0][1] * (a[1][0] * b[2] - b[1] * a[2][0])) + b[0] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]));
}

// One Newton step of the quadratic fit at (L, R, C) and the acceptance tests, written once over an accessor dv(L, R, C)
// so that the in-tile first step (DoG planes in LDS, extrema_kernel) and the iterative path (global memory,
// refine_kernel) evaluate the very same expressions.
struct FitOff { float xi, xr, xc; };
template <class DV>
__device__ __forceinline__ FitOff fit_step(DV dv, int L, int R, int C) {
    const float img_scale = 1.0f / (float)(255 * FIXPT_SCALE);
    const float deriv_scale = img_scale * 0.5f, second_scale = img_scale, cross_scale = img_scale * 0.25f;
    float dD[3];
    dD[0] = (dv(L, R, C + 1) - dv(L, R, C - 1)) * deriv_scale;
    dD[1] = (dv(L, R + 1, C) - dv(L, R - 1, C)) * deriv_scale;
    dD[2] = (dv(L + 1, R, C) - dv(L - 1, R, C)) * deriv_scale;
    const float v2 = dv(L, R, C) * 2.0f;
    const float dxx = (dv(L, R, C + 1) + dv(L, R, C - 1) - v2) * second_scale;
    const float dyy = (dv(L, R + 1, C) + dv(L, R - 1, C) - v2) * second_scale;
    const float dss = (dv(L + 1, R, C) + dv(L - 1, R, C) - v2) * second_scale;
    const float dxy = (dv(L, R + 1, C + 1) - dv(L, R + 1, C - 1) - dv(L, R - 1, C + 1) + dv(L, R - 1, C - 1)) * cross_scale;
    const float dxs = (dv(L + 1, R, C + 1) - dv(L + 1, R, C - 1) - dv(L - 1, R, C + 1) + dv(L - 1, R, C - 1)) * cross_scale;
    const float dys = (dv(L + 1, R + 1, C) - dv(L + 1, R - 1, C) - dv(L - 1, R + 1, C) + dv(L - 1, R - 1, C)) * cross_scale;
    const float A[3][3] = {{dxx, dxy, dxs}, {dxy, dyy, dys}, {dxs, dys, dss}};
    float X[3];
    solve3(A, dD, X);
    FitOff f; f.xi = -X[2]; f.xr = -X[1]; f.xc = -X[0];
    return f;
}
// contrast and edge tests at the converged location; contr is the interpolated response
template <class DV>
__device__ __forceinline__ bool fit_accept(DV dv, int L, int R, int C, FitOff f, float contrast_thr, float edge_thr, float& contr) {
    const float img_scale = 1.0f / (float)(255 * FIXPT_SCALE);
    const float deriv_scale = img_scale * 0.5f, second_scale = img_scale, cross_scale = img_scale * 0.25f;
    float dD0 = (dv(L, R, C + 1) - dv(L, R, C - 1)) * deriv_scale;
    float dD1 = (dv(L, R + 1, C) - dv(L, R - 1, C)) * deriv_scale;
    float dD2 = (dv(L + 1, R, C) - dv(L - 1, R, C)) * deriv_scale;
    const float t = ((0.0f + dD0 * f.xc) + dD1 * f.xr) + dD2 * f.xi;          // Matx::dot: s = 0; s += a[i] * b[i]
    contr = dv(L, R, C) * img_scale + t * 0.5f;
    if (fabsf(contr) * (float)N_LAYERS < contrast_thr) return false;
    const float v2 = dv(L, R, C) * 2.0f;
    const float dxx = (dv(L, R, C + 1) + dv(L, R, C - 1) - v2) * second_scale;
    const float dyy = (dv(L, R + 1, C) + dv(L, R - 1, C) - v2) * second_scale;
    const float dxy = (dv(L, R + 1, C + 1) - dv(L, R + 1, C - 1) - dv(L, R - 1, C + 1) + dv(L, R - 1, C - 1)) * cross_scale;
    const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
    if (det <= 0.0f || (tr * tr) * edge_thr >= ((edge_thr + 1.0f) * (edge_thr + 1.0f)) * det) return false;
    return true;
}
// 0: converged, 1: dead (diverged / NaN), 2: keep iterating
__device__ __forceinline__ int fit_state(FitOff f) {
    if (fabsf(f.xi) < 0.5f && fabsf(f.xr) < 0.5f && fabsf(f.xc) < 0.5f) return 0;
    if (fabsf(f.xi) > 7.0e8f || fabsf(f.xr) > 7.0e8f || fabsf(f.xc) > 7.0e8f) return 1;
    if (!(f.xi == f.xi) || !(f.xr == f.xr) || !(f.xc == f.xc)) return 1;
    return 2;
}

__global__ __launch_bounds__(256) void extrema_kernel(OctaveDev oc, int octave, unsigned long long* cand, unsigned* count, unsigned cap, unsigned* overflow, BatchStride bs,
                                                      float* cube, unsigned cube_cap) {
    {
        const size_t f = blockIdx.y;
#pragma unroll
        for (int l = 0; l < N_LEVELS; l++) oc.lv[l] += f * bs.pyr;
        cand += f * bs.cand; count += f * CCNT_STRIDE; overflow += f * CNT_STRIDE; cube += f * bs.cube;
    }
    // staged window: rows y0-1 .. y0+EH, columns x0-4 .. x0+EW+3 (16-byte aligned so that interior tiles load float4)
    constexpr int PC = EW + 8;                 // 72 columns
    constexpr int P4 = PC / 4;                 // 18 float4 per row
    constexpr int RW = EH + 2;                 // 18 rows
    __shared__ v4f s_d4[5][RW * P4];
    __shared__ unsigned long long s_list[ECAP];   // candidates of this tile: one global atomic per workgroup
    __shared__ unsigned s_n, s_base;
    const int tid = threadIdx.x;
    // XCD-aware tile order: consecutive tiles (horizontal neighbours, which share their halo columns' cache lines) run on
    // the same XCD, i.e. behind the same L2 -- with the default round-robin every halo line came from HBM again
    // (measured: 2.2x the algorithmic bytes at the fabric).
    const int tiles_x = (oc.w + EW - 1) / EW, tiles_y = (oc.h + EH - 1) / EH;
    const int tile = xcd_remap(blockIdx.x, tiles_x * tiles_y);
    const int tyy = tile / tiles_x, txx = tile - tyy * tiles_x;
    const int x0 = txx * EW, y0 = tyy * EH;
    if (tid == 0) s_n = 0;
    const bool vec = ((oc.w & 3) == 0) && (x0 - 4 >= 0) && (x0 + EW + 4 <= oc.w) && ((reinterpret_cast<uintptr_t>(oc.lv[0]) & 7) == 0);
    if (vec) {
        // centre columns x0 .. x0+EW-1: whole 256-byte runs (two 128-byte lines per row and level), float4 per lane
        for (int idx = tid; idx < RW * (EW / 4); idx += 256) {
            const int ry = idx / (EW / 4), c4 = idx - ry * (EW / 4);
            int gy = y0 - 1 + ry;
            gy = gy < 0 ? 0 : (gy > oc.h - 1 ? oc.h - 1 : gy);      // clamped halo rows are never used by valid pixels (5 px border)
            const size_t o = (size_t)gy * oc.w + (x0 + 4 * c4);
            v4f g[N_LEVELS];
#pragma unroll
            for (int l = 0; l < N_LEVELS; l++) g[l] = ld4(oc.lv[l] + o);
#pragma unroll
            for (int l = 0; l < 5; l++) s_d4[l][ry * P4 + 1 + c4] = g[l + 1] - g[l];
        }
        // the two halo columns x0-1 and x0+EW (lines the neighbouring tiles fetch anyway)
        if (tid < 2 * RW) {
            const int ry = tid >> 1, side = tid & 1;
            int gy = y0 - 1 + ry;
            gy = gy < 0 ? 0 : (gy > oc.h - 1 ? oc.h - 1 : gy);
            const size_t o = (size_t)gy * oc.w + (side ? x0 + EW : x0 - 1);
            float g[N_LEVELS];
#pragma unroll
            for (int l = 0; l < N_LEVELS; l++) g[l] = ld1(oc.lv[l] + o);
#pragma unroll
            for (int l = 0; l < 5; l++) reinterpret_cast<float*>(s_d4[l])[ry * PC + (side ? 4 + EW : 3)] = g[l + 1] - g[l];
        }
    } else {
        for (int idx = tid; idx < RW * PC; idx += 256) {
            const int ry = idx / PC, rx = idx - ry * PC;
            int gy = y0 - 1 + ry, gx = x0 - 4 + rx;
            gy = gy < 0 ? 0 : (gy > oc.h - 1 ? oc.h - 1 : gy);
            gx = gx < 0 ? 0 : (gx > oc.w - 1 ? oc.w - 1 : gx);
            const size_t o = (size_t)gy * oc.w + gx;
            float g[N_LEVELS];
#pragma unroll
            for (int l = 0; l < N_LEVELS; l++) g[l] = ld1(oc.lv[l] + o);
#pragma unroll
            for (int l = 0; l < 5; l++) reinterpret_cast<float*>(s_d4[l])[idx] = g[l + 1] - g[l];
        }
    }
    __syncthreads();
    // one item per lane: 4 adjacent pixels of one row.  All 5 DoG planes' 3x6 windows go to registers (one 128-bit and two
    // 32-bit LDS reads per row), column-wise 3-row max/min are shared by the 4 pixels, and the 26-neighbour test becomes
    // "val >= max of the neighbours" / "val <= min of the neighbours" without data-dependent branches.
    for (int item = tid; item < EH * (EW / 4); item += 256) {
        const int ly = item / (EW / 4), xg = item - ly * (EW / 4);
        const int r = y0 + ly;
        float cm[5][6], cn[5][6], mid[5][6], top[5][6], bot[5][6];
#pragma unroll
        for (int pl = 0; pl < 5; pl++) {
            const float* base = reinterpret_cast<const float*>(s_d4[pl]) + (ly + 1) * PC + 4 * xg + 4;
#pragma unroll
            for (int rr = -1; rr <= 1; rr++) {
                const float* q = base + rr * PC;
                const v4f c4 = *reinterpret_cast<const v4f*>(q);
                float v[6] = {q[-1], c4.x, c4.y, c4.z, c4.w, q[4]};
#pragma unroll
                for (int j = 0; j < 6; j++) { if (rr == -1) top[pl][j] = v[j]; else if (rr == 0) mid[pl][j] = v[j]; else bot[pl][j] = v[j]; }
            }
#pragma unroll
            for (int j = 0; j < 6; j++) {
                cm[pl][j] = fmaxf(fmaxf(top[pl][j], mid[pl][j]), bot[pl][j]);
                cn[pl][j] = fminf(fminf(top[pl][j], mid[pl][j]), bot[pl][j]);
            }
        }
        // all 12 tests of the item without a branch (same exact predicate as extrema_stream: |val| >= max(val > 0 ? mx : -mn, 21), DoG values are integers);
        // the rare hits are emitted afterwards
        unsigned hit = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = k + 1;
#pragma unroll
            for (int layer = 1; layer <= N_LAYERS; layer++) {
                const float val = mid[layer][j];
                // neighbours: full 3x3 of the two adjacent planes + the 8 in-plane ones
                float mx = fmaxf(fmaxf(cm[layer - 1][j - 1], cm[layer - 1][j]), cm[layer - 1][j + 1]);
                mx = fmaxf(mx, fmaxf(fmaxf(cm[layer + 1][j - 1], cm[layer + 1][j]), cm[layer + 1][j + 1]));
                mx = fmaxf(mx, fmaxf(fmaxf(cm[layer][j - 1], cm[layer][j + 1]), fmaxf(top[layer][j], bot[layer][j])));
                float mn = fminf(fminf(cn[layer - 1][j - 1], cn[layer - 1][j]), cn[layer - 1][j + 1]);
                mn = fminf(mn, fminf(fminf(cn[layer + 1][j - 1], cn[layer + 1][j]), cn[layer + 1][j + 1]));
                mn = fminf(mn, fminf(fminf(cn[layer][j - 1], cn[layer][j + 1]), fminf(top[layer][j], bot[layer][j])));
                const float q = val > 0.0f ? mx : -mn;
                hit |= fabsf(val) >= fmaxf(q, DOG_THRESHOLD_P1) ? (1u << ((layer - 1) * 4 + k)) : 0u;
            }
        }
        unsigned cmask = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { const int c = x0 + 4 * xg + k; cmask |= (c >= IMG_BORDER && c < oc.w - IMG_BORDER) ? (0x111u << k) : 0u; }
        hit = (r >= IMG_BORDER && r < oc.h - IMG_BORDER) ? (hit & cmask) : 0u;
        while (hit) {
            const int bb = __builtin_ctz(hit); hit &= hit - 1;
            const int layer = bb / 4 + 1, c = x0 + 4 * xg + (bb & 3);
            const unsigned long long rec = ((unsigned long long)octave << 48) | ((unsigned long long)layer << 40) | ((unsigned long long)r << 20) | (unsigned long long)c;
            const unsigned slot = atomicAdd(&s_n, 1u);
            if (slot < ECAP) s_list[slot] = rec;
            else {                                                                           // tile with > 128 extrema (flat image)
                const unsigned reg = ((unsigned)tile >> REG_SHIFT) & (NREG - 1);
                const unsigned g = atomicAdd(&count[reg * REG_STRIDE], 1u);
                if (g < cap) cand[(size_t)reg * cap + g] = rec; else *overflow = 1;
            }
        }
    }
    __syncthreads();
    const unsigned nloc = s_n < ECAP ? s_n : ECAP;
    const unsigned reg = ((unsigned)tile >> REG_SHIFT) & (NREG - 1);
    if (tid == 0 && nloc) s_base = atomicAdd(&count[reg * REG_STRIDE], nloc);
    __syncthreads();
    // Each candidate also leaves with its 3x3x3 DoG neighbourhood (27 floats in a 128-byte record, straight from the LDS
    // planes): the first Newton step of refine_kernel -- the only one for two candidates out of three -- then reads one line
    // instead of twelve cold ones scattered over four pyramid levels.  Bit 63 of the record says the cube exists.
    for (unsigned i = tid; i < nloc; i += 256) {
        const unsigned g = s_base + i;
        if (g < cap) cand[(size_t)reg * cap + g] = s_list[i] | (g < cube_cap ? (1ull << 63) : 0ull); else *overflow = 1;
    }
    for (unsigned idx = tid; idx < nloc * 27; idx += 256) {
        const unsigned ci = idx / 27, e = idx - ci * 27;
        const unsigned g = s_base + ci;
        if (g >= cube_cap) continue;
        const unsigned long long rec = s_list[ci];
        const int L0 = (int)((rec >> 40) & 0xff), R0 = (int)((rec >> 20) & 0xfffff), C0 = (int)(rec & 0xfffff);
        const int dl = (int)(e / 9) - 1, dr = (int)((e / 3) % 3) - 1, dc = (int)(e % 3) - 1;
        cube[((size_t)reg * 32 + e) * cube_cap + g] = reinterpret_cast<const float*>(s_d4[L0 + dl])[(R0 + dr - y0 + 1) * PC + (C0 + dc - x0) + 4];
    }
}

// ---- extrema_stream: the same test, streamed -------------------------------------------------------------------
// One WAVE owns a strip of 256 columns (4 per lane) and walks down its rows: every row of the six levels is read once
// (XD rows are in flight while the current one is processed), the 3-wide extremes of the five DoG planes of three
// consecutive rows live in registers, the neighbours' columns come through DPP wave shifts, and nothing waits on a
// workgroup barrier.  The raw DoG rows of the window also sit in a wave-private LDS ring (plane, row mod 3, column).
// The hot loop issues no GLOBAL memory operation besides those row loads: a candidate (rare) is parked in a wave-private
// LDS list together with its 3x3x3 DoG neighbourhood, read from the ring; the list and the neighbourhoods go to global
// memory when the list is half full and at the end of the segment.
constexpr int XCAP = 144;                       // candidate records buffered per wave (8 bytes each)
constexpr int XNB_CAP = 64;                     // the first XNB_CAP of them also have their neighbourhood parked; the list is emptied when XNB_CAP / 2 are in it, between runs of the row loop
constexpr int XRING_DW = 5 * 3 * 128;           // the ring: 5 planes x 3 rows x 256 columns of 16 bits = 7680 B per wave
constexpr int XNB_DW = 18;                      // a parked neighbourhood: 3 planes x 3 rows x the two packed dwords (4 columns) that hold columns c-1 .. c+1
constexpr int XLDS_BYTES = 4 * (XRING_DW * 4 + XCAP * 8 + XNB_CAP * XNB_DW * 4);
static_assert(XWAVES * XLDS_BYTES <= 160 * 1024 && XLDS_BYTES <= 53 * 1024, "extrema_stream: ring + list must leave room for XWAVES workgroups per CU");
// The DoG values are 16-bit integers and stay PACKED, two columns per register, from the level rows to the test: v_pk_sub_i16 forms
// them straight from the loaded level words (no unpacking), v_pk_max_i16 / v_pk_min_i16 take the extremes of two columns at a time and
// the 16-bit compares read either half (SDWA).  Half the registers of the float form of round 3 (4 waves per SIMD instead of 2) and
// three quarters of its instructions.
typedef short s2 __attribute__((ext_vector_type(2)));
struct XRow { uint2 m[N_LEVELS]; };             // one row of the six levels: 4 packed 16-bit pixels per lane
struct XDog { s2 m[5][2]; };                    // five DoG planes: columns (0,1) and (2,3) of the lane
__device__ __forceinline__ s2 as_s2(unsigned v) { return __builtin_bit_cast(s2, v); }
__device__ __forceinline__ unsigned as_u(s2 v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ s2 pmax(s2 a, s2 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ s2 pmin(s2 a, s2 b) { return __builtin_elementwise_min(a, b); }
// lane l gets v of lane l -+ 1; the end lane gets 0 (bound_ctrl): lanes 0 and 63 only carry the neighbours' columns, what they compute
// is never used, and without an 'old' value no v_mov has to precede the DPP move
__device__ __forceinline__ unsigned dpp_lower(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, true); }
__device__ __forceinline__ unsigned dpp_upper(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /* wave_shl:1 */, 0xf, 0xf, true); }

// 26-neighbour test of the centre row B (rows A above, C below): bit (layer-1)*4 + k set for an extremum at column k.
// val >= every one of its 26 neighbours  <=>  val == the maximum of the 3x3x3 block around it (the block holds val itself), and that
// maximum is separable: the 3-row column extremes of a plane, their 3-wide horizontal extremes (neighbour lanes through DPP, the
// shifted column pairs through v_alignbit), the extremes of three adjacent planes.
// |val| > 20 && ((val > 0 && val >= all) || (val < 0 && val <= all))  <=>  val == max(M27, 21) || val == min(m27, -21)  (val <= M27 always).
__device__ __forceinline__ unsigned xtest_row(const XDog& A, const XDog& B, const XDog& C, int xm, int clo, int chi, bool row_ok) {
    s2 hx[5][2], hn[5][2];                         // extremes of the 3x3 block of every plane around the lane's columns (0,1) and (2,3)
#pragma unroll
    for (int p = 0; p < 5; p++) {
        auto h3 = [](s2 c01, s2 c23, bool mx, s2& o01, s2& o23) {
            const unsigned u01 = as_u(c01), u23 = as_u(c23);
            const unsigned l23 = dpp_lower(u23), r01 = dpp_upper(u01);                    // the left lane's columns (2,3), the right lane's (0,1)
            const s2 s_m0 = as_s2(__builtin_amdgcn_alignbit(u01, l23, 16));               // columns (-1, 0)
            const s2 s_12 = as_s2(__builtin_amdgcn_alignbit(u23, u01, 16));               // columns ( 1, 2)
            const s2 s_34 = as_s2(__builtin_amdgcn_alignbit(r01, u23, 16));               // columns ( 3, 4)
            if (mx) { o01 = pmax(pmax(s_m0, c01), s_12); o23 = pmax(pmax(s_12, c23), s_34); }
            else    { o01 = pmin(pmin(s_m0, c01), s_12); o23 = pmin(pmin(s_12, c23), s_34); }
        };
        h3(pmax(pmax(A.m[p][0], B.m[p][0]), C.m[p][0]), pmax(pmax(A.m[p][1], B.m[p][1]), C.m[p][1]), true, hx[p][0], hx[p][1]);
        h3(pmin(pmin(A.m[p][0], B.m[p][0]), C.m[p][0]), pmin(pmin(A.m[p][1], B.m[p][1]), C.m[p][1]), false, hn[p][0], hn[p][1]);
    }
    unsigned hit = 0;
    const s2 t21 = {21, 21}, tm21 = {-21, -21};
#pragma unroll
    for (int layer = 1; layer <= N_LAYERS; layer++) {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const s2 val = B.m[layer][r];
            const s2 mx = pmax(pmax(pmax(hx[layer - 1][r], hx[layer][r]), hx[layer + 1][r]), t21);
            const s2 mn = pmin(pmin(pmin(hn[layer - 1][r], hn[layer][r]), hn[layer + 1][r]), tm21);
            const bool h0 = (val.x == mx.x) | (val.x == mn.x), h1 = (val.y == mx.y) | (val.y == mn.y);      // lane masks: the | is scalar
            hit = (hit << 2) | (h0 ? 2u : 0u) | (h1 ? 1u : 0u);                                             // bit 11 - ((layer-1)*4 + k)
        }
    }
    if (!row_ok || hit == 0) return 0u;
    // (rare per lane) back to bit (layer-1)*4 + k, columns outside the strip / the border masked
    unsigned out = 0;
#pragma unroll
    for (int b = 0; b < 12; b++) out |= ((hit >> (11 - b)) & 1u) << b;
    unsigned cmask = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) cmask |= (xm + k >= clo && xm + k < chi) ? (0x111u << k) : 0u;
    return out & cmask;
}

// The row loop's form of the same test, horizontal extremes first: the 3-wide extremes of a row's planes are formed ONCE, when the row enters
// the window (maximum and minimum share the neighbour lanes' columns and the shifted pairs), and the test of a centre row takes the extremes of
// its three rows.  Maxima commute, so the 3x3x3 extremes are the same numbers as xtest_row's (rows first); 105 instead of 130 instructions per
// row step for the block extremes, at 48 more registers (the kernel has them: three waves per SIMD).
struct XH { s2 hx[5][2], hn[5][2]; };           // per plane: 3-wide maxima / minima around the lane's columns (0,1) and (2,3)
struct XCen { s2 v[3][2]; };                    // the row's own values of the three tested planes
__device__ __forceinline__ void xrow_extremes(const XDog& d, XH& h, XCen& c) {
#pragma unroll
    for (int p = 0; p < 5; p++) {
        const unsigned u01 = as_u(d.m[p][0]), u23 = as_u(d.m[p][1]);
        const unsigned l23 = dpp_lower(u23), r01 = dpp_upper(u01);
        const s2 s_m0 = as_s2(__builtin_amdgcn_alignbit(u01, l23, 16));
        const s2 s_12 = as_s2(__builtin_amdgcn_alignbit(u23, u01, 16));
        const s2 s_34 = as_s2(__builtin_amdgcn_alignbit(r01, u23, 16));
        h.hx[p][0] = pmax(pmax(s_m0, d.m[p][0]), s_12); h.hx[p][1] = pmax(pmax(s_12, d.m[p][1]), s_34);
        h.hn[p][0] = pmin(pmin(s_m0, d.m[p][0]), s_12); h.hn[p][1] = pmin(pmin(s_12, d.m[p][1]), s_34);
    }
#pragma unroll
    for (int l = 0; l < 3; l++) { c.v[l][0] = d.m[l + 1][0]; c.v[l][1] = d.m[l + 1][1]; }
}
__device__ __forceinline__ unsigned xtest_rows(const XH& A, const XH& B, const XH& C, const XCen& cen, int xm, int clo, int chi, bool row_ok) {
    s2 hx[5][2], hn[5][2];
#pragma unroll
    for (int p = 0; p < 5; p++)
#pragma unroll
        for (int r = 0; r < 2; r++) { hx[p][r] = pmax(pmax(A.hx[p][r], B.hx[p][r]), C.hx[p][r]); hn[p][r] = pmin(pmin(A.hn[p][r], B.hn[p][r]), C.hn[p][r]); }
    unsigned hit = 0;
    const s2 t21 = {21, 21}, tm21 = {-21, -21};
#pragma unroll
    for (int layer = 1; layer <= N_LAYERS; layer++) {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const s2 val = cen.v[layer - 1][r];
            const s2 mx = pmax(pmax(pmax(hx[layer - 1][r], hx[layer][r]), hx[layer + 1][r]), t21);
            const s2 mn = pmin(pmin(pmin(hn[layer - 1][r], hn[layer][r]), hn[layer + 1][r]), tm21);
            const bool h0 = (val.x == mx.x) | (val.x == mn.x), h1 = (val.y == mx.y) | (val.y == mn.y);
            hit = (hit << 2) | (h0 ? 2u : 0u) | (h1 ? 1u : 0u);
        }
    }
    if (!row_ok || hit == 0) return 0u;
    unsigned out = 0;
#pragma unroll
    for (int b = 0; b < 12; b++) out |= ((hit >> (11 - b)) & 1u) << b;
    unsigned cmask = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) cmask |= (xm + k >= clo && xm + k < chi) ? (0x111u << k) : 0u;
    return out & cmask;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(XWAVES, XWAVES)))
void extrema_stream(OctaveDev oc, int octave, unsigned long long* cand, unsigned* count, unsigned cap, unsigned* overflow, BatchStride bs,
                    float* cube, unsigned cube_cap, int L, int nstrip, int nseg, int nb, int xsw /* columns per strip: multiple of 4, <= XSW */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // wave-uniform by construction; readfirstlane tells the compiler, so that rows, segments and their branches live in scalar registers
    int unit = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + wave);
    const int per = nstrip * nseg, fr = unit / per;
    if (fr >= nb) return;
    unit -= fr * per;
    {
        const size_t f = (size_t)fr;
#pragma unroll
        for (int l = 0; l < N_LEVELS; l++) oc.lv[l] += f * bs.pyr;
        cand += f * bs.cand; count += f * CCNT_STRIDE; overflow += f * CNT_STRIDE; cube += f * bs.cube;
    }
    const int seg = unit / nstrip, strip = unit - seg * nstrip;
    const int xs = strip * xsw, y0 = seg * L;       // the strip's own columns are [xs, xs + xsw)
    const int lact = (oc.h - y0 < L) ? oc.h - y0 : L;
    const unsigned reg = (unsigned)unit & (NREG - 1);
    const int xm = xs - 4 + 4 * lane;               // lane 0: the four columns left of the strip, lane 63: the four right of it
    const int xl = xm < 0 ? 0 : (xm < oc.w - 4 ? xm : oc.w - 4);
    int clo = xs > IMG_BORDER ? xs : IMG_BORDER, chi = xs + xsw < oc.w - IMG_BORDER ? xs + xsw : oc.w - IMG_BORDER;
    if (lane == 0 || lane == 63) { clo = 0; chi = 0; }
    const int hm1 = oc.h - 1;
    auto load_row = [&](int r, XRow& q) {
        r = r < 0 ? 0 : (r > hm1 ? hm1 : r);                      // clamped rows are only ever neighbours of border pixels
        const size_t o = (size_t)r * oc.w + xl;
#pragma unroll
        for (int l = 0; l < N_LEVELS; l++) q.m[l] = *reinterpret_cast<const uint2*>(oc.lv[l] + o);
    };
    auto to_dog = [&](const XRow& q, XDog& d) {     // 16-bit differences of levels in [0, 255 * 48]: no overflow
#pragma unroll
        for (int p = 0; p < 5; p++) { d.m[p][0] = as_s2(q.m[p + 1].x) - as_s2(q.m[p].x); d.m[p][1] = as_s2(q.m[p + 1].y) - as_s2(q.m[p].y); }
    };
    // Candidates are rare per lane but not per wave (a 12 MP frame has ~2 per wave-row): a hit appends its 8-byte record and its 3x3x3
    // DoG neighbourhood to a wave-private LDS list (slots from a ballot, the list length is wave-uniform and lives in a scalar); the
    // list goes to the region's candidate list and cube buffer behind one region-counter atomic per flush, in extrema_kernel's format.
    // The neighbourhood comes from LDS, not from memory: gathered with global loads at flush time (round 3), every flush stalled its
    // wave for the round trip of 36 scattered loads of rows that had long left the L2 -- a third of this kernel's time.
    // The ring: dword d of a (plane, row) holds columns 2d, 2d+1 of the wave's 256 (lane l: dwords 2l, 2l+1) and lives at
    // [d * 15 + plane * 3 + row slot], so that the 18 dwords of a neighbourhood are 9 two-dword reads off one address.  The LDS
    // operations of a wave execute in order: a row written by all lanes is readable by any of them without a barrier.
    __shared__ unsigned s_ring[4][XRING_DW];
    __shared__ unsigned long long s_rec[4][XCAP];
    __shared__ uint2 s_nb[4][XNB_CAP][XNB_DW / 2];
    static_assert(sizeof(s_ring) + sizeof(s_rec) + sizeof(s_nb) == XLDS_BYTES, "XLDS_BYTES");
    auto ring_put = [&](const XDog& d, int slot) {
        unsigned* q = &s_ring[wave][lane * 30 + slot];
#pragma unroll
        for (int p = 0; p < 5; p++) { q[p * 3] = as_u(d.m[p][0]); q[p * 3 + 15] = as_u(d.m[p][1]); }
    };
    int nq = 0;                                      // wave-uniform
    auto wave_sync = [&]() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); };
    // flush<CUBES>: the row loop's candidates leave with bit 63 set and their cube (those that found room in s_nb, and where the region's
    // cube buffer has room), the slow loop's without: refine_kernel gathers those itself
    auto flush = [&](auto cubes) {
        constexpr bool CUBES = decltype(cubes)::value;
        if (nq == 0) return;
        wave_sync();
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&count[reg * REG_STRIDE], (unsigned)nq);
        base = __shfl(base, 0);
        for (int idx = lane; idx < nq; idx += 64) {
            const unsigned g = base + (unsigned)idx;
            if (g >= cap) { *overflow = 1; continue; }
            const unsigned long long rec = s_rec[wave][idx];
            const bool has = CUBES && idx < XNB_CAP && g < cube_cap;
            cand[(size_t)reg * cap + g] = rec | (has ? (1ull << 63) : 0ull);
            if (has) {
                // the four columns of the parked dwords start at c - 1 (c even: sh = 16 drops column c - 2) or at c - 1 exactly (c odd)
                const int sh = (rec & 1ull) ? 0 : 16;
                float* cb = cube + (size_t)reg * 32 * cube_cap + g;                                     // [element][candidate]: coalesced across the lanes
#pragma nounroll                                                                                        // (rolled: 27 store addresses at once would spill the row loop's window)
                for (int i = 0; i < XNB_DW / 2; i++, cb += (size_t)3 * cube_cap) {                      // i = plane * 3 + row: elements 3i .. 3i + 2
                    const uint2 wv = s_nb[wave][idx][i];
                    const unsigned long long ww = (((unsigned long long)wv.y << 32) | wv.x) >> sh;
                    cb[0] = (float)(int)(short)(ww & 0xffffu);
                    cb[cube_cap] = (float)(int)(short)((ww >> 16) & 0xffffu);
                    cb[(size_t)2 * cube_cap] = (float)(int)(short)((ww >> 32) & 0xffffu);
                }
            }
        }
        wave_sync();
        nq = 0;
    };
    // emit<SB>: SB >= 0 is the row loop's form, SB the ring slot of the centre row: it never touches global memory (false = the list is
    // full, nothing of this row was kept); a run of rows denser than XNB_CAP / 2 candidates parks the excess as bare records, which
    // costs those candidates their cube and nothing else.  SB < 0 is the slow loop's form: no neighbourhood, and it empties the list on the spot
    auto emit = [&](unsigned hit, int rc, auto sbc) -> bool {
        constexpr int SB = decltype(sbc)::value;
        constexpr bool IN_LOOP = SB >= 0;
        const int nq0 = nq;
        while (__builtin_amdgcn_ballot_w64(hit != 0)) {
            const bool mine = hit != 0;
            const int bb = mine ? __builtin_ctz(hit) : 0;
            hit &= hit - 1;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(mine);
            const int add = __builtin_popcountll(m);
            if (nq + add > XCAP) {
                if constexpr (IN_LOOP) { nq = nq0; return false; }
                else flush(std::false_type{});
            }
            if constexpr (IN_LOOP) wave_sync();                                                         // the ring rows written by the other lanes
            if (mine) {
                const int layer = bb / 4 + 1, k = bb & 3, c = xm + k;
                const int slot = nq + __builtin_popcountll(m & ((1ull << lane) - 1ull));
                s_rec[wave][slot] = ((unsigned long long)octave << 48) | ((unsigned long long)layer << 40) | ((unsigned long long)rc << 20) | (unsigned long long)c;
                if (IN_LOOP && slot < XNB_CAP) {
                    // columns c-1 .. c+1 = 4 * lane + k - 1 .. + 1 of the wave's 256 lie in dwords d0, d0 + 1 (lanes 1 .. 62 only: 1 <= d0 <= 125)
                    const unsigned* q = &s_ring[wave][(2 * lane + ((k + 1) >> 1) - 1) * 15 + (layer - 1) * 3];
                    uint2* nbp = s_nb[wave][slot];
                    uint2 v[XNB_DW / 2];                                                                // every read before the first write: the reads stay in flight together
#pragma unroll
                    for (int pl = 0; pl < 3; pl++)
#pragma unroll
                        for (int dr = 0; dr < 3; dr++) {
                            const int o = pl * 3 + (SB + dr + 2) % 3;                                   // dr = 0: the row above the centre
                            v[pl * 3 + dr] = make_uint2(q[o], q[o + 15]);
                        }
#pragma unroll
                    for (int i = 0; i < XNB_DW / 2; i++) nbp[i] = v[i];
                }
            }
            nq += add;
        }
        return true;
    };
    // rows t-1 and t as row extremes (ring slots 0 and 1), rows t+1 .. t+XD in flight
    XH win[3];
    XCen cen[3];
    XRow nxt[XD];
    auto prime = [&](int t) {
        XRow q; XDog dq;
        load_row(y0 + t - 1, q); to_dog(q, dq); ring_put(dq, 0); xrow_extremes(dq, win[0], cen[0]);
        load_row(y0 + t, q); to_dog(q, dq); ring_put(dq, 1); xrow_extremes(dq, win[1], cen[1]);
#pragma unroll
        for (int d = 0; d < XD; d++) load_row(y0 + t + 1 + d, nxt[d]);
    };
    prime(0);
    // The row loop holds NO global memory operation besides its row loads: the candidate list is emptied between runs of the loop, never
    // inside (a store or the returning atomic of flush() anywhere in the loop body made the compiler wait for ALL outstanding loads at
    // the top of every row, the prefetched rows included: 73 -> 55 us per 12 MP frame).  A run ends when XNB_CAP / 2 candidates are
    // parked; a group of rows that would overflow the records (> XCAP - XNB_CAP / 2 extrema in 6 rows of 248 columns: noise, not
    // photographs) sends the wave into the plain loop below for the rest of its segment.
    int tb = 0, t_slow = -1;
    for (bool done = false; !done;) {
        for (;;) {
            if (tb >= lact) { done = true; break; }
            if (nq > XNB_CAP / 2) break;
            auto step = [&](auto jc) -> bool {
                constexpr int j = decltype(jc)::value;
                const int tt = tb + j;
                if (tt >= lact) return false;
                const int rc = y0 + tt;
                XH& A = win[j % 3]; XH& B = win[(j + 1) % 3]; XH& Cc = win[(j + 2) % 3];
                { XDog dq; to_dog(nxt[j % XD], dq); ring_put(dq, (j + 2) % 3); xrow_extremes(dq, Cc, cen[(j + 2) % 3]); }
                load_row(rc + 1 + XD, nxt[j % XD]);           // the bottom row of XD steps ahead, in flight meanwhile
                const unsigned hit = xtest_rows(A, B, Cc, cen[(j + 1) % 3], xm, clo, chi, rc >= IMG_BORDER && rc < oc.h - IMG_BORDER);
                if (!emit(hit, rc, std::integral_constant<int, (j + 1) % 3>{})) { t_slow = tt; return false; }
                return true;
            };
            if (!static_rows<0, 3 * XD>(step)) { done = true; break; }
            tb += 3 * XD;
        }
        flush(std::true_type{});
    }
    if (t_slow >= 0) {
        for (int tt = t_slow; tt < lact; tt++) {
            const int rc = y0 + tt;
            XRow q; XDog A, B, Cc;
            load_row(rc - 1, q); to_dog(q, A);
            load_row(rc, q); to_dog(q, B);
            load_row(rc + 1, q); to_dog(q, Cc);
            emit(xtest_row(A, B, Cc, xm, clo, chi, rc >= IMG_BORDER && rc < oc.h - IMG_BORDER), rc, std::integral_constant<int, -1>{});
        }
        flush(std::false_type{});
    }
}

constexpr unsigned KEY_BINS = 65536;         // top-k: the frame's histogram of the refined records' 16-bit response keys (select_unique_kernel)
#ifdef MI355_REFINE_STATS
// measurement build (scratch/refine_movers.py): refine_kernel runs every trajectory out and counts what the candidates do, summed over
// all frames since the last reset; the words are named in that script
__device__ unsigned long long g_refine_stats[40];
#define RSTATN(k, v) atomicAdd(&g_refine_stats[k], (unsigned long long)(v))
#define RSTAT(k) RSTATN(k, 1)
#endif
__global__ __launch_bounds__(256) void refine_kernel(PyrDev P, const unsigned long long* cand_all, const unsigned* cand_counts, unsigned cand_cap, unsigned* cand_total,
                                                     float contrast_thr, float edge_thr, float sigma,
                                                     Refined* out, unsigned* out_count, unsigned out_cap, unsigned* out_resp, BatchStride bs,
                                                     const float* cube_all, unsigned cube_cap, unsigned* khist /* top-k: KEY_BINS words per frame; keep-all: null */) {
    const size_t fr = blockIdx.z, foff = fr * bs.pyr;             // frame of the batch
    cube_all += fr * bs.cube;
    cand_all += fr * bs.cand; cand_counts += fr * CCNT_STRIDE; cand_total += fr * CNT_STRIDE;
    out += fr * bs.refined; out_count += fr * CNT_STRIDE; out_resp += fr * bs.refined;
    // blockIdx.y = region of the candidate list (extrema_kernel spreads its appends over NREG counters)
    const unsigned reg = blockIdx.y;
    unsigned n = cand_counts[reg * REG_STRIDE];
    if (n > cand_cap) n = cand_cap;
    const unsigned long long* cand = cand_all + (size_t)reg * cand_cap;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64) {      // total for the host: one region per lane
        unsigned tot = cand_counts[threadIdx.x * REG_STRIDE];
        for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
        if (threadIdx.x == 0) cand_total[0] = tot;
    }
    unsigned n_circ = 0u;                        // this lane's circling candidates dropped before their steps ran out
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned long long pk = cand[i];
        const int o = (int)((pk >> 48) & 0xff);
        int L = (int)((pk >> 40) & 0xff), R = (int)((pk >> 20) & 0xfffff), C = (int)(pk & 0xfffff);
        const unsigned start = ((unsigned)L << 28) | ((unsigned)R << 14) | (unsigned)C;      // generation order inside the octave: layer, row, column of the extremum
        const OctaveDev& oc = P.oc[o];
        auto dv = [&](int l, int r, int c) { return dogv(oc, foff, l, r, c); };
        FitOff f = {0.0f, 0.0f, 0.0f};
        int it = 0;
        bool alive = true, accepted = false;
        float contr = 0.0f;
        // Every Newton step works on the 3x3x3 DoG neighbourhood of its location held in registers: the one extrema_kernel saved next to the
        // candidate (bit 63; straight from its LDS planes; first step only), or gathered here -- three rows of four levels, the three columns
        // inside the four that start at the even column (C - 1) & ~1: twelve 8-byte loads instead of the ~50 two-byte ones the fit and the
        // acceptance tests read through dogv().  Round 4 gathered for the first step only and sent the candidates that move on (one in three)
        // through dogv() for their later steps; a mover's next location shares most of its 64-byte sectors with the last one, so gathering
        // again costs little memory and a quarter of the load instructions.  (Odd level widths: dogv() throughout.)
        const bool from_cube = (pk >> 63) != 0;
        const bool can_gather = (oc.w & 1) == 0 && (foff & 1) == 0;
        float cv[27];
        auto gather = [&](int l, int r, int c) {
            const int a0 = (c - 1) & ~1, sh = ((c - 1) & 1) * 16;
            int v[4][9];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const lvl_t* lp = oc.lv[l - 1 + q] + foff;
#pragma unroll
                for (int dr = 0; dr < 3; dr++) {
                    const uint2_a4 wv = *reinterpret_cast<const uint2_a4*>(lp + (size_t)(r - 1 + dr) * oc.w + a0);      // 4-byte aligned: a0, the row pitch and the frame offset are even
                    const unsigned long long ww = (((unsigned long long)wv.y << 32) | wv.x) >> sh;
                    v[q][dr * 3 + 0] = (int)(short)(ww & 0xffffu); v[q][dr * 3 + 1] = (int)(short)((ww >> 16) & 0xffffu); v[q][dr * 3 + 2] = (int)(short)((ww >> 32) & 0xffffu);
                }
            }
#pragma unroll
            for (int dl = 0; dl < 3; dl++)
#pragma unroll
                for (int e = 0; e < 9; e++) cv[dl * 9 + e] = (float)(v[dl + 1][e] - v[dl][e]);
        };
        // A fit step is a function of its location alone (fit_step reads the 27 DoG values around it, the same integers from the cube,
        // gather() and dogv()), and a location the candidate was fitted at before was left with "move": converged, rejected and diverged
        // all end the loop.  So a move that lands on such a location repeats from there for ever; the candidate can only run out of
        // steps and be dropped -- it is dropped at once.  The new location is compared with the last two and with the first, packed like
        // `start` (which is the first): one more register.  Of the at most four earlier locations that leaves out the second, at the last
        // test only -- a 3-cycle entered after one step runs its steps out as before (rare: profiles/refine_movers_stats.txt), as do
        // the candidates of levels too large for the packing.
        const bool track = oc.w <= 16384 && oc.h <= 16384;
        unsigned seen = 0xffffffffu;                                                  // the location before the last (all ones: layer 15, never a location)
#ifdef MI355_REFINE_STATS
        int circ_at = 0, wasted = 0;
        unsigned h1 = 0xffffffffu, h2 = 0xffffffffu, h3 = 0xffffffffu;
        bool moved = false;
        RSTAT(4);
#endif
        // the move of a step that did not converge; false: the candidate is dead (out of bounds, or back on a location of its own)
        auto move = [&]() -> bool {
            const int dC = (int)rintf(f.xc), dR = (int)rintf(f.xr), dL = (int)rintf(f.xi);
            const unsigned here = ((unsigned)L << 28) | ((unsigned)R << 14) | (unsigned)C;
            C += dC; R += dR; L += dL;
            if (L < 1 || L > N_LAYERS || C < IMG_BORDER || C >= oc.w - IMG_BORDER || R < IMG_BORDER || R >= oc.h - IMG_BORDER) return false;
            const unsigned now = ((unsigned)L << 28) | ((unsigned)R << 14) | (unsigned)C;
            const bool back = track && it + 1 < MAX_INTERP && (now == here || now == seen || now == start);      // (the last step's move ends the loop anyway)
            seen = here;
#ifdef MI355_REFINE_STATS
            moved = true;
            const bool back4 = track && it + 1 < MAX_INTERP && (now == here || now == h1 || now == h2 || now == h3);      // against all four
            h3 = h2; h2 = h1; h1 = here;
            if (back4 && !circ_at) { circ_at = it + 1; if (!back) RSTAT(32); }
            return true;                                                              // the measurement build runs every trajectory out
#else
            if (back) n_circ++;
            return !back;
#endif
        };
        if (from_cube || can_gather) {
            for (; it < MAX_INTERP; it++) {
                if (it == 0 && from_cube) {
                    const float* cb = cube_all + (size_t)reg * 32 * cube_cap + i;       // [element][candidate]: coalesced across the lanes
#pragma unroll
                    for (int e = 0; e < 27; e++) cv[e] = cb[(size_t)e * cube_cap];
                } else if (can_gather) {
#ifdef MI355_REFINE_STATS
                    RSTAT(it ? it - 1 : 31);
                    if (it) {                                                          // the move that led here, from the location it left
                        const int dL = L - (int)(seen >> 28), dR = R - (int)((seen >> 14) & 0x3fffu), dC = C - (int)(seen & 0x3fffu);
                        const int big = dL < -1 || dL > 1 || dR < -1 || dR > 1 || dC < -1 || dC > 1;
                        const int pat = big ? 4 : dC ? 3 : (dR && dL) ? 2 : dL ? 1 : dR ? 0 : 5;
                        RSTAT((circ_at ? 23 : 17) + pat);
                        if (circ_at) wasted++; else RSTATN(29, pat == 0 ? 4 : pat == 1 ? 6 : pat == 2 ? 8 : 12);
                    }
#endif
                    gather(L, R, C);
                } else break;                                                          // (a saved cube on an odd-width level: the later steps through dogv())
                const int L0 = L, R0 = R, C0 = C;
                auto dvc = [&](int l, int r, int c) { return cv[(l - L0 + 1) * 9 + (r - R0 + 1) * 3 + (c - C0 + 1)]; };
                f = fit_step(dvc, L, R, C);
                const int stt = fit_state(f);
#ifdef MI355_REFINE_STATS
                if (stt == 1) RSTAT(9);
                if (stt == 0) { RSTAT(moved ? 7 : 6); if (circ_at) RSTAT(30); }
#endif
                if (stt == 1) { alive = false; break; }
                if (stt == 0) { accepted = fit_accept(dvc, L, R, C, f, contrast_thr, edge_thr, contr); alive = accepted; break; }
                if (!move()) { alive = false; break; }
            }
#ifdef MI355_REFINE_STATS
            if (moved) RSTAT(5);
            if (it < MAX_INTERP && !accepted && alive == false && fit_state(f) == 2) { RSTAT(8); if (circ_at) RSTAT(30); }
            if (it >= MAX_INTERP) { RSTAT(10); RSTAT(circ_at ? 10 + circ_at : 15); RSTATN(16, wasted); }
#endif
            if (!alive || (can_gather && !accepted)) continue;                       // dead, rejected, or still moving after MAX_INTERP steps
        }
        if (!accepted) {
            for (; it < MAX_INTERP; it++) {
                f = fit_step(dv, L, R, C);
                const int stt = fit_state(f);
                if (stt == 0) break;
                if (stt == 1) { alive = false; break; }
                if (!move()) { alive = false; break; }
            }
            if (!alive || it >= MAX_INTERP) continue;
            if (!fit_accept(dv, L, R, C, f, contrast_thr, edge_thr, contr)) continue;
        }
        // duplicates: several start points may converge to one location, and each of them is stored (the records carry identical values
        // but for `start`: the same fit on the same 27 integers).  Top-k mode drops them where the list is short -- unique_compact_lds(), among
        // the few thousand points that are oriented at all; keep-all keeps the record of the smallest start key (below)
        // one atomic per wave, not per point: ~67 000 points of a 12 MP frame on ONE counter serialise in the L2 (0.65 ms per batch measured)
        const unsigned long long act = __ballot(1);
        const int leader = __builtin_ctzll(act), lane_id = (int)(threadIdx.x & 63);
        unsigned slot = 0;
        if (lane_id == leader) slot = atomicAdd(out_count, (unsigned)__builtin_popcountll(act));
        slot = __shfl(slot, leader) + (unsigned)__builtin_popcountll(act & ((1ull << lane_id) - 1ull));
        if (slot < out_cap) {
            Refined rr;
            rr.o = o; rr.layer = L; rr.r = R; rr.c = C; rr.xi = f.xi; rr.xr = f.xr; rr.xc = f.xc; rr.contr = contr;
            rr.scl = sigma * det_exp2f(((float)L + f.xi) / (float)N_LAYERS);
            rr.start = start;
            out[slot] = rr;
            out_resp[slot] = __float_as_uint(fabsf(contr));
            if (khist) {
                // the selection's histogram: one count per stored record.  The responses share their exponent byte, so the counts fall on a few
                // hundred words per frame: equal keys inside the wave are merged with ballots first, as topk_kernel does with its digits
                const unsigned key = (__float_as_uint(fabsf(contr)) >> 15) & 0xffffu;
                unsigned long long peers = __ballot(1);
#pragma unroll
                for (int b = 0; b < 16; b++) {
                    const unsigned long long bm = __ballot((key >> b) & 1u);
                    peers &= ((key >> b) & 1u) ? bm : ~bm;
                }
                if ((peers & ((1ull << lane_id) - 1ull)) == 0ull) atomicAdd(&khist[fr * KEY_BINS + key], (unsigned)__popcll(peers));
            }
            // keep-all (nfeatures <= 0): OpenCV's list is in generation order and of several start points that converge to one location the
            // FIRST in that order keeps it -- every start point is stored, the location remembers its smallest start key, keepall_live_kernel
            // keeps the record that holds it.  The key is entered only once the record has its slot: keepall_reset_kernel walks the STORED
            // records, so "entry below all ones <=> a stored record points at it" holds also for a frame that overflows the list
            if (P.mins[o]) atomicMin(&P.mins[o][fr * bs.mins + ((size_t)R * oc.w + C) * 4 + (size_t)L], start);
        }
    }
    // the frame's counter 6 (mi355_last_sift_counters): one atomic per wave that has something to add
    for (int off = 32; off > 0; off >>= 1) n_circ += __shfl_xor(n_circ, off);
    if ((threadIdx.x & 63) == 0 && n_circ) atomicAdd(&cand_total[6], n_circ);
}

// ---- keep-all (nfeatures <= 0, cv::SIFT's default of its own: every keypoint, in OpenCV's generation order) ------------------------------
// The reference's one committed run was made this way (tests/test_sift_reference_run.py).  No response threshold, no top-k: every refined
// point that holds its location's smallest start key is oriented, and the keypoints leave in the order (octave, start layer / row / column,
// orientation bin) -- the order of OpenCV's vector when retainBest does not run.  Not a hot path: the ranks are counted by brute force.
__global__ __launch_bounds__(256) void keepall_live_kernel(PyrDev P, const Refined* ref, const unsigned* ref_count, unsigned ref_cap, unsigned* ctrl, unsigned* list, BatchStride bs) {
    const size_t fr = blockIdx.y;
    ref += fr * bs.refined; ref_count += fr * CNT_STRIDE; ctrl += fr * CNT_STRIDE; list += fr * bs.refined;
    unsigned n = *ref_count;
    if (n > ref_cap) n = ref_cap;
    const int lane = threadIdx.x & 63;
    for (unsigned i0 = blockIdx.x * blockDim.x; i0 < n; i0 += gridDim.x * blockDim.x) {      // uniform trip count per wave
        const unsigned i = i0 + threadIdx.x;
        bool take = false;
        if (i < n) {
            const Refined rr = ref[i];
            const size_t bit = ((size_t)rr.r * P.oc[rr.o].w + rr.c) * 4 + (size_t)rr.layer;
            take = P.mins[rr.o][fr * bs.mins + bit] == rr.start;
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(take);
        if (m) {
            const int first = __builtin_ctzll(m);
            unsigned base = 0;
            if (lane == first) base = atomicAdd(&ctrl[2], (unsigned)__builtin_popcountll(m));
            base = __shfl(base, first);
            if (take) list[base + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = i;
        }
    }
}
// the start-key table is all ones between batches: the locations this batch touched are put back
__global__ __launch_bounds__(256) void keepall_reset_kernel(PyrDev P, const Refined* ref, const unsigned* ref_count, unsigned ref_cap, BatchStride bs) {
    const size_t fr = blockIdx.y;
    ref += fr * bs.refined; ref_count += fr * CNT_STRIDE;
    unsigned n = *ref_count;
    if (n > ref_cap) n = ref_cap;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const Refined rr = ref[i];
        P.mins[rr.o][fr * bs.mins + ((size_t)rr.r * P.oc[rr.o].w + rr.c) * 4 + (size_t)rr.layer] = 0xffffffffu;
    }
}

// ---------- K4: orientation ---------------------------------------------------------------------------------------
struct KpRec {
    unsigned resp_bits; int o, layer, r, c, bin;
    float ptx, pty, scl, angle, xi;
    unsigned start;                     // keep-all: the refined point's start key
};

// ---- one record per location ---------------------------------------------------------------------------------------
// refine_kernel stores a record for every start point that was accepted, and start points that converged to one (octave, layer, row,
// column) left identical records.  Each location is oriented once: the workgroup that lists the points of an orientation pass enters
// their locations into an open-addressing hash table and lists a point only if its location was not there yet.  Which of several
// identical records stays is immaterial (the total order is established by top-k).  The table: UNIQ_LDS slots of the workgroup's LDS
// for up to UNIQ_LDS / 2 points (pass 0 of a usual frame: nfeatures + margin and the ties at the threshold); beyond that, and for
// pass 1, the frame's candidate list, which is dead once refine_kernel has run -- cleared by the workgroup that uses it, as far as it
// uses it (twice the points, rounded up to a power of two), so the common path clears nothing in memory.
constexpr unsigned UNIQ_LDS = 8192;
constexpr unsigned long long UNIQ_EMPTY = ~0ull;      // no location's key: the octave field of loc_key() is below MAX_OCT
__device__ __forceinline__ unsigned long long loc_key(int o, int layer, int r, int c) {      // make_layout(): r, c < 2^20
    return ((unsigned long long)(unsigned)o << 48) | ((unsigned long long)(unsigned)layer << 44) | ((unsigned long long)(unsigned)r << 22) | (unsigned long long)(unsigned)c;
}
// true: the key entered the table with this call.  At most mask + 1 probes; a full table is reported as the frame's overflow
__device__ __forceinline__ bool uniq_insert(unsigned long long* tab, unsigned mask, unsigned long long key, int* overflow) {
    unsigned h = (unsigned)((key * 0x9e3779b97f4a7c15ull) >> 32) & mask;
    for (unsigned probe = 0; probe <= mask; probe++) {
        const unsigned long long old = atomicCAS(&tab[h], UNIQ_EMPTY, key);
        if (old == UNIQ_EMPTY) return true;
        if (old == key) return false;
        h = (h + 1u) & mask;
    }
    *overflow = 1;
    return false;
}
// a compaction step of whole waves: the lanes with `take` append `value` to dst[0 .. cap) behind *counter (a word of LDS); returns the slot
__device__ __forceinline__ unsigned wave_append(bool take, unsigned value, unsigned* dst, unsigned cap, unsigned* counter) {
    const int lane = threadIdx.x & 63;
    const unsigned long long bm = __builtin_amdgcn_ballot_w64(take);
    if (!bm) return 0xffffffffu;
    const int first = __builtin_ctzll(bm);
    unsigned base = 0;
    if (lane == first) base = atomicAdd(counter, (unsigned)__builtin_popcountll(bm));      // (LDS: a returning global atomic per wave and trip was a round trip each)
    base = __shfl(base, first) + (unsigned)__builtin_popcountll(bm & ((1ull << lane) - 1ull));
    if (take && base < cap) dst[base] = value;
    return take ? base : 0xffffffffu;
}
// One workgroup of 1024, the table in memory: list <- the indices i < n with lo <= resp[i] < hi, one per location; returns how many.
// m: an upper bound of the points in that range; g_tab: g_cap slots, a power of two >= 1024.  The location is tested inside the walk (a
// dependent load of the record in every trip that lists a point): for the rare lists that LDS does not hold, and for pass 1.
__device__ __forceinline__ unsigned unique_compact_mem(const Refined* ref, const unsigned* resp, unsigned n, unsigned lo, unsigned hi, unsigned m,
                                                       unsigned long long* g_tab, unsigned g_cap, unsigned* list, unsigned* s_cnt, int* overflow) {
    const int tid = threadIdx.x;
    unsigned size = 1024;
    while (size < 2u * m && size < g_cap) size <<= 1;
    for (unsigned i = tid; i < size; i += 1024) g_tab[i] = UNIQ_EMPTY;
    if (tid == 0) *s_cnt = 0;
    __syncthreads();
    const unsigned nr = (n + 1023u) & ~1023u;
    for (unsigned i0 = tid; i0 < nr; i0 += 8 * 1024) {
        unsigned vv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const unsigned i = i0 + 1024u * u; vv[u] = i < n ? resp[i] : 0u; }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const unsigned i = i0 + 1024u * u;
            bool take = i < n && vv[u] >= lo && vv[u] < hi;
            if (take) { const Refined& rr = ref[i]; take = uniq_insert(g_tab, size - 1u, loc_key(rr.o, rr.layer, rr.r, rr.c), overflow); }
            wave_append(take, i, list, n, s_cnt);
        }
    }
    __syncthreads();
    return *s_cnt;
}
// The same with the table in LDS (s_tab: UNIQ_LDS slots), for at most UNIQ_LDS / 2 points with response >= lo.  The walk only compacts
// their indices into s_idx (UNIQ_LDS / 2 words); the records are read from that short list -- a dependent load in ceil(m / 1024) = 3
// trips, where testing inside the walk puts one into most of a wave's ~78 (one lane in 35 is listed).
__device__ __forceinline__ unsigned unique_compact_lds(const Refined* ref, const unsigned* resp, unsigned n, unsigned lo,
                                                       unsigned long long* s_tab, unsigned* s_idx, unsigned* list, unsigned* s_cnt /* two words of LDS */, int* overflow) {
    const int tid = threadIdx.x;
    for (unsigned i = tid; i < UNIQ_LDS; i += 1024) s_tab[i] = UNIQ_EMPTY;
    if (tid == 0) { s_cnt[0] = 0; s_cnt[1] = 0; }
    __syncthreads();
    const unsigned nr = (n + 1023u) & ~1023u;
    for (unsigned i0 = tid; i0 < nr; i0 += 8 * 1024) {
        unsigned vv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const unsigned i = i0 + 1024u * u; vv[u] = i < n ? resp[i] : 0u; }      // 8 loads in flight (one at a time: a round trip per trip)
#pragma unroll
        for (int u = 0; u < 8; u++) { const unsigned i = i0 + 1024u * u; wave_append(i < n && vv[u] >= lo, i, s_idx, UNIQ_LDS / 2, &s_cnt[1]); }
    }
    __syncthreads();
    const unsigned ma = s_cnt[1] < UNIQ_LDS / 2 ? s_cnt[1] : UNIQ_LDS / 2;
    for (unsigned j0 = 0; j0 < ma; j0 += 1024) {
        const unsigned j = j0 + tid;
        bool take = j < ma;
        unsigned i = 0;
        if (take) { i = s_idx[j]; const Refined& rr = ref[i]; take = uniq_insert(s_tab, UNIQ_LDS - 1u, loc_key(rr.o, rr.layer, rr.r, rr.c), overflow); }
        wave_append(take, i, list, n, &s_cnt[0]);
    }
    __syncthreads();
    return s_cnt[0];
}

// Only the nfeatures strongest keypoints survive, and the response is known before the orientation: a threshold T such that at
// least `want` = nfeatures + margin refined records have response >= T.  Pass 0 orients those, each location once; if that turns out
// to yield fewer than nfeatures keypoints (points without any histogram peak, several records of one location among the `want`),
// top-k raises a flag and pass 1 orients the rest -- same final result as orienting everything, ~35x less work in the common case.
// T comes from the frame's histogram of the 16-bit keys (resp_bits >> 15) & 0xffff -- the exponent byte and the top eight mantissa
// bits -- which refine_kernel filled: T = lower edge of the first key, from the top, at which the count of records with a key at or
// above it reaches `want` (what two 8-bit radix passes over the responses give: tests/test_sift_select_ref.py).  One workgroup per
// frame reads the 65 536 words once, 64 consecutive keys per thread, puts them back to zero for the work area's next batch, and then
// walks the ~80 000 responses ONCE to list the points at or above T (latency, not bandwidth: 32 workgroups on the whole chip).
__global__ __launch_bounds__(1024) void select_unique_kernel(const Refined* ref, BatchStride bs,
                                                             const unsigned* resp /* |response| bits of the refined points */, const unsigned* ref_count, unsigned ref_cap,
                                                             unsigned want, unsigned* ctrl /* [0]=T bits [1]=fallback flag [2]=listed points >= T [3]=listed points < T (pass 1) */, size_t resp_stride,
                                                             unsigned* list /* indices of the points >= T, one per location: what orientation pass 0 walks */,
                                                             unsigned* khist /* KEY_BINS words per frame */, unsigned long long* g_tab, unsigned g_cap, int* overflow) {
    ref += (size_t)blockIdx.y * bs.refined; g_tab += (size_t)blockIdx.y * bs.cand; overflow += (size_t)blockIdx.y * CNT_STRIDE; khist += (size_t)blockIdx.y * KEY_BINS;
    resp += (size_t)blockIdx.y * resp_stride; ref_count += (size_t)blockIdx.y * CNT_STRIDE; ctrl += (size_t)blockIdx.y * CNT_STRIDE;
    list += (size_t)blockIdx.y * resp_stride;
    __shared__ unsigned s_idx[UNIQ_LDS / 2], s_wtot[16], s_sel[2], s_cnt[2];
    __shared__ unsigned long long s_tab[UNIQ_LDS];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    unsigned n = *ref_count;
    if (n > ref_cap) n = ref_cap;
    // thread t holds the keys 64 t .. 64 t + 63 (16 loads of 16 bytes in flight), and leaves zeros behind
    unsigned hv[64];
    {
        uint4* hp = reinterpret_cast<uint4*>(khist) + (size_t)tid * 16;
#pragma unroll
        for (int q = 0; q < 16; q++) { const uint4 v = hp[q]; hv[4 * q] = v.x; hv[4 * q + 1] = v.y; hv[4 * q + 2] = v.z; hv[4 * q + 3] = v.w; }
#pragma unroll
        for (int q = 0; q < 16; q++) hp[q] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (n <= want) {                                  // everything is oriented, each location once
        if (n <= UNIQ_LDS / 2) unique_compact_lds(ref, resp, n, 0u, s_tab, s_idx, list, s_cnt, overflow);
        else unique_compact_mem(ref, resp, n, 0u, 0xffffffffu, n, g_tab, g_cap, list, s_cnt, overflow);
        if (tid == 0) { ctrl[0] = 0; ctrl[1] = 0; ctrl[2] = s_cnt[0]; }
        return;
    }
    // records with a key at or above the lowest of this thread's: its own, those of the higher lanes of its wave, those of the higher waves
    unsigned own = 0;
#pragma unroll
    for (int b = 0; b < 64; b++) own += hv[b];
    unsigned suf = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const unsigned v = __shfl_down(suf, off); if (lane + off < 64) suf += v; }
    if (lane == 0) s_wtot[wv] = suf;
    if (tid == 0) { s_sel[0] = 0; s_sel[1] = n; }
    __syncthreads();
    for (int w = wv + 1; w < 16; w++) suf += s_wtot[w];
    // n > want records are in the histogram (one per stored record), so exactly one thread's keys take the count past `want`
    if (suf >= want && suf - own < want) {
        unsigned cum = suf - own, key = 0, m = 0;
        bool found = false;
#pragma unroll
        for (int b = 63; b >= 0; b--) {
            if (!found && cum + hv[b] >= want) { found = true; key = (unsigned)tid * 64u + (unsigned)b; m = cum + hv[b]; }
            cum += hv[b];
        }
        s_sel[0] = key << 15; s_sel[1] = m;
    }
    __syncthreads();
    // the points at or above the threshold, compacted (order free: the total order is established by top-k), so that the
    // orientation pass hands exactly one point to each wave instead of letting 4096 waves look for ~2300 among ~80 000
    const unsigned T = s_sel[0], m = s_sel[1] < n ? s_sel[1] : n;      // m: how many records lie at or above T
    if (2u * m <= UNIQ_LDS) unique_compact_lds(ref, resp, n, T, s_tab, s_idx, list, s_cnt, overflow);
    else unique_compact_mem(ref, resp, n, T, 0xffffffffu, m, g_tab, g_cap, list, s_cnt, overflow);
    if (tid == 0) { ctrl[0] = T; ctrl[1] = 0; ctrl[2] = s_cnt[0]; }
}

// ---------- gradient of a level sample (K4 orientations, K5 descriptors) ----------------------------------------------------------
// Both kernels hand one keypoint to a wave, so the level a wave samples is the same for its 64 lanes: the callers pick it with
// readfirstlane'd octave and layer, which leaves its address in scalar registers, and a lane carries the sample's byte offset in 32 bits.
// The four loads then take scalar base + vector offset, with the +-1 column in the instruction's immediate.  (Indexed with size_t per
// lane, the four addresses cost three 64-bit multiply-adds and six 64-bit shift-adds per sample.)
// Why 32 bits hold the offset: make_layout() refuses a frame with 4 w h + 1024 > 0xfffffff0, so w h < 2^30, no level has more samples
// than the frame, and a sample is 2 bytes: every byte offset inside a level is below 2^31 (the largest frame in use, 16384^2 in keep-all
// mode, reaches 2^29).  Callers pass 1 <= r <= rows - 2 and 1 <= c <= cols - 2, so r - 1 and c - 1 do not wrap below zero.
static_assert(sizeof(lvl_t) == 2, "level_taps forms byte offsets of 2-byte samples in 32 bits");
// The samples right, left, above and below (r, c) as loaded, 16 bits each: nothing is computed from them here (not even the widening to
// int), so a caller can issue the loads of one sample and consume those of another before it waits for these.
struct LevelTaps { lvl_t e, w, n, s; };
__device__ __forceinline__ LevelTaps level_taps(const lvl_t* lvl, int cols, int r, int c) {      // lvl, cols: wave-uniform
    const char* b = (const char*)lvl;
    const unsigned row = 2u * (unsigned)cols, o = 2u * ((unsigned)r * (unsigned)cols + (unsigned)c);
    LevelTaps t;
    t.e = *(const lvl_t*)(b + o + 2); t.w = *(const lvl_t*)(b + o - 2);
    t.n = *(const lvl_t*)(b + (o - row)); t.s = *(const lvl_t*)(b + (o + row));
    return t;
}
// dx = right - left, dy = above - below, as int differences of the int16 samples (exact for any sample values)
__device__ __forceinline__ void level_grad(const LevelTaps& t, float& dx, float& dy) {
    dx = (float)((int)t.e - (int)t.w); dy = (float)((int)t.n - (int)t.s);
}

constexpr int OCAP = 256;                     // emitted keypoints buffered per workgroup between flushes
__global__ __launch_bounds__(256) void orient_kernel(PyrDev P, const Refined* ref, const unsigned* ref_count, unsigned ref_cap,
                                                     KpRec* out, unsigned* out_resp, unsigned* out_count, unsigned out_cap,
                                                     const unsigned* ctrl, int pass, BatchStride bs, const unsigned* list) {
    const size_t fr = blockIdx.y, foff = fr * bs.pyr;             // frame of the batch
    ref += fr * bs.refined; ref_count += fr * CNT_STRIDE; out += fr * bs.kps; out_resp += fr * bs.kps; out_count += fr * CNT_STRIDE; ctrl += fr * CNT_STRIDE;
    list += fr * bs.refined;
    __shared__ unsigned long long s_hq[4][ORI_BINS];
    const unsigned Tbits = ctrl[0];
    if (pass == 1 && (ctrl[1] == 0 || Tbits == 0)) return;      // fallback pass not needed
    __shared__ float s_hist[4][ORI_BINS + 4];
    __shared__ KpRec s_out[OCAP];             // one global atomic per flush instead of one per keypoint
    __shared__ unsigned s_on, s_obase;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned n = *ref_count;
    if (n > ref_cap) n = ref_cap;
    // either pass walks a compacted list with one point per location: pass 0 the points >= T (select_unique_kernel), pass 1 those below
    // (listed by the top-k workgroup that asked for the pass); keep-all: the live records (keepall_live_kernel)
    { const unsigned nl = ctrl[pass == 0 ? 2 : 3]; n = nl < n ? nl : n; }
    if (tid == 0) s_on = 0;
    __syncthreads();
    for (unsigned base = blockIdx.x * 4; base < n; base += gridDim.x * 4) {        // uniform trip count per workgroup
        unsigned k = base + wv;
        const bool take = k < n;
        if (take) {
            k = list[k];
            const Refined rr = ref[k];
            const OctaveDev& oc = P.oc[__builtin_amdgcn_readfirstlane(rr.o)];                     // one keypoint per wave: scalar level, width and height
            const lvl_t* img = oc.lv[__builtin_amdgcn_readfirstlane(rr.layer)] + foff;
            const int radius = (int)rintf(4.5f * rr.scl);
            const float osig = 1.5f * rr.scl;
            const float expf_scale = -1.0f / (2.0f * osig * osig);
            const int side = 2 * radius + 1, S = side * side;
            if (lane < ORI_BINS) s_hq[wv][lane] = 0ull;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
            // 4 samples per lane per trip: the 16 gradient loads of a trip are issued before any is consumed
            // lane l takes the samples [l * per, (l + 1) * per) in turn: one division per lane, then a running row / column
            const int per = (S + 63) / 64;
            int sc = lane * per, ic = sc / side, jc = sc - ic * side;
            for (int k0 = 0; k0 < per; k0 += 4) {
                LevelTaps tv[4]; int d2v[4]; bool okv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int s = k0 + u < per ? sc : S;
                    const int i = ic - radius, j = jc - radius;
                    sc++; jc++;
                    if (jc == side) { jc = 0; ic++; }
                    const int y = rr.r + i, x = rr.c + j;
                    okv[u] = (s < S) && !(y <= 0 || y >= oc.h - 1 || x <= 0 || x >= oc.w - 1);
                    d2v[u] = i * i + j * j;
                    tv[u] = LevelTaps{0, 0, 0, 0};
                    if (okv[u]) tv[u] = level_taps(img, oc.w, y, x);
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (!okv[u]) continue;
                    float dx, dy;
                    level_grad(tv[u], dx, dy);
                    const float wgt = det_expf((float)d2v[u] * expf_scale);
                    const float ang = det_atan2deg(dy, dx);
                    const float mag = sqrtf(dx * dx + dy * dy);
                    int b = (int)rintf(((float)ORI_BINS / 360.0f) * ang);
                    if (b >= ORI_BINS) b -= ORI_BINS;
                    if (b < 0) b += ORI_BINS;
                    const float t = wgt * mag;
                    // order-free by definition; 0 <= t <= sqrt(2) x 255 x 48 (a weight times a square root): 32 bits hold t x 2^10 and the
                    // 64-bit addend's high word is zero, not a sign extension
                    atomicAdd(&s_hq[wv][b], (unsigned long long)(unsigned)(int)rintf(t * HIST_Q));
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
            if (lane < ORI_BINS) s_hist[wv][lane] = (float)(long long)s_hq[wv][lane] * (1.0f / HIST_Q);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
            float hs = 0.0f;
            if (lane < ORI_BINS) {
                const float m2 = s_hist[wv][(lane + ORI_BINS - 2) % ORI_BINS], m1 = s_hist[wv][(lane + ORI_BINS - 1) % ORI_BINS];
                const float p1 = s_hist[wv][(lane + 1) % ORI_BINS], p2 = s_hist[wv][(lane + 2) % ORI_BINS];
                hs = ((m2 + p2) * (1.0f / 16.0f) + (m1 + p1) * (4.0f / 16.0f)) + s_hist[wv][lane] * (6.0f / 16.0f);
            }
            float omax = hs;                                            // max over lanes (order independent)
            for (int off = 32; off > 0; off >>= 1) { const float o2 = __shfl_xor(omax, off); omax = o2 > omax ? o2 : omax; }
            const float hl = __shfl(hs, lane > 0 ? lane - 1 : ORI_BINS - 1);
            const float hr = __shfl(hs, lane < ORI_BINS - 1 ? lane + 1 : 0);
            const float mag_thr = omax * 0.8f;
            if (lane < ORI_BINS && hs > hl && hs > hr && hs >= mag_thr) {
                float bf = (float)lane + (0.5f * (hl - hr)) / ((hl - 2.0f * hs) + hr);
                bf = bf < 0.0f ? (float)ORI_BINS + bf : (bf >= (float)ORI_BINS ? bf - (float)ORI_BINS : bf);
                KpRec kr;
                kr.resp_bits = __float_as_uint(fabsf(rr.contr));
                kr.o = rr.o; kr.layer = rr.layer; kr.r = rr.r; kr.c = rr.c; kr.bin = lane;
                kr.ptx = (float)rr.c + rr.xc; kr.pty = (float)rr.r + rr.xr; kr.scl = rr.scl; kr.xi = rr.xi; kr.start = rr.start;
                kr.angle = (360.0f / (float)ORI_BINS) * bf;
                const unsigned slot = atomicAdd(&s_on, 1u);            // LDS counter; <= 18 peaks x 4 waves per trip
                if (slot < OCAP) s_out[slot] = kr;
            }
        }
        __syncthreads();
        // flush when the next trip (<= 4 x 18 peaks) might not fit, and after the last trip
        const bool last = base + gridDim.x * 4 >= n;
        if (s_on > OCAP - 72 || last) {
            const unsigned cntl = s_on < OCAP ? s_on : OCAP;
            if (tid == 0 && cntl) s_obase = atomicAdd(out_count, cntl);
            __syncthreads();
            for (unsigned i = tid; i < cntl; i += 256) {
                const unsigned g = s_obase + i;
                if (g < out_cap) { out[g] = s_out[i]; out_resp[g] = s_out[i].resp_bits; }
            }
            __syncthreads();
            if (tid == 0) s_on = 0;
            __syncthreads();
        }
    }
}

// ---------- K4b: strongest nfeatures in the total order -------------------------------------------------------------
constexpr int TOPK_CAP = 4096;      // survivors handed to the sort (nfeatures + ties)

struct SelRec { float ptx, pty, scl, angle; int o, layer; };

__device__ __forceinline__ unsigned long long tie_key(const KpRec& k) {
    return ((unsigned long long)k.o << 52) | ((unsigned long long)k.layer << 48) | ((unsigned long long)k.r << 28) | ((unsigned long long)k.c << 8) | (unsigned long long)k.bin;
}

__global__ __launch_bounds__(1024) void topk_kernel(const KpRec* kps, const unsigned* resp, const unsigned* kp_count, unsigned kp_cap, int nfeatures,
                                                    FrameOuts outs, SelRec* out_sel, int* out_n, int* overflow, unsigned* ctrl, int pass, BatchStride bs,
                                                    const Refined* ref, const unsigned* ref_resp, const unsigned* ref_count, unsigned ref_cap,      // pass 0: what a fallback pass lists from
                                                    unsigned* list, unsigned long long* g_tab, unsigned g_cap, int* fell_back) {
    const size_t fr = blockIdx.x;                                 // one workgroup per frame of the batch
    ref += fr * bs.refined; ref_resp += fr * bs.refined; ref_count += fr * CNT_STRIDE; list += fr * bs.refined; g_tab += fr * bs.cand; fell_back += fr * CNT_STRIDE;
    kps += fr * bs.kps; resp += fr * bs.kps; kp_count += fr * CNT_STRIDE; out_sel += fr * bs.sel; out_n += fr * CNT_STRIDE; overflow += fr * CNT_STRIDE; ctrl += fr * CNT_STRIDE;
    mi355_keypoint* out_kp = outs.kp[0];
#pragma unroll
    for (int q = 1; q < SIFT_BATCH_MAX; q++) if ((int)fr == q) out_kp = outs.kp[q];
    __shared__ unsigned s_hist[256];
    if (pass == 1 && (ctrl[1] == 0 || ctrl[0] == 0)) return;     // fallback pass not needed
    __shared__ unsigned s_misc[8];
    __shared__ unsigned long long s_k0[TOPK_CAP];      // ~resp_bits (descending response first)
    __shared__ unsigned long long s_k1[TOPK_CAP];      // tie key
    __shared__ unsigned s_idx[TOPK_CAP];
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned N = *kp_count;
    if (N > kp_cap) { N = kp_cap; if (tid == 0) *overflow = 1; }
    const unsigned K = (unsigned)nfeatures;
    unsigned thresh = 0;                                // select everything with resp_bits >= thresh
    if (N > K) {
        // radix select of the K-th largest resp_bits, MSB first; equal digits inside a wave are merged with
        // ballots before touching the LDS histogram (responses share their exponent byte: one hot bin)
        unsigned prefix = 0, want = K;
        const unsigned Nr = (N + 1023u) & ~1023u;
        for (int pass = 0; pass < 4; pass++) {
            const int shift = 24 - 8 * pass;
            for (int i = tid; i < 256; i += 1024) s_hist[i] = 0;
            __syncthreads();
            const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
            for (unsigned i0 = tid; i0 < Nr; i0 += 8 * 1024) {
                unsigned vv[8];
#pragma unroll
                for (int u = 0; u < 8; u++) { const unsigned i = i0 + 1024u * u; vv[u] = i < N ? resp[i] : 0u; }      // 8 loads in flight
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const unsigned i = i0 + 1024u * u;
                    if (i0 + 1024u * u - tid >= Nr) break;                     // wave-uniform
                    const unsigned v = vv[u];
                    const bool valid = (i < N) && ((v & himask) == prefix);
                    const unsigned d = (v >> shift) & 255u;
                    unsigned long long peers = __ballot(valid);
#pragma unroll
                    for (int b = 0; b < 8; b++) {
                        const unsigned long long m = __ballot(valid && ((d >> b) & 1u));
                        peers &= ((d >> b) & 1u) ? m : ~m;
                    }
                    if (valid && (peers & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&s_hist[d], (unsigned)__popcll(peers));
                }
            }
            __syncthreads();
            if (tid == 0) {
                unsigned cum = 0; int b = 255;
                for (; b >= 0; b--) { if (cum + s_hist[b] >= want) break; cum += s_hist[b]; }
                if (b < 0) b = 0;
                s_misc[0] = (unsigned)b; s_misc[1] = want - cum;
            }
            __syncthreads();
            prefix |= s_misc[0] << shift; want = s_misc[1];
            __syncthreads();
        }
        thresh = prefix;
    }
    if (tid == 0) s_misc[2] = 0;
    for (int i = tid; i < TOPK_CAP; i += 1024) { s_k0[i] = ~0ull; s_k1[i] = ~0ull; s_idx[i] = 0xffffffffu; }
    __syncthreads();
    for (unsigned i0 = tid; i0 < N; i0 += 8 * 1024) {
        unsigned vv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const unsigned i = i0 + 1024u * u; vv[u] = i < N ? resp[i] : 0u; }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const unsigned i = i0 + 1024u * u;
            if (i < N && vv[u] >= thresh) {
                const KpRec k = kps[i];
                const unsigned slot = atomicAdd(&s_misc[2], 1u);
                if (slot < TOPK_CAP) { s_k0[slot] = (unsigned long long)(~k.resp_bits); s_k1[slot] = tie_key(k); s_idx[slot] = i; }
            }
        }
    }
    __syncthreads();
    unsigned M = s_misc[2];
    if (M > TOPK_CAP) { M = TOPK_CAP; if (tid == 0) *overflow = 1; }
    // retainBest keeps every keypoint tied with the nfeatures-th response; the feature record holds SEL_STRIDE: more than that (nfeatures
    // close to 2048 and a tie at the boundary) is reported as an overflow rather than cut off silently
    if (N > K && M > (unsigned)SEL_STRIDE && tid == 0) *overflow = 1;
    // bitonic sort by (k0, k1) of the smallest power of two >= M (padding keys are all-ones and stay last)
    int SN = 64;
    while ((unsigned)SN < M) SN <<= 1;
    for (int k = 2; k <= SN; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < SN; i += 1024) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a0 = s_k0[i], a1 = s_k1[i], b0 = s_k0[ixj], b1 = s_k1[ixj];
                    const bool gt = (a0 > b0) || (a0 == b0 && a1 > b1);
                    const bool up = (i & k) == 0;
                    if (gt == up) {
                        s_k0[i] = b0; s_k1[i] = b1; s_k0[ixj] = a0; s_k1[ixj] = a1;
                        const unsigned t = s_idx[i]; s_idx[i] = s_idx[ixj]; s_idx[ixj] = t;
                    }
                }
            }
            __syncthreads();
        }
    }
    // KeyPointsFilter::retainBest keeps everything whose response is >= the K-th strongest: the M survivors of the threshold are exactly
    // those (ties with the K-th included), up to the feature record's capacity
    const unsigned keep = N > K ? (M < (unsigned)SEL_STRIDE ? M : (unsigned)SEL_STRIDE) : M;
    for (unsigned i = tid; i < keep; i += 1024) {
        const KpRec k = kps[s_idx[i]];
        // image coordinates: kpt.pt = (c + xc) * (1 << octave), kpt.size = sigma * 2^((layer + xi) / 3) * (1 << octave) * 2 (no doubled octave)
        const float s2 = (float)(1 << k.o);
        mi355_keypoint kp;
        kp.x = k.ptx * s2; kp.y = k.pty * s2; kp.size = (k.scl * s2) * 2.0f; kp.angle = k.angle;
        kp.response = __uint_as_float(k.resp_bits);
        kp.octave = (k.o & 255) | (k.layer << 8) | (((int)rintf((k.xi + 0.5f) * 255.0f)) << 16);
        kp.class_id = -1;
        out_kp[i] = kp;
        SelRec sr; sr.ptx = k.ptx; sr.pty = k.pty; sr.scl = k.scl; sr.angle = k.angle; sr.o = k.o; sr.layer = k.layer;
        out_sel[i] = sr;
    }
    // pass 0 oriented only the refined points with response >= T: fewer than nfeatures keypoints came out while
    // weaker refined points exist -> orient those too (pass 1) and select again
    const unsigned Tbits = ctrl[0];
    const bool fall = pass == 0 && Tbits != 0 && keep < K;        // uniform over the workgroup
    if (tid == 0) {
        *out_n = (int)keep;
        if (fall) { ctrl[1] = 1; *fell_back = 1; }
    }
    if (fall) {
        // rare, and may be slow: the points below T, each location once (records of one location share their response, so all of them lie
        // on one side of T), through a table in the frame's dead candidate list that this workgroup clears for itself
        unsigned nr = *ref_count;
        if (nr > ref_cap) nr = ref_cap;
        __syncthreads();                                          // s_misc[2] (M) has been read by everyone
        const unsigned cnt = unique_compact_mem(ref, ref_resp, nr, 0u, Tbits, nr, g_tab, g_cap, list, &s_misc[2], overflow);
        if (tid == 0) ctrl[3] = cnt;
    }
}

// keep-all: a keypoint's place in the output = the number of keypoints with a smaller (octave, start key, orientation bin); the keys are
// distinct (one refined record per start point, one keypoint per bin).  The octave takes 4 bits (MAX_OCT = 16), the start key 30, the bin 6:
// a key is below 2^44, and key << 18 | index (index < MI355_SIFT_KEEPALL_LIMIT = 2^18) still orders by the key alone.
__device__ __forceinline__ unsigned long long keepall_key(const KpRec& k) {
    return ((unsigned long long)k.o << 40) | ((unsigned long long)k.start << 6) | (unsigned long long)k.bin;
}

__device__ __forceinline__ void keepall_emit(const KpRec& k, mi355_keypoint* out_kp, SelRec* out_sel, unsigned pos) {
    const float s2 = (float)(1 << k.o);
    mi355_keypoint kp;
    kp.x = k.ptx * s2; kp.y = k.pty * s2; kp.size = (k.scl * s2) * 2.0f; kp.angle = k.angle;
    kp.response = __uint_as_float(k.resp_bits);
    kp.octave = (k.o & 255) | (k.layer << 8) | (((int)rintf((k.xi + 0.5f) * 255.0f)) << 16);
    kp.class_id = -1;
    out_kp[pos] = kp;
    SelRec sr; sr.ptx = k.ptx; sr.pty = k.pty; sr.scl = k.scl; sr.angle = k.angle; sr.o = k.o; sr.layer = k.layer;
    out_sel[pos] = sr;
}

// The frame's counters: more keypoints than the work area holds is an overflow (cnt[4]); more than the ctx's ceiling (option "keepall_max")
// fails the frame without one -- the host reads that from the keypoint count, cnt[2].  Either way nothing is written and n_sel = 0.
__device__ __forceinline__ bool keepall_fits(unsigned N, unsigned kp_cap, unsigned kmax, int* out_n, int* overflow, bool writer) {
    if (N <= kp_cap && N <= kmax) return true;
    if (writer) { if (N > kp_cap) *overflow = 1; *out_n = 0; }
    return false;
}

// The rank in O(N log N), two launches.  Phase A (keepall_sort_tiles_kernel): every workgroup sorts a tile of KA_TILE keys (key << 18 | index)
// in LDS, bitonic, and writes it to the frame's scratch area padded with all-ones.  A frame of one tile is done there: the sorted position is
// the output position.  Phase B (keepall_place_kernel, frames of more than one tile): a keypoint's position = the sum over the tiles of the
// number of keys there below its own (lower_bound, 13 probes of a KA_TILE-sized tile; in its own tile that is its place in the tile).

__global__ __launch_bounds__(1024) void keepall_sort_tiles_kernel(const KpRec* kps, const unsigned* kp_count, unsigned kp_cap, unsigned kmax, unsigned long long* sorted,
                                                                  size_t sorted_stride, FrameOuts outs, SelRec* out_sel, BatchStride bs) {
    const size_t fr = blockIdx.y;
    kps += fr * bs.kps; kp_count += fr * CNT_STRIDE; sorted += fr * sorted_stride; out_sel += fr * bs.sel;
    const unsigned N = *kp_count;
    if (N > kp_cap || N > kmax) return;                                 // keepall_place_kernel reports it
    const unsigned t0 = blockIdx.x * KA_TILE;
    if (t0 >= N) return;
    __shared__ unsigned long long s[KA_TILE];
    const int tid = threadIdx.x;
    for (int q = tid; q < KA_TILE; q += 1024) s[q] = t0 + q < N ? (keepall_key(kps[t0 + q]) << 18) | (unsigned long long)(t0 + q) : ~0ull;
    __syncthreads();
    // wave w owns the pairs [128 w, 128 w + 128): while j <= 128 they stay inside its block of 256 keys and the wave only syncs with itself;
    // a workgroup barrier stands after every step with j >= 256 and before the first one (63 of the 78 steps take none)
    const int lane = tid & 63, p0 = (tid >> 6) * 128 + lane;
    for (int k = 2; k <= KA_TILE; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int h = 0; h < 2; h++) {                                  // compare-exchange pair p: (i, i + j), i with bit j clear
                const int p = p0 + 64 * h, i = 2 * p - (p & (j - 1)), ixj = i + j;
                const unsigned long long a = s[i], b = s[ixj];
                if ((a > b) == ((i & k) == 0)) { s[i] = b; s[ixj] = a; }
            }
            if (j >= 256 || (j == 1 && k >= 256)) __syncthreads();
            else { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }
        }
    }
    if (N <= (unsigned)KA_TILE) {
        mi355_keypoint* out_kp = outs.kp[0];
#pragma unroll
        for (int q = 1; q < SIFT_BATCH_MAX; q++) if ((int)fr == q) out_kp = outs.kp[q];
        for (unsigned q = tid; q < N; q += 1024) keepall_emit(kps[(unsigned)(s[q] & 0x3ffffu)], out_kp, out_sel, q);
        return;
    }
    for (int q = tid; q < KA_TILE; q += 1024) sorted[t0 + q] = s[q];
}

__global__ __launch_bounds__(256) void keepall_place_kernel(const KpRec* kps, const unsigned* kp_count, unsigned kp_cap, unsigned kmax, const unsigned long long* sorted,
                                                            size_t sorted_stride, FrameOuts outs, SelRec* out_sel, int* out_n, int* overflow, BatchStride bs) {
    const size_t fr = blockIdx.y;
    kps += fr * bs.kps; kp_count += fr * CNT_STRIDE; sorted += fr * sorted_stride; out_sel += fr * bs.sel; out_n += fr * CNT_STRIDE; overflow += fr * CNT_STRIDE;
    const unsigned N = *kp_count;
    if (!keepall_fits(N, kp_cap, kmax, out_n, overflow, blockIdx.x == 0 && threadIdx.x == 0)) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) *out_n = (int)N;
    if (N <= (unsigned)KA_TILE) return;                                 // one tile: keepall_sort_tiles_kernel wrote it
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    mi355_keypoint* out_kp = outs.kp[0];
#pragma unroll
    for (int q = 1; q < SIFT_BATCH_MAX; q++) if ((int)fr == q) out_kp = outs.kp[q];
    const KpRec k = kps[i];
    const unsigned long long key = keepall_key(k) << 18;                // below every composite of this key: lower_bound counts smaller keys only
    const unsigned nt = (N + KA_TILE - 1) / KA_TILE;
    unsigned rank = 0, t = 0;
    for (; t + 4 <= nt; t += 4) {                                       // four independent searches in flight
        unsigned pos[4] = {0u, 0u, 0u, 0u};
        const unsigned long long* a = sorted + (size_t)t * KA_TILE;
        for (unsigned step = KA_TILE / 2; step > 0; step >>= 1) {
#pragma unroll
            for (int u = 0; u < 4; u++) if (a[(size_t)u * KA_TILE + pos[u] + step - 1] < key) pos[u] += step;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) rank += pos[u] + (a[(size_t)u * KA_TILE + pos[u]] < key ? 1u : 0u);
    }
    for (; t < nt; t++) {
        const unsigned long long* a = sorted + (size_t)t * KA_TILE;
        unsigned pos = 0;
        for (unsigned step = KA_TILE / 2; step > 0; step >>= 1) if (a[pos + step - 1] < key) pos += step;
        rank += pos + (a[pos] < key ? 1u : 0u);
    }
    keepall_emit(k, out_kp, out_sel, rank);
}

// ---------- K5: descriptors -----------------------------------------------------------------------------------------
// One WAVE per keypoint, four keypoints per workgroup (16 frames x 2000 keypoints as 256-thread workgroups of their own were
// dispatch- and latency-bound: each lane looped over ~20 samples with four dependent 2-byte loads each).  A lane tests four
// samples of the window per round; the samples that pass are queued and consumed 64 at a time, and the four gradient loads of a
// trip are issued one trip ahead of their use (below); the histogram lives in wave-private LDS.
__global__ __launch_bounds__(256) void describe_kernel(PyrDev P, const SelRec* sel, const int* n_sel, FrameOuts outs, BatchStride bs) {
    const size_t fr = blockIdx.y, foff = fr * bs.pyr;             // frame of the batch
    sel += fr * bs.sel; n_sel += fr * CNT_STRIDE;
    uint8_t* desc = outs.d8[0];
#pragma unroll
    for (int q = 1; q < SIFT_BATCH_MAX; q++) if ((int)fr == q) desc = outs.d8[q];
    constexpr int d = 4, n = 8, HB = (d + 2) * (d + 2) * (n + 2);
    __shared__ unsigned long long s_hq4[4][HB];
    __shared__ float s_dst4[4][128];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int kidx = blockIdx.x * 4 + wv;
    if (kidx >= *n_sel) return;
    unsigned long long* s_hq = s_hq4[wv];
    float* s_dst = s_dst4[wv];
    auto wave_sync = [&]() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); };
    const SelRec k = sel[kidx];
    const OctaveDev& oc = P.oc[__builtin_amdgcn_readfirstlane(k.o)];                          // one keypoint per wave: scalar level, width and height
    const lvl_t* img = oc.lv[__builtin_amdgcn_readfirstlane(k.layer)] + foff;
    const int rows = oc.h, cols = oc.w;
    for (int i = lane; i < HB; i += 64) s_hq[i] = 0ull;
    wave_sync();
    const int px = (int)rintf(k.ptx), py = (int)rintf(k.pty);
    float sin_t, cos_t;
    det_sincosdeg(k.angle, sin_t, cos_t);
    const float bins_per_deg = (float)n / 360.0f;
    const float exp_scale = -1.0f / ((float)(d * d) * 0.5f);
    const float hist_width = 3.0f * k.scl;
    const int radius = (int)rintf(hist_width * 1.4142135623730951f * (float)(d + 1) * 0.5f);
    cos_t = cos_t / hist_width; sin_t = sin_t / hist_width;
    const int side = 2 * radius + 1, S = side * side;
    // Only about half of the window's samples fall inside the rotated 4 x 4 grid.  The cheap part -- the sample's grid coordinates and the
    // test -- runs for all of them; the samples that pass are queued (window row, column packed into one word) in a wave-private LDS list
    // and the expensive part (four loads, atan2, exp, eight fixed-point atomics) runs on full waves of queued samples: 34 -> 24 us per
    // 12 MP frame.  The sums are order-free, so the order of the queue does not matter.
    __shared__ int s_q4[4][64 * 5];
    int* s_q = s_q4[wv];
    int qn = 0;                                       // wave-uniform
    // One full trip of 64 queued samples stays pending: its list word and its four samples, loaded and not yet consumed.  It is accumulated
    // when the next full trip's loads have been issued (possibly after further rounds of the cheap test, which hide its latency as well) or
    // in the tail, so no trip waits for its own loads with nothing else to do.
    bool pending = false;                             // wave-uniform
    int p_word = 0;
    LevelTaps p_taps = {0, 0, 0, 0};
    // The expensive part in two halves, so that a trip's four loads are in flight while the trip before it is accumulated: fetch() issues
    // the loads of a queued sample, heavy() consumes them.
    auto fetch = [&](int packed) {
        const int i = (int)((unsigned)packed >> 16) - 32768, j = (int)((unsigned)packed & 0xffffu) - 32768;
        return level_taps(img, cols, py + i, px + j);
    };
    auto heavy = [&](int packed, const LevelTaps& taps) {
        const int i = (int)((unsigned)packed >> 16) - 32768, j = (int)((unsigned)packed & 0xffffu) - 32768;
        const float c_rot = (float)j * cos_t - (float)i * sin_t;
        const float r_rot = (float)j * sin_t + (float)i * cos_t;
        float rbin = r_rot + (float)(d / 2) - 0.5f;
        float cbin = c_rot + (float)(d / 2) - 0.5f;
        float dx, dy;
        level_grad(taps, dx, dy);
        const float ori = det_atan2deg(dy, dx);
        const float mag = sqrtf(dx * dx + dy * dy) * det_expf((c_rot * c_rot + r_rot * r_rot) * exp_scale);
        float obin = (ori - k.angle) * bins_per_deg;
        const float r0f = floorf(rbin), c0f = floorf(cbin), o0f = floorf(obin);
        rbin -= r0f; cbin -= c0f; obin -= o0f;
        const int r0 = (int)r0f, c0 = (int)c0f;
        int o0 = (int)o0f;
        if (o0 < 0) o0 += n;
        if (o0 >= n) o0 -= n;
        const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
        const float v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11;
        const float v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
        const float v_rco111 = v_rc11 * obin, v_rco110 = v_rc11 - v_rco111;
        const float v_rco101 = v_rc10 * obin, v_rco100 = v_rc10 - v_rco101;
        const float v_rco011 = v_rc01 * obin, v_rco010 = v_rc01 - v_rco011;
        const float v_rco001 = v_rc00 * obin, v_rco000 = v_rc00 - v_rco001;
        const int idx = ((r0 + 1) * (d + 2) + c0 + 1) * (n + 2) + o0;
        // order-free accumulation: rint(v * 2^10) as 64-bit integers.  v <= sqrt(2) x 255 x 48, so v x 2^10 fits 32 bits (one
        // v_cvt_i32_f32 instead of the 64-bit conversion sequence).  And v >= 0, so the addend's high word is zero and not a sign extension:
        // mag is a square root times det_expf (a positive polynomial times a power of two, or 0); rbin, cbin and obin are x - floor(x), in
        // [0, 1]; a product of a >= 0 and a factor in [0, 1] rounds to at most a (a is itself a float and rounding is monotone), so each
        // v_*1 lies in [0, a] and each v_*0 = a - v_*1 is >= 0.
#define FIXQ(v) ((unsigned long long)(unsigned)(int)rintf((v) * HIST_Q))
        atomicAdd(&s_hq[idx], FIXQ(v_rco000)); atomicAdd(&s_hq[idx + 1], FIXQ(v_rco001));
        atomicAdd(&s_hq[idx + (n + 2)], FIXQ(v_rco010)); atomicAdd(&s_hq[idx + (n + 3)], FIXQ(v_rco011));
        atomicAdd(&s_hq[idx + (d + 2) * (n + 2)], FIXQ(v_rco100)); atomicAdd(&s_hq[idx + (d + 2) * (n + 2) + 1], FIXQ(v_rco101));
        atomicAdd(&s_hq[idx + (d + 3) * (n + 2)], FIXQ(v_rco110)); atomicAdd(&s_hq[idx + (d + 3) * (n + 2) + 1], FIXQ(v_rco111));
#undef FIXQ
    };
    // lane l tests the samples [l * per, (l + 1) * per) in turn (one division per lane, then running row / column)
    const int per = (S + 63) / 64;
    int sc = lane * per, ic = sc / side, jc = sc - ic * side;
    for (int k0 = 0; k0 < per; k0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int kk = k0 + u;
            const int i = ic - radius, j = jc - radius;
            const float c_rot = (float)j * cos_t - (float)i * sin_t;
            const float r_rot = (float)j * sin_t + (float)i * cos_t;
            const float rbin = r_rot + (float)(d / 2) - 0.5f;
            const float cbin = c_rot + (float)(d / 2) - 0.5f;
            const int r = py + i, c = px + j;
            const bool ok = kk < per && sc < S && (rbin > -1.0f && rbin < (float)d && cbin > -1.0f && cbin < (float)d && r > 0 && r < rows - 1 && c > 0 && c < cols - 1);
            const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
            if (ok) s_q[qn + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = (int)(((unsigned)(i + 32768) << 16) | (unsigned)(j + 32768));
            qn += __builtin_popcountll(m);
            sc++; jc++;
            if (jc == side) { jc = 0; ic++; }
        }
        wave_sync();
        while (qn >= 64) {
            qn -= 64;
            const int word = s_q[qn + lane];
            const LevelTaps taps = fetch(word);
            if (pending) heavy(p_word, p_taps);
            p_word = word; p_taps = taps; pending = true;
        }
        wave_sync();
    }
    const bool tail = lane < qn;
    int t_word = 0;
    LevelTaps t_taps = {0, 0, 0, 0};
    if (tail) { t_word = s_q[lane]; t_taps = fetch(t_word); }
    if (pending) heavy(p_word, p_taps);
    if (tail) heavy(t_word, t_taps);
    wave_sync();
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int t = lane + 64 * half;
        const int cell = t >> 3, q = t & 7, i = cell >> 2, j = cell & 3;
        const int idx = ((i + 1) * (d + 2) + (j + 1)) * (n + 2);
        float v = (float)(long long)s_hq[idx + q] * (1.0f / HIST_Q);
        if (q < 2) v = v + (float)(long long)s_hq[idx + n + q] * (1.0f / HIST_Q);       // circular orientation wrap
        s_dst[t] = v;
    }
    wave_sync();
    // sequential norms: the accumulation order is part of the definition.  The squares are formed by the 64 lanes, the
    // running sum visits them in index order through lane broadcasts
    float a = s_dst[lane], b = s_dst[lane + 64];
    auto seq_sum = [&](float va, float vb) {
        const float sa = va * va, sb = vb * vb;
        float acc = 0.0f;
#pragma unroll
        for (int q = 0; q < 64; q++) acc = acc + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sa), q));
#pragma unroll
        for (int q = 0; q < 64; q++) acc = acc + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sb), q));
        return acc;
    };
    const float thr = sqrtf(seq_sum(a, b)) * 0.2f;
    a = a < thr ? a : thr; b = b < thr ? b : thr;
    const float nn = sqrtf(seq_sum(a, b));
    const float fac = 512.0f / (nn > 1.1920929e-7f ? nn : 1.1920929e-7f);
    const float va = rintf(a * fac), vb = rintf(b * fac);
    desc[(size_t)kidx * 128 + lane] = (uint8_t)(va < 0.0f ? 0 : (va > 255.0f ? 255 : (int)va));
    desc[(size_t)kidx * 128 + lane + 64] = (uint8_t)(vb < 0.0f ? 0 : (vb > 255.0f ? 255 : (int)vb));
}

// ---------- host ---------------------------------------------------------------------------------------------------
// the blur kernel of a launch, among those this library carries (sift_plan routes a level to a streamed one only where one exists)
struct BlurFn { void (*stream)(Blur16Args, int, int, int); void (*tile)(Blur16Args); };
template <bool BGR>
BlurFn blur_kernel(const Launch& L) {
    const bool w4 = L.waves == 4;
    if (L.kind == BLUR_STREAM) {
        if constexpr (BGR) return {w4 ? blur16_stream<6, true, false, 4> : blur16_stream<6, true, false, 3>, nullptr};
        else switch (L.radius) {
            case 5: return {w4 ? blur16_stream<5, false, false, 4> : blur16_stream<5, false, false, 3>, nullptr};
            case 6: return {w4 ? blur16_stream<6, false, false, 4> : blur16_stream<6, false, false, 3>, nullptr};
            case 8: if (L.ds) return {w4 ? blur16_stream<8, false, true, 4> : blur16_stream<8, false, true, 3>, nullptr};
                    return {w4 ? blur16_stream<8, false, false, 4> : blur16_stream<8, false, false, 3>, nullptr};
            case 10: return {blur16_stream<10, false, false, 3>, nullptr};
            case 13: return {blur16_stream<13, false, false, 3>, nullptr};
        }
    }
    switch (L.radius) {
#define CASE(RR) case RR: return {nullptr, blur16_tile<RR, BGR>};
        CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#undef CASE
    }
    return {nullptr, nullptr};
}

// the device buffers of a batch work area: every per-frame buffer nb times, a stride of the layout apart
struct SiftBufs {
    DevBuf pyr;                              // all Gaussian levels
    DevBuf cand, refined, kps, kresp, sel, counters, rhist, ccnt;
    DevBuf khist;                            // top-k: per frame, the histogram of the refined records' response keys; all zero between batches
    DevBuf olist;                            // per frame: indices of the refined points at or above the response threshold
    DevBuf mins;                             // keep-all (nfeatures <= 0): smallest start key per refined location, all ones between batches
    DevBuf ksort;                            // keep-all: per frame, its keys sorted tile by tile (keepall_sort_tiles_kernel)
    DevBuf cube;                             // 3x3x3 DoG neighbourhoods of the first cube_cap candidates of every region (128 B each)
    hipError_t reserve(const Layout& l, int nb, hipStream_t st) {
        const Strides& bs = l.bs;
        const struct { DevBuf* b; size_t bytes; } want[] = {
            {&pyr, bs.pyr * sizeof(lvl_t)}, {&cand, bs.cand * sizeof(unsigned long long)},
            {&refined, bs.refined * sizeof(Refined)}, {&kps, bs.kps * sizeof(KpRec)}, {&kresp, bs.kps * sizeof(unsigned)}, {&sel, bs.sel * sizeof(SelRec)},
            {&mins, bs.mins * sizeof(unsigned)}, {&ksort, l.ksort_stride * sizeof(unsigned long long)}, {&counters, CNT_STRIDE * sizeof(unsigned)},
            {&rhist, bs.refined * sizeof(unsigned)}, {&khist, l.keepall ? 0 : KEY_BINS * sizeof(unsigned)}, {&olist, bs.refined * sizeof(unsigned)}, {&ccnt, CCNT_STRIDE * sizeof(unsigned)}, {&cube, bs.cube * sizeof(float)}};
        for (const auto& w : want) {
            if (!w.bytes) { w.b->release(); continue; }      // mins, ksort without keep-all; khist with it
            if (const hipError_t e = w.b->reserve((size_t)nb * w.bytes); e != hipSuccess) return e;
        }
        // keep-all's start keys are kept all ones between batches (keepall_reset_kernel).  The layout still numbers a claim bitmap per octave
        // (Strides::claimed): nothing backs it, duplicates leave in unique_compact_lds() / _mem()
        // top-k's key histograms are kept zero likewise: select_unique_kernel puts back what refine_kernel counted
        return l.keepall ? hipMemsetAsync(mins.p, 0xff, (size_t)nb * bs.mins * sizeof(unsigned), st) : hipMemsetAsync(khist.p, 0, (size_t)nb * KEY_BINS * sizeof(unsigned), st);
    }
    void release() { for (DevBuf* b : {&pyr, &khist, &cand, &refined, &kps, &kresp, &sel, &counters, &rhist, &ccnt, &olist, &mins, &ksort, &cube}) b->release(); }
};

}  // namespace

#ifdef MI355_REFINE_STATS
extern "C" int mi355_debug_refine_stats(unsigned long long* out40, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return MI355_ERR_FAILED;
    if (out40 && hipMemcpyFromSymbol(out40, HIP_SYMBOL(g_refine_stats), sizeof(g_refine_stats)) != hipSuccess) return MI355_ERR_FAILED;
    if (reset) { const unsigned long long z[40] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_refine_stats), z, sizeof(z)) != hipSuccess) return MI355_ERR_FAILED; }
    return MI355_OK;
}
#endif

// One batch work area: room for `nb` frames and one stream.  Frames handed to mi_sift_extract_dev() collect in `pend`; a full batch
// (or a flush) is enqueued by sift_run_batch() on that ONE in-order stream -- no reliance on how the runtime maps streams to hardware
// queues -- and every launch covers all frames of the batch (the frame is a grid dimension, or a factor of a streamed kernel's
// units): the pyramid octave by octave as sift_plan::pyramid_launches lists it (a base blur or a downsample, five blurs, one
// extrema test), then refine, selection, orientation, top-k and descriptors once each.  The latency-bound launches (30 tiny blurs,
// single-workgroup selections) are thus paid once per batch instead of once per frame.
struct SiftWork {
    Layout lay;                              // of the frames the buffers are sized for (lay.w == 0: none yet)
    int nb = 0;                              // frames the buffers hold
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;               // recorded after the last launch of the latest batch
    SiftBufs b;
    PyrDev P;                                // pointers of frame 0
    BatchStride bs;
    struct Pend { int img_id; const uint8_t* d_bgr; int ws; hipEvent_t ev; };   // ev: recorded once the batch is enqueued (optional)
    std::vector<Pend> pend;
};

constexpr int SIFT_SLOTS_MAX = 4;            // batch work areas (each with its own stream) that may be in flight
#define SIFT_SLOTS (ctx->sift_nslots)

void mi_sift_release(mi355_ctx* ctx) {
    for (SiftWork* s : ctx->sift_slots) {
        if (!s) continue;
        if (s->stream) { (void)hipStreamSynchronize(s->stream); (void)hipStreamDestroy(s->stream); }
        if (s->done) (void)hipEventDestroy(s->done);
        s->b.release();
        delete s;
    }
    ctx->sift_slots.clear();
    if (ctx->sift_in_ev) { (void)hipEventDestroy(ctx->sift_in_ev); ctx->sift_in_ev = nullptr; }
    for (int* p : ctx->pinned_chunks) (void)hipHostFree(p);
    ctx->pinned_chunks.clear();
    ctx->pinned_used = 0;
}

static int sift_run_batch(mi355_ctx* ctx, SiftWork* s);

// enqueues every partly filled batch
int mi_sift_flush(mi355_ctx* ctx) {
    int rc = MI355_OK;
    for (SiftWork* s : ctx->sift_slots) if (s && !s->pend.empty()) { const int r = sift_run_batch(ctx, s); if (r != MI355_OK) rc = r; }
    return rc;
}

// adopts the keypoint count of a finished frame from pinned memory
static int adopt_counts(mi355_ctx* ctx, int img_id, Features& f) {
    f.pending = false;
    if (!f.h_cnt) { f.n = 0; return MI355_OK; }               // its batch failed to launch
    const volatile int* c = f.h_cnt;
    for (int i = 0; i < 8; i++) ctx->last_counts[i] = c[i];
    if ((unsigned)c[0] > f.caps[0] || (unsigned)c[1] > f.caps[1] || (unsigned)c[2] > f.caps[2] || c[4]) {
        ctx->set_error("sift: candidate buffer overflow (image " + std::to_string(img_id) + " has more extrema than the buffers assume)");
        f.n = 0;
        return MI355_ERR_FAILED;
    }
    if (f.kp_limit > 0 && c[2] > f.kp_limit) {                 // keep-all: more keypoints than the ceiling the frame was extracted under
        ctx->set_error("sift: keep-all frame (image " + std::to_string(img_id) + ") has " + std::to_string(c[2]) + " keypoints, more than keepall_max=" +
                       std::to_string(f.kp_limit));
        f.n = 0;
        return MI355_ERR_FAILED;
    }
    f.n = c[3];
    return MI355_OK;
}

// waits for every in-flight frame and adopts the keypoint counts that landed in pinned memory
int mi_resolve_features(mi355_ctx* ctx) {
    int rc = mi_sift_flush(ctx);
    bool any = false;
    for (auto& kv : ctx->feats) if (kv.second.pending) { any = true; break; }
    if (!any) { ctx->batch_events_used = 0; return rc; }
    for (SiftWork* s : ctx->sift_slots) if (s && s->stream) MI_HIP(hipStreamSynchronize(s->stream));
    for (auto& kv : ctx->feats) {
        if (!kv.second.pending) continue;
        const int r = adopt_counts(ctx, kv.first, kv.second);
        if (r != MI355_OK) rc = r;
    }
    ctx->batch_events_used = 0;
    return rc;
}

// the same for the given frames only: the host waits for THEIR batches (batch events), later batches keep running -- a caller
// that matches pairs while the rest of the survey is still in detect+describe overlaps the two (bench.py, window surveys)
int mi_resolve_features_of(mi355_ctx* ctx, const int* ids, int n) {
    int rc = MI355_OK;
    bool parked = false;
    for (int k = 0; k < n && !parked; k++) {
        auto it = ctx->feats.find(ids[k]);
        if (it != ctx->feats.end() && it->second.pending && !it->second.h_cnt && !it->second.ready) parked = true;
    }
    if (parked) rc = mi_sift_flush(ctx);                      // some of them still wait for their batch to fill: enqueue it
    for (int k = 0; k < n; k++) {
        auto it = ctx->feats.find(ids[k]);
        if (it == ctx->feats.end() || !it->second.pending) continue;
        Features& f = it->second;
        if (f.ready) MI_HIP(hipEventSynchronize(f.ready));
        else { const int r = mi_resolve_features(ctx); if (r != MI355_OK) rc = r; continue; }
        const int r = adopt_counts(ctx, it->first, f);
        if (r != MI355_OK) rc = r;
    }
    return rc;
}

static constexpr size_t PINNED_CHUNK = 4096;   // frames per pinned chunk

static int* pinned_slot(mi355_ctx* ctx) {
    const size_t chunk = ctx->pinned_used / PINNED_CHUNK, off = ctx->pinned_used % PINNED_CHUNK;
    if (chunk >= ctx->pinned_chunks.size()) {
        int* p = nullptr;
        if (hipHostMalloc((void**)&p, PINNED_CHUNK * 8 * sizeof(int), hipHostMallocDefault) != hipSuccess) return nullptr;
        ctx->pinned_chunks.push_back(p);
    }
    ctx->pinned_used++;
    return ctx->pinned_chunks[chunk] + off * 8;
}

// sizes the work area for nb frames of the layout (nothing to do while the key and nb stay) and points P at frame 0
static int sift_prepare(mi355_ctx* ctx, SiftWork* s, const Layout& lay, int nb) {
    if (s->lay.same_key(lay) && s->nb == nb) return MI355_OK;
    MI_HIP(hipStreamSynchronize(s->stream));
    MI_HIP(s->b.reserve(lay, nb, s->stream));
    // with the layout's offsets and strides (multiples of 64 elements) every level and frame copy then starts on a 128-byte boundary
    if (((uintptr_t)s->b.pyr.p) & 127) { ctx->set_error("sift: work area is not 128-byte aligned"); return MI355_ERR_FAILED; }
    memset(&s->P, 0, sizeof(s->P));
    for (int o = 0; o < lay.n_oct; o++) {
        const Octave& oc = lay.oc[o];
        s->P.oc[o].w = oc.w; s->P.oc[o].h = oc.h;
        for (int i = 0; i < N_LEVELS; i++) s->P.oc[o].lv[i] = s->b.pyr.as<lvl_t>() + oc.lv[i];
        s->P.mins[o] = lay.keepall ? s->b.mins.as<unsigned>() + oc.mins : nullptr;
    }
    s->P.n_oct = lay.n_oct;
    s->bs = BatchStride{lay.bs.pyr, lay.bs.cand, lay.bs.refined, lay.bs.kps, lay.bs.cube, lay.bs.sel, lay.bs.mins};
    s->lay = lay; s->nb = nb;
    return MI355_OK;
}

// Accepts one frame: it joins the current batch, which is enqueued once it holds its sift_plan::batch_frames frames (or on a
// flush: any call that needs features, mi355_synchronize, or n_kp != NULL).  The frame memory must stay valid and
// unchanged until then.  Returns without waiting; the keypoint count is adopted later by mi_resolve_features().
int mi_sift_extract_dev(mi355_ctx* ctx, int img_id, const uint8_t* d_bgr, int w, int h, int ws, int* n_kp) {
    if (ctx->p.n_octave_layers != N_LAYERS || ctx->p.sigma != 1.6f) { ctx->set_error("sift: this build implements nOctaveLayers=3, sigma=1.6 (the reference's SIFT(2000,3,0.01,20))"); return MI355_ERR_ARG; }
    if (ctx->p.nfeatures > 2048) { ctx->set_error("sift: nfeatures must be in [1,2048], or <= 0 for cv::SIFT's keep-all (up to keepall_max=" + std::to_string(ctx->keepall_max) + " keypoints per frame)"); return MI355_ERR_ARG; }
    const bool keepall = ctx->p.nfeatures <= 0;
    const int kmax = keepall ? ctx->keepall_max : 0;
    if (keepall && (w > 16384 || h > 16384)) { ctx->set_error("sift: keep-all frames are at most 16384 x 16384"); return MI355_ERR_ARG; }
    std::string refused;
    const Layout lay = make_layout(w, h, keepall, kmax, refused);
    if (!refused.empty()) { ctx->set_error(refused); return MI355_ERR_ARG; }
    if (ctx->sift_slots.empty()) {
        ctx->sift_slots.resize(SIFT_SLOTS_MAX, nullptr);
        MI_HIP(hipEventCreateWithFlags(&ctx->sift_in_ev, hipEventDisableTiming));
    }
    if (ctx->sift_next >= SIFT_SLOTS) ctx->sift_next = 0;
    const int slot = ctx->sift_next;
    if (!ctx->sift_slots[slot]) {
        ctx->sift_slots[slot] = new SiftWork();
        MI_HIP(hipStreamCreateWithFlags(&ctx->sift_slots[slot]->stream, hipStreamNonBlocking));
        MI_HIP(hipEventCreateWithFlags(&ctx->sift_slots[slot]->done, hipEventDisableTiming));
    }
    SiftWork* s = ctx->sift_slots[slot];
    int rc = MI355_OK;
    static const size_t total_mem = [] { size_t fr = 0, tot = 0; return hipMemGetInfo(&fr, &tot) == hipSuccess ? tot : (size_t)0; }();
    const int nb = batch_frames(w, h, keepall, ctx->sift_batch, SIFT_SLOTS, total_mem);
    if (!s->pend.empty() && !(s->lay.same_key(lay) && s->nb == nb)) { rc = sift_run_batch(ctx, s); if (rc != MI355_OK) return rc; }   // size or ceiling change: close the batch
    rc = sift_prepare(ctx, s, lay, nb);
    if (rc != MI355_OK) return rc;
    auto fit = ctx->feats.find(img_id);
    if (fit != ctx->feats.end() && fit->second.pending) { rc = mi_resolve_features(ctx); if (rc != MI355_OK) return rc; }   // same id re-extracted while in flight
    Features& f = ctx->feats[img_id];
    f.w = w; f.h = h;
    MI_HIP(f.kp.reserve(sizeof(mi355_keypoint) * (size_t)(keepall ? kmax : 2048)));
    MI_HIP(f.d8.reserve((size_t)128 * (size_t)(keepall ? kmax : 2048)));
    f.pending = true; f.h_cnt = nullptr; f.ready = nullptr; f.n = 0;
    s->pend.push_back({img_id, d_bgr, ws, ctx->pend_event});
    if ((int)s->pend.size() >= nb) {
        rc = sift_run_batch(ctx, s);
        if (rc != MI355_OK) return rc;
    }
    if (ctx->pinned_used >= PINNED_CHUNK * 64) {           // recycle the pinned pool when nothing is pending any more
        rc = mi_resolve_features(ctx);
        if (rc != MI355_OK) return rc;
        ctx->pinned_used = 0;
    }
    if (n_kp) {
        rc = mi_resolve_features(ctx);
        if (rc != MI355_OK) return rc;
        *n_kp = f.n;
    }
    return MI355_OK;
}

// one batch on its way to the device: what the steps of sift_run_batch share
struct BatchRun {
    mi355_ctx* ctx; SiftWork* s; hipStream_t st;
    std::vector<SiftWork::Pend> pend;        // the batch's n frames
    std::vector<Features*> fs;
    int n;
    unsigned* cnt;                           // per frame: [0] candidates [1] refined [2] keypoints [3] n_sel [4] overflow [5] pass 1 ran [8..11] ctrl
    FrameOuts outs;
    int enqueue_pyramid();
    void enqueue_keypoints();
    int publish_batch();
};

// the pyramid and the extrema test, octave by octave: sift_plan decides the launches, this fills in the pointers
int BatchRun::enqueue_pyramid() {
    const PyramidTaps& taps = pyramid_taps();
    Routes routes = {ctx->blur_stream, ctx->xstream_min_w, ctx->xstream_min_frames, true};
    routes.narrow = ctx->narrow_routes;
    for (const SiftWork::Pend& p : pend) routes.base_frames_aligned = routes.base_frames_aligned && ((uintptr_t)p.d_bgr & 3) == 0 && (p.ws & 3) == 0 && p.ws >= 3 * s->lay.w;
    for (const Launch& L : pyramid_launches(s->lay, n, routes)) {
        const OctaveDev& oc = s->P.oc[L.octave];
        const dim3 grid(L.gx, L.gy, L.gz), block(256);
        switch (L.kind) {
            case BLUR_STREAM: case BLUR_TILE: {
                const bool base = L.level == 0;       // straight from the caller's frames: gray x 48 formed on the fly
                const Taps& t = base ? taps.base : taps.lv[L.level];
                Blur16Args a; memset(&a, 0, sizeof(a));
                a.w = oc.w; a.h = oc.h; a.tiles_x = (oc.w + T16W - 1) / T16W; a.tiles_y = (oc.h + T16H - 1) / T16H;
                a.fstride = s->bs.pyr; a.nb = n;
                if (base) for (int k = 0; k < n; k++) { a.bgr[k] = pend[k].d_bgr; a.bgr_ws[k] = pend[k].ws; }
                else a.src = oc.lv[L.level - 1];
                a.dst = oc.lv[L.level];
                if (L.ds) a.ds = s->P.oc[L.octave + 1].lv[0];
                memcpy(a.k, t.k, sizeof(float) * (2 * t.r + 1));
                const BlurFn k = base ? blur_kernel<true>(L) : blur_kernel<false>(L);
                if (!k.stream && !k.tile) { ctx->set_error("sift: unsupported kernel radius"); return MI355_ERR_FAILED; }
                ProfScope ps(ctx, k.stream ? "gauss_stream" : "gauss", L.bytes, st);
                if (k.stream) {
                    for (int i = 0; i <= t.r; i++) { a.kp[2 * i] = a.k[i]; a.kp[2 * i + 1] = i ? a.k[i - 1] : 0.0f; }
                    hipLaunchKernelGGL(k.stream, grid, block, 0, st, a, L.L, L.nstrip, L.nseg);
                } else hipLaunchKernelGGL(k.tile, grid, block, 0, st, a);
                break;
            }
            case DOWNSAMPLE: {
                const OctaveDev& pv = s->P.oc[L.octave - 1];
                ProfScope ps(ctx, "downsample", L.bytes, st);
                hipLaunchKernelGGL(downsample16, grid, block, 0, st, pv.lv[N_LAYERS], pv.w, oc.lv[0], oc.w, oc.h, s->bs.pyr);
                break;
            }
            case EXTREMA_STREAM: case EXTREMA_TILE: {
                ProfScope ps(ctx, "extrema", L.bytes, st);
                const SiftBufs& d = s->b;
                if (L.kind == EXTREMA_STREAM) hipLaunchKernelGGL(extrema_stream, grid, block, 0, st, oc, L.octave, d.cand.as<unsigned long long>(), d.ccnt.as<unsigned>(), s->lay.cand_cap, cnt + 4, s->bs,
                                                                 d.cube.as<float>(), s->lay.cube_cap, L.L, L.nstrip, L.nseg, n, L.xsw);
                else hipLaunchKernelGGL(extrema_kernel, grid, block, 0, st, oc, L.octave, d.cand.as<unsigned long long>(), d.ccnt.as<unsigned>(), s->lay.cand_cap, cnt + 4, s->bs, d.cube.as<float>(), s->lay.cube_cap);
                break;
            }
        }
    }
    return MI355_OK;
}

// the keypoint stages of all n frames, one launch each
void BatchRun::enqueue_keypoints() {
    const SiftBufs& d = s->b;
    const Layout& lay = s->lay;
    const BatchStride bs = s->bs;
    const unsigned kmax = (unsigned)lay.kmax;
    // top-k: the hash table of unique_compact_mem() where LDS does not hold it -- the frame's candidate list, dead after refine_kernel; the largest
    // power of two of slots in it (make_layout: >= 4 px0 + 65536 candidates for at most px0 / 8 + 65536 refined points, so twice the points fit)
    unsigned uniq_cap = 1024;
    while ((size_t)uniq_cap * 2 <= bs.cand && uniq_cap < (1u << 31)) uniq_cap <<= 1;
    {
        ProfScope ps(ctx, "refine", 0.0, st);
        hipLaunchKernelGGL(refine_kernel, dim3(REFINE_GX, NREG, n), dim3(256), 0, st, s->P, d.cand.as<unsigned long long>(), d.ccnt.as<unsigned>(), lay.cand_cap, cnt + 0,
                           ctx->p.contrast_threshold, ctx->p.edge_threshold, 1.6f, d.refined.as<Refined>(), cnt + 1, lay.ref_cap, d.rhist.as<unsigned>(), bs, d.cube.as<float>(), lay.cube_cap,
                           lay.keepall ? nullptr : d.khist.as<unsigned>());
    }
    {
        // keep-all: every refined point that holds its location's smallest start key is oriented; top-k: one point per location above the response threshold of nfeatures + margin
        ProfScope ps(ctx, "kp_select", 0.0, st);
        if (lay.keepall) {
            hipLaunchKernelGGL(keepall_live_kernel, dim3(256, n), dim3(256), 0, st, s->P, d.refined.as<Refined>(), cnt + 1, lay.ref_cap, cnt + 8, d.olist.as<unsigned>(), bs);
            hipLaunchKernelGGL(keepall_reset_kernel, dim3(256, n), dim3(256), 0, st, s->P, d.refined.as<Refined>(), cnt + 1, lay.ref_cap, bs);
        } else {
            hipLaunchKernelGGL(select_unique_kernel, dim3(1, n), dim3(1024), 0, st, d.refined.as<Refined>(), bs, d.rhist.as<unsigned>(), cnt + 1, lay.ref_cap,
                               (unsigned)ctx->p.nfeatures + (unsigned)ctx->select_margin, cnt + 8, bs.refined, d.olist.as<unsigned>(), d.khist.as<unsigned>(), d.cand.as<unsigned long long>(), uniq_cap,
                               reinterpret_cast<int*>(cnt + 4));
        }
    }
    // top-k: pass 1 (everything below the response threshold) exits at once unless top-k asked for it; keep-all: one pass, the keypoints leave in generation order
    for (int pass = 0; pass < (lay.keepall ? 1 : 2); pass++) {
        {
            ProfScope ps(ctx, "orient", 0.0, st);
            hipLaunchKernelGGL(orient_kernel, dim3(ctx->num_cu * 4, n), dim3(256), 0, st, s->P, d.refined.as<Refined>(), cnt + 1, lay.ref_cap,
                               d.kps.as<KpRec>(), d.kresp.as<unsigned>(), cnt + 2, lay.kp_cap, cnt + 8, pass, bs, d.olist.as<unsigned>());
        }
        ProfScope ps(ctx, "topk", 0.0, st);
        if (lay.keepall) {
            hipLaunchKernelGGL(keepall_sort_tiles_kernel, dim3((kmax + KA_TILE - 1) / KA_TILE, n), dim3(1024), 0, st, d.kps.as<KpRec>(), cnt + 2, lay.kp_cap, kmax,
                               d.ksort.as<unsigned long long>(), lay.ksort_stride, outs, d.sel.as<SelRec>(), bs);
            hipLaunchKernelGGL(keepall_place_kernel, dim3((kmax + 255) / 256, n), dim3(256), 0, st, d.kps.as<KpRec>(), cnt + 2, lay.kp_cap, kmax,
                               d.ksort.as<const unsigned long long>(), lay.ksort_stride, outs, d.sel.as<SelRec>(), reinterpret_cast<int*>(cnt + 3), reinterpret_cast<int*>(cnt + 4), bs);
        } else {
            hipLaunchKernelGGL(topk_kernel, dim3(n), dim3(1024), 0, st, d.kps.as<KpRec>(), d.kresp.as<unsigned>(), cnt + 2, lay.kp_cap, ctx->p.nfeatures,
                               outs, d.sel.as<SelRec>(), reinterpret_cast<int*>(cnt + 3), reinterpret_cast<int*>(cnt + 4), cnt + 8, pass, bs,
                               d.refined.as<Refined>(), d.rhist.as<unsigned>(), cnt + 1, lay.ref_cap, d.olist.as<unsigned>(), d.cand.as<unsigned long long>(), uniq_cap,
                               reinterpret_cast<int*>(cnt + 5));
        }
    }
    ProfScope ps(ctx, "describe", 0.0, st);
    hipLaunchKernelGGL(describe_kernel, dim3(((int)bs.sel + 3) / 4, n), dim3(256), 0, st, s->P, d.sel.as<SelRec>(), reinterpret_cast<const int*>(cnt + 3), outs, bs);
}

// hands the batch's results over: the matcher's operands, the counters into pinned slots, and the events that say so
int BatchRun::publish_batch() {
    const Layout& lay = s->lay;
    // the matcher's operands of all n frames in one launch, their counters in one strided copy (n launches + n copies of ~5 us each kept
    // the batch's stream, and a pipeline slot, busy for 0.3 ms per batch of 32)
    { int rc = mi_finish_features_batch(ctx, fs.data(), n, reinterpret_cast<const int*>(cnt + 3), (int)CNT_STRIDE, st, lay.keepall ? lay.kmax : 2048); if (rc != MI355_OK) return rc; }
    if (ctx->pinned_used % PINNED_CHUNK + (size_t)n > PINNED_CHUNK) ctx->pinned_used += PINNED_CHUNK - ctx->pinned_used % PINNED_CHUNK;   // n slots in one chunk
    int* h0 = nullptr;
    for (int k = 0; k < n; k++) {
        int* hc = pinned_slot(ctx);
        if (!hc) { ctx->set_error("sift: pinned alloc failed"); return MI355_ERR_NOMEM; }
        if (k == 0) h0 = hc;
        Features& f = *fs[k];
        f.h_cnt = hc; f.pending = true; f.n = 0;
        f.caps[0] = 0xffffffffu; f.caps[1] = lay.ref_cap; f.caps[2] = lay.kp_cap;      // candidate overflow is flagged by the kernel (cnt[4])
        f.kp_limit = lay.keepall ? lay.kmax : 0;
    }
    MI_HIP(hipMemcpy2DAsync(h0, 8 * sizeof(int), cnt, CNT_STRIDE * sizeof(unsigned), 8 * sizeof(unsigned), (size_t)n, hipMemcpyDeviceToHost, st));
    MI_HIP(hipEventRecord(s->done, st));
    // the batch's own event: mi_resolve_features_of() waits for it, not for the streams
    if (ctx->batch_events_used >= ctx->batch_events.size()) {
        hipEvent_t e = nullptr;
        MI_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->batch_events.push_back(e);
    }
    hipEvent_t e = ctx->batch_events[ctx->batch_events_used++];
    MI_HIP(hipEventRecord(e, st));
    for (int k = 0; k < n; k++) fs[k]->ready = e;
    for (int k = 0; k < n; k++) if (pend[k].ev) MI_HIP(hipEventRecord(pend[k].ev, st));
    return MI355_OK;
}

static int sift_run_batch(mi355_ctx* ctx, SiftWork* s) {
    BatchRun b = {};
    b.ctx = ctx; b.s = s;
    b.pend.swap(s->pend);
    const int n = b.n = (int)b.pend.size();
    if (n == 0) return MI355_OK;
    ctx->sift_next = (ctx->sift_next + 1) % SIFT_SLOTS;     // the next batch collects in the next work area
    const hipStream_t st = b.st = s->stream;
    // the frames were produced on the caller's stream
    MI_HIP(hipEventRecord(ctx->sift_in_ev, ctx->stream));
    MI_HIP(hipStreamWaitEvent(st, ctx->sift_in_ev, 0));
    // (measurement mode) the previous batch's pyramid + extrema first.  The wait stands BEFORE the memsets: an event recorded right
    // after a wait takes the end of the stream's last command as its time, which would put the waiting into the first bracket
    const bool serial_heavy = ctx->serial_heavy != 0;
    if (serial_heavy && ctx->heavy_ev_valid) MI_HIP(hipStreamWaitEvent(st, ctx->heavy_ev, 0));
    b.cnt = s->b.counters.as<unsigned>();
    MI_HIP(hipMemsetAsync(b.cnt, 0, (size_t)n * CNT_STRIDE * sizeof(unsigned), st));
    MI_HIP(hipMemsetAsync(s->b.ccnt.p, 0, (size_t)n * CCNT_STRIDE * sizeof(unsigned), st));
    for (int k = 0; k < n; k++) {
        Features* f = &ctx->feats[b.pend[k].img_id];
        b.fs.push_back(f);
        b.outs.kp[k] = f->kp.as<mi355_keypoint>(); b.outs.d8[k] = f->d8.as<uint8_t>();
    }
    { const int rc = b.enqueue_pyramid(); if (rc != MI355_OK) return rc; }
    if (serial_heavy) {
        if (!ctx->heavy_ev) MI_HIP(hipEventCreateWithFlags(&ctx->heavy_ev, hipEventDisableTiming));
        MI_HIP(hipEventRecord(ctx->heavy_ev, st)); ctx->heavy_ev_valid = true;
    }
    b.enqueue_keypoints();
    MI_HIP(hipGetLastError());
    return b.publish_batch();
}

// a frame parked with event `ev` still waits for its batch to fill: enqueue that batch now (the event gets recorded)
int mi_sift_flush_if_parked(mi355_ctx* ctx, hipEvent_t ev) {
    for (SiftWork* s : ctx->sift_slots) {
        if (!s) continue;
        for (const SiftWork::Pend& p : s->pend) if (p.ev == ev) return sift_run_batch(ctx, s);
    }
    return MI355_OK;
}
