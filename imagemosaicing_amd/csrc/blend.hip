// csrc/blend.hip -- multiband blend of the warped chips, replacing
//   detail::MultiBandBlender blender(false, band); prepare / feed per chip / blend; convertTo(CV_8U)
//   (MosaicImage.cpp:2296-2299, 2451-2486).
// The arithmetic is OpenCV 2.4.0's (binaries only; the reference commits no blended output).  The definition implemented here --
// 16-bit Laplacian pyramids, float weight pyramids, [1 4 6 4 1] REDUCE / EXPAND in integer arithmetic, every rounding and border --
// is the one stated at the top of oracle/oracle_blend.c, which also lists what was checked against the reference's DLLs and the one
// known divergence (the binary's reassociated float REDUCE); the parity test compares the output bytes with that oracle.
// All kernels are streaming stencils over at most a few hundred MB.  Level 0 of a chip's pyramids is never stored (round 4): it IS the
// chip (u8 -> i16, extended by reflection) and mask / 255 (extended by zeros), so the first REDUCE and the level-0 Laplacian read the
// chip and the mask themselves (4 bytes per pixel instead of 10 written and 20 read).  The REDUCE chains of up to 32 chips run as five
// batched launches (blockIdx.z = chip; they are independent of one another); the accumulation into the canvas pyramids stays one chip
// after the other, in chip order, because the float weight sums make the order per pixel part of the result: per chip 5 x Laplacian +
// accumulate (a 2 x 2 fine block per thread, never stored) and the top level's accumulate.
#include "common.h"
#include "chips.h"
#include "blend_plan.h"

namespace bp = blend_plan;

namespace {

__device__ __forceinline__ int reflect101d(int p, int n) { if (n == 1) return 0; while (p < 0 || p >= n) { if (p < 0) p = -p; else p = 2 * n - 2 - p; } return p; }
__device__ __forceinline__ int reflectd(int p, int n) { while (p < 0 || p >= n) { if (p < 0) p = -p - 1; else p = 2 * n - 1 - p; } return p; }
__device__ __forceinline__ short sat16d(int v) { return (short)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

// Pointers read from a structure in memory are generic to the compiler (flat loads, and no unaligned vector loads: the 24-byte reads
// below came out as 24 byte loads); in the global address space an unaligned run of bytes is one or two vector loads.
#define GLOBAL_U8(p) ((const __attribute__((address_space(1))) uint8_t*)(p))
__device__ __forceinline__ void load_run(const void* p, unsigned* out, int nbytes_const8) {      // nbytes: 8, 20 or 24
    const __attribute__((address_space(1))) uint8_t* g = GLOBAL_U8(p);
    if (nbytes_const8 == 8) __builtin_memcpy(out, (const void __attribute__((address_space(1)))*)g, 8);
    else if (nbytes_const8 == 20) __builtin_memcpy(out, (const void __attribute__((address_space(1)))*)g, 20);
    else __builtin_memcpy(out, (const void __attribute__((address_space(1)))*)g, 24);
}

// level 0 of one chip's region: chip extended by reflection (edge pixel included), weight = mask / 255 extended by zeros
__global__ __launch_bounds__(256) void blend_prep_kernel(const uint8_t* chip, int cws, const uint8_t* mask, int mws, int cw, int ch,
                                                         int left, int top, int rw, int rh, short* g0, float* w0) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= rw) return;
    const int sx = reflectd(x - left, cw), sy = reflectd(y - top, ch);
    const uint8_t* p = chip + (size_t)sy * cws + 3 * sx;
    short* g = g0 + ((size_t)y * rw + x) * 3;
    g[0] = (short)p[0]; g[1] = (short)p[1]; g[2] = (short)p[2];
    float w = 0.0f;
    if (y - top >= 0 && y - top < ch && x - left >= 0 && x - left < cw) w = (float)mask[(size_t)(y - top) * mws + (x - left)] * (float)(1.0 / 255.0);
    w0[(size_t)y * rw + x] = w;
}

// The geometry -- Win, ChipP, MAX_BANDS, chip_windows and the plan of a call -- is host code of its own: blend_plan.h.  The kernels keep a
// parameter type of this name in this namespace: it is part of their names, "(anonymous namespace)::pyr_down0_batch_kernel((anonymous
// namespace)::ChipP const*, short*, float*)", which profiles/ quote.
using bp::MAX_BANDS;
using bp::Win;
struct ChipP : bp::ChipP {};
static_assert(sizeof(ChipP) == sizeof(bp::ChipP), "the device array is filled from blend_plan::ChipP");
// pixel offset of level l >= 1 behind tmp
__device__ __forceinline__ size_t level_off(int rw, int rh, int l) { size_t o = 0; for (int m = 1; m < l; m++) o += (size_t)(rw >> m) * (rh >> m); return o; }

// REDUCE: i16 x 3 in integers (so the 5x5 product form equals the oracle's rows-then-columns form: rows [1 4 6 4 1] . pixels, then
// columns, (sum + 128) >> 8) and f32 weights in the oracle's order (6 c + 4 (l + r) + ll + rr per row, the same over the rows, / 256).
// REDUCE of both pyramids of a chip in one launch, two horizontally adjacent outputs per thread: their 5-tap windows share three of the
// seven source columns, and away from the left / right border those seven pixels are 42 contiguous, 4-byte aligned bytes (11 32-bit
// loads per row instead of 30 16-bit ones).  The sums are the ones of pyr_down16_kernel / pyr_down_f_kernel, term for term.
__device__ __forceinline__ void pyr_down_pair_body(const short* src, const float* srcw, int w, int h, short* dst, float* dstw, const Win win) {
    const int dw = w >> 1, x0 = (win.x0 & ~1) + (blockIdx.x * 256 + threadIdx.x) * 2, y = win.y0 + blockIdx.y;
    if (x0 >= dw || y >= (h >> 1) || x0 > win.x1 || y > win.y1) return;
    const bool two = x0 + 1 < dw;
    const int wt[5] = {1, 4, 6, 4, 1};
    const bool interior = 2 * x0 - 2 >= 0 && 2 * x0 + 4 < w;
    int xs[7];
#pragma unroll
    for (int j = 0; j < 7; j++) xs[j] = reflect101d(2 * x0 - 2 + j, w);
    int acc[2][3] = {{0, 0, 0}, {0, 0, 0}};
    float fr[2][5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const int sy = reflect101d(2 * y - 2 + k, h);
        const short* s = src + (size_t)sy * w * 3;
        short px[7][3];
        if (interior) {
            const unsigned* p = reinterpret_cast<const unsigned*>(s + 3 * (2 * x0 - 2));      // 12 (x0 - 1) bytes into a row of 6 w bytes, w even
            unsigned u[11];
#pragma unroll
            for (int q = 0; q < 11; q++) u[q] = p[q];
#pragma unroll
            for (int j = 0; j < 7; j++)
#pragma unroll
                for (int c = 0; c < 3; c++) { const int e = 3 * j + c; px[j][c] = (short)((e & 1) ? (u[e >> 1] >> 16) : (u[e >> 1] & 0xffff)); }
        } else {
#pragma unroll
            for (int j = 0; j < 7; j++) { px[j][0] = s[3 * xs[j]]; px[j][1] = s[3 * xs[j] + 1]; px[j][2] = s[3 * xs[j] + 2]; }
        }
#pragma unroll
        for (int o = 0; o < 2; o++) {
            int r[3] = {0, 0, 0};
#pragma unroll
            for (int j = 0; j < 5; j++) { r[0] += wt[j] * px[2 * o + j][0]; r[1] += wt[j] * px[2 * o + j][1]; r[2] += wt[j] * px[2 * o + j][2]; }
            acc[o][0] += wt[k] * r[0]; acc[o][1] += wt[k] * r[1]; acc[o][2] += wt[k] * r[2];
        }
        const float* sw = srcw + (size_t)sy * w;
        float f[7];
#pragma unroll
        for (int j = 0; j < 7; j++) f[j] = sw[xs[j]];
#pragma unroll
        for (int o = 0; o < 2; o++) fr[o][k] = f[2 * o + 2] * 6.0f + (f[2 * o + 1] + f[2 * o + 3]) * 4.0f + f[2 * o] + f[2 * o + 4];
    }
#pragma unroll
    for (int o = 0; o < 2; o++) {
        if (o == 1 && !two) break;
        short* d = dst + ((size_t)y * dw + x0 + o) * 3;
        d[0] = sat16d((acc[o][0] + 128) >> 8); d[1] = sat16d((acc[o][1] + 128) >> 8); d[2] = sat16d((acc[o][2] + 128) >> 8);
        const float v = fr[o][2] * 6.0f + (fr[o][1] + fr[o][3]) * 4.0f + fr[o][0] + fr[o][4];
        dstw[(size_t)y * dw + x0 + o] = v * (1.0f / 256.0f);
    }
}
// level l -> l + 1 (l >= 1) of every chip of a batch; the grid covers the largest chip
__global__ __launch_bounds__(256) void pyr_down_pair_batch_kernel(const ChipP* cp, int l, short* g, float* wp) {
    const ChipP& c = cp[blockIdx.z];
    const size_t a = c.tmp + level_off(c.rw, c.rh, l), b = c.tmp + level_off(c.rw, c.rh, l + 1);
    const Win win = l + 1 <= MAX_BANDS ? c.cwin[l + 1] : Win{0, 0, (c.rw >> (l + 1)) - 1, (c.rh >> (l + 1)) - 1};
    pyr_down_pair_body(g + a * 3, wp + a, c.rw >> l, c.rh >> l, g + b * 3, wp + b, win);
}

// Level 0 -> 1 straight from the chip and its mask: the level-0 value at region pixel (x, y) is (short)chip[reflect(x - left), reflect(y - top)]
// (the chip extended by BORDER_REFLECT, edge pixel included), the weight mask / 255 inside the chip and 0 outside -- what blend_prep_kernel
// used to store.  Same sums as pyr_down_pair_body, term for term.  Away from the borders the seven pixels of a row are 21 contiguous
// bytes: six unaligned 32-bit loads (three bytes of slack inside the row), the seven mask bytes two.
__global__ __launch_bounds__(256) void pyr_down0_batch_kernel(const ChipP* cp, short* g, float* wp) {
    const ChipP& c = cp[blockIdx.z];
    const int w = c.rw, h = c.rh;
    const Win win = c.cwin[1];
    const int dw = w >> 1, x0 = (win.x0 & ~1) + (blockIdx.x * 256 + threadIdx.x) * 2, y = win.y0 + blockIdx.y;
    if (x0 >= dw || y >= (h >> 1) || x0 > win.x1 || y > win.y1) return;
    short* dst = g + c.tmp * 3;
    float* dstw = wp + c.tmp;
    const bool two = x0 + 1 < dw;
    const int wt[5] = {1, 4, 6, 4, 1};
    const int cx0 = 2 * x0 - 2 - c.left;                                   // chip column of the first of the seven
    const bool interior = 2 * x0 - 2 >= 0 && 2 * x0 + 4 < w && cx0 >= 0 && cx0 + 8 < c.cw;
    int xs[7]; bool xin[7];
    if (!interior) {
#pragma unroll
        for (int j = 0; j < 7; j++) { const int xr = reflect101d(2 * x0 - 2 + j, w) - c.left; xin[j] = xr >= 0 && xr < c.cw; xs[j] = reflectd(xr, c.cw); }
    }
    int acc[2][3] = {{0, 0, 0}, {0, 0, 0}};
    float fr[2][5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const int yr = reflect101d(2 * y - 2 + k, h) - c.top;
        const bool yin = yr >= 0 && yr < c.ch;
        const int sy = reflectd(yr, c.ch);
        const __attribute__((address_space(1))) uint8_t* s = GLOBAL_U8(c.chip) + (size_t)sy * c.cws;
        const __attribute__((address_space(1))) uint8_t* m = GLOBAL_U8(c.mask) + (size_t)sy * c.mws;
        short px[7][3];
        float f[7];
        if (interior) {
            // the horizontal [1 4 6 4 1] of both outputs and the three channels straight on the packed bytes: pixel j, channel ch is byte
            // 3 j + ch of the run, so a dword meets a constant vector of tap weights (zeros on the other channels' bytes) in one
            // v_dot4_u32_u8 -- 27 of them per row instead of 21 byte extractions and 30 multiply-adds; the same integers
            unsigned u[6];
            load_run((const void*)(s + 3 * cx0), u, 24);
#pragma unroll
            for (int o = 0; o < 2; o++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    unsigned r = 0;
#pragma unroll
                    for (int q = 0; q < 6; q++) {
                        unsigned wq = 0;
#pragma unroll
                        for (int b = 0; b < 4; b++) {
                            const int e = 4 * q + b, jj = e / 3 - 2 * o;
                            if (e % 3 == ch && jj >= 0 && jj < 5) wq |= (unsigned)wt[jj] << (8 * b);
                        }
                        if (wq) r = __builtin_amdgcn_udot4(u[q], wq, r, false);
                    }
                    acc[o][ch] += wt[k] * (int)r;
                }
            unsigned mv[2];
            load_run((const void*)(m + cx0), mv, 8);
#pragma unroll
            for (int j = 0; j < 7; j++) f[j] = yin ? (float)((mv[j >> 2] >> (8 * (j & 3))) & 0xffu) * (float)(1.0 / 255.0) : 0.0f;
        } else {
#pragma unroll
            for (int j = 0; j < 7; j++) {
                px[j][0] = (short)s[3 * xs[j]]; px[j][1] = (short)s[3 * xs[j] + 1]; px[j][2] = (short)s[3 * xs[j] + 2];
                f[j] = (yin && xin[j]) ? (float)m[xs[j]] * (float)(1.0 / 255.0) : 0.0f;
            }
#pragma unroll
            for (int o = 0; o < 2; o++) {
                int r[3] = {0, 0, 0};
#pragma unroll
                for (int j = 0; j < 5; j++) { r[0] += wt[j] * px[2 * o + j][0]; r[1] += wt[j] * px[2 * o + j][1]; r[2] += wt[j] * px[2 * o + j][2]; }
                acc[o][0] += wt[k] * r[0]; acc[o][1] += wt[k] * r[1]; acc[o][2] += wt[k] * r[2];
            }
        }
#pragma unroll
        for (int o = 0; o < 2; o++) fr[o][k] = f[2 * o + 2] * 6.0f + (f[2 * o + 1] + f[2 * o + 3]) * 4.0f + f[2 * o] + f[2 * o + 4];
    }
#pragma unroll
    for (int o = 0; o < 2; o++) {
        if (o == 1 && !two) break;
        short* d = dst + ((size_t)y * dw + x0 + o) * 3;
        d[0] = sat16d((acc[o][0] + 128) >> 8); d[1] = sat16d((acc[o][1] + 128) >> 8); d[2] = sat16d((acc[o][2] + 128) >> 8);
        const float v = fr[o][2] * 6.0f + (fr[o][1] + fr[o][3]) * 4.0f + fr[o][0] + fr[o][4];
        dstw[(size_t)y * dw + x0 + o] = v * (1.0f / 256.0f);
    }
}

// horizontal EXPAND value (before the vertical combination) at fine column X of coarse row s (3 channels, channel c)
__device__ __forceinline__ int up_h(const short* s, int w, int X, int c) {
    const int x = X >> 1;
    if (w == 1) return s[c] * 8;
    if (!(X & 1)) {
        if (x == 0) return s[c] * 6 + s[3 + c] * 2;
        if (x == w - 1) return s[3 * (w - 2) + c] + s[3 * (w - 1) + c] * 7;
        return s[3 * (x - 1) + c] + s[3 * x + c] * 6 + s[3 * (x + 1) + c];
    }
    if (x == w - 1) return s[3 * (w - 1) + c] * 8;
    return (s[3 * x + c] + s[3 * (x + 1) + c]) * 4;
}

// up_h at the fine columns 2x and 2x + 1 for the three channels of one coarse row; away from the left / right border the three coarse
// pixels are 18 contiguous bytes (one 20-byte run instead of nine 2-byte loads)
__device__ __forceinline__ void up_h_pair(const short* row, int w, int x, int* he, int* ho) {
    if (x >= 1 && x + 1 < w) {
        unsigned u[5];
        load_run(row + 3 * (x - 1), u, 20);
        short v[9];
#pragma unroll
        for (int e = 0; e < 9; e++) v[e] = (short)((e & 1) ? (u[e >> 1] >> 16) : (u[e >> 1] & 0xffffu));
#pragma unroll
        for (int c = 0; c < 3; c++) { he[c] = v[c] + v[3 + c] * 6 + v[6 + c]; ho[c] = (v[3 + c] + v[6 + c]) * 4; }
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) { he[c] = up_h(row, w, 2 * x, c); ho[c] = up_h(row, w, 2 * x + 1, c); }
    }
}

// fine = sat16(fine - EXPAND(coarse)) (SUB) or sat16(EXPAND(coarse) + fine); coarse is w x h, fine 2w x 2h
template <bool SUB>
__global__ __launch_bounds__(256) void pyr_up16_combine_kernel(const short* coarse, int w, int h, short* fine, int Y0 = 0) {
    const int X = blockIdx.x * 256 + threadIdx.x, Y = Y0 + blockIdx.y;      // fine rows Y0 .. Y0 + gridDim.y - 1
    if (X >= 2 * w) return;
    const int y = Y >> 1;
    const int ym = (y == 0) ? (h > 1 ? 1 : 0) : y - 1, yp = (y == h - 1) ? h - 1 : y + 1;
    const short* rm = coarse + (size_t)ym * w * 3;
    const short* r0 = coarse + (size_t)y * w * 3;
    const short* rp = coarse + (size_t)yp * w * 3;
    short* f = fine + ((size_t)Y * 2 * w + X) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        int v;
        if (!(Y & 1)) v = up_h(rm, w, X, c) + up_h(r0, w, X, c) * 6 + up_h(rp, w, X, c);
        else v = (up_h(r0, w, X, c) + up_h(rp, w, X, c)) * 4;
        const int up = sat16d((v + 32) >> 6);
        f[c] = SUB ? sat16d((int)f[c] - up) : sat16d(up + (int)f[c]);
    }
}

// Laplacian level of a chip and its accumulation in one pass: lap = sat16(fine - EXPAND(coarse)) is formed in registers and added to the
// canvas, never stored (the separate in-place pyr_up16_combine<true> + blend_accumulate pair moved 12 more bytes per pixel and was a
// third of the blend's kernel time).  Both levels stay Gaussian, so the levels can be taken in any order.
// One thread per COARSE pixel = a 2 x 2 block of fine pixels: the 3 x 3 coarse neighbourhood is read once for the four of them (a thread
// per fine pixel issued 27 two-byte loads each and ran at a quarter of the bandwidth the bytes need).
__device__ __forceinline__ void blend_lap_accumulate_body(const short* coarse, int w, int h, const short* fine, const float* wgt, int ox, int oy,
                                                          short* dl, float* dw, int DW, int x, int y) {
    if (x >= w) return;
    const int FW = 2 * w;
    {
        // A pixel whose weight is +0 leaves the canvas as it is: (short)((float)lap * 0.0f) = 0 and sum + 0.0f = sum (the weight sums start
        // at +0 and only grow).  With FindMasksByDistMap's masks a chip's weights vanish outside its own cell of the mosaic (+ the reach of
        // the REDUCE filter at this level) -- 98 % of a chip's pixels when 2000 chips share a 20000^2 canvas -- so the block is judged by its
        // four weights before anything else is read.
        const float2 wa = *reinterpret_cast<const float2*>(wgt + (size_t)(2 * y) * FW + 2 * x);
        const float2 wb = *reinterpret_cast<const float2*>(wgt + (size_t)(2 * y + 1) * FW + 2 * x);
        if (wa.x == 0.0f && wa.y == 0.0f && wb.x == 0.0f && wb.y == 0.0f && !__builtin_signbit(wa.x + wa.y + wb.x + wb.y)) return;
    }
    const int ym = (y == 0) ? (h > 1 ? 1 : 0) : y - 1, yp = (y == h - 1) ? h - 1 : y + 1;
    const short* rows[3] = {coarse + (size_t)ym * w * 3, coarse + (size_t)y * w * 3, coarse + (size_t)yp * w * 3};
    int he[3][3], ho[3][3];                               // horizontal EXPAND values at fine columns 2x (even) and 2x + 1 (odd), per row and channel
#pragma unroll
    for (int r = 0; r < 3; r++) up_h_pair(rows[r], w, x, he[r], ho[r]);
    // the two fine pixels of a row are 12 contiguous bytes: three 32-bit loads / stores instead of six 16-bit ones, the weights as one
    // 64-bit access.  On the canvas side they are naturally aligned (the fine column 2x, the region offset ox and the row pitches are even).
    // On the chip side they need not be: ChipP::tmp is a running sum of level sizes and a chip whose top level is odd x odd (224 x 160 at
    // five bands: 7 x 5) leaves every level of the next chips at an odd pixel offset -- 2 bytes off for the 32-bit words, 4 bytes off for the
    // float2.  Global memory on gfx950 takes unaligned vector accesses and the values are the same ones (tests/test_gpu_blend_edges.py,
    // odd_offsets: 40 chips, odd offsets inside both batches).
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
        const int Y = 2 * y + dy;
        const size_t fi = (size_t)Y * FW + 2 * x;
        const size_t di = (size_t)(oy + Y) * DW + (ox + 2 * x);
        const float2 wv2 = *reinterpret_cast<const float2*>(wgt + fi);
        const unsigned* fp = reinterpret_cast<const unsigned*>(fine + fi * 3);
        unsigned* dp = reinterpret_cast<unsigned*>(dl + di * 3);
        const unsigned f0 = fp[0], f1 = fp[1], f2 = fp[2];
        unsigned d0 = dp[0], d1 = dp[1], d2 = dp[2];
        const short fv[6] = {(short)(f0 & 0xffff), (short)(f0 >> 16), (short)(f1 & 0xffff), (short)(f1 >> 16), (short)(f2 & 0xffff), (short)(f2 >> 16)};
        short dv[6] = {(short)(d0 & 0xffff), (short)(d0 >> 16), (short)(d1 & 0xffff), (short)(d1 >> 16), (short)(d2 & 0xffff), (short)(d2 >> 16)};
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const float wv = dx ? wv2.y : wv2.x;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int hm = dx ? ho[0][c] : he[0][c], h0 = dx ? ho[1][c] : he[1][c], hp = dx ? ho[2][c] : he[2][c];
                const int v = dy ? (h0 + hp) * 4 : hm + h0 * 6 + hp;
                const int up = sat16d((v + 32) >> 6);
                const short lap = sat16d((int)fv[3 * dx + c] - up);
                dv[3 * dx + c] = (short)(dv[3 * dx + c] + (short)((float)lap * wv));
            }
        }
        dp[0] = (unsigned)(unsigned short)dv[0] | ((unsigned)(unsigned short)dv[1] << 16);
        dp[1] = (unsigned)(unsigned short)dv[2] | ((unsigned)(unsigned short)dv[3] << 16);
        dp[2] = (unsigned)(unsigned short)dv[4] | ((unsigned)(unsigned short)dv[5] << 16);
        float2* wp2 = reinterpret_cast<float2*>(dw + di);
        float2 a2 = *wp2; a2.x += wv2.x; a2.y += wv2.y; *wp2 = a2;
    }
}

__global__ __launch_bounds__(256) void blend_lap_accumulate_kernel(const short* coarse, int w, int h, const short* fine, const float* wgt, int ox, int oy,
                                                                   short* dl, float* dw, int DW) {
    blend_lap_accumulate_body(coarse, w, h, fine, wgt, ox, oy, dl, dw, DW, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

// Levels 1 .. bands of one chip in ONE launch (blockIdx.y walks the rows of all of them): the Laplacian levels 1 .. bands - 1 and the top
// (Gaussian) level.  Launched one by one the small levels cost ~8 us each whatever their size: four of the six launches per chip.
struct LapLevels {
    int n;                                   // entries: n - 1 Laplacian levels, then the top level
    int row0[MAX_BANDS + 1];                 // first grid row of entry i (row0[n] = grid rows)
    int w[MAX_BANDS], h[MAX_BANDS], ox[MAX_BANDS], oy[MAX_BANDS], DW[MAX_BANDS];
    int x0[MAX_BANDS], y0[MAX_BANDS], x1[MAX_BANDS];     // first thread column / row and last thread column of the entry's active window
    size_t fine[MAX_BANDS], coarse[MAX_BANDS];      // pixel offsets into the chip pyramid (g / wp)
    long long dst[MAX_BANDS];                       // ... and into the canvas pyramids (dl / dw): may be negative for a stripe (the level's rows above the stripe are not stored)
};
__global__ __launch_bounds__(256) void blend_lap_levels_kernel(LapLevels L, const short* g, const float* wp, short* dl, float* dw) {
    int i = 0;
#pragma unroll 1
    while (i + 1 < L.n && (int)blockIdx.y >= L.row0[i + 1]) i++;
    const int y = L.y0[i] + (blockIdx.y - L.row0[i]), x = L.x0[i] + blockIdx.x * 256 + threadIdx.x;      // the level's active window (ChipP::twin)
    if (i + 1 < L.n) {
        if (x > L.x1[i]) return;
        blend_lap_accumulate_body(g + L.coarse[i] * 3, L.w[i], L.h[i], g + L.fine[i] * 3, wp + L.fine[i], L.ox[i], L.oy[i], dl + L.dst[i] * 3, dw + L.dst[i], L.DW[i], x, y);
    } else {
        // top level: canvas Laplacian += (short)(Gaussian * weight), canvas weight += weight (blend_accumulate_kernel)
        const int lw = L.w[i];
        if (x >= lw || x > L.x1[i]) return;
        const float wv = wp[L.fine[i] + (size_t)y * lw + x];
        if (wv == 0.0f && !__builtin_signbit(wv)) return;      // adds nothing (see blend_lap_accumulate_body)
        const long long di = L.dst[i] + (long long)(L.oy[i] + y) * L.DW[i] + (L.ox[i] + x);
        const short* s = g + (L.fine[i] + (size_t)y * lw + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) dl[di * 3 + c] = (short)(dl[di * 3 + c] + (short)((float)s[c] * wv));
        dw[di] += wv;
    }
}

// The same for level 0, whose Gaussian level is the chip itself (see pyr_down0_batch_kernel): fine values from the chip extended by
// reflection, weights mask / 255 inside the chip and 0 outside.  Inside the chip the two fine pixels of a row are six contiguous bytes.
// A row's two pixels are written as three 32-bit words only when BOTH have a weight: then both belong to this chip's cell and no other chip
// has a weight there.  Otherwise each pixel with a weight is updated on its own (16-bit accesses) and a pixel without one is not touched --
// so with masks that partition the canvas (FindMasksByDistMap) the chips write disjoint bytes at level 0, in any order: the batch form
// below runs the level-0 accumulation of up to 32 chips as one launch (per chip it was ~10 us of stream time whatever the window's size).
__device__ __forceinline__ void blend_lap0_body(const ChipP& c, const short* coarse, int ox, int oy, short* dl, float* dw, int DW) {
    const int w = c.rw >> 1, h = c.rh >> 1;
    const int x = c.twin[0].x0 + blockIdx.x * 256 + threadIdx.x, y = c.twin[0].y0 + blockIdx.y;
    if (x >= w || x > c.twin[0].x1 || y > c.twin[0].y1) return;      // (the rows matter: a stripe's canvas pyramids hold the stripe's rows only)
    const int cx = 2 * x - c.left;                            // chip column of the even fine pixel
    const bool xfast = cx >= 0 && cx + 3 < c.cw;              // both columns inside the chip and the 8-byte read inside the row
    {
        // the block's four mask bytes first: all zero (or outside the chip) = four weights of +0, which leave the canvas as it is
        // (blend_lap_accumulate_body); only the chip's own cell of the mosaic goes on
        unsigned any = 0;
#pragma unroll
        for (int dy = 0; dy < 2; dy++) {
            const int cy = 2 * y + dy - c.top;
            if (cy < 0 || cy >= c.ch) continue;
            const uint8_t* mrow = c.mask + (size_t)cy * c.mws;
            if (cx >= 0 && cx < c.cw) any |= mrow[cx];
            if (cx + 1 >= 0 && cx + 1 < c.cw) any |= mrow[cx + 1];
        }
        if (!any) return;
    }
    const int ym = (y == 0) ? (h > 1 ? 1 : 0) : y - 1, yp = (y == h - 1) ? h - 1 : y + 1;
    const short* rows[3] = {coarse + (size_t)ym * w * 3, coarse + (size_t)y * w * 3, coarse + (size_t)yp * w * 3};
    int he[3][3], ho[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++) up_h_pair(rows[r], w, x, he[r], ho[r]);
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
        const int Y = 2 * y + dy;
        const int cy = Y - c.top;
        const bool yin = cy >= 0 && cy < c.ch;
        const int sy = reflectd(cy, c.ch);
        const uint8_t* srow = c.chip + (size_t)sy * c.cws;
        const uint8_t* mrow = c.mask + (size_t)sy * c.mws;
        short fv[6]; float wv2[2];
        if (xfast) {
            unsigned u[2];
            load_run(srow + 3 * cx, u, 8);
#pragma unroll
            for (int e = 0; e < 6; e++) fv[e] = (short)((u[e >> 2] >> (8 * (e & 3))) & 0xffu);
            wv2[0] = yin ? (float)mrow[cx] * (float)(1.0 / 255.0) : 0.0f;
            wv2[1] = yin ? (float)mrow[cx + 1] * (float)(1.0 / 255.0) : 0.0f;
        } else {
#pragma unroll
            for (int dx = 0; dx < 2; dx++) {
                const int xr = cx + dx, sx = reflectd(xr, c.cw);
                fv[3 * dx] = (short)srow[3 * sx]; fv[3 * dx + 1] = (short)srow[3 * sx + 1]; fv[3 * dx + 2] = (short)srow[3 * sx + 2];
                wv2[dx] = (yin && xr >= 0 && xr < c.cw) ? (float)mrow[sx] * (float)(1.0 / 255.0) : 0.0f;
            }
        }
        const size_t di = (size_t)(oy + Y) * DW + (ox + 2 * x);
        short add[6];
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const float wv = wv2[dx];
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const int hm = dx ? ho[0][ch] : he[0][ch], h0 = dx ? ho[1][ch] : he[1][ch], hp = dx ? ho[2][ch] : he[2][ch];
                const int v = dy ? (h0 + hp) * 4 : hm + h0 * 6 + hp;
                const int up = sat16d((v + 32) >> 6);
                const short lap = sat16d((int)fv[3 * dx + ch] - up);
                add[3 * dx + ch] = (short)((float)lap * wv);
            }
        }
        if (wv2[0] != 0.0f && wv2[1] != 0.0f) {
            unsigned* dp = reinterpret_cast<unsigned*>(dl + di * 3);
            const unsigned d0 = dp[0], d1 = dp[1], d2 = dp[2];
            short dv[6] = {(short)(d0 & 0xffff), (short)(d0 >> 16), (short)(d1 & 0xffff), (short)(d1 >> 16), (short)(d2 & 0xffff), (short)(d2 >> 16)};
#pragma unroll
            for (int e = 0; e < 6; e++) dv[e] = (short)(dv[e] + add[e]);
            dp[0] = (unsigned)(unsigned short)dv[0] | ((unsigned)(unsigned short)dv[1] << 16);
            dp[1] = (unsigned)(unsigned short)dv[2] | ((unsigned)(unsigned short)dv[3] << 16);
            dp[2] = (unsigned)(unsigned short)dv[4] | ((unsigned)(unsigned short)dv[5] << 16);
            float2* wp2 = reinterpret_cast<float2*>(dw + di);
            float2 a2 = *wp2; a2.x += wv2[0]; a2.y += wv2[1]; *wp2 = a2;
        } else {
#pragma unroll
            for (int dx = 0; dx < 2; dx++) {
                if (wv2[dx] == 0.0f) continue;                        // adds nothing (blend_lap_accumulate_body)
                short* dp = dl + (di + dx) * 3;
#pragma unroll
                for (int ch = 0; ch < 3; ch++) dp[ch] = (short)(dp[ch] + add[3 * dx + ch]);
                dw[di + dx] += wv2[dx];
            }
        }
    }
}
__global__ __launch_bounds__(256) void blend_lap0_accumulate_kernel(ChipP c, const short* coarse, int ox, int oy, short* dl, float* dw, int DW) {
    blend_lap0_body(c, coarse, ox, oy, dl, dw, DW);
}
// level 0 of every chip of a batch (blockIdx.z = chip; the grid covers the largest window): only for masks that partition the canvas
__global__ __launch_bounds__(256) void blend_lap0_accumulate_batch_kernel(const ChipP* cp, const short* g, short* dl, float* dw, int DW) {
    const ChipP& c = cp[blockIdx.z];
    blend_lap0_body(c, g + c.tmp * 3, c.tlx, c.tly, dl, dw, DW);
}

// canvas Laplacian += (short)(chip Laplacian * weight), canvas weight += weight, over the chip's region at this level
__global__ __launch_bounds__(256) void blend_accumulate_kernel(const short* g, const float* wgt, int lw, int lh, int ox, int oy, short* dl, float* dw, int DW) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= lw) return;
    const float wv = wgt[(size_t)y * lw + x];
    const size_t di = (size_t)(oy + y) * DW + (ox + x);
    const short* s = g + ((size_t)y * lw + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) dl[di * 3 + c] = (short)(dl[di * 3 + c] + (short)((float)s[c] * wv));
    dw[di] += wv;
}

__global__ __launch_bounds__(256) void blend_normalize_kernel(short* dl, const float* dw, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float d = dw[i] + 1e-5f;
#pragma unroll
    for (int c = 0; c < 3; c++) dl[i * 3 + c] = (short)((float)dl[i * 3 + c] / d);
}

__global__ __launch_bounds__(256) void blend_finalize_kernel(const short* dl, const float* dw, int Wp, int W, uint8_t* out, int ows, int row0 = 0) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = row0 + blockIdx.y;      // canvas row; `out` starts at canvas row row0
    if (x >= W) return;
    const size_t di = (size_t)y * Wp + x;
    uint8_t* o = out + (size_t)blockIdx.y * ows + 3 * x;
    if (!(dw[di] > 1e-5f)) { o[0] = 0; o[1] = 0; o[2] = 0; return; }
#pragma unroll
    for (int c = 0; c < 3; c++) { const int v = dl[di * 3 + c]; o[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
}

inline dim3 grid2(int w, int h) { return dim3((unsigned)((w + 255) / 256), (unsigned)h); }

// where the finished canvas goes: the caller's device buffer (d_rows != NULL: rows of ws bytes, the first one is the plan's first output
// row; nothing is copied to the host), or a malloc'd host canvas
struct BlendOut { uint8_t* d_rows; int ws; uint8_t** host; int* ow; int* oh; int* ows; };

// One blend: the plan, the chips that take part, and the device side -- the batch's chip pyramids (g, wp: levels >= 1) and the canvas
// pyramids (dl, dw), which vlap / vwgt address by canvas coordinates.  set != NULL: the chip stage's set (the one-call forms: chips and
// masks in HBM, FindMasksByDistMap's masks with their owned boxes, the pixels still to be made); NULL: the direct form's host chips,
// staged one batch at a time.
struct Blender {
    mi355_ctx* ctx; const bp::Plan& p; chips::ChipSet* set; hipStream_t st;
    std::vector<bp::ChipP> par;
    short* g; float* wp; short* dl; float* dw; const ChipP* d_par;
    bool lap0_batched;
    short* vlap(int l) const { return dl + p.voff[l] * 3; }
    float* vwgt(int l) const { return dw + p.voff[l]; }

    // host chips of one batch to "blend_chip" / "blend_mask"; the batch's ChipP then point there
    int stage_batch(const bp::Batch& bt) {
        uint8_t* dchip = ctx->buf("blend_chip").as<uint8_t>();
        uint8_t* dmask = ctx->buf("blend_mask").as<uint8_t>();
        size_t co = 0, mo = 0;
        for (int i = bt.b0; i < bt.b1; i++) {
            const size_t cb = (size_t)par[i].cws * par[i].ch, mb = (size_t)par[i].mws * par[i].ch;
            MI_HIP(hipMemcpyAsync(dchip + co, par[i].chip, cb, hipMemcpyHostToDevice, st));
            MI_HIP(hipMemcpyAsync(dmask + mo, par[i].mask, mb, hipMemcpyHostToDevice, st));
            par[i].chip = dchip + co; par[i].mask = dmask + mo;
            co += (cb + 15) & ~(size_t)15; mo += (mb + 15) & ~(size_t)15;
        }
        return MI355_OK;
    }

    // no pyramid: level 0 is the only level; it is materialised and accumulated (the path of bands = 0)
    void accumulate_flat(const bp::Batch& bt) {
        for (int i = bt.b0; i < bt.b1; i++) {
            const bp::ChipP& c = par[i];
            hipLaunchKernelGGL(blend_prep_kernel, grid2(c.rw, c.rh), dim3(256), 0, st, c.chip, c.cws, c.mask, c.mws, c.cw, c.ch, c.left, c.top, c.rw, c.rh, g + c.tmp * 3, wp + c.tmp);
            hipLaunchKernelGGL(blend_accumulate_kernel, grid2(c.rw, c.rh), dim3(256), 0, st, g + c.tmp * 3, wp + c.tmp, c.rw, c.rh, c.tlx, c.tly, vlap(0), vwgt(0), p.Wp);
        }
    }

    // The launches that take a whole batch.  REDUCE chains: independent of one another and of the canvas (grids: the largest active window
    // of the batch at that level, in threads of two outputs).  Level 0 of the whole batch at once when the masks partition the canvas.
    void batch_launches(const bp::Batch& bt) {
        const unsigned B = (unsigned)(bt.b1 - bt.b0);
        auto red_grid = [&](int l1) {
            int tw = 1, th = 1;
            for (int i = bt.b0; i < bt.b1; i++) {
                const Win wn = l1 <= MAX_BANDS ? par[i].cwin[l1] : Win{0, 0, (par[i].rw >> l1) - 1, (par[i].rh >> l1) - 1};
                const int t = (wn.x1 - (wn.x0 & ~1)) / 2 + 1, hh = wn.y1 - wn.y0 + 1;
                tw = t > tw ? t : tw; th = hh > th ? hh : th;
            }
            return dim3((unsigned)((tw + 255) / 256), (unsigned)th, B);
        };
        hipLaunchKernelGGL(pyr_down0_batch_kernel, red_grid(1), dim3(256), 0, st, d_par + bt.b0, g, wp);
        for (int l = 1; l < p.nb; l++)
            hipLaunchKernelGGL(pyr_down_pair_batch_kernel, red_grid(l + 1), dim3(256), 0, st, d_par + bt.b0, l, g, wp);
        if (!lap0_batched) return;
        int tw = 1, th = 1;
        for (int i = bt.b0; i < bt.b1; i++) { const Win t = par[i].twin[0]; tw = t.x1 - t.x0 + 1 > tw ? t.x1 - t.x0 + 1 : tw; th = t.y1 - t.y0 + 1 > th ? t.y1 - t.y0 + 1 : th; }
        hipLaunchKernelGGL(blend_lap0_accumulate_batch_kernel, dim3((unsigned)((tw + 255) / 256), (unsigned)th, B), dim3(256), 0, st, d_par + bt.b0, g, vlap(0), vwgt(0), p.Wp);
    }

    // More than MAX_BANDS levels: level by level, whole levels (the windows hold MAX_BANDS).  That takes a canvas side above 65 536 with
    // band > 16 and about 170 GB of pyramids: no test reaches this arm, it is kept as it was.
    void accumulate_chip_by_level(const bp::ChipP& c, const std::vector<size_t>& roff) {
        const int nb = p.nb, Wp = p.Wp, tlx = c.tlx, tly = c.tly, rw = c.rw, rh = c.rh;
        for (int l = 1; l < nb; l++)
            hipLaunchKernelGGL(blend_lap_accumulate_kernel, grid2(rw >> (l + 1), rh >> (l + 1)), dim3(256), 0, st, g + roff[l + 1] * 3, rw >> (l + 1), rh >> (l + 1),
                               g + roff[l] * 3, wp + roff[l], tlx >> l, tly >> l, vlap(l), vwgt(l), Wp >> l);
        hipLaunchKernelGGL(blend_accumulate_kernel, grid2(rw >> nb, rh >> nb), dim3(256), 0, st, g + roff[nb] * 3, wp + roff[nb], rw >> nb, rh >> nb, tlx >> nb, tly >> nb,
                           vlap(nb), vwgt(nb), Wp >> nb);
    }

    // One chip into the canvas pyramids: Laplacian level l = Gaussian l - EXPAND(Gaussian l + 1), accumulated as it is formed.  Level 0 on its
    // own unless the batch took it; the levels 1 .. nb as one launch.
    void accumulate_chip(const bp::ChipP& c) {
        const int nb = p.nb;
        std::vector<size_t> roff(nb + 2, 0);                      // levels >= 1 behind c.tmp
        roff[1] = c.tmp;
        for (int l = 1; l < nb; l++) roff[l + 1] = roff[l] + (size_t)(c.rw >> l) * (c.rh >> l);
        if (!lap0_batched && c.twin[0].y1 >= c.twin[0].y0)
            hipLaunchKernelGGL(blend_lap0_accumulate_kernel, grid2(c.twin[0].x1 - c.twin[0].x0 + 1, c.twin[0].y1 - c.twin[0].y0 + 1), dim3(256), 0, st, ChipP{c}, g + roff[1] * 3, c.tlx, c.tly,
                               vlap(0), vwgt(0), p.Wp);
        if (nb > MAX_BANDS) return accumulate_chip_by_level(c, roff);
        LapLevels L; memset(&L, 0, sizeof(L));
        int grows = 0, maxw = 0;                                           // (an empty window -- a stripe -- has y1 = y0 - 1: no rows)
        for (int l = 1; l <= nb; l++) {
            // Laplacian level l < nb: one thread per pixel of level l + 1; the top level: one per pixel, no coarser level
            const int i = L.n++, tl = l < nb ? l + 1 : nb;
            L.row0[i] = grows; L.w[i] = c.rw >> tl; L.h[i] = c.rh >> tl; L.ox[i] = c.tlx >> l; L.oy[i] = c.tly >> l; L.DW[i] = p.Wp >> l;
            L.fine[i] = roff[l]; L.coarse[i] = l < nb ? roff[l + 1] : 0; L.dst[i] = p.voff[l];
            const Win t = c.twin[l];
            L.x0[i] = t.x0; L.y0[i] = t.y0; L.x1[i] = t.x1;
            grows += t.y1 - t.y0 + 1; maxw = t.x1 - t.x0 + 1 > maxw ? t.x1 - t.x0 + 1 : maxw;
        }
        L.row0[L.n] = grows;
        if (grows > 0 && maxw > 0) hipLaunchKernelGGL(blend_lap_levels_kernel, grid2(maxw, grows), dim3(256), 0, st, L, g, wp, dl, dw);
    }

    // the canvas pyramids to the canvas: normalise every level, collapse from the top
    void normalise_and_collapse() {
        for (int l = 0; l <= p.nb; l++) {
            const size_t cnt = p.level_px(l);
            hipLaunchKernelGGL(blend_normalize_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, dl + p.loff[l] * 3, dw + p.loff[l], cnt);
        }
        for (int l = p.nb - 1; l >= 0; l--)       // collapse: rows nlo[l] .. nhi[l] of level l from the rows of level l + 1 they read (all stored: stripe_levels)
            hipLaunchKernelGGL((pyr_up16_combine_kernel<false>), grid2(p.Wp >> l, p.nhi[l] - p.nlo[l] + 1), dim3(256), 0, st, vlap(l + 1), p.Wp >> (l + 1), p.Hp >> (l + 1), vlap(l), p.nlo[l]);
    }

    // level 0 as bytes: into the caller's device rows, or through "blend_out" into a malloc'd host canvas (never a stripe: vlap(0) is dl there)
    int write_out(const BlendOut& out) {
        const int W = p.W, row0 = p.striped ? p.row0 : 0, rows = p.striped ? p.rows : p.H;
        const int ows = out.d_rows ? out.ws : (W * 3 + 3) & ~3;
        uint8_t* dst = out.d_rows;
        if (!dst) { DevBuf& dout = ctx->buf("blend_out"); MI_HIP(dout.reserve((size_t)ows * rows)); dst = dout.as<uint8_t>(); }
        MI_HIP(hipMemsetAsync(dst, 0, (size_t)ows * rows, st));
        hipLaunchKernelGGL(blend_finalize_kernel, grid2(W, rows), dim3(256), 0, st, vlap(0), vwgt(0), p.Wp, W, dst, ows, row0);
        MI_HIP(hipGetLastError());
        if (!out.d_rows) {
            uint8_t* host = (uint8_t*)malloc((size_t)ows * rows);
            if (!host) return MI355_ERR_NOMEM;
            hipError_t e = hipMemcpyAsync(host, dst, (size_t)ows * rows, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { free(host); ctx->set_error(std::string("multiband_blend: ") + hipGetErrorString(e)); return MI355_ERR_DEVICE; }
            *out.host = host;
        }
        if (out.ow) *out.ow = W;
        if (out.oh) *out.oh = rows;
        if (out.ows) *out.ows = ows;
        return MI355_OK;
    }
};

// chips / masks / info / n: the direct form's host arrays (set == NULL)
int blend_core(mi355_ctx* ctx, chips::ChipSet* set, const uint8_t* const* chips, const uint8_t* const* masks, const mi355_chip_info* info, int n,
               const bp::Plan& p, const BlendOut& out) {
    const int nb = p.nb;
    const int* owned = set && !set->owned.empty() ? set->owned.data() : nullptr;
    std::vector<const uint8_t*> dc, dm;                          // the set's chips and masks as pointers
    if (set) {
        n = set->n(); info = set->info.data();
        dc.resize(n > 0 ? n : 1); dm.resize(n > 0 ? n : 1);
        for (int v = 0; v < n; v++) { dc[v] = ctx->buf("chip_imgs").as<uint8_t>() + set->chip_off[v]; dm[v] = ctx->buf("chip_masks").as<uint8_t>() + set->mask_off[v]; }
        chips = dc.data(); masks = dm.data();
    }
    if (n < 0 || (n > 0 && (!chips || !masks || !info)) || p.W <= 0 || p.H <= 0 || p.band < 0 || (!out.host && !out.d_rows)) { ctx->set_error("multiband_blend: bad arguments"); return MI355_ERR_ARG; }
    if (p.striped && (p.row0 < 0 || p.rows < 1 || p.row0 + p.rows > p.H || !owned || !out.d_rows)) { ctx->set_error("multiband_blend: bad stripe"); return MI355_ERR_ARG; }
    const hipStream_t st = ctx->stream;
    DevBuf& dlap = ctx->buf("blend_dst_lap");
    DevBuf& dwgt = ctx->buf("blend_dst_w");
    MI_HIP(dlap.reserve(p.loff[nb + 1] * 3 * sizeof(short)));
    MI_HIP(dwgt.reserve(p.loff[nb + 1] * sizeof(float)));
    DevBuf& glap = ctx->buf("blend_src_lap");
    DevBuf& gwgt = ctx->buf("blend_src_w");
    DevBuf& dpar = ctx->buf("blend_chip_params");
    bp::Feed feed;
    if (!bp::feed_regions(p, chips, masks, info, n, owned, feed)) { ctx->set_error("multiband_blend: chip outside the canvas"); return MI355_ERR_ARG; }
    const int nc = (int)feed.par.size();
    const bp::Batches batches = bp::make_batches(feed.par, nb, !set);
    // every buffer is sized once, up front: the work below is then pure stream-ordered copies and launches (no allocation, no
    // synchronisation between chips or batches)
    MI_HIP(glap.reserve(batches.max_px * 3 * sizeof(short) + 16));
    MI_HIP(gwgt.reserve(batches.max_px * sizeof(float) + 16));
    MI_HIP(dpar.reserve((size_t)(nc > 0 ? nc : 1) * sizeof(ChipP)));
    if (!set) { MI_HIP(ctx->buf("blend_chip").reserve(batches.max_cb + 16)); MI_HIP(ctx->buf("blend_mask").reserve(batches.max_mb + 16)); }
    if (set && !set->pixels_made) {
        // the chips hold no pixels yet: each chip's are made inside the part of the chip its active windows read (chip_pixel_window); here
        // the windows of all chips go to the device, the launches follow batch by batch
        std::vector<int> wins((size_t)4 * (nc > 0 ? nc : 1));
        for (int i = 0; i < nc; i++) {
            int x0 = 0, y0 = 0, x1 = feed.par[i].cw - 1, y1 = feed.par[i].ch - 1;
            if (nb >= 1 && nb <= MAX_BANDS) bp::chip_pixel_window(feed.par[i], x0, y0, x1, y1);
            wins[4 * i] = x0; wins[4 * i + 1] = y0; wins[4 * i + 2] = x1; wins[4 * i + 3] = y1;
        }
        const int rc = mi_chip_pixels_prepare(ctx, *set, nc, feed.chip.data(), wins.data());
        if (rc != MI355_OK) return rc;
    }
    Blender b{ctx, p, set, st, std::move(feed.par), glap.as<short>(), gwgt.as<float>(), dlap.as<short>(), dwgt.as<float>(), dpar.as<ChipP>(),
              owned != nullptr && nb <= MAX_BANDS};      // level 0 batched: the masks are this device's FindMasksByDistMap masks
    if (set && nb > 0 && nc > 0) {
        MI_HIP(hipMemcpyAsync(dpar.p, b.par.data(), (size_t)nc * sizeof(ChipP), hipMemcpyHostToDevice, st));   // one copy, not one per batch
        MI_HIP(hipStreamSynchronize(st));      // `par` is a local and the device-canvas path returns without another wait: the copy must have read it (the stream holds little here: the stage before ended with a wait)
    }
    // the canvas pyramids start from zero (after the wait above, so that the host does not sit through them)
    MI_HIP(hipMemsetAsync(dlap.p, 0, p.loff[nb + 1] * 3 * sizeof(short), st));
    MI_HIP(hipMemsetAsync(dwgt.p, 0, p.loff[nb + 1] * sizeof(float), st));
    for (const bp::Batch& bt : batches.v) {
        if (!set) { const int rc = b.stage_batch(bt); if (rc != MI355_OK) return rc; }
        if (set && !set->pixels_made) { const int rc = mi_chip_pixels_launch(ctx, *set, bt.b0, bt.b1 - bt.b0); if (rc != MI355_OK) return rc; }      // the batch's chip pixels, one launch (the seam forms made whole chips)
        if (nb == 0) b.accumulate_flat(bt);
        else {
            // the chips' parameters of this batch (the slot of the previous batch may still be read: one slot per batch, sized once)
            if (!set) MI_HIP(hipMemcpyAsync(dpar.as<ChipP>() + bt.b0, b.par.data() + bt.b0, (size_t)(bt.b1 - bt.b0) * sizeof(ChipP), hipMemcpyHostToDevice, st));      // (device chips: all of them at once, above)
            b.batch_launches(bt);
            for (int i = bt.b0; i < bt.b1; i++) b.accumulate_chip(b.par[i]);      // chip after chip, in chip order
        }
        MI_HIP(hipGetLastError());
    }
    b.normalise_and_collapse();
    return b.write_out(out);
}

}  // namespace

int mi_multiband_blend(mi355_ctx* ctx, const uint8_t* const* chips, const uint8_t* const* masks, const mi355_chip_info* info, int n,
                       int W, int H, int band, uint8_t** out, int* ow, int* oh, int* ows_out) {
    return blend_core(ctx, nullptr, chips, masks, info, n, bp::make_plan(W, H, band), BlendOut{nullptr, 0, out, ow, oh, ows_out});
}

// The whole of LaplacianPyramidBlending (MosaicImage.cpp:2205-2510) without leaving the device between its stages: chips
// and masks (mi_chips_and_masks_dev) feed the blender straight from HBM; only the finished canvas goes back to the host.
int mi_mosaic_blended(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                      const uint8_t* keep, int band, uint8_t** out, int* ow, int* oh, int* ows_out) {
    chips::ChipSet set;
    const int rc = mi_chips_and_masks_dev(ctx, imgs, w, h, ws, n, h9s, keep, chips::Request{chips::Request::BLEND_HOST}, set);
    if (rc != MI355_OK) return rc;
    return blend_core(ctx, &set, nullptr, nullptr, nullptr, 0, bp::make_plan(set.W, set.H, band), BlendOut{nullptr, 0, out, ow, oh, ows_out});
}

// The same with the survey resident in HBM: device frames in, device canvas out (C5: frames + chips + masks + distance maps + both
// pyramid sets co-resident).  Enqueues on the ctx stream.
// row0, rows: one STRIPE of the canvas (rows < 0: all of it) -- a rank's part of the blended mosaic, the counterpart of mi_mosaic_refined_dev's
// stripes.  d_canvas then holds the rows row0 .. row0 + rows - 1 only.  The canvas geometry stays the whole canvas's; the rank forms the chips
// that reach its rows (+ the pyramids' reach: stripe_levels / stripe_mask_rows), their ownership there, and the rows of every canvas pyramid level
// its output rows depend on -- the same values the whole canvas holds there, so stripes put side by side are the whole canvas byte for byte.
int mi_mosaic_blended_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                          const uint8_t* keep, int band, uint8_t* d_canvas, int cw, int ch, int cws, int row0, int rows, uint8_t* cover_only) {
    if (!d_canvas && !cover_only) return MI355_ERR_ARG;
    int lw = 0, lh = 0;
    { int rc = mi_blend_layout(w, h, n, h9s, keep, &lw, &lh); if (rc != MI355_OK) return rc; }
    if (lw != cw || lh != ch || cws < 3 * cw || (cws & 3)) { ctx->set_error("mosaic_blended_dev: canvas geometry does not match mi355_blend_layout"); return MI355_ERR_ARG; }
    if (rows < 0) { row0 = 0; rows = ch; }
    if (row0 < 0 || rows < 1 || row0 + rows > ch) { ctx->set_error("mosaic_blended_dev: bad stripe"); return MI355_ERR_ARG; }
    const bp::Plan p = bp::make_plan(cw, ch, band, row0, rows);
    int mr0 = 0, mr1 = ch - 1;
    if (p.striped) bp::stripe_mask_rows(p.nlo, p.nhi, ch, mr0, mr1);
    chips::ChipSet set;
    int rc = mi_chips_and_masks_dev(ctx, d_imgs, w, h, ws, n, h9s, keep, chips::Request{chips::Request::BLEND_DEVICE, 1, mr0, mr1, cover_only}, set);
    if (rc != MI355_OK || cover_only) return rc;         // cover_only (mi355_mosaic_stripe_cover): the frames whose chips reach the stripe (+ the pyramids' reach) are marked, nothing was enqueued
    DevBuf& full = ctx->buf("blend_full_canvas");      // copy_out: the whole canvas goes here, the rows asked for are copied out
    const hipError_t e = p.copy_out ? full.reserve((size_t)cws * ch) : hipSuccess;
    if (e != hipSuccess) { ctx->set_error(std::string("mosaic_blended_dev: ") + hipGetErrorString(e)); return MI355_ERR_NOMEM; }
    rc = blend_core(ctx, &set, nullptr, nullptr, nullptr, 0, p, BlendOut{p.copy_out ? full.as<uint8_t>() : d_canvas, cws, nullptr, nullptr, nullptr, nullptr});
    if (rc == MI355_OK && p.copy_out && hipMemcpyAsync(d_canvas, full.as<uint8_t>() + (size_t)row0 * cws, (size_t)rows * cws, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) rc = MI355_ERR_DEVICE;
    return rc;
}

// The one-call blend along optimised seams (blend_seam.hip: definition, kernels, entry checks): the chip stage in its seam form -- whole chips,
// the cell map unless one is given, the ownership that follows it -- and the blender as it is, on the owned boxes.  Whole canvas only.
int mi_mosaic_blended_seam_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                               const uint8_t* keep, int band, const mi355_seamcut_params* params, const uint16_t* d_cells, int gw, int gh,
                               uint8_t* d_canvas, int cw, int ch, int cws) {
    if (!d_canvas || cws < 3 * cw || (cws & 3)) { ctx->set_error("mosaic_blended_seam_dev: canvas geometry does not match mi355_blend_layout"); return MI355_ERR_ARG; }
    chips::Request req{chips::Request::SEAM_DEVICE};
    req.seam.params = params; req.seam.gw = gw; req.seam.gh = gh;
    req.seam.make_cells = d_cells == nullptr;
    req.seam.d_cells = const_cast<uint16_t*>(d_cells);           // (read only unless make_cells)
    if (!d_cells) {
        DevBuf& dcells = ctx->buf("blend_seam_cells");
        MI_HIP(dcells.reserve(sizeof(uint16_t) * (size_t)gw * gh));
        req.seam.d_cells = dcells.as<uint16_t>();
    }
    chips::ChipSet set;
    const int rc = mi_chips_and_masks_dev(ctx, d_imgs, w, h, ws, n, h9s, keep, req, set);
    if (rc != MI355_OK) return rc;
    if (set.W != cw || set.H != ch) { ctx->set_error("mosaic_blended_seam_dev: canvas geometry does not match mi355_blend_layout"); return MI355_ERR_ARG; }
    return blend_core(ctx, &set, nullptr, nullptr, nullptr, 0, bp::make_plan(cw, ch, band), BlendOut{d_canvas, cws, nullptr, nullptr, nullptr, nullptr});
}
