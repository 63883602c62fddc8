// csrc/sharp.hip -- frame sharpness (gfx950): the Laplacian energy of every frame over the ground it shares with its listed partners, measured
// on the canvas lattice through the refined render's own map and sample (include/mi355_mosaic.h, "frame sharpness"; mosaic_frame.h).
//
//   sharp_stats_kernel   the hot path.  The work list is the gain statistics' (stats_tiles.h): tiles of 64 x 16 lattice points over each
//                        listed pair's canvas-box intersection (pair tiles) and, where the caller asks for per-frame records, over each frame's
//                        own box (cover tiles).  One launch for all of them; one lane per lattice column, 4 lattice rows per lane.  At a
//                        point a frame is mapped at five canvas pixels (the point and its 4-neighbours, each through frame_src on its own
//                        integer pixel: nothing is stepped); where all five have a sample they are gathered (frame_sample3: load_quad3, the
//                        render's loads), turned to gray and combined to L.  A pair tile walks frame a's five samples first and frame b's only
//                        where a has a Laplacian, so the ten samples are never held together.  n, L^2 and centre gray are summed in 32-bit
//                        registers (a workgroup's 1024 points x 1020^2 = 1.07e9 < 2^32, gray below 2^18), reduced across the wave with
//                        shuffles, and land with one 64-bit vector atomic per field per workgroup in a device record array: integer sums,
//                        so the result does not depend on the order the workgroups run in.
// The walk over a tile's points is gain_stats_kernel's, spelled out here a third time (the note above that kernel says why it is not a
// callable); what happens at a point is this file's own.  The parameter checks, the solve and the selection are host-only: sharp_solve.cpp
// (sharp.h).
#include "common.h"
#include "sharp.h"
#include "hmath.h"
#include "mosaic_frame.h"
#include "stats_tiles.h"
#include <algorithm>
#include <cstddef>

namespace {

using namespace mi_sharp;

__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off);
    return v;
}

// tie_refine.hip's tie_gray: the integer gray of a B, G, R sample
__device__ __forceinline__ int sharp_gray(unsigned b, unsigned g, unsigned r) { return (int)((1868u * b + 9617u * g + 4899u * r + 8192u) >> 14); }

// the gray of frame f's sample at a source coordinate frame_src gave and src_inside accepted
__device__ __forceinline__ int gray_at(const FrameDev& f, float xs, float ys) {
    unsigned b, g, r;
    frame_sample3(f, xs, ys, b, g, r);
    return sharp_gray(b, g, r);
}

// Frame f at canvas pixel (x, y): whether it has a Laplacian there and, if so, L and the centre gray gc.  The five pixels must lie in the
// frame's clipped canvas box (which lies in the canvas: this is also 1 <= x <= cw - 2, 1 <= y <= ch - 2) and map into [0, w - 1) x [0, h - 1).
// Every source coordinate is the render's for its own integer pixel: (float)xD - dGx, (float)yD - dGy, then frame_src.
__device__ __forceinline__ bool frame_laplacian(const FrameDev& f, float w1, float h1, int x, int y, float dGx, float dGy, int& L, int& gc) {
    if (x - 1 < f.begX || x + 1 > f.endX || y - 1 < f.begY || y + 1 > f.endY) return false;
    const float xc = (float)x - dGx, xw = (float)(x - 1) - dGx, xe = (float)(x + 1) - dGx;
    const float yc = (float)y - dGy, yn = (float)(y - 1) - dGy, ys = (float)(y + 1) - dGy;
    float sx0, sy0, sx1, sy1, sx2, sy2, sx3, sy3, sx4, sy4;
    frame_src(f, xc, yc, sx0, sy0);
    frame_src(f, xw, yc, sx1, sy1);
    frame_src(f, xe, yc, sx2, sy2);
    frame_src(f, xc, yn, sx3, sy3);
    frame_src(f, xc, ys, sx4, sy4);
    if (!(src_inside(sx0, sy0, w1, h1) && src_inside(sx1, sy1, w1, h1) && src_inside(sx2, sy2, w1, h1) && src_inside(sx3, sy3, w1, h1) &&
          src_inside(sx4, sy4, w1, h1)))
        return false;
    gc = gray_at(f, sx0, sy0);
    L = 4 * gc - gray_at(f, sx1, sy1) - gray_at(f, sx2, sy2) - gray_at(f, sx3, sy3) - gray_at(f, sx4, sy4);
    return true;
}

// pair_acc: 5 accumulators per pair record (n, e_a, e_b, s_a, s_b); frame_acc: 3 per frame (n, e, s), cover tiles only
__global__ __launch_bounds__(256) void sharp_stats_kernel(const FrameDev* fr, const GainTile* tiles, int step, float dGx, float dGy, int cw, int ch,
                                                          unsigned long long* pair_acc, unsigned long long* frame_acc) {
    const GainTile t = tiles[blockIdx.x];
    const int lx = t.lx0 + (threadIdx.x & 63), ly0 = t.ly0 + (threadIdx.x >> 6);
    const FrameDev& fa = fr[t.a];
    const float wa1 = (float)(fa.w - 1), ha1 = (float)(fa.h - 1);
    const int x = lx * step;
    const bool col = lx <= t.lx1 && x >= 1 && x <= cw - 2;
    unsigned v[5] = {0u, 0u, 0u, 0u, 0u};                        // pair: n, e_a, e_b, s_a, s_b; cover: n, e, s
    if (t.b < 0) {
        for (int r = 0; r < GT_Y / 4; r++) {
            const int ly = ly0 + 4 * r, y = ly * step;
            int L, g;
            if (col && ly <= t.ly1 && y >= 1 && y <= ch - 2 && frame_laplacian(fa, wa1, ha1, x, y, dGx, dGy, L, g)) {
                v[0] += 1u; v[1] += (unsigned)(L * L); v[2] += (unsigned)g;
            }
        }
    } else {
        const FrameDev& fb = fr[t.b];
        const float wb1 = (float)(fb.w - 1), hb1 = (float)(fb.h - 1);
        for (int r = 0; r < GT_Y / 4; r++) {
            const int ly = ly0 + 4 * r, y = ly * step;
            int La, ga, Lb, gb;
            if (col && ly <= t.ly1 && y >= 1 && y <= ch - 2 && frame_laplacian(fa, wa1, ha1, x, y, dGx, dGy, La, ga) &&
                frame_laplacian(fb, wb1, hb1, x, y, dGx, dGy, Lb, gb)) {
                v[0] += 1u; v[1] += (unsigned)(La * La); v[2] += (unsigned)(Lb * Lb); v[3] += (unsigned)ga; v[4] += (unsigned)gb;
            }
        }
    }
    __shared__ unsigned s_v[4][5];
    const int nv = t.b < 0 ? 3 : 5;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = 0; i < nv; i++) {
        const unsigned s = wave_sum_u(v[i]);                     // at most 256 x 1020^2 < 2^29 per wave
        if (lane == 0) s_v[wave][i] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < nv) {
        const int i = threadIdx.x;
        const unsigned long long s = (unsigned long long)s_v[0][i] + s_v[1][i] + s_v[2][i] + s_v[3][i];
        if (s != 0) {
            unsigned long long* dst = t.b < 0 ? frame_acc + 3 * (size_t)t.rec + i : pair_acc + 5 * (size_t)t.rec + i;
            atomicAdd(dst, s);
        }
    }
}

int sharp_stats(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s, const int32_t* pairs_ab,
                int n_pairs, int step, mi355_sharp_pair_stats* pair_stats, mi355_sharp_frame_stats* frame_stats) {
    if (n_pairs > 0 && !pair_stats) { ctx->set_error("sharp_stats: NULL argument or n_pairs < 0"); return MI355_ERR_ARG; }
    StatsFrames s;
    { const int rc = stats_setup(ctx, "sharp_stats: ", d_imgs, w, h, ws, n, h9s, pairs_ab, n_pairs, step, nullptr, s); if (rc != MI355_OK) return rc; }
    int cw, ch, cws;
    float dG[2];
    if (mi355_mosaic_layout(w, h, n, h9s, &cw, &ch, &cws, dG) != MI355_OK) { ctx->set_error("sharp_stats: no image with h[8] != 0 / empty canvas"); return MI355_ERR_FAILED; }
    std::vector<GainTile> tiles;
    if (frame_stats) s.push_cover_tiles(tiles, step);
    for (int p = 0; p < n_pairs; p++) s.push_pair_tiles(tiles, pairs_ab[2 * p], pairs_ab[2 * p + 1], p, step);
    const size_t n_acc = (size_t)n_pairs * 5 + (size_t)n * 3;
    DevBuf& dt = ctx->buf("sharp_tiles"); DevBuf& dacc = ctx->buf("sharp_acc");
    MI_HIP(dt.reserve(sizeof(GainTile) * std::max<size_t>(tiles.size(), 1)));
    MI_HIP(dacc.reserve(sizeof(unsigned long long) * n_acc));
    if (!tiles.empty()) MI_HIP(hipMemcpyAsync(dt.p, tiles.data(), sizeof(GainTile) * tiles.size(), hipMemcpyHostToDevice, ctx->stream));
    MI_HIP(hipMemsetAsync(dacc.p, 0, sizeof(unsigned long long) * n_acc, ctx->stream));
    unsigned long long* pair_acc = dacc.as<unsigned long long>();
    unsigned long long* frame_acc = pair_acc + (size_t)n_pairs * 5;
    for (size_t t0 = 0; t0 < tiles.size(); t0 += (size_t)1 << 30) {     // grid.x < 2^31
        const size_t nt = std::min(tiles.size() - t0, (size_t)1 << 30);
        ProfScope ps(ctx, "sharp_stats", 0.0);
        hipLaunchKernelGGL(sharp_stats_kernel, dim3((unsigned)nt), dim3(256), 0, ctx->stream, s.d_fr, dt.as<GainTile>() + t0, step, s.dG[0], s.dG[1], cw, ch,
                           pair_acc, frame_acc);
        MI_HIP(hipGetLastError());
    }
    std::vector<unsigned long long> acc(n_acc);
    MI_HIP(hipMemcpyAsync(acc.data(), dacc.p, sizeof(unsigned long long) * n_acc, hipMemcpyDeviceToHost, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));                 // s.fr / tiles are locals
    for (int p = 0; p < n_pairs; p++) {
        mi355_sharp_pair_stats& st = pair_stats[p];
        const unsigned long long* a = acc.data() + 5 * (size_t)p;
        st.a = pairs_ab[2 * p]; st.b = pairs_ab[2 * p + 1];
        st.n = (int64_t)a[0]; st.e_a = (int64_t)a[1]; st.e_b = (int64_t)a[2]; st.s_a = (int64_t)a[3]; st.s_b = (int64_t)a[4];
    }
    if (frame_stats)
        for (int k = 0; k < n; k++) {
            const unsigned long long* a = acc.data() + (size_t)n_pairs * 5 + 3 * (size_t)k;
            frame_stats[k].n = (int64_t)a[0]; frame_stats[k].e = (int64_t)a[1]; frame_stats[k].s = (int64_t)a[2];
        }
    return MI355_OK;
}

}  // namespace

extern "C" int mi355_sharp_stats_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                     const int32_t* pairs_ab, int n_pairs, int step, mi355_sharp_pair_stats* pair_stats, mi355_sharp_frame_stats* frame_stats) {
    LOCKED_PROLOGUE
    return sharp_stats(ctx, d_imgs, w, h, ws, n, h9s, pairs_ab, n_pairs, step, pair_stats, frame_stats);
}

extern "C" int mi355_sharpness_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                   const int32_t* pairs_ab, int n_pairs, const mi355_sharp_params* p, float* sharp, uint8_t* status) {
    LOCKED_PROLOGUE
    mi355_sharp_params dp;
    if (!p) { mi355_default_sharp_params(&dp); p = &dp; }
    std::string err;
    if (!status) { ctx->set_error("sharpness: NULL argument or n_pairs < 0"); return MI355_ERR_ARG; }
    if (!check_sharp_params(*p, true, err) || !check_frames_n(n, err)) { ctx->set_error("sharpness: " + err); return MI355_ERR_ARG; }
    std::vector<mi355_sharp_pair_stats> st((size_t)std::max(n_pairs, 1));
    int rc = sharp_stats(ctx, d_imgs, w, h, ws, n, h9s, pairs_ab, n_pairs, p->step, st.data(), nullptr);
    if (rc != MI355_OK) return rc;
    rc = select_sharp_frames(st.data(), n_pairs, n, *p, status, sharp, err);
    if (rc != MI355_OK) { ctx->set_error("sharpness: " + err); return rc; }
    return MI355_OK;
}
