// csrc/local_warp.hip -- local registration (gfx950): per-frame residual warps from the tie points (include/mi355_mosaic.h, "local
// registration").  Compiled with -ffp-contract=off: the double chains of a tie are the header's, one rounding per operation, and they are
// ONE piece of source for the kernel and the host twin (lw_tie below); everything summed is an integer, so the order of the sums is free.
//
//   tie_residual_kernel   one workgroup of 256 lanes per pair record, a lane per tie (two passes above 256 ties).  The contributions of the
//                         record's two frames are gathered in LDS (two blocks of 7 NN + 8 64-bit sums, 32 KB at the 16 x 16 grid) with
//                         64-bit integer LDS adds -- a tie touches at most 17 sums per side --, then the non-zero entries are flushed with
//                         one 64-bit global atomic each into the per-frame blocks a hipMemsetAsync cleared.  A record whose ties fall into
//                         a few cells flushes a few dozen atomics instead of 34 per tie; integer adds are exact in any order, so the sums
//                         do not depend on the launch.  Records that are not processed are decided in the first instructions.
//   local_warp_kernel     undistort_kernel's shape (frame_pass.h): one launch over all frames of a call, 256 lanes on 1024 columns x 8
//                         rows, a lane owns 4 adjacent pixels in each row.  The frame's nodes (at most 289 x 2 ints, Q8) are copied to LDS
//                         once per workgroup; the column terms (i0, fx) are formed once per lane with the only two integer divisions, the
//                         row terms (j0, fy) once per row.  Per pixel: four 8-byte LDS reads, the Q24 bilinear form in integers, two f32
//                         multiply-adds, the clamp, texel_sample3.  With displacements of a few pixels the lanes of a wave read the same
//                         nearly contiguous runs of two source rows as undistortion's do.  Clamped pixels are counted per wave.
//   Its floor is HBM: 3 w h bytes read and 3 w h written per frame.
#include "common.h"
#include "envelope_chol.h"
#include "frame_pass.h"
#include "mosaic_frame.h"
#include <cmath>

#define LW_HD __host__ __device__ __forceinline__

namespace {

constexpr int LW_MAX_GRID = 16;
constexpr int LW_MAX_NODES = (LW_MAX_GRID + 1) * (LW_MAX_GRID + 1);
constexpr int LW_MAX_STRIDE = MI355_LOCAL_WARP_STATS_STRIDE(LW_MAX_GRID, LW_MAX_GRID);
constexpr int LW_NT = 256;

struct LwGeo { double H[9], I[9]; int32_t w, h, part, _pad; };
struct LwArgs { int32_t gx, gy, n, stride; double max_res2, max_shift; };
static_assert(sizeof(LwGeo) == 160, "local warp frame record");

// P(M, x, y) of the header; den is returned for the caller's test
LW_HD void lw_map(const double* M, double x, double y, double& X, double& Y, double& den) {
    den = (M[6] * x + M[7] * y) + M[8];
    X = ((M[0] * x + M[1] * y) + M[2]) / den;
    Y = ((M[3] * x + M[4] * y) + M[5]) / den;
}

// where the sums of a frame live in its block
LW_HD int lw_tail(const LwArgs& g) { return 7 * (g.gx + 1) * (g.gy + 1); }

// a kept side in frame k: its 17 sums through add(index in the frame's block, value)
template <class Add> LW_HD void lw_side_sums(const LwArgs& g, const LwGeo& f, double qx, double qy, double dx, double dy, Add& add) {
    const int NX = g.gx + 1, NN = NX * (g.gy + 1);
    const double sx = (qx * (double)g.gx) / (double)(f.w - 1), sy = (qy * (double)g.gy) / (double)(f.h - 1);
    const int cx = min((int)sx, g.gx - 1), cy = min((int)sy, g.gy - 1);
    const int fx = (int)floor((sx - (double)cx) * 256.0 + 0.5), fy = (int)floor((sy - (double)cy) * 256.0 + 0.5);
    const int64_t dqx = (int64_t)floor(dx * 256.0 + 0.5), dqy = (int64_t)floor(dy * 256.0 + 0.5);
    const int64_t w00 = (int64_t)(256 - fx) * (256 - fy), w10 = (int64_t)fx * (256 - fy), w01 = (int64_t)(256 - fx) * fy, w11 = (int64_t)fx * fy;
    const int p00 = cy * NX + cx, p10 = p00 + 1, p01 = p00 + NX, p11 = p01 + 1;
    add(p00, w00 * w00); add(p10, w10 * w10); add(p01, w01 * w01); add(p11, w11 * w11);
    add(NN + p00, w00 * w10); add(NN + p01, w01 * w11);                   // E
    add(2 * NN + p00, w00 * w01); add(2 * NN + p10, w10 * w11);           // S
    add(3 * NN + p00, w00 * w11);                                         // SE
    add(4 * NN + p10, w10 * w01);                                         // SW
    add(5 * NN + p00, w00 * dqx); add(5 * NN + p10, w10 * dqx); add(5 * NN + p01, w01 * dqx); add(5 * NN + p11, w11 * dqx);
    add(6 * NN + p00, w00 * dqy); add(6 * NN + p10, w10 * dqy); add(6 * NN + p01, w01 * dqy); add(6 * NN + p11, w11 * dqy);
    add(7 * NN + 0, 1);
    add(7 * NN + 1, dqx * dqx + dqy * dqy);
}

// one tie of a processed record: the header's steps 1 to 4; addi / addj take the sums of frame i / frame j
template <class Add> LW_HD void lw_tie(const LwArgs& g, const LwGeo& fi, const LwGeo& fj, double ax, double ay, double bx, double by, Add& addi, Add& addj) {
    const int T = lw_tail(g);
    double cix, ciy, cjx, cjy, di, dj;
    lw_map(fi.H, ax, ay, cix, ciy, di);
    lw_map(fj.H, bx, by, cjx, cjy, dj);
    if (!(di > 0.0 && di <= 1.79769313486231570815e308 && dj > 0.0 && dj <= 1.79769313486231570815e308)) { addi(T + 2, 1); addj(T + 2, 1); return; }
    const double rx = cjx - cix, ry = cjy - ciy;
    if (rx * rx + ry * ry > g.max_res2) { addi(T + 3, 1); addj(T + 3, 1); return; }
    const double mx = cix + 0.5 * rx, my = ciy + 0.5 * ry;
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const LwGeo& f = s ? fj : fi;
        Add& add = s ? addj : addi;
        const double px = s ? bx : ax, py = s ? by : ay;
        double qx, qy, dq;
        lw_map(f.I, mx, my, qx, qy, dq);
        const double dx = px - qx, dy = py - qy;
        const bool kept = qx >= 0.0 && qx <= (double)(f.w - 1) && qy >= 0.0 && qy <= (double)(f.h - 1) && fabs(dx) <= g.max_shift && fabs(dy) <= g.max_shift;
        if (kept) lw_side_sums(g, f, qx, qy, dx, dy, add);
        else add(T + 4, 1);
    }
}

LW_HD bool lw_record_ok(int accepted, int n_in, int i, int j, int n) {
    return accepted != 0 && n_in >= 1 && n_in <= MI355_MAX_SELECTED && i >= 0 && j >= 0 && i < n && j < n && i != j;
}

struct LwLdsAdd {
    unsigned long long* base;
    LW_HD void operator()(int idx, int64_t v) const {
#if defined(__HIP_DEVICE_COMPILE__)
        if (v) atomicAdd(base + idx, (unsigned long long)v);
#endif
    }
};
struct LwHostAdd {
    int64_t* base;
    LW_HD void operator()(int idx, int64_t v) const { base[idx] += v; }
};

__global__ __launch_bounds__(LW_NT) void tie_residual_kernel(const mi355_pair_result* recs, const LwGeo* geo, LwArgs g, unsigned long long* stats) {
    __shared__ unsigned long long acc[2][LW_MAX_STRIDE];
    const int rec = blockIdx.x, tid = threadIdx.x;
    const mi355_pair_result& e = recs[rec];
    const int pi = e.i, pj = e.j, nin = e.n_in;
    bool ok = lw_record_ok(e.accepted, nin, pi, pj, g.n);
    if (ok) ok = geo[pi].part != 0 && geo[pj].part != 0;          // the indices are inside the table
    if (!ok) {                                                    // the same in every lane
        if (tid == 0) atomicAdd(stats + (size_t)g.n * (size_t)g.stride, 1ull);
        return;
    }
    for (int q = tid; q < g.stride; q += LW_NT) { acc[0][q] = 0ull; acc[1][q] = 0ull; }
    __syncthreads();
    const LwGeo fi = geo[pi], fj = geo[pj];
    LwLdsAdd addi = {acc[0]}, addj = {acc[1]};
    for (int k = tid; k < nin; k += LW_NT)
        lw_tie(g, fi, fj, (double)e.a[k].x, (double)e.a[k].y, (double)e.b[k].x, (double)e.b[k].y, addi, addj);
    __syncthreads();
    unsigned long long* si = stats + (size_t)pi * (size_t)g.stride;
    unsigned long long* sj = stats + (size_t)pj * (size_t)g.stride;
    for (int q = tid; q < g.stride; q += LW_NT) {
        const unsigned long long vi = acc[0][q], vj = acc[1][q];
        if (vi) atomicAdd(si + q, vi);
        if (vj) atomicAdd(sj + q, vj);
    }
}

__global__ __launch_bounds__(FP_NT) void local_warp_kernel(const PassFrame* frames, int nf, const int2* nodes, int gx, int gy, unsigned long long* n_clamped) {
    __shared__ int2 nd[LW_MAX_NODES];
    // the record of this workgroup's frame: the last one with first_block <= blockIdx.x (first_block ascends); the same in every lane
    int lo = 0, hi = nf - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (frames[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
    const PassFrame f = frames[lo];
    const int NX = gx + 1, NN = NX * (gy + 1);
    for (int q = threadIdx.x; q < NN; q += FP_NT) nd[q] = nodes[(size_t)f.k * (size_t)NN + q];
    __syncthreads();
    const int b = (int)blockIdx.x - f.first_block;
    const int by = b / f.bx_n, bx = b - by * f.bx_n;
    const int u0 = bx * FP_BW + FP_PX * (int)threadIdx.x, v0 = by * FP_ROWS;
    const int wm = f.w - 1, hm = f.h - 1;
    const float w1 = (float)wm, h1 = (float)hm;
    int i0[FP_PX], fx[FP_PX];
#pragma unroll
    for (int i = 0; i < FP_PX; i++) {
        const int x = min(u0 + i, wm);                           // a lane's columns past the row end are not stored; their terms stay in range
        const int num = x * gx;
        i0[i] = min(num / wm, gx - 1);
        fx[i] = ((num - i0[i] * wm) * 256) / wm;
    }
    const bool whole = u0 + FP_PX - 1 < f.w;
    const bool dwords = whole && (((uintptr_t)f.dst | (uintptr_t)(unsigned)f.ws_dst) & 3) == 0;
    const size_t col = 3 * (size_t)u0;
    int cnt = 0;                                                 // clamped pixels of the wave (wave-uniform)
    for (int v = v0; v < v0 + FP_ROWS && v < f.h; v++) {
        const int numy = v * gy;
        const int j0 = min(numy / hm, gy - 1);
        const int fy = ((numy - j0 * hm) * 256) / hm;
        const int2* r0 = nd + j0 * NX;
        const int2* r1 = r0 + NX;
        uint32_t out[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < FP_PX; i++) {
            const int2 n00 = r0[i0[i]], n10 = r0[i0[i] + 1], n01 = r1[i0[i]], n11 = r1[i0[i] + 1];
            const int gxw = 256 - fx[i];
            const int Dx = (256 - fy) * (gxw * n00.x + fx[i] * n10.x) + fy * (gxw * n01.x + fx[i] * n11.x);
            const int Dy = (256 - fy) * (gxw * n00.y + fx[i] * n10.y) + fy * (gxw * n01.y + fx[i] * n11.y);
            const float xr = (float)(u0 + i) + (float)Dx * 0x1p-24f, yr = (float)v + (float)Dy * 0x1p-24f;
            const float xs = xr < 0.0f ? 0.0f : xr > w1 ? w1 : xr, ys = yr < 0.0f ? 0.0f : yr > h1 ? h1 : yr;
            const bool mine = u0 + i < f.w;
            cnt += __popcll(__ballot(mine && (xs != xr || ys != yr)));
            unsigned vb = 0, vg = 0, vr = 0;
            if (mine) {                                          // xs, ys lie in the closed frame: 0 <= xi <= w - 2, 0 <= yi <= h - 2
                const int xi = min((int)xs, f.w - 2), yi = min((int)ys, f.h - 2);
                texel_sample3(f.src, f.w, f.ws_src, xi, yi, ys - (float)yi, xs - (float)xi, vb, vg, vr);
            }
            out[(3 * i) >> 2] |= vb << (8 * ((3 * i) & 3));
            out[(3 * i + 1) >> 2] |= vg << (8 * ((3 * i + 1) & 3));
            out[(3 * i + 2) >> 2] |= vr << (8 * ((3 * i + 2) & 3));
        }
        uint8_t* drow = f.dst + (size_t)v * f.ws_dst + col;
        if (dwords) {
            uint32_t* d32 = reinterpret_cast<uint32_t*>(drow);
            d32[0] = out[0]; d32[1] = out[1]; d32[2] = out[2];
        } else {
#pragma unroll
            for (int j = 0; j < 3 * FP_PX; j++)
                if (u0 + j / 3 < f.w) drow[j] = (uint8_t)(out[j >> 2] >> (8 * (j & 3)));
        }
    }
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_clamped + f.k, (unsigned long long)cnt);
}

// ---- checks ---------------------------------------------------------------------------------------------------------------------------
bool lw_grid_ok(int gx, int gy, std::string& err) {
    if (gx < 1 || gx > LW_MAX_GRID) { err = "grid_x=" + std::to_string(gx) + " outside [1, 16]"; return false; }
    if (gy < 1 || gy > LW_MAX_GRID) { err = "grid_y=" + std::to_string(gy) + " outside [1, 16]"; return false; }
    return true;
}

bool lw_fits(int k, int w, int h, int gx, int gy, std::string& err) {
    if (gx > w - 1) { err = "frame " + std::to_string(k) + ": grid_x=" + std::to_string(gx) + " > w-1=" + std::to_string(w - 1); return false; }
    if (gy > h - 1) { err = "frame " + std::to_string(k) + ": grid_y=" + std::to_string(gy) + " > h-1=" + std::to_string(h - 1); return false; }
    return true;
}

bool lw_params_ok(const mi355_local_warp_params& p, std::string& err) {
    if (!lw_grid_ok(p.grid_x, p.grid_y, err)) return false;
    const double v[4] = {p.max_residual, p.max_shift, p.smooth, p.prior};
    static const char* const names[4] = {"max_residual", "max_shift", "smooth", "prior"};
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(v[i])) { err = std::string(names[i]) + " is not finite"; return false; }
    if (p.max_residual <= 0.0) { err = "max_residual=" + std::to_string(p.max_residual) + " <= 0"; return false; }
    if (p.max_shift <= 0.0 || p.max_shift > 64.0) { err = "max_shift=" + std::to_string(p.max_shift) + " outside (0, 64]"; return false; }
    if (p.smooth < 0.0) { err = "smooth=" + std::to_string(p.smooth) + " < 0"; return false; }
    if (p.prior <= 0.0) { err = "prior=" + std::to_string(p.prior) + " <= 0"; return false; }
    if (p.min_ties < 0) { err = "min_ties=" + std::to_string(p.min_ties) + " < 0"; return false; }
    if (p.reserved != 0) { err = "reserved=" + std::to_string(p.reserved) + " must be 0"; return false; }
    return true;
}

// The frame table of a statistics call: the doubles of h9s, the inverse by the header's formula, who takes part; the checks of the frames
// that do.
bool lw_geometry(const int* w, const int* h, const float* h9s, int n, const mi355_local_warp_params& p, LwGeo* geo, std::string& err) {
    for (int k = 0; k < n; k++) {
        LwGeo& f = geo[k];
        memset(&f, 0, sizeof(f));
        const float* m = h9s + 9 * (size_t)k;
        if (m[8] == 0.0f) continue;
        for (int q = 0; q < 9; q++) f.H[q] = (double)m[q];
        const double a = f.H[0], b = f.H[1], c = f.H[2], d = f.H[3], e = f.H[4], ff = f.H[5], g = f.H[6], hh = f.H[7], i = f.H[8];
        const double A[9] = {e * i - ff * hh, c * hh - b * i, b * ff - c * e, ff * g - d * i, a * i - c * g, c * d - a * ff, d * hh - e * g, b * g - a * hh, a * e - b * d};
        const double det = (a * A[0] + b * A[3]) + c * A[6];
        bool finite = true;
        for (int q = 0; q < 9; q++) { f.I[q] = A[q] / det; finite = finite && std::isfinite(f.I[q]); }
        if (!finite) continue;
        if (!fp_check_size(w[k], h[k], err)) { err = "frame " + std::to_string(k) + ": " + err; return false; }
        if (!lw_fits(k, w[k], h[k], p.grid_x, p.grid_y, err)) return false;
        f.w = w[k]; f.h = h[k]; f.part = 1;
    }
    return true;
}

LwArgs lw_args(const mi355_local_warp_params& p, int n) {
    LwArgs g;
    g.gx = p.grid_x; g.gy = p.grid_y; g.n = n; g.stride = MI355_LOCAL_WARP_STATS_STRIDE(p.grid_x, p.grid_y);
    g.max_res2 = p.max_residual * p.max_residual; g.max_shift = p.max_shift;
    return g;
}

// the checks the statistics entry points share; `p` receives the parameters in force
bool lw_stats_checks(const char* who, int n_pairs, const void* results, const int* w, const int* h, const float* h9s, int n, const void* out,
                     const mi355_local_warp_params* params, mi355_local_warp_params& p, std::string& err) {
    if (params) p = *params; else mi355_default_local_warp_params(&p);
    if (!lw_params_ok(p, err)) { err = std::string(who) + ": " + err; return false; }
    if (n < 0 || n > FP_MAX_FRAMES) { err = std::string(who) + ": n=" + std::to_string(n) + " outside [0, 65535]"; return false; }
    if (n_pairs < 0) { err = std::string(who) + ": n_pairs=" + std::to_string(n_pairs) + " < 0"; return false; }
    const char* null = !out ? "stats" : (n_pairs > 0 && !results) ? "results" : (n > 0 && !w) ? "w" : (n > 0 && !h) ? "h" : (n > 0 && !h9s) ? "h9s" : nullptr;
    if (null) { err = std::string(who) + ": " + null + " is NULL"; return false; }
    return true;
}

// The frame table of a statistics call in the ctx's pinned staging area (valid until the next statistics call): the checks of the frames
// that take part, once per call.  `who` ends in ": ".
int stats_stage(mi355_ctx* ctx, const std::string& who, const int* w, const int* h, const float* h9s, int n, const mi355_local_warp_params& p, const LwGeo*& geo) {
    const size_t gb = sizeof(LwGeo) * (size_t)(n > 0 ? n : 1);
    HostBuf& stage = ctx->hbuf("local_warp_geo_host");
    MI_HIP(stage.reserve(gb));
    MI_HIP(ctx->buf("local_warp_geo").reserve(gb));
    MI_HIP(hipStreamSynchronize(ctx->stream));            // the previous call's upload has left the staging area
    std::string err;
    if (!lw_geometry(w, h, h9s, n, p, stage.as<LwGeo>(), err)) { ctx->set_error(who + err); return MI355_ERR_ARG; }
    geo = stage.as<LwGeo>();
    return MI355_OK;
}

// the staged table to the device, d_stats cleared, one launch over the records
int stats_launch(mi355_ctx* ctx, const mi355_pair_result* d_results, int n_pairs, int n, const mi355_local_warp_params& p, int64_t* d_stats) {
    const LwArgs g = lw_args(p, n);
    MI_HIP(hipMemsetAsync(d_stats, 0, sizeof(int64_t) * ((size_t)n * (size_t)g.stride + 8), ctx->stream));
    if (n_pairs == 0) return MI355_OK;
    DevBuf& dgeo = ctx->buf("local_warp_geo");
    MI_HIP(hipMemcpyAsync(dgeo.p, ctx->hbuf("local_warp_geo_host").p, sizeof(LwGeo) * (size_t)(n > 0 ? n : 1), hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, "tie_residuals", (double)sizeof(mi355_pair_result) * (double)n_pairs);
        hipLaunchKernelGGL(tie_residual_kernel, dim3((unsigned)n_pairs), dim3(LW_NT), 0, ctx->stream, d_results, dgeo.as<LwGeo>(), g,
                           reinterpret_cast<unsigned long long*>(d_stats));
    }
    MI_HIP(hipGetLastError());
    return MI355_OK;
}

int tie_residual_stats(mi355_ctx* ctx, const mi355_pair_result* d_results, int n_pairs, const int* w, const int* h, const float* h9s, int n,
                       const mi355_local_warp_params* params, int64_t* d_stats) {
    mi355_local_warp_params p;
    std::string err;
    if (!lw_stats_checks("tie_residual_stats_dev", n_pairs, d_results, w, h, h9s, n, d_stats, params, p, err)) { ctx->set_error(err); return MI355_ERR_ARG; }
    const LwGeo* geo = nullptr;
    { const int rc = stats_stage(ctx, "tie_residual_stats_dev: ", w, h, h9s, n, p, geo); if (rc != MI355_OK) return rc; }
    return stats_launch(ctx, d_results, n_pairs, n, p, d_stats);
}

// a grid value as its Q8 node (the header's nq); the caller has checked that it is finite and inside [-64, 64]
inline int32_t lw_node_q8(float g) { return (int32_t)std::floor((double)g * 256.0 + 0.5); }

// ---- solve ----------------------------------------------------------------------------------------------------------------------------
// one frame: false when a pivot is not positive
bool lw_solve_frame(const int64_t* s, const mi355_local_warp_params& p, float* grid, mi355_local_warp_report* rep) {
    const int gx = p.grid_x, gy = p.grid_y, NX = gx + 1, NY = gy + 1, NN = NX * NY;
    const int64_t* tail = s + 7 * NN;
    mi355_local_warp_report r;
    memset(&r, 0, sizeof(r));
    r.n_ties = tail[0]; r.rej_den = tail[2]; r.rej_residual = tail[3]; r.rej_side = tail[4];
    for (int q = 0; q < 2 * NN; q++) grid[q] = 0.0f;
    const double nt = (double)tail[0], dd = (double)tail[1] / 65536.0;
    if (tail[0] > 0) r.rms_before = std::sqrt(dd / nt);
    r.rms_after = r.rms_before;
    bool ok = true;
    if (tail[0] >= (int64_t)(p.min_ties > 1 ? p.min_ties : 1)) {
        const int bw = NX + 1;
        const size_t W = (size_t)bw + 1;
        std::vector<double> Nb((size_t)NN * W, 0.0), gxs((size_t)NN), gys((size_t)NN);
        std::vector<int> fst((size_t)NN);
        auto at = [&](int i, int j) -> double& { return Nb[(size_t)i * W + (size_t)(j - i + bw)]; };       // j <= i
        const double k32 = 4294967296.0, k24 = 16777216.0;
        for (int v = 0; v < NY; v++)
            for (int u = 0; u < NX; u++) {
                const int q = v * NX + u;
                fst[q] = q > bw ? q - bw : 0;
                const int deg = (u > 0) + (u < gx) + (v > 0) + (v < gy);
                at(q, q) = ((double)s[q] / k32 + p.smooth * (double)deg) + p.prior;
                if (u < gx) at(q + 1, q) = (double)s[NN + q] / k32 - p.smooth;
                if (v < gy) at(q + NX, q) = (double)s[2 * NN + q] / k32 - p.smooth;
                if (u < gx && v < gy) at(q + NX + 1, q) = (double)s[3 * NN + q] / k32;
                if (u > 0 && v < gy) at(q + NX - 1, q) = (double)s[4 * NN + q] / k32;
                gxs[q] = (double)s[5 * NN + q] / k24;
                gys[q] = (double)s[6 * NN + q] / k24;
            }
        const std::vector<double> bxs = gxs, bys = gys;
        ok = envelope_cholesky(Nb.data(), NN, bw, fst);
        if (ok) {
            envelope_solve(Nb.data(), NN, bw, fst, gxs.data(), gys.data());
            // the fit's residual at the ties: dd - 2 g.b + g^T S g over both components
            double quad = 0.0, lin = 0.0;
            for (int c = 0; c < 2; c++) {
                const double* gq = c ? gys.data() : gxs.data();
                const double* bq = c ? bys.data() : bxs.data();
                for (int v = 0; v < NY; v++)
                    for (int u = 0; u < NX; u++) {
                        const int q = v * NX + u;
                        lin += gq[q] * bq[q];
                        double off = 0.0;
                        if (u < gx) off += ((double)s[NN + q] / k32) * gq[q + 1];
                        if (v < gy) off += ((double)s[2 * NN + q] / k32) * gq[q + NX];
                        if (u < gx && v < gy) off += ((double)s[3 * NN + q] / k32) * gq[q + NX + 1];
                        if (u > 0 && v < gy) off += ((double)s[4 * NN + q] / k32) * gq[q + NX - 1];
                        quad += gq[q] * (((double)s[q] / k32) * gq[q] + 2.0 * off);
                    }
            }
            const double res = (dd - 2.0 * lin) + quad;
            r.rms_after = std::sqrt((res > 0.0 ? res : 0.0) / nt);
            double big = 0.0;
            for (int q = 0; q < NN; q++) {
                const double cx = gxs[q] < -p.max_shift ? -p.max_shift : gxs[q] > p.max_shift ? p.max_shift : gxs[q];
                const double cy = gys[q] < -p.max_shift ? -p.max_shift : gys[q] > p.max_shift ? p.max_shift : gys[q];
                grid[2 * q] = (float)cx; grid[2 * q + 1] = (float)cy;
                big = std::fmax(big, std::fmax(std::fabs((double)grid[2 * q]), std::fabs((double)grid[2 * q + 1])));
            }
            r.max_shift = big;
            r.solved = 1;
        }
    }
    if (rep) *rep = r;
    return ok;
}

int lw_solve(const int64_t* stats, int n, const mi355_local_warp_params& p, float* grids, mi355_local_warp_report* report, std::string& err) {
    const int NN = (p.grid_x + 1) * (p.grid_y + 1), stride = MI355_LOCAL_WARP_STATS_STRIDE(p.grid_x, p.grid_y);
    for (int k = 0; k < n; k++) {
        const int64_t* s = stats + (size_t)k * stride;
        for (int q = 0; q < 5 * NN; q++)
            if (s[q] < 0) { err = "frame " + std::to_string(k) + ": weight sum " + std::to_string(q) + " is negative"; return MI355_ERR_ARG; }
        for (int q = 0; q < 5; q++)
            if (s[7 * NN + q] < 0) { err = "frame " + std::to_string(k) + ": count " + std::to_string(q) + " is negative"; return MI355_ERR_ARG; }
    }
    std::vector<char> bad((size_t)n, 0);
    parallel_chunks((size_t)n, host_threads(), [&](size_t lo, size_t hi) {
        for (size_t k = lo; k < hi; k++)
            bad[k] = !lw_solve_frame(stats + k * (size_t)stride, p, grids + k * 2 * (size_t)NN, report ? report + k : nullptr);
    });
    for (int k = 0; k < n; k++)
        if (bad[k]) { err = "frame " + std::to_string(k) + ": the system is not positive definite in double"; return MI355_ERR_FAILED; }
    return MI355_OK;
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------------
int apply_local_warps(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws_src, const int* ws_dst, int n,
                      int grid_x, int grid_y, const float* grids, int64_t* n_clamped) {
    const std::string who = "apply_local_warps: ";
    std::string err;
    if (n < 0 || n > FP_MAX_FRAMES) { ctx->set_error(who + "n=" + std::to_string(n) + " outside [0, 65535]"); return MI355_ERR_ARG; }
    if (!lw_grid_ok(grid_x, grid_y, err)) { ctx->set_error(who + err); return MI355_ERR_ARG; }
    if (n == 0) return MI355_OK;
    if (!grids) { ctx->set_error(who + "grids is NULL"); return MI355_ERR_ARG; }
    const int NN = (grid_x + 1) * (grid_y + 1);
    std::vector<int32_t> nq((size_t)n * 2 * NN);
    for (size_t q = 0; q < nq.size(); q++) {
        const double g = (double)grids[q];
        if (!std::isfinite(g) || g < -64.0 || g > 64.0) {
            ctx->set_error(who + "frame " + std::to_string(q / (2 * (size_t)NN)) + ": grid value " + std::to_string(q % (2 * (size_t)NN)) + " is not finite or outside [-64, 64]");
            return MI355_ERR_ARG;
        }
        nq[q] = lw_node_q8(grids[q]);
    }
    if (w && h)
        for (int k = 0; k < n; k++)
            if (fp_check_size(w[k], h[k], err) && !lw_fits(k, w[k], h[k], grid_x, grid_y, err)) { ctx->set_error(who + err); return MI355_ERR_ARG; }
    unsigned long long* d_cnt = nullptr;
    const int2* d_nodes = nullptr;
    return fp_run_frames(ctx, who, "local_warp", d_src, d_dst, w, h, ws_src, ws_dst, n, n_clamped,
                         [&]() {
                             DevBuf& dn = ctx->buf("local_warp_nodes");
                             MI_HIP(dn.reserve(sizeof(int32_t) * nq.size()));
                             MI_HIP(hipMemcpyAsync(dn.p, nq.data(), sizeof(int32_t) * nq.size(), hipMemcpyHostToDevice, ctx->stream));
                             MI_HIP(hipStreamSynchronize(ctx->stream));          // nq is this call's local
                             d_nodes = dn.as<int2>();
                             d_cnt = ctx->buf("local_warp_outside").as<unsigned long long>();
                             return (int)MI355_OK;
                         },
                         [&](const PassFrame* table, int nf, int blocks, double bytes) {
                             ProfScope ps(ctx, "local_warp", bytes);
                             hipLaunchKernelGGL(local_warp_kernel, dim3((unsigned)blocks), dim3(FP_NT), 0, ctx->stream, table, nf, d_nodes, grid_x, grid_y, d_cnt);
                         });
}

}  // namespace

extern "C" void mi355_default_local_warp_params(mi355_local_warp_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->grid_x = 8; p->grid_y = 6; p->min_ties = 8;
    p->max_residual = 8.0; p->max_shift = 8.0; p->smooth = 2.0; p->prior = 0.25;
}

extern "C" int mi355_tie_residual_stats_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n_pairs, const int* w, const int* h, const float* h9s, int n,
                                            const mi355_local_warp_params* p, int64_t* d_stats) {
    LOCKED_PROLOGUE
    return tie_residual_stats(ctx, d_results, n_pairs, w, h, h9s, n, p, d_stats);
}

extern "C" int mi355_tie_residual_stats_host(const mi355_pair_result* results, int n_pairs, const int* w, const int* h, const float* h9s, int n,
                                             const mi355_local_warp_params* params, int64_t* stats) {
    mi355_local_warp_params p;
    std::string err;
    if (!lw_stats_checks("tie_residual_stats_host", n_pairs, results, w, h, h9s, n, stats, params, p, err)) { mi_set_host_error(err); return MI355_ERR_ARG; }
    std::vector<LwGeo> geo((size_t)(n > 0 ? n : 1));
    if (!lw_geometry(w, h, h9s, n, p, geo.data(), err)) { mi_set_host_error("tie_residual_stats_host: " + err); return MI355_ERR_ARG; }
    const LwArgs g = lw_args(p, n);
    memset(stats, 0, sizeof(int64_t) * ((size_t)n * (size_t)g.stride + 8));
    for (int r = 0; r < n_pairs; r++) {
        const mi355_pair_result& e = results[r];
        if (!lw_record_ok(e.accepted, e.n_in, e.i, e.j, n) || !geo[e.i].part || !geo[e.j].part) { stats[(size_t)n * g.stride]++; continue; }
        LwHostAdd addi = {stats + (size_t)e.i * g.stride}, addj = {stats + (size_t)e.j * g.stride};
        for (int k = 0; k < e.n_in; k++)
            lw_tie(g, geo[e.i], geo[e.j], (double)e.a[k].x, (double)e.a[k].y, (double)e.b[k].x, (double)e.b[k].y, addi, addj);
    }
    return MI355_OK;
}

extern "C" int mi355_solve_local_warps(const int64_t* stats, int n, const mi355_local_warp_params* params, float* grids, mi355_local_warp_report* report) {
    mi355_local_warp_params p;
    if (params) p = *params; else mi355_default_local_warp_params(&p);
    std::string err;
    if (!lw_params_ok(p, err)) { mi_set_host_error("solve_local_warps: " + err); return MI355_ERR_ARG; }
    if (n < 0 || n > FP_MAX_FRAMES) { mi_set_host_error("solve_local_warps: n=" + std::to_string(n) + " outside [0, 65535]"); return MI355_ERR_ARG; }
    if (n == 0) return MI355_OK;
    if (!stats || !grids) { mi_set_host_error(std::string("solve_local_warps: ") + (!stats ? "stats" : "grids") + " is NULL"); return MI355_ERR_ARG; }
    const int rc = lw_solve(stats, n, p, grids, report, err);
    if (rc != MI355_OK) mi_set_host_error("solve_local_warps: " + err);
    return rc;
}

extern "C" int mi355_apply_local_warps_dev(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws_src,
                                           const int* ws_dst, int n, int grid_x, int grid_y, const float* grids, int64_t* n_clamped) {
    LOCKED_PROLOGUE
    return apply_local_warps(ctx, d_src, d_dst, w, h, ws_src, ws_dst, n, grid_x, grid_y, grids, n_clamped);
}

// caller holds the ctx lock; host_results: the records are on the host and are uploaded after the checks
static int local_register(mi355_ctx* ctx, const mi355_pair_result* d_results, bool host_results, int n_pairs, uint8_t* const* d_imgs, const int* w, const int* h,
                          const int* ws, int n, const float* h9s, const mi355_local_warp_params* params, float* grids_out, mi355_local_warp_report* report_out) {
    const std::string who = "local_register: ";
    mi355_local_warp_params p;
    if (params) p = *params; else mi355_default_local_warp_params(&p);
    std::string err;
    if (!lw_params_ok(p, err)) { ctx->set_error(who + err); return MI355_ERR_ARG; }
    if (n < 0 || n > FP_MAX_FRAMES) { ctx->set_error(who + "n=" + std::to_string(n) + " outside [0, 65535]"); return MI355_ERR_ARG; }
    if (n_pairs < 0) { ctx->set_error(who + "n_pairs=" + std::to_string(n_pairs) + " < 0"); return MI355_ERR_ARG; }
    if (n == 0) return MI355_OK;
    if (!d_imgs || !w || !h || !ws || !h9s || (n_pairs > 0 && !d_results)) {
        ctx->set_error(who + (!d_imgs ? "d_imgs" : !w ? "w" : !h ? "h" : !ws ? "ws" : !h9s ? "h9s" : "d_results") + " is NULL");
        return MI355_ERR_ARG;
    }
    // the frame table, once; the frames that take part must be there before anything runs
    const LwGeo* geo = nullptr;
    { const int rc = stats_stage(ctx, who, w, h, h9s, n, p, geo); if (rc != MI355_OK) return rc; }
    for (int k = 0; k < n; k++) {
        if (!geo[k].part) continue;
        if (!d_imgs[k]) { ctx->set_error(who + "frame " + std::to_string(k) + ": d_imgs is NULL"); return MI355_ERR_ARG; }
        if (ws[k] < 3 * w[k]) { ctx->set_error(who + "frame " + std::to_string(k) + ": ws=" + std::to_string(ws[k]) + " < 3 w=" + std::to_string(3 * w[k])); return MI355_ERR_ARG; }
    }
    if (host_results && n_pairs > 0) {
        DevBuf& drec = ctx->buf("local_warp_records");
        MI_HIP(drec.reserve(sizeof(mi355_pair_result) * (size_t)n_pairs));
        MI_HIP(hipMemcpyAsync(drec.p, d_results, sizeof(mi355_pair_result) * (size_t)n_pairs, hipMemcpyHostToDevice, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));            // the caller's records may be pageable
        d_results = drec.as<mi355_pair_result>();
    }
    const int stride = MI355_LOCAL_WARP_STATS_STRIDE(p.grid_x, p.grid_y), NN = (p.grid_x + 1) * (p.grid_y + 1);
    const size_t nvals = (size_t)n * (size_t)stride + 8;
    DevBuf& dst = ctx->buf("local_warp_stats");
    MI_HIP(dst.reserve(sizeof(int64_t) * nvals));
    { const int rc = stats_launch(ctx, d_results, n_pairs, n, p, dst.as<int64_t>()); if (rc != MI355_OK) return rc; }
    std::vector<int64_t> stats(nvals);
    MI_HIP(hipMemcpyAsync(stats.data(), dst.p, sizeof(int64_t) * nvals, hipMemcpyDeviceToHost, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<float> grids((size_t)n * 2 * NN);
    std::vector<mi355_local_warp_report> rep((size_t)n);
    { const int rc = lw_solve(stats.data(), n, p, grids.data(), rep.data(), err); if (rc != MI355_OK) { ctx->set_error(who + err); return rc; } }
    // in place on the frames with a non-zero Q8 node: nodes that are all zero are the identity, byte for byte (the solve's values lie
    // inside [-max_shift, max_shift])
    std::vector<const uint8_t*> src; std::vector<uint8_t*> dstp; std::vector<int> ww, hh, pitch; std::vector<float> gsel;
    for (int k = 0; k < n; k++) {
        bool any = false;
        for (int q = 0; q < 2 * NN; q++) any = any || lw_node_q8(grids[(size_t)k * 2 * NN + q]) != 0;
        if (!any) continue;
        src.push_back(d_imgs[k]); dstp.push_back(d_imgs[k]); ww.push_back(w[k]); hh.push_back(h[k]); pitch.push_back(ws[k]);
        gsel.insert(gsel.end(), grids.begin() + (size_t)k * 2 * NN, grids.begin() + (size_t)(k + 1) * 2 * NN);
    }
    if (!src.empty()) {
        const int rc = apply_local_warps(ctx, src.data(), dstp.data(), ww.data(), hh.data(), pitch.data(), pitch.data(), (int)src.size(), p.grid_x, p.grid_y, gsel.data(), nullptr);
        if (rc != MI355_OK) return rc;
    }
    if (grids_out) memcpy(grids_out, grids.data(), sizeof(float) * grids.size());
    if (report_out) memcpy(report_out, rep.data(), sizeof(mi355_local_warp_report) * rep.size());
    return MI355_OK;
}

extern "C" int mi355_local_register_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n_pairs, uint8_t* const* d_imgs, const int* w, const int* h,
                                        const int* ws, int n, const float* h9s, const mi355_local_warp_params* params, float* grids_out,
                                        mi355_local_warp_report* report_out) {
    LOCKED_PROLOGUE
    return local_register(ctx, d_results, false, n_pairs, d_imgs, w, h, ws, n, h9s, params, grids_out, report_out);
}

extern "C" int mi355_local_register_results(mi355_ctx* ctx, const mi355_pair_result* results, int n_pairs, uint8_t* const* d_imgs, const int* w, const int* h,
                                            const int* ws, int n, const float* h9s, const mi355_local_warp_params* params, float* grids_out,
                                            mi355_local_warp_report* report_out) {
    LOCKED_PROLOGUE
    return local_register(ctx, results, true, n_pairs, d_imgs, w, h, ws, n, h9s, params, grids_out, report_out);
}
