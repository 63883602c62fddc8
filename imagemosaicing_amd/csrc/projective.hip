// csrc/projective.hip -- the device half of the projective refinement (include/mi355_mosaic.h, "projective refinement of the global
// alignment"): the normal-equation block of every pair record at the current parameters, and the entry points that run the host loop
// (projective_solve.cpp) on blocks formed here.  Compiled with -ffp-contract=off like the host twin: the same chain of separately rounded
// double operations per sum, so the refinement gives the same bits from either.
#include "common.h"
#include "projective.h"

int mi_compact_accepted(mi355_ctx* ctx, const mi355_pair_result* d_in, int n, mi355_pair_result* d_out, int* d_n_out);     // comm.hip

namespace {

constexpr int PJ_CHUNK = 32;                      // inliers per pass: lanes 0..31 form image i's side of one inlier each, lanes 32..63 image j's
constexpr int PJ_LD = 2 * MI_PROJ_ROW;            // an inlier's rows in LDS: X[17] | Y[17]

// A wave per pair record, four per workgroup (pair_moments_kernel's launch).  The 153 sums of a block are the lower triangle of
// X X^T + Y Y^T over the inliers' 17-rows X = [Rx | rx], Y = [Ry | ry]; sum s (= r(r+1)/2 + c) belongs to lane s mod 64 -- a lane owns whole
// sums, up to three, and walks the inliers in order: no atomics, no reduction across lanes.  The rows cost ten f64 divisions per inlier, so
// they are formed once per inlier (one side per lane, 32 inliers per pass) and passed through LDS; every wave of the workgroup makes the
// same number of passes (the largest of the four records'), so the barriers are reached by all.
__global__ __launch_bounds__(256) void pair_normal_blocks_kernel(const mi355_pair_result* in, int n, const double* h8, const uint8_t* part, int n_images,
                                                                 mi355_pair_normal_block* out) {
    __shared__ double rows[4][PJ_CHUNK][PJ_LD];
    const int wv = threadIdx.x >> 6, t = threadIdx.x & 63, p = blockIdx.x * 4 + wv;
    int cnt = 0, keep = 0, pi = 0, pj = 0;
    if (p < n) {
        const mi355_pair_result& e = in[p];
        pi = e.i; pj = e.j;
        if (mi_proj_used(e.accepted, e.n_in, pi, pj, part, n_images, &keep)) cnt = e.n_in;
    }
    int cmax = 0;                                  // the workgroup's largest count, found by every lane alike
    for (int q = 0; q < 4; q++) {
        const int pq = blockIdx.x * 4 + q;
        if (pq >= n) continue;
        const mi355_pair_result& e = in[pq];
        int kq = 0;
        if (mi_proj_used(e.accepted, e.n_in, e.i, e.j, part, n_images, &kq) && e.n_in > cmax) cmax = e.n_in;
    }
    // this lane's sums: s = t, t + 64, t + 128 (the last only below 153) -> (r, c) of the 17 x 17 lower triangle
    int sr[3], sc[3];
    for (int q = 0; q < 3; q++) {
        int s = t + 64 * q;
        if (s >= MI_PROJ_SUMS) s = 0;
        int r = 0;
        while ((r + 1) * (r + 2) / 2 <= s) r++;
        sr[q] = r; sc[q] = s - r * (r + 1) / 2;
    }
    double acc[3] = {0.0, 0.0, 0.0};
    const int side = t >> 5, kq = t & 31;
    for (int k0 = 0; k0 < cmax; k0 += PJ_CHUNK) {
        const int k = k0 + kq;
        double U = 0.0, V = 0.0;
        if (k < cnt) {
            const mi355_pair_result& e = in[p];
            const mi355_sfpoint pt = side ? e.b[k] : e.a[k];
            double* X = rows[wv][kq] + 8 * side;
            mi_proj_side(h8 + (size_t)8 * (side ? pj : pi), (double)pt.x, (double)pt.y, side ? -1.0 : 1.0, X, X + MI_PROJ_ROW, U, V);
        }
        const double Ub = __shfl(U, kq + 32), Vb = __shfl(V, kq + 32);      // image j's side of the same inlier
        if (k < cnt && side == 0) { rows[wv][kq][16] = Ub - U; rows[wv][kq][MI_PROJ_ROW + 16] = Vb - V; }
        __syncthreads();
        const int m = cnt - k0 < PJ_CHUNK ? cnt - k0 : PJ_CHUNK;
        for (int kk = 0; kk < m; kk++) {
            const double* X = rows[wv][kk];
            const double* Y = X + MI_PROJ_ROW;
            for (int q = 0; q < 3; q++) {
                double v = acc[q];
                v = v + X[sr[q]] * X[sc[q]];
                v = v + Y[sr[q]] * Y[sc[q]];
                acc[q] = v;
            }
        }
        __syncthreads();
    }
    if (p >= n) return;
    mi355_pair_normal_block& o = out[p];
    if (t == 0) { o.i = pi; o.j = pj; o.n_in = keep; o._pad = 0; }
    for (int q = 0; q < 3; q++) {
        const int s = t + 64 * q;
        if (s >= MI_PROJ_SUMS) break;
        if (s < 136) o.N[s] = acc[q]; else if (s < 152) o.g[s - 136] = acc[q]; else o.cost = acc[q];
    }
}
static_assert(sizeof(mi355_pair_normal_block) == 1240, "normal block record");

// caller holds the ctx lock: parameters and flags to the device (through pinned memory: the caller's arrays may be gone before the copy runs), one launch
int launch_blocks(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, const double* h8, const uint8_t* part, int n_images, mi355_pair_normal_block* d_out) {
    const size_t hb = sizeof(double) * 8 * (size_t)n_images, total = hb + (size_t)n_images;
    HostBuf& stage = ctx->hbuf("proj_params_host");
    DevBuf& dpar = ctx->buf("proj_params");
    MI_HIP(stage.reserve(total));
    MI_HIP(dpar.reserve(total));
    MI_HIP(hipStreamSynchronize(ctx->stream));            // the previous call's upload has left the staging area
    memcpy(stage.p, h8, hb);
    memcpy(stage.as<uint8_t>() + hb, part, (size_t)n_images);
    MI_HIP(hipMemcpyAsync(dpar.p, stage.p, total, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(pair_normal_blocks_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, d_results, n, dpar.as<double>(), dpar.as<uint8_t>() + hb, n_images, d_out);
    MI_HIP(hipGetLastError());
    return MI355_OK;
}

// the loop's blocks from the device: per trial one launch and one copy into pinned memory of the ctx
struct DevSource : ProjectiveSource {
    mi355_ctx* ctx;
    const mi355_pair_result* d_rec;
    int n;
    int blocks(const double* h8, const uint8_t* part, int n_images, const mi355_pair_normal_block** out, int* n_out, std::string& err) override {
        DevBuf& dblk = ctx->buf("proj_blocks");
        HostBuf& hblk = ctx->hbuf("proj_blocks_host");
        const size_t bytes = sizeof(mi355_pair_normal_block) * (size_t)(n > 0 ? n : 1);
        int rc = MI355_OK;
        if (dblk.reserve(bytes) != hipSuccess || hblk.reserve(bytes) != hipSuccess) { ctx->set_error("projective_refine_dev: no memory for the blocks"); rc = MI355_ERR_NOMEM; }
        if (rc == MI355_OK && n > 0) {
            rc = launch_blocks(ctx, d_rec, n, h8, part, n_images, dblk.as<mi355_pair_normal_block>());
            if (rc == MI355_OK) rc = copy_back(dblk, hblk, sizeof(mi355_pair_normal_block) * (size_t)n);
        }
        if (rc != MI355_OK) { err = ctx->err; return rc; }
        *out = hblk.as<mi355_pair_normal_block>(); *n_out = n;
        return MI355_OK;
    }
    int copy_back(DevBuf& d, HostBuf& hb, size_t bytes) {
        MI_HIP(hipMemcpyAsync(hb.p, d.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));
        return MI355_OK;
    }
};

}  // namespace

extern "C" int mi355_pair_normal_blocks_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, const double* h8, const uint8_t* part, int n_images,
                                            mi355_pair_normal_block* d_out) {
    LOCKED_PROLOGUE
    if (n < 0 || n_images < 1 || !h8 || !part || (n > 0 && (!d_results || !d_out))) { ctx->set_error("pair_normal_blocks_dev: bad arguments (n, n_images or a NULL pointer)"); return MI355_ERR_ARG; }
    if (n == 0) return MI355_OK;
    return launch_blocks(ctx, d_results, n, h8, part, n_images, d_out);
}

extern "C" int mi355_global_projective_refine_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n_pairs, int n_images, const int32_t* w, const int32_t* h,
                                                  const int32_t* fixed, const int32_t* label, const mi355_image_transform* start, const mi355_projective_params* params,
                                                  mi355_image_transform* out, mi355_projective_report* report) {
    LOCKED_PROLOGUE
    std::string err;
    if (n_pairs < 0 || (n_pairs > 0 && !d_results)) { ctx->set_error("projective_refine_dev: n_pairs = " + std::to_string(n_pairs) + " or NULL records"); return MI355_ERR_ARG; }
    { const int rc = mi_projective_check(n_images, w, h, start, params, out, err); if (rc != MI355_OK) { ctx->set_error(err); return rc; } }
    // the accepted records to the front, once: the trials' launches and copies then walk those alone
    int n_acc = 0;
    DevBuf& dcomp = ctx->buf("proj_compact");
    if (n_pairs > 0) {
        DevBuf& dcnt = ctx->buf("ag_res_counts");
        MI_HIP(dcnt.reserve(sizeof(int) * 64));
        MI_HIP(dcomp.reserve(sizeof(mi355_pair_result) * (size_t)n_pairs));
        { const int rc = mi_compact_accepted(ctx, d_results, n_pairs, dcomp.as<mi355_pair_result>(), dcnt.as<int>()); if (rc != MI355_OK) return rc; }
        MI_HIP(hipMemcpyAsync(&n_acc, dcnt.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));
    }
    DevSource src;
    src.ctx = ctx; src.d_rec = dcomp.as<mi355_pair_result>(); src.n = n_acc;
    const int rc = mi_projective_refine(src, n_images, w, h, fixed, label, start, params, out, report, err);
    if (rc != MI355_OK) ctx->set_error(err);
    return rc;
}
