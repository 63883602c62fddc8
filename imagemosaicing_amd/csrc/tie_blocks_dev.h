// csrc/tie_blocks_dev.h -- the device skeleton of the tie-driven refinements' block kernels (projective.hip, calib.hip): everything but how
// a tie's two rows are formed, which is the Former's; and the device side of their loops' round trips.  Included by those two units only.
#pragma once
#include "common.h"
#include "tie_blocks.h"

constexpr int TB_CHUNK = 32;                      // ties per pass: lanes 0..31 form image i's side of one tie each, lanes 32..63 image j's

// A wave per pair record, four per workgroup (pair_moments_kernel's launch).  The sums of a block are the lower triangle of X X^T + Y Y^T
// over the ties' rows X[ROW], Y[ROW] (tie_blocks.h); sum s belongs to lane s mod 64 -- a lane owns whole sums and walks the ties in order:
// no atomics, no reduction across lanes.  The rows are expensive (divisions, a fixed point), so they are formed once per tie (one side per
// lane, 32 ties per pass) and passed through LDS: rows[wave][tie] = X | Y.
//
// The barriers: every wave of the workgroup makes the same number of passes, the largest of the four records' counts, which every lane
// finds alike from the four records themselves (Former::count is a function of the arguments and the record alone), and each pass
// reaches both barriers outside any condition.  A wave whose record is shorter, unused or past n walks the passes with live = false.
//
// A Former (one object per lane, built from its Args, the kernel's third argument):
//   ROW, Block      the row length, the output block (N, g, cost as mi_tri_store splits them)
//   count(a, in, p, n)   static: record p's tie count if it is used (p < n), else 0
//   open(in, p, n)       the wave's own record: its state into the lane, -> count(a, in, p, n)
//   form(live, side, kq, k, row)   this lane's half of tie k's rows into row = rows[wave][kq].  All 64 lanes call it in every pass, live or
//                        not: the __shfl between the two sides of a tie are in here
//   head(o, cnt)         lane 0: the block's i, j, n_in and what else leads it
template <class Former>
__global__ __launch_bounds__(256) void tie_blocks_kernel(const mi355_pair_result* in, int n, typename Former::Args a, typename Former::Block* out) {
    constexpr int ROW = Former::ROW, SUMS = ROW * (ROW + 1) / 2, NQ = (SUMS + 63) / 64;
    __shared__ double rows[4][TB_CHUNK][2 * ROW];
    const int wv = threadIdx.x >> 6, t = threadIdx.x & 63, p = blockIdx.x * 4 + wv;
    Former f(a);
    const int cnt = f.open(in, p, n);
    int cmax = 0;                                  // the workgroup's largest count, found by every lane alike
    for (int q = 0; q < 4; q++) {
        const int cq = Former::count(a, in, blockIdx.x * 4 + q, n);
        if (cq > cmax) cmax = cq;
    }
    // this lane's sums: s = t, t + 64, ... (only below SUMS) -> (r, c) of the lower triangle
    int sr[NQ], sc[NQ];
    double acc[NQ];
    for (int q = 0; q < NQ; q++) {
        const int s = t + 64 * q;
        mi_tri_rc(s < SUMS ? s : 0, sr[q], sc[q]);
        acc[q] = 0.0;
    }
    const int side = t >> 5, kq = t & 31;
    for (int k0 = 0; k0 < cmax; k0 += TB_CHUNK) {
        const int k = k0 + kq;
        f.form(k < cnt, side, kq, k, rows[wv][kq]);
        __syncthreads();
        const int m = cnt - k0 < TB_CHUNK ? cnt - k0 : TB_CHUNK;
        for (int kk = 0; kk < m; kk++) {
            const double* X = rows[wv][kk];
            const double* Y = X + ROW;
            for (int q = 0; q < NQ; q++) {
                double v = acc[q];
                v = v + X[sr[q]] * X[sc[q]];
                v = v + Y[sr[q]] * Y[sc[q]];
                acc[q] = v;
            }
        }
        __syncthreads();
    }
    if (p >= n) return;
    typename Former::Block& o = out[p];
    if (t == 0) f.head(o, cnt);
    for (int q = 0; q < NQ; q++) {
        const int s = t + 64 * q;
        if (s >= SUMS) break;
        mi_tri_store<ROW>(o, s, acc[q]);
    }
}

// The device side of a loop over blocks of the accepted records (projective.hip, calib.hip); the caller holds the ctx lock, `prefix` names
// the loop's own ctx buffers.
// the accepted records to the front of `prefix`_compact, once: the trials' launches and copies then walk those alone
inline int mi_compact_for_loop(mi355_ctx* ctx, const std::string& prefix, const mi355_pair_result* d_in, int n, const mi355_pair_result** d_out, int* n_acc) {
    *n_acc = 0;
    DevBuf& dcomp = ctx->buf(prefix + "_compact");
    if (n > 0) {
        DevBuf& dcnt = ctx->buf("ag_res_counts");
        MI_HIP(dcnt.reserve(sizeof(int) * 64));
        MI_HIP(dcomp.reserve(sizeof(mi355_pair_result) * (size_t)n));
        { const int rc = mi_compact_accepted(ctx, d_in, n, dcomp.as<mi355_pair_result>(), dcnt.as<int>()); if (rc != MI355_OK) return rc; }
        MI_HIP(hipMemcpyAsync(n_acc, dcnt.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));
    }
    *d_out = dcomp.as<mi355_pair_result>();
    return MI355_OK;
}
// two byte ranges, one behind the other, into `prefix`_params through pinned memory (the caller's arrays may be gone before the copy runs)
inline int mi_upload_params(mi355_ctx* ctx, const std::string& prefix, const void* a, size_t na, const void* b, size_t nb, uint8_t** d_params) {
    HostBuf& stage = ctx->hbuf(prefix + "_params_host");
    DevBuf& dpar = ctx->buf(prefix + "_params");
    MI_HIP(stage.reserve(na + nb));
    MI_HIP(dpar.reserve(na + nb));
    MI_HIP(hipStreamSynchronize(ctx->stream));            // the previous call's upload has left the staging area
    memcpy(stage.p, a, na);
    memcpy(stage.as<uint8_t>() + na, b, nb);
    MI_HIP(hipMemcpyAsync(dpar.p, stage.p, na + nb, hipMemcpyHostToDevice, ctx->stream));
    *d_params = dpar.as<uint8_t>();
    return MI355_OK;
}
// a trial's blocks: launch(d_blocks) into `prefix`_blocks, one copy into the pinned `prefix`_blocks_host, a synchronise.  nomem: the
// message of MI355_ERR_NOMEM for a failed reserve (NULL: a device error like any other call's)
template <class Block, class Launch>
int mi_blocks_round_trip(mi355_ctx* ctx, const std::string& prefix, int n, const char* nomem, Launch&& launch, const Block** out) {
    DevBuf& dblk = ctx->buf(prefix + "_blocks");
    HostBuf& hblk = ctx->hbuf(prefix + "_blocks_host");
    const size_t bytes = sizeof(Block) * (size_t)(n > 0 ? n : 1);
    if (nomem && (dblk.reserve(bytes) != hipSuccess || hblk.reserve(bytes) != hipSuccess)) { ctx->set_error(nomem); return MI355_ERR_NOMEM; }
    MI_HIP(dblk.reserve(bytes));
    MI_HIP(hblk.reserve(bytes));
    if (n > 0) {
        { const int rc = launch(dblk.as<Block>()); if (rc != MI355_OK) return rc; }
        MI_HIP(hipMemcpyAsync(hblk.p, dblk.p, sizeof(Block) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));
    }
    *out = hblk.as<Block>();
    return MI355_OK;
}
