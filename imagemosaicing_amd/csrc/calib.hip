// csrc/calib.hip -- the device half of the lens self-calibration (include/mi355_mosaic.h, "lens self-calibration"): the normal-equation
// block of every pair record at the current camera and states, and the entry points that run the host loop (calib_solve.cpp) on blocks
// formed here.  Compiled with -ffp-contract=off like the host twin: the same chain of separately rounded double operations per sum
// (calib.h), so the calibration gives the same bits from either.
#include "common.h"
#include "calib.h"

int mi_compact_accepted(mi355_ctx* ctx, const mi355_pair_result* d_in, int n, mi355_pair_result* d_out, int* d_n_out);     // comm.hip

namespace {

constexpr int CB_CHUNK = 32;                      // ties per pass: lanes 0..31 form image i's side of one tie each, lanes 32..63 image j's
constexpr int CB_LD = 2 * MI_CAL_ROW;             // a tie's rows in LDS: X[14] | Y[14]
constexpr size_t CB_HEAD = 64;                    // a record's bytes in front of its tie lists: i, j, n_in, n_selected, ok, accepted, H[9], _pad
static_assert(offsetof(mi355_pair_result, a) == CB_HEAD && offsetof(mi355_pair_result, H) == 24, "pair record head");

// A wave per pair record, four per workgroup (pair_normal_blocks_kernel's launch).  The 105 sums of a block are the lower triangle of
// X X^T + Y Y^T over the ties' 14-rows; sum s (= r(r+1)/2 + c) belongs to lane s mod 64 -- a lane owns whole sums, up to two, and walks the
// ties in order: no atomics, no reduction across lanes.  The fixed-point undistortion (a division per step) and the 2 x 2 inverse are the
// expensive part, so they are done once per tie and side (one side per lane, 32 ties per pass); image j's lane chains its side through the
// state and hands the projected point and the chained derivatives to image i's lane by __shfl; the rows pass through LDS.  A bad tie's
// rows are zeros, which leave every sum's bits as they are (a sum starts at +0.0 and can never become -0.0).  Every wave of the workgroup
// makes the same number of passes (the largest of the four records'), so the barriers are reached by all.
// cam9: fx, fy, cx, cy, k1, k2, p1, p2, k3; h8: n x 8, one state per record.
__global__ __launch_bounds__(256) void pair_calib_blocks_kernel(const mi355_pair_result* in, int n, const double* h8, const double* cam9, int min_ties,
                                                                mi355_pair_calib_block* out) {
    __shared__ double rows[4][CB_CHUNK][CB_LD];
    const int wv = threadIdx.x >> 6, t = threadIdx.x & 63, p = blockIdx.x * 4 + wv;
    mi355_camera cam;
    cam.fx = cam9[0]; cam.fy = cam9[1]; cam.cx = cam9[2]; cam.cy = cam9[3]; cam.k1 = cam9[4]; cam.k2 = cam9[5]; cam.p1 = cam9[6]; cam.p2 = cam9[7]; cam.k3 = cam9[8];
    int cnt = 0, pi = 0, pj = 0;
    double h[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < n) {
        const mi355_pair_result& e = in[p];
        pi = e.i; pj = e.j;
        for (int k = 0; k < 8; k++) h[k] = h8[(size_t)8 * p + k];
        if (mi_cal_used(e.accepted, e.n_in, pi, pj, min_ties, h)) cnt = e.n_in;
    }
    int cmax = 0;                                  // the workgroup's largest count, found by every lane alike
    for (int q = 0; q < 4; q++) {
        const int pq = blockIdx.x * 4 + q;
        if (pq >= n) continue;
        const mi355_pair_result& e = in[pq];
        if (mi_cal_used(e.accepted, e.n_in, e.i, e.j, min_ties, h8 + (size_t)8 * pq) && e.n_in > cmax) cmax = e.n_in;
    }
    // this lane's sums: s = t and t + 64 (the second only below 105) -> (r, c) of the 14 x 14 lower triangle
    int sr[2], sc[2];
    for (int q = 0; q < 2; q++) {
        int s = t + 64 * q;
        if (s >= MI_CAL_SUMS) s = 0;
        int r = 0;
        while ((r + 1) * (r + 2) / 2 <= s) r++;
        sr[q] = r; sc[q] = s - r * (r + 1) / 2;
    }
    double acc[2] = {0.0, 0.0};
    int n_bad = 0;
    const int side = t >> 5, kq = t & 31;
    for (int k0 = 0; k0 < cmax; k0 += CB_CHUNK) {
        const int k = k0 + kq;
        const bool live = k < cnt;
        CalSide sd;
        sd.x = 0.0; sd.y = 0.0; sd.good = false;
        for (int m = 0; m < 5; m++) { sd.gx[m] = 0.0; sd.gy[m] = 0.0; }
        CalChain ch;
        ch.px = 0.0; ch.py = 0.0; ch.good = false;
        for (int m = 0; m < 5; m++) { ch.cx[m] = 0.0; ch.cy[m] = 0.0; }
        for (int c = 0; c < 8; c++) { ch.X[c] = 0.0; ch.Y[c] = 0.0; }
        if (live) {
            const mi355_pair_result& e = in[p];
            const mi355_sfpoint pt = side ? e.b[k] : e.a[k];
            mi_cal_undistort(cam, (double)pt.x, (double)pt.y, sd);
            if (side) mi_cal_chain(cam, h, sd, ch);
        }
        // image j's side of the same tie to image i's lane, and image i's verdict to image j's lane
        const double px = __shfl(ch.px, kq + 32), py = __shfl(ch.py, kq + 32);
        double cx[5], cy[5];
        for (int m = 0; m < 5; m++) { cx[m] = __shfl(ch.cx[m], kq + 32); cy[m] = __shfl(ch.cy[m], kq + 32); }
        const int good_b = __shfl((int)ch.good, kq + 32), good_a = __shfl((int)sd.good, kq);
        const bool good = good_a && good_b;
        if (live) {
            double* X = rows[wv][kq];
            double* Y = X + MI_CAL_ROW;
            if (side) {
                for (int c = 0; c < 8; c++) { X[c] = good ? ch.X[c] : 0.0; Y[c] = good ? ch.Y[c] : 0.0; }
            } else {
                double xr[6], yr[6];
                mi_cal_close(cam, sd, px, py, cx, cy, xr, yr);
                for (int c = 0; c < 6; c++) { X[8 + c] = good ? xr[c] : 0.0; Y[8 + c] = good ? yr[c] : 0.0; }
            }
        }
        n_bad += __popcll(__ballot(live && side == 0 && !good));
        __syncthreads();
        const int m = cnt - k0 < CB_CHUNK ? cnt - k0 : CB_CHUNK;
        for (int kk = 0; kk < m; kk++) {
            const double* X = rows[wv][kk];
            const double* Y = X + MI_CAL_ROW;
            for (int q = 0; q < 2; q++) {
                double v = acc[q];
                v = v + X[sr[q]] * X[sc[q]];
                v = v + Y[sr[q]] * Y[sc[q]];
                acc[q] = v;
            }
        }
        __syncthreads();
    }
    if (p >= n) return;
    mi355_pair_calib_block& o = out[p];
    if (t == 0) { o.i = pi; o.j = pj; o.n_in = cnt; o.n_bad = n_bad; }
    for (int q = 0; q < 2; q++) {
        const int s = t + 64 * q;
        if (s >= MI_CAL_SUMS) break;
        if (s < 91) o.N[s] = acc[q]; else if (s < 104) o.g[s - 91] = acc[q]; else o.cost = acc[q];
    }
}

// caller holds the ctx lock: states and camera to the device (through pinned memory: the caller's arrays may be gone before the copy runs), one launch
int launch_blocks(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, const double* h8, const mi355_camera& cam, int min_ties, mi355_pair_calib_block* d_out) {
    const size_t hb = sizeof(double) * 8 * (size_t)n, total = hb + sizeof(double) * 9;
    HostBuf& stage = ctx->hbuf("calib_params_host");
    DevBuf& dpar = ctx->buf("calib_params");
    MI_HIP(stage.reserve(total));
    MI_HIP(dpar.reserve(total));
    MI_HIP(hipStreamSynchronize(ctx->stream));            // the previous call's upload has left the staging area
    memcpy(stage.p, h8, hb);
    const double c9[9] = {cam.fx, cam.fy, cam.cx, cam.cy, cam.k1, cam.k2, cam.p1, cam.p2, cam.k3};
    memcpy(stage.as<uint8_t>() + hb, c9, sizeof(c9));
    MI_HIP(hipMemcpyAsync(dpar.p, stage.p, total, hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, "calibrate", (double)n * (sizeof(mi355_pair_result) + sizeof(mi355_pair_calib_block)));
        hipLaunchKernelGGL(pair_calib_blocks_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, d_results, n, dpar.as<double>(), dpar.as<double>() + (size_t)8 * n, min_ties, d_out);
    }
    MI_HIP(hipGetLastError());
    return MI355_OK;
}

// the loop's records on the device: per trial one launch and one copy of the blocks into pinned memory of the ctx
struct DevSource : CalibSource {
    mi355_ctx* ctx;
    const mi355_pair_result* d_rec;
    int n;
    int count() override { return n; }
    int fail(std::string& err, int rc) { err = ctx->err; return rc; }
    int heads(CalibHead* out, std::string& err) override {
        HostBuf& hh = ctx->hbuf("calib_heads_host");
        const int rc = copy_heads(hh);
        if (rc != MI355_OK) return fail(err, rc);
        for (int p = 0; p < n; p++) {
            const uint8_t* e = hh.as<uint8_t>() + CB_HEAD * (size_t)p;
            memcpy(&out[p].i, e, sizeof(int32_t) * 3);              // i, j, n_in lead the record
            memcpy(out[p].H, e + offsetof(mi355_pair_result, H), sizeof(float) * 9);
        }
        return MI355_OK;
    }
    int copy_heads(HostBuf& hh) {
        MI_HIP(hh.reserve(CB_HEAD * (size_t)n));
        MI_HIP(hipMemcpy2DAsync(hh.p, CB_HEAD, d_rec, sizeof(mi355_pair_result), CB_HEAD, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));
        return MI355_OK;
    }
    int blocks(const double* h8, const mi355_camera& cam, int min_ties, const mi355_pair_calib_block** out, std::string& err) override {
        const int rc = run(h8, cam, min_ties);
        if (rc != MI355_OK) return fail(err, rc);
        *out = ctx->hbuf("calib_blocks_host").as<mi355_pair_calib_block>();
        return MI355_OK;
    }
    int run(const double* h8, const mi355_camera& cam, int min_ties) {
        DevBuf& dblk = ctx->buf("calib_blocks");
        HostBuf& hblk = ctx->hbuf("calib_blocks_host");
        const size_t bytes = sizeof(mi355_pair_calib_block) * (size_t)n;
        MI_HIP(dblk.reserve(bytes));
        MI_HIP(hblk.reserve(bytes));
        { const int rc = launch_blocks(ctx, d_rec, n, h8, cam, min_ties, dblk.as<mi355_pair_calib_block>()); if (rc != MI355_OK) return rc; }
        MI_HIP(hipMemcpyAsync(hblk.p, dblk.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));
        return MI355_OK;
    }
    int record(int p, mi355_pair_result* out, std::string& err) override {
        const int rc = fetch(p, out);
        return rc == MI355_OK ? rc : fail(err, rc);
    }
    int fetch(int p, mi355_pair_result* out) {
        MI_HIP(hipMemcpyAsync(out, d_rec + p, sizeof(mi355_pair_result), hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));
        return MI355_OK;
    }
};

}  // namespace

extern "C" int mi355_pair_calib_blocks_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, const double* h8, const mi355_camera* cam, int min_ties,
                                           mi355_pair_calib_block* d_out) {
    LOCKED_PROLOGUE
    std::string err;
    { const int rc = mi_calib_check_blocks("pair_calib_blocks_dev", n, d_results, h8, cam, min_ties, d_out, err); if (rc != MI355_OK) { ctx->set_error(err); return rc; } }
    if (n == 0) return MI355_OK;
    return launch_blocks(ctx, d_results, n, h8, *cam, min_ties, d_out);
}

extern "C" int mi355_calibrate_lens_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n_pairs, const mi355_camera* start, const mi355_calib_params* params,
                                        mi355_camera* out, mi355_calib_report* report) {
    LOCKED_PROLOGUE
    std::string err;
    if (n_pairs < 0 || (n_pairs > 0 && !d_results)) {
        ctx->set_error("calibrate_lens_dev: n_pairs = " + std::to_string(n_pairs) + (n_pairs < 0 ? " (not negative)" : " with NULL records"));
        return MI355_ERR_ARG;
    }
    { const int rc = mi_calib_check("calibrate_lens_dev", start, params, err); if (rc != MI355_OK) { ctx->set_error(err); return rc; } }
    if (!out) { ctx->set_error("calibrate_lens_dev: NULL out"); return MI355_ERR_ARG; }
    // the accepted records to the front, once: the trials' launches and copies then walk those alone
    int n_acc = 0;
    DevBuf& dcomp = ctx->buf("calib_compact");
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
    const int rc = mi_calibrate_lens(src, start, params, out, report, err);
    if (rc != MI355_OK) ctx->set_error(err);
    return rc;
}
