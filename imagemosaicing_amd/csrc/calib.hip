// csrc/calib.hip -- the device half of the lens self-calibration (include/mi355_mosaic.h, "lens self-calibration"): the normal-equation
// block of every pair record at the current camera and states, and the entry points that run the host loop (calib_solve.cpp) on blocks
// formed here.  Compiled with -ffp-contract=off like the host twin: the same chain of separately rounded double operations per sum
// (calib.h), so the calibration gives the same bits from either.
#include "tie_blocks_dev.h"
#include "calib.h"

namespace {

constexpr size_t CB_HEAD = 64;                    // a record's bytes in front of its tie lists: i, j, n_in, n_selected, ok, accepted, H[9], _pad
static_assert(offsetof(mi355_pair_result, a) == CB_HEAD && offsetof(mi355_pair_result, H) == 24, "pair record head");

// The rows of tie_blocks_kernel for the calibration: the 14-rows of calib.h.  The fixed-point undistortion (a division per step) and the
// 2 x 2 inverse are the expensive part, so they are done once per tie and side; image j's lane chains its side through the state and hands
// the projected point and the chained derivatives to image i's lane by __shfl.  A bad tie's rows are zeros, which leave every sum's bits
// as they are (a sum starts at +0.0 and can never become -0.0).
// Args: cam9 = fx, fy, cx, cy, k1, k2, p1, p2, k3; h8: n x 8, one state per record.
struct CalibFormer {
    static constexpr int ROW = MI_CAL_ROW;
    using Block = mi355_pair_calib_block;
    struct Args { const double* h8; const double* cam9; int min_ties; };
    Args a;
    mi355_camera cam;
    const mi355_pair_result* e = nullptr;
    int pi = 0, pj = 0, n_bad = 0;
    double h[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    __device__ __forceinline__ CalibFormer(const Args& a_) : a(a_) {
        const double* c = a.cam9;
        cam.fx = c[0]; cam.fy = c[1]; cam.cx = c[2]; cam.cy = c[3]; cam.k1 = c[4]; cam.k2 = c[5]; cam.p1 = c[6]; cam.p2 = c[7]; cam.k3 = c[8];
    }
    __device__ __forceinline__ static int count(const Args& a, const mi355_pair_result* in, int p, int n) {
        return p < n && mi_cal_used(in[p].accepted, in[p].n_in, in[p].i, in[p].j, a.min_ties, a.h8 + (size_t)8 * p) ? in[p].n_in : 0;
    }
    __device__ __forceinline__ int open(const mi355_pair_result* in, int p, int n) {
        e = in + p;
        if (p >= n) return 0;
        pi = e->i; pj = e->j;
        for (int k = 0; k < 8; k++) h[k] = a.h8[(size_t)8 * p + k];
        return mi_cal_used(e->accepted, e->n_in, pi, pj, a.min_ties, h) ? e->n_in : 0;
    }
    __device__ __forceinline__ void form(bool live, int side, int kq, int k, double* X) {
        CalSide sd = {};                           // zeros and not good: what a lane that is not live hands over
        CalChain ch = {};
        if (live) {
            const mi355_sfpoint pt = side ? e->b[k] : e->a[k];
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
            double* Y = X + ROW;
            if (side) {
                for (int c = 0; c < 8; c++) { X[c] = good ? ch.X[c] : 0.0; Y[c] = good ? ch.Y[c] : 0.0; }
            } else {
                double xr[6], yr[6];
                mi_cal_close(cam, sd, px, py, cx, cy, xr, yr);
                for (int c = 0; c < 6; c++) { X[8 + c] = good ? xr[c] : 0.0; Y[8 + c] = good ? yr[c] : 0.0; }
            }
        }
        n_bad += __popcll(__ballot(live && side == 0 && !good));
    }
    __device__ __forceinline__ void head(Block& o, int cnt) const { o.i = pi; o.j = pj; o.n_in = cnt; o.n_bad = n_bad; }
};

// caller holds the ctx lock: states and camera to the device, one launch
int launch_blocks(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, const double* h8, const mi355_camera& cam, int min_ties, mi355_pair_calib_block* d_out) {
    const size_t hb = sizeof(double) * 8 * (size_t)n;
    const double c9[9] = {cam.fx, cam.fy, cam.cx, cam.cy, cam.k1, cam.k2, cam.p1, cam.p2, cam.k3};
    uint8_t* dpar = nullptr;
    { const int rc = mi_upload_params(ctx, "calib", h8, hb, c9, sizeof(c9), &dpar); if (rc != MI355_OK) return rc; }
    {
        ProfScope ps(ctx, "calibrate", (double)n * (sizeof(mi355_pair_result) + sizeof(mi355_pair_calib_block)));
        hipLaunchKernelGGL(tie_blocks_kernel<CalibFormer>, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, d_results, n,
                           CalibFormer::Args{reinterpret_cast<const double*>(dpar), reinterpret_cast<const double*>(dpar + hb), min_ties}, d_out);
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
    template <class F> int guarded(std::string& err, F&& f) {            // a device error's message lives in the ctx: hand it to the loop
        const int rc = f();
        if (rc != MI355_OK) err = ctx->err;
        return rc;
    }
    int heads(CalibHead* out, std::string& err) override {
        return guarded(err, [&]() -> int {
            HostBuf& hh = ctx->hbuf("calib_heads_host");
            MI_HIP(hh.reserve(CB_HEAD * (size_t)n));
            MI_HIP(hipMemcpy2DAsync(hh.p, CB_HEAD, d_rec, sizeof(mi355_pair_result), CB_HEAD, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
            MI_HIP(hipStreamSynchronize(ctx->stream));
            for (int p = 0; p < n; p++) {
                const uint8_t* e = hh.as<uint8_t>() + CB_HEAD * (size_t)p;
                memcpy(&out[p].i, e, sizeof(int32_t) * 3);              // i, j, n_in lead the record
                memcpy(out[p].H, e + offsetof(mi355_pair_result, H), sizeof(float) * 9);
            }
            return MI355_OK;
        });
    }
    int blocks(const double* h8, const mi355_camera& cam, int min_ties, const mi355_pair_calib_block** out, std::string& err) override {
        return guarded(err, [&] { return mi_blocks_round_trip(ctx, "calib", n, nullptr, [&](mi355_pair_calib_block* d) { return launch_blocks(ctx, d_rec, n, h8, cam, min_ties, d); }, out); });
    }
    int record(int p, mi355_pair_result* out, std::string& err) override {
        return guarded(err, [&]() -> int {
            MI_HIP(hipMemcpyAsync(out, d_rec + p, sizeof(mi355_pair_result), hipMemcpyDeviceToHost, ctx->stream));
            MI_HIP(hipStreamSynchronize(ctx->stream));
            return MI355_OK;
        });
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
    DevSource src;
    src.ctx = ctx;
    { const int rc = mi_compact_for_loop(ctx, "calib", d_results, n_pairs, &src.d_rec, &src.n); if (rc != MI355_OK) return rc; }
    const int rc = mi_calibrate_lens(src, start, params, out, report, err);
    if (rc != MI355_OK) ctx->set_error(err);
    return rc;
}
