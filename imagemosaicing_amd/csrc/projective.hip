// csrc/projective.hip -- the device half of the projective refinement (include/mi355_mosaic.h, "projective refinement of the global
// alignment"): the normal-equation block of every pair record at the current parameters, and the entry points that run the host loop
// (projective_solve.cpp) on blocks formed here.  Compiled with -ffp-contract=off like the host twin: the same chain of separately rounded
// double operations per sum, so the refinement gives the same bits from either.
#include "tie_blocks_dev.h"
#include "projective.h"

namespace {

// the rows of tie_blocks_kernel for this refinement: X = [Rx | rx], Y = [Ry | ry], ten f64 divisions per inlier; image j's lane hands its
// U, V to image i's lane, which closes the rows with the residual
struct NormalFormer {
    static constexpr int ROW = MI_PROJ_ROW;
    using Block = mi355_pair_normal_block;
    struct Args { const double* h8; const uint8_t* part; int n_images; };
    Args a;
    const mi355_pair_result* e = nullptr;
    int pi = 0, pj = 0, keep = 0;
    __device__ __forceinline__ NormalFormer(const Args& a_) : a(a_) {}
    __device__ __forceinline__ static int count(const Args& a, const mi355_pair_result* in, int p, int n, int* keep_n = nullptr) {
        int k = 0;
        return p < n && mi_proj_used(in[p].accepted, in[p].n_in, in[p].i, in[p].j, a.part, a.n_images, keep_n ? keep_n : &k) ? in[p].n_in : 0;
    }
    __device__ __forceinline__ int open(const mi355_pair_result* in, int p, int n) {
        e = in + p;
        if (p < n) { pi = e->i; pj = e->j; }
        return count(a, in, p, n, &keep);
    }
    __device__ __forceinline__ void form(bool live, int side, int kq, int k, double* row) {
        double U = 0.0, V = 0.0;
        if (live) {
            const mi355_sfpoint pt = side ? e->b[k] : e->a[k];
            double* X = row + 8 * side;
            mi_proj_side(a.h8 + (size_t)8 * (side ? pj : pi), (double)pt.x, (double)pt.y, side ? -1.0 : 1.0, X, X + ROW, U, V);
        }
        const double Ub = __shfl(U, kq + 32), Vb = __shfl(V, kq + 32);      // image j's side of the same inlier
        if (live && side == 0) { row[16] = Ub - U; row[ROW + 16] = Vb - V; }
    }
    // a malformed accepted record keeps its n_in
    __device__ __forceinline__ void head(Block& o, int) const { o.i = pi; o.j = pj; o.n_in = keep; o._pad = 0; }
};
static_assert(sizeof(mi355_pair_normal_block) == 1240, "normal block record");

// caller holds the ctx lock: parameters and flags to the device, one launch
int launch_blocks(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, const double* h8, const uint8_t* part, int n_images, mi355_pair_normal_block* d_out) {
    const size_t hb = sizeof(double) * 8 * (size_t)n_images;
    uint8_t* dpar = nullptr;
    { const int rc = mi_upload_params(ctx, "proj", h8, hb, part, (size_t)n_images, &dpar); if (rc != MI355_OK) return rc; }
    hipLaunchKernelGGL(tie_blocks_kernel<NormalFormer>, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, d_results, n,
                       NormalFormer::Args{reinterpret_cast<const double*>(dpar), dpar + hb, n_images}, d_out);
    MI_HIP(hipGetLastError());
    return MI355_OK;
}

// the loop's blocks from the device: per trial one launch and one copy into pinned memory of the ctx
struct DevSource : ProjectiveSource {
    mi355_ctx* ctx;
    const mi355_pair_result* d_rec;
    int n;
    int blocks(const double* h8, const uint8_t* part, int n_images, const mi355_pair_normal_block** out, int* n_out, std::string& err) override {
        const int rc = mi_blocks_round_trip(ctx, "proj", n, "projective_refine_dev: no memory for the blocks",
                                            [&](mi355_pair_normal_block* d) { return launch_blocks(ctx, d_rec, n, h8, part, n_images, d); }, out);
        if (rc != MI355_OK) err = ctx->err;
        *n_out = n;
        return rc;
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
    DevSource src;
    src.ctx = ctx;
    { const int rc = mi_compact_for_loop(ctx, "proj", d_results, n_pairs, &src.d_rec, &src.n); if (rc != MI355_OK) return rc; }
    const int rc = mi_projective_refine(src, n_images, w, h, fixed, label, start, params, out, report, err);
    if (rc != MI355_OK) ctx->set_error(err);
    return rc;
}
