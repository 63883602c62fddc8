// csrc/verify.hip -- pair verification (gfx950): the kernels, their host twins and the entry points (include/mi355_mosaic.h, "pair
// verification").  Compiled with -ffp-contract=off: the double chains are the header's, one rounding per operation, and they are ONE piece of
// source for the kernels and the host twins (verify.h).  Every kernel gives a wave a record (or an edge), four waves to a workgroup --
// pair_moments_kernel's launch -- and has no atomic: a wave's results are its own (the one barrier, in pair_residuals_kernel, stands
// between a wave's LDS writes and its lane 0 reading them).
//
//   pair_edges_kernel      the box of b[0 .. n_in) by the lanes (keys of the floats' total order, reduced across the wave with integer
//                          minimum and maximum: exact in any order), F, its adjugate inverse and the flags by lane 0.
//   pair_cycles_kernel     the lanes stride over the shorter adjacency list of the edge's two frames and look each neighbour up in the
//                          other by binary search; a lane that finds a common neighbour walks the triangle's nine control points (27 maps,
//                          54 f64 divisions); counts and the minimum are reduced across the wave.  The edges it reads (176 B each) are the
//                          neighbours' own: at C5's ~60-fold overlap they stay in L2.
//   pair_residuals_kernel  the lanes form the r2 of the ties (two maps each) into LDS, lane 0 adds them in tie order.
//   verify_apply_kernel    the record copy in 16-byte pieces with the demoted records' ok, accepted and H cleared on the way.
#include "common.h"
#include "verify.h"
#include <algorithm>
#include <cmath>
#include <cstddef>

namespace {

constexpr int VF_NT = 256;                 // four waves

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { for (int s = 32; s > 0; s >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, s); v = o < v ? o : v; } return v; }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { for (int s = 32; s > 0; s >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, s); v = o > v ? o : v; } return v; }
__device__ __forceinline__ int wave_sum_i32(int v) { for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s); return v; }
__device__ __forceinline__ double wave_min_f64(double v) { for (int s = 32; s > 0; s >>= 1) { const double o = __shfl_xor(v, s); v = o < v ? o : v; } return v; }

// the box of a usable record's b list, keys in and out
struct VfBox { uint32_t x0, y0, x1, y1; };
VF_HD void vf_box_init(VfBox& b) { b.x0 = b.y0 = 0xffffffffu; b.x1 = b.y1 = 0u; }
VF_HD void vf_box_add(VfBox& b, float x, float y) {
    const uint32_t kx = vf_key(x), ky = vf_key(y);
    b.x0 = kx < b.x0 ? kx : b.x0; b.x1 = kx > b.x1 ? kx : b.x1;
    b.y0 = ky < b.y0 ? ky : b.y0; b.y1 = ky > b.y1 ? ky : b.y1;
}
VF_HD void vf_edge_close(const mi355_pair_result& e, bool usable, const VfBox& b, mi355_pair_edge& o) {
    __builtin_memset(&o, 0, sizeof(o));
    o.i = e.i; o.j = e.j; o.n_in = e.n_in;
    if (!usable) return;
    o.box[0] = vf_unkey(b.x0); o.box[1] = vf_unkey(b.y0); o.box[2] = vf_unkey(b.x1); o.box[3] = vf_unkey(b.y1);
    vf_edge_matrices(e.H, o);
}

__global__ __launch_bounds__(VF_NT) void pair_edges_kernel(const mi355_pair_result* in, int n, int n_images, mi355_pair_edge* out) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), t = threadIdx.x & 63;
    if (p >= n) return;
    const mi355_pair_result& e = in[p];
    const bool usable = vf_usable(e.accepted, e.n_in, e.i, e.j, n_images);      // the same in every lane
    VfBox b;
    vf_box_init(b);
    if (usable) {
        const int cnt = e.n_in;
        for (int k = t; k < cnt; k += 64) vf_box_add(b, e.b[k].x, e.b[k].y);
        b.x0 = wave_min_u32(b.x0); b.y0 = wave_min_u32(b.y0); b.x1 = wave_max_u32(b.x1); b.y1 = wave_max_u32(b.y1);
    }
    if (t == 0) {
        mi355_pair_edge o;
        vf_edge_close(e, usable, b, o);
        out[p] = o;
    }
}

// the entry of frame k in the sorted list [lo, hi) of adj, or -1
VF_HD int vf_find(const VfAdj* adj, int lo, int hi, int k) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const int v = adj[mid].nbr;
        if (v == k) return mid;
        if (v < k) lo = mid + 1; else hi = mid;
    }
    return -1;
}
// the triangle of edge e over the common neighbour whose entries are qi (in frame i's list) and qj (in frame j's list)
VF_HD void vf_one_triangle(const mi355_pair_edge* edges, const mi355_pair_edge& e, const VfAdj& qi, const VfAdj& qj, double tol2, int& n_ok, int& n_bad, double& min_e2) {
    const mi355_pair_edge& ej = edges[qj.edge2 >> 1];                 // between j and k: bit set = j is its i, its F maps k -> j
    const mi355_pair_edge& ei = edges[qi.edge2 >> 1];                 // between i and k: bit set = i is its i, its F maps k -> i
    const double* Mkj = (qj.edge2 & 1u) ? ej.B : ej.F;
    const double* Mik = (qi.edge2 & 1u) ? ei.F : ei.B;
    double E;
    const bool ok = vf_triangle(e, Mkj, Mik, E);
    vf_count(ok, E, tol2, n_ok, n_bad, min_e2);
}

__global__ __launch_bounds__(VF_NT) void pair_cycles_kernel(const mi355_pair_edge* edges, int n, const int32_t* row, const VfAdj* adj, double tol2, mi355_pair_cycle* out) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), t = threadIdx.x & 63;
    if (p >= n) return;
    const mi355_pair_edge& e = edges[p];
    int n_ok = 0, n_bad = 0;
    double min_e2 = INFINITY;
    if (e.flags & MI355_EDGE_TESTABLE) {                            // the same in every lane; a testable edge's frames are inside the table
        const int i0 = row[e.i], i1 = row[e.i + 1], j0 = row[e.j], j1 = row[e.j + 1];
        const bool walk_i = (i1 - i0) <= (j1 - j0);
        const int w0 = walk_i ? i0 : j0, w1 = walk_i ? i1 : j1, s0 = walk_i ? j0 : i0, s1 = walk_i ? j1 : i1;
        for (int q = w0 + t; q < w1; q += 64) {
            const int f = vf_find(adj, s0, s1, adj[q].nbr);
            if (f < 0) continue;
            vf_one_triangle(edges, e, adj[walk_i ? q : f], adj[walk_i ? f : q], tol2, n_ok, n_bad, min_e2);
        }
        n_ok = wave_sum_i32(n_ok); n_bad = wave_sum_i32(n_bad); min_e2 = wave_min_f64(min_e2);
    }
    if (t == 0) { mi355_pair_cycle o; o.n_ok = n_ok; o.n_bad = n_bad; o.min_e2 = min_e2; out[p] = o; }
}

// lane 0's part of a record's residual, shared with the host twin: r2[k] in tie order
VF_HD void vf_residual_close(const double* r2, int cnt, mi355_pair_residual& o) {
    double sum = 0.0, mx = 0.0;
    int used = 0, den = 0;
    for (int k = 0; k < cnt; k++) {
        const double v = r2[k];
        if (v == -1.0) { den++; continue; }
        sum = sum + v;
        mx = v > mx ? v : mx;
        used++;
    }
    o.n_used = used; o.n_den = den; o.sum_r2 = vf_canon(sum); o.max_r2 = mx;
}

__global__ __launch_bounds__(VF_NT) void pair_residuals_kernel(const mi355_pair_result* in, int n, const float* h9s, const int32_t* label, int n_images, mi355_pair_residual* out) {
    __shared__ double r2[4][MI355_MAX_SELECTED];
    const int wv = threadIdx.x >> 6, p = blockIdx.x * 4 + wv, t = threadIdx.x & 63;
    const bool live = p < n;                        // every wave reaches the barrier, a wave past n with nothing to do
    const mi355_pair_result& e = in[live ? p : 0];
    int cnt = 0;
    if (live && vf_measured(e.accepted, e.n_in, e.i, e.j, n_images, h9s, label)) {      // the same in every lane
        cnt = e.n_in;
        double Hi[9], Hj[9];
        for (int q = 0; q < 9; q++) { Hi[q] = (double)h9s[9 * (size_t)e.i + q]; Hj[q] = (double)h9s[9 * (size_t)e.j + q]; }
        for (int k = t; k < cnt; k += 64)
            r2[wv][k] = vf_tie_r2(Hi, Hj, (double)e.a[k].x, (double)e.a[k].y, (double)e.b[k].x, (double)e.b[k].y);
    }
    __syncthreads();
    if (live && t == 0) {
        mi355_pair_residual o;
        o.i = e.i; o.j = e.j;
        vf_residual_close(r2[wv], cnt, o);
        out[p] = o;
    }
}

// the apply pass: a record is 604 pieces of 16 bytes; ok, accepted and H are bytes 16 .. 59
static_assert(sizeof(mi355_pair_result) == 9664 && offsetof(mi355_pair_result, ok) == 16 && offsetof(mi355_pair_result, _pad) == 60, "pair record layout");
__global__ __launch_bounds__(VF_NT) void verify_apply_kernel(const mi355_pair_result* in, int n, const uint8_t* demote, mi355_pair_result* out) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), t = threadIdx.x & 63;
    if (p >= n) return;
    const bool dm = demote[p] != 0;
    if (!dm && in == out) return;
    const uint4* s = reinterpret_cast<const uint4*>(in + p);
    uint4* d = reinterpret_cast<uint4*>(out + p);
    for (int q = t; q < (int)(sizeof(mi355_pair_result) / 16); q += 64) {
        uint4 v = s[q];
        if (dm) {
            if (q == 1 || q == 2) v = make_uint4(0u, 0u, 0u, 0u);
            else if (q == 3) { v.x = 0u; v.y = 0u; v.z = 0u; }
        }
        d[q] = v;
    }
}
void apply_host(const mi355_pair_result* in, int n, const uint8_t* demote, mi355_pair_result* out) {
    for (int p = 0; p < n; p++) {
        if (out != in) memcpy(out + p, in + p, sizeof(mi355_pair_result));
        if (!demote[p]) continue;
        out[p].ok = 0; out[p].accepted = 0;
        for (int q = 0; q < 9; q++) out[p].H[q] = 0.0f;
    }
}

// ---- host twins -------------------------------------------------------------------------------------------------------------------
void edges_host(const mi355_pair_result* r, int n, int n_images, mi355_pair_edge* out) {
    for (int p = 0; p < n; p++) {
        const mi355_pair_result& e = r[p];
        const bool usable = vf_usable(e.accepted, e.n_in, e.i, e.j, n_images);
        VfBox b;
        vf_box_init(b);
        if (usable) for (int k = 0; k < e.n_in; k++) vf_box_add(b, e.b[k].x, e.b[k].y);
        vf_edge_close(e, usable, b, out[p]);
    }
}
void cycles_host(const mi355_pair_edge* edges, int n, const int32_t* row, const VfAdj* adj, double tol2, mi355_pair_cycle* out) {
    for (int p = 0; p < n; p++) {
        const mi355_pair_edge& e = edges[p];
        int n_ok = 0, n_bad = 0;
        double min_e2 = INFINITY;
        if (e.flags & MI355_EDGE_TESTABLE) {
            const int i0 = row[e.i], i1 = row[e.i + 1], j0 = row[e.j], j1 = row[e.j + 1];
            for (int q = i0; q < i1; q++) {
                const int f = vf_find(adj, j0, j1, adj[q].nbr);
                if (f >= 0) vf_one_triangle(edges, e, adj[q], adj[f], tol2, n_ok, n_bad, min_e2);
            }
        }
        out[p].n_ok = n_ok; out[p].n_bad = n_bad; out[p].min_e2 = min_e2;
    }
}
void residuals_host(const mi355_pair_result* r, int n, const float* h9s, const int32_t* label, int n_images, mi355_pair_residual* out) {
    double r2[MI355_MAX_SELECTED];
    for (int p = 0; p < n; p++) {
        const mi355_pair_result& e = r[p];
        int cnt = 0;
        if (vf_measured(e.accepted, e.n_in, e.i, e.j, n_images, h9s, label)) {
            cnt = e.n_in;
            double Hi[9], Hj[9];
            for (int q = 0; q < 9; q++) { Hi[q] = (double)h9s[9 * (size_t)e.i + q]; Hj[q] = (double)h9s[9 * (size_t)e.j + q]; }
            for (int k = 0; k < cnt; k++) r2[k] = vf_tie_r2(Hi, Hj, (double)e.a[k].x, (double)e.a[k].y, (double)e.b[k].x, (double)e.b[k].y);
        }
        memset(&out[p], 0, sizeof(out[p]));
        out[p].i = e.i; out[p].j = e.j;
        vf_residual_close(r2, cnt, out[p]);
    }
}

// ---- argument checks ----------------------------------------------------------------------------------------------------------------
bool images_ok(const char* who, int n, int n_images, std::string& err) {
    if (n < 0) { err = std::string(who) + ": n=" + std::to_string(n) + " < 0"; return false; }
    if (n_images < 1 || n_images > VF_MAX_IMAGES) { err = std::string(who) + ": n_images=" + std::to_string(n_images) + " outside [1, 65535]"; return false; }
    return true;
}
bool tol_ok(const char* who, double cycle_tol, std::string& err) {
    if (!(vf_finite(cycle_tol) && cycle_tol > 0.0)) { err = std::string(who) + ": cycle_tol=" + std::to_string(cycle_tol) + " must be finite and > 0"; return false; }
    return true;
}

// ---- device launches (the ctx lock is held) -----------------------------------------------------------------------------------------
int launch_edges(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, int n_images, mi355_pair_edge* d_out) {
    ProfScope ps(ctx, "pair_edges", (double)sizeof(mi355_pair_result) * (double)n);
    hipLaunchKernelGGL(pair_edges_kernel, dim3((n + 3) / 4), dim3(VF_NT), 0, ctx->stream, d_results, n, n_images, d_out);
    MI_HIP(hipGetLastError());
    return MI355_OK;
}

// host bytes into a named device buffer through a pinned staging area of the same name (the caller's arrays may be gone before the copy runs)
int upload(mi355_ctx* ctx, const std::string& name, const void* a, size_t na, const void* b, size_t nb, uint8_t** d) {
    HostBuf& stage = ctx->hbuf(name + "_host");
    DevBuf& dev = ctx->buf(name);
    MI_HIP(stage.reserve(na + nb + 16));
    MI_HIP(dev.reserve(na + nb + 16));
    MI_HIP(hipStreamSynchronize(ctx->stream));            // the previous upload has left the staging area
    if (na) memcpy(stage.p, a, na);
    if (nb) memcpy(stage.as<uint8_t>() + na, b, nb);
    if (na + nb) MI_HIP(hipMemcpyAsync(dev.p, stage.p, na + nb, hipMemcpyHostToDevice, ctx->stream));
    *d = dev.as<uint8_t>();
    return MI355_OK;
}

// the cycles of n edges (d_edges: on the device already) over the adjacency; the results land in the ctx's pinned "verify_cycles_host"
int run_cycles(mi355_ctx* ctx, const mi355_pair_edge* d_edges, int n, int n_images, const std::vector<int32_t>& row, const std::vector<VfAdj>& adj, double cycle_tol,
               const mi355_pair_cycle** out) {
    DevBuf& dcyc = ctx->buf("verify_cycles");
    HostBuf& hcyc = ctx->hbuf("verify_cycles_host");
    const size_t bytes = sizeof(mi355_pair_cycle) * (size_t)(n > 0 ? n : 1);
    MI_HIP(dcyc.reserve(bytes));
    MI_HIP(hcyc.reserve(bytes));
    *out = hcyc.as<mi355_pair_cycle>();
    if (n == 0) return MI355_OK;
    const size_t rb = sizeof(int32_t) * (size_t)(n_images + 1), ab = sizeof(VfAdj) * adj.size();       // rb is a multiple of 4, VfAdj needs 4
    uint8_t* dadj = nullptr;
    { const int rc = upload(ctx, "verify_adj", row.data(), rb, adj.data(), ab, &dadj); if (rc != MI355_OK) return rc; }
    {
        ProfScope ps(ctx, "pair_cycles", (double)sizeof(mi355_pair_edge) * (double)n + (double)(rb + ab));
        hipLaunchKernelGGL(pair_cycles_kernel, dim3((n + 3) / 4), dim3(VF_NT), 0, ctx->stream, d_edges, n, reinterpret_cast<const int32_t*>(dadj),
                           reinterpret_cast<const VfAdj*>(dadj + rb), cycle_tol * cycle_tol, dcyc.as<mi355_pair_cycle>());
    }
    MI_HIP(hipGetLastError());
    MI_HIP(hipMemcpyAsync(hcyc.p, dcyc.p, sizeof(mi355_pair_cycle) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}

int launch_residuals(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, const float* h9s, const int32_t* label, int n_images, mi355_pair_residual* d_out) {
    const size_t hb = sizeof(float) * 9 * (size_t)n_images, lb = label ? sizeof(int32_t) * (size_t)n_images : 0;
    uint8_t* dpar = nullptr;
    { const int rc = upload(ctx, "verify_h9s", h9s, hb, label, lb, &dpar); if (rc != MI355_OK) return rc; }
    {
        ProfScope ps(ctx, "pair_residuals", (double)sizeof(mi355_pair_result) * (double)n);
        hipLaunchKernelGGL(pair_residuals_kernel, dim3((n + 3) / 4), dim3(VF_NT), 0, ctx->stream, d_results, n, reinterpret_cast<const float*>(dpar),
                           label ? reinterpret_cast<const int32_t*>(dpar + hb) : nullptr, n_images, d_out);
    }
    MI_HIP(hipGetLastError());
    return MI355_OK;
}

// a device array of n records into a pinned buffer of the ctx, complete on return
template <class T> int download(mi355_ctx* ctx, const std::string& name, const T* d, int n, const T** out) {
    HostBuf& h = ctx->hbuf(name);
    MI_HIP(h.reserve(sizeof(T) * (size_t)(n > 0 ? n : 1)));
    if (n > 0) {
        MI_HIP(hipMemcpyAsync(h.p, d, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));
    }
    *out = h.as<T>();
    return MI355_OK;
}

// the loop's records from the device
struct DevSource : VerifySource {
    mi355_ctx* ctx;
    const mi355_pair_result* d_rec;
    int n, n_images;
    template <class F> int run(F&& f, std::string& err) { const int rc = f(); if (rc != MI355_OK) err = ctx->err; return rc; }
    int moments(const mi355_pair_moments** out, std::string& err) override {
        return run([&]() -> int {
            DevBuf& d = ctx->buf("verify_moments");
            MI_HIP(d.reserve(sizeof(mi355_pair_moments) * (size_t)(n > 0 ? n : 1)));
            if (n > 0) { const int rc = mi_pair_moments(ctx, d_rec, n, d.as<mi355_pair_moments>()); if (rc != MI355_OK) return rc; }
            return download(ctx, "verify_moments_host", d.as<mi355_pair_moments>(), n, out);
        }, err);
    }
    int edges(const mi355_pair_edge** out, std::string& err) override {
        return run([&]() -> int {
            DevBuf& d = ctx->buf("verify_edges");
            MI_HIP(d.reserve(sizeof(mi355_pair_edge) * (size_t)(n > 0 ? n : 1)));
            if (n > 0) { const int rc = launch_edges(ctx, d_rec, n, n_images, d.as<mi355_pair_edge>()); if (rc != MI355_OK) return rc; }
            return download(ctx, "verify_edges_host", d.as<mi355_pair_edge>(), n, out);
        }, err);
    }
    int cycles(const mi355_pair_edge*, const std::vector<int32_t>& row, const std::vector<VfAdj>& adj, double cycle_tol, const mi355_pair_cycle** out, std::string& err) override {
        return run([&]() -> int { return run_cycles(ctx, ctx->buf("verify_edges").as<mi355_pair_edge>(), n, n_images, row, adj, cycle_tol, out); }, err);
    }
    int residuals(const float* h9s, const int32_t* label, const mi355_pair_residual** out, std::string& err) override {
        return run([&]() -> int {
            DevBuf& d = ctx->buf("verify_residuals");
            MI_HIP(d.reserve(sizeof(mi355_pair_residual) * (size_t)(n > 0 ? n : 1)));
            if (n > 0) { const int rc = launch_residuals(ctx, d_rec, n, h9s, label, n_images, d.as<mi355_pair_residual>()); if (rc != MI355_OK) return rc; }
            return download(ctx, "verify_residuals_host", d.as<mi355_pair_residual>(), n, out);
        }, err);
    }
};

// ... and from host records, by the host twins
struct HostSource : VerifySource {
    const mi355_pair_result* r;
    int n, n_images;
    std::vector<mi355_pair_moments> mom;
    std::vector<mi355_pair_edge> edg;
    std::vector<mi355_pair_cycle> cyc;
    std::vector<mi355_pair_residual> res;
    int moments(const mi355_pair_moments** out, std::string& err) override {
        mom.resize((size_t)(n > 0 ? n : 1));
        // mi355_pair_moments_host stops at a record with n_in > 400; the device kernel gives it its n_in and no sums, and the loop refuses it
        for (int p = 0; p < n; p++) {
            if (r[p].accepted && r[p].n_in > MI355_MAX_SELECTED) { memset(&mom[p], 0, sizeof(mom[p])); mom[p].i = r[p].i; mom[p].j = r[p].j; mom[p].n_in = r[p].n_in; continue; }
            if (mi355_pair_moments_host(r + p, 1, &mom[p]) != MI355_OK) { err = "verify_pairs_results: the moments of record " + std::to_string(p); return MI355_ERR_ARG; }
        }
        *out = mom.data();
        return MI355_OK;
    }
    int edges(const mi355_pair_edge** out, std::string&) override {
        edg.resize((size_t)(n > 0 ? n : 1));
        edges_host(r, n, n_images, edg.data());
        *out = edg.data();
        return MI355_OK;
    }
    int cycles(const mi355_pair_edge* e, const std::vector<int32_t>& row, const std::vector<VfAdj>& adj, double cycle_tol, const mi355_pair_cycle** out, std::string&) override {
        cyc.resize((size_t)(n > 0 ? n : 1));
        cycles_host(e, n, row.data(), adj.data(), cycle_tol * cycle_tol, cyc.data());
        *out = cyc.data();
        return MI355_OK;
    }
    int residuals(const float* h9s, const int32_t* label, const mi355_pair_residual** out, std::string&) override {
        res.resize((size_t)(n > 0 ? n : 1));
        residuals_host(r, n, h9s, label, n_images, res.data());
        *out = res.data();
        return MI355_OK;
    }
};

const char* verify_null(int n_pairs, const void* in, const void* out, const void* label_out, const void* transforms_out) {
    return (n_pairs > 0 && !in) ? "the records" : (n_pairs > 0 && !out) ? "the output records" : !label_out ? "label_out" : !transforms_out ? "transforms_out" : nullptr;
}

}  // namespace

extern "C" void mi355_default_verify_params(mi355_verify_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->cycle_tol = 6.0; p->gate_abs = 3.0; p->gate_k = 4.0; p->max_rounds = 8; p->bridges = 1;
}

extern "C" int mi355_pair_edges_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, int n_images, mi355_pair_edge* d_out) {
    LOCKED_PROLOGUE
    std::string err;
    if (!images_ok("pair_edges_dev", n, n_images, err)) { ctx->set_error(err); return MI355_ERR_ARG; }
    if (n > 0 && (!d_results || !d_out)) { ctx->set_error(std::string("pair_edges_dev: ") + (!d_results ? "d_results" : "d_out") + " is NULL"); return MI355_ERR_ARG; }
    if (n == 0) return MI355_OK;
    return launch_edges(ctx, d_results, n, n_images, d_out);
}

extern "C" int mi355_pair_edges_host(const mi355_pair_result* r, int n, int n_images, mi355_pair_edge* out) {
    std::string err;
    if (!images_ok("pair_edges_host", n, n_images, err)) { mi_set_host_error(err); return MI355_ERR_ARG; }
    if (n > 0 && (!r || !out)) { mi_set_host_error(std::string("pair_edges_host: ") + (!r ? "r" : "out") + " is NULL"); return MI355_ERR_ARG; }
    edges_host(r, n, n_images, out);
    return MI355_OK;
}

extern "C" int mi355_pair_cycles_dev(mi355_ctx* ctx, const mi355_pair_edge* edges, int n, int n_images, double cycle_tol, mi355_pair_cycle* out) {
    LOCKED_PROLOGUE
    std::string err;
    if (!images_ok("pair_cycles_dev", n, n_images, err) || !tol_ok("pair_cycles_dev", cycle_tol, err)) { ctx->set_error(err); return MI355_ERR_ARG; }
    if (n > 0 && (!edges || !out)) { ctx->set_error(std::string("pair_cycles_dev: ") + (!edges ? "edges" : "out") + " is NULL"); return MI355_ERR_ARG; }
    if (n == 0) return MI355_OK;
    std::vector<int32_t> row;
    std::vector<VfAdj> adj;
    if (mi_verify_adjacency(edges, n, n_images, row, adj, err) != MI355_OK) { ctx->set_error("pair_cycles_dev: " + err); return MI355_ERR_ARG; }
    uint8_t* dedges = nullptr;
    { const int rc = upload(ctx, "verify_edges_up", edges, sizeof(mi355_pair_edge) * (size_t)n, nullptr, 0, &dedges); if (rc != MI355_OK) return rc; }
    const mi355_pair_cycle* res = nullptr;
    { const int rc = run_cycles(ctx, reinterpret_cast<const mi355_pair_edge*>(dedges), n, n_images, row, adj, cycle_tol, &res); if (rc != MI355_OK) return rc; }
    memcpy(out, res, sizeof(mi355_pair_cycle) * (size_t)n);
    return MI355_OK;
}

extern "C" int mi355_pair_cycles_host(const mi355_pair_edge* edges, int n, int n_images, double cycle_tol, mi355_pair_cycle* out) {
    std::string err;
    if (!images_ok("pair_cycles_host", n, n_images, err) || !tol_ok("pair_cycles_host", cycle_tol, err)) { mi_set_host_error(err); return MI355_ERR_ARG; }
    if (n > 0 && (!edges || !out)) { mi_set_host_error(std::string("pair_cycles_host: ") + (!edges ? "edges" : "out") + " is NULL"); return MI355_ERR_ARG; }
    if (n == 0) return MI355_OK;
    std::vector<int32_t> row;
    std::vector<VfAdj> adj;
    if (mi_verify_adjacency(edges, n, n_images, row, adj, err) != MI355_OK) { mi_set_host_error("pair_cycles_host: " + err); return MI355_ERR_ARG; }
    cycles_host(edges, n, row.data(), adj.data(), cycle_tol * cycle_tol, out);
    return MI355_OK;
}

extern "C" int mi355_pair_residuals_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n, const float* h9s, const int32_t* label, int n_images,
                                        mi355_pair_residual* d_out) {
    LOCKED_PROLOGUE
    std::string err;
    if (!images_ok("pair_residuals_dev", n, n_images, err)) { ctx->set_error(err); return MI355_ERR_ARG; }
    if (!h9s || (n > 0 && (!d_results || !d_out))) { ctx->set_error(std::string("pair_residuals_dev: ") + (!h9s ? "h9s" : !d_results ? "d_results" : "d_out") + " is NULL"); return MI355_ERR_ARG; }
    if (n == 0) return MI355_OK;
    return launch_residuals(ctx, d_results, n, h9s, label, n_images, d_out);
}

extern "C" int mi355_pair_residuals_host(const mi355_pair_result* r, int n, const float* h9s, const int32_t* label, int n_images, mi355_pair_residual* out) {
    std::string err;
    if (!images_ok("pair_residuals_host", n, n_images, err)) { mi_set_host_error(err); return MI355_ERR_ARG; }
    if (!h9s || (n > 0 && (!r || !out))) { mi_set_host_error(std::string("pair_residuals_host: ") + (!h9s ? "h9s" : !r ? "r" : "out") + " is NULL"); return MI355_ERR_ARG; }
    residuals_host(r, n, h9s, label, n_images, out);
    return MI355_OK;
}

extern "C" int mi355_verify_pairs_dev(mi355_ctx* ctx, const mi355_pair_result* d_results, int n_pairs, int n_images, const int32_t* fixed,
                                      const mi355_verify_params* params, mi355_pair_result* d_out, int32_t* label_out, mi355_image_transform* transforms_out,
                                      mi355_verify_report* report, mi355_verify_summary* summary) {
    LOCKED_PROLOGUE
    std::string err;
    mi355_verify_params p;
    if (mi_verify_check(n_pairs, n_images, params, p, err) != MI355_OK) { ctx->set_error("verify_pairs_dev: " + err); return MI355_ERR_ARG; }
    if (const char* null = verify_null(n_pairs, d_results, d_out, label_out, transforms_out)) { ctx->set_error(std::string("verify_pairs_dev: ") + null + " is NULL"); return MI355_ERR_ARG; }
    DevSource src;
    src.ctx = ctx; src.d_rec = d_results; src.n = n_pairs; src.n_images = n_images;
    std::vector<uint8_t> demote((size_t)(n_pairs > 0 ? n_pairs : 1), 0);
    const int rc = mi_verify_loop(src, n_pairs, n_images, fixed, p, demote.data(), label_out, transforms_out, report, summary, err);
    if (rc != MI355_OK) { ctx->set_error("verify_pairs_dev: " + err); return rc; }
    if (n_pairs == 0) return MI355_OK;
    uint8_t* ddem = nullptr;
    { const int rc2 = upload(ctx, "verify_demote", demote.data(), (size_t)n_pairs, nullptr, 0, &ddem); if (rc2 != MI355_OK) return rc2; }
    hipLaunchKernelGGL(verify_apply_kernel, dim3((n_pairs + 3) / 4), dim3(VF_NT), 0, ctx->stream, d_results, n_pairs, ddem, d_out);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}

extern "C" int mi355_verify_pairs_results(const mi355_pair_result* r, int n_pairs, int n_images, const int32_t* fixed, const mi355_verify_params* params,
                                          mi355_pair_result* out, int32_t* label_out, mi355_image_transform* transforms_out, mi355_verify_report* report,
                                          mi355_verify_summary* summary) {
    std::string err;
    mi355_verify_params p;
    if (mi_verify_check(n_pairs, n_images, params, p, err) != MI355_OK) { mi_set_host_error("verify_pairs_results: " + err); return MI355_ERR_ARG; }
    if (const char* null = verify_null(n_pairs, r, out, label_out, transforms_out)) { mi_set_host_error(std::string("verify_pairs_results: ") + null + " is NULL"); return MI355_ERR_ARG; }
    HostSource src;
    src.r = r; src.n = n_pairs; src.n_images = n_images;
    std::vector<uint8_t> demote((size_t)(n_pairs > 0 ? n_pairs : 1), 0);
    const int rc = mi_verify_loop(src, n_pairs, n_images, fixed, p, demote.data(), label_out, transforms_out, report, summary, err);
    if (rc != MI355_OK) { mi_set_host_error("verify_pairs_results: " + err); return rc; }
    apply_host(r, n_pairs, demote.data(), out);
    return MI355_OK;
}
