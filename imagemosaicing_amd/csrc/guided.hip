// csrc/guided.hip -- guided matching (opt-in): ties of a pair under a KNOWN transform (gfx950).
//
// The pair stage takes the global 1-NN of every descriptor and keeps the best 30 % by distance; on frames that overlap by a third or less the true
// matches are a minority of that list.  Here the caller says where frame j lies in frame i (a guide G, image j -> image i: the pair's own H, a chain
// of neighbouring H's, the global alignment) and every keypoint of frame j looks for its partner only among the keypoints of frame i within `radius`
// of its predicted position.  The definition is in include/mi355_mosaic.h, section "guided matching"; tests/guided_ref.py restates it in numpy.
//
// Kernel shape: a workgroup per pair.  Frame i's positions are staged once in LDS (2048 x 8 B); a lane owns a query and walks the positions two at
// a time at a wave-uniform address (an LDS broadcast: no bank conflicts).  Descriptor work happens only on a hit -- rare: 0.1 .. 0.5 candidates per
// query on real frames -- with the matcher's own operands: d = n8_i[k] + n8_j[q] - 2 dot(s8_i[k], s8_j[q]) is the exact squared distance of the u8
// rows (the 128 shift cancels in differences), 32 packed int8 dot instructions per hit.  The one-to-one rule is a 64-bit integer minimum per
// keypoint k of frame i on the packed key (d1 << 11 | q) in LDS; the survivors are compacted (their order there does not matter: the keys are
// distinct) and sorted by (d1, q, k) with the bitonic network of select_kernel over the next power of two.  No float atomics, nothing depends on
// which wave runs first.
#include "common.h"
#include "hmath.h"
#include <algorithm>
#include <cmath>

namespace {

#define GLOBAL_PTR(T, p) ((const __attribute__((address_space(1))) T*)(p))

constexpr int GM_MAXKP = 2048;       // keypoints per frame this stage takes (one feature record; keep-all frames are out of scope)
constexpr int GM_NT = 1024;          // threads per workgroup: two queries a lane on full frames (a small batch is bound by one workgroup's time)

struct GuidedPair {
    const float2* xy_i; const int8_t* s8_i; const int* n8_i;
    const float2* xy_j; const int8_t* s8_j; const int* n8_j;
    int n_i, n_j;
    float G[9];
    int _pad;
};

struct GuidedArgs { float radius2; int max_dist2; float ratio2; int use_ratio; int max_selected; };

typedef int gi32x4 __attribute__((ext_vector_type(4)));
typedef float gf32x2 __attribute__((ext_vector_type(2)));      // a float2 as the compiler's own vector: HIP's float2 is a class, which an address-space pointer cannot name

// exact squared distance of two descriptor rows from the matcher's operands
__device__ __forceinline__ int desc_dist2(const int8_t* s8_a, const int* n8_a, int ka, const int8_t* s8_b, const int* n8_b, int kb) {
    const int8_t* ra = s8_a + (size_t)ka * 128;
    const int8_t* rb = s8_b + (size_t)kb * 128;
    int dot = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const gi32x4 va = *GLOBAL_PTR(gi32x4, ra + 16 * c), vb = *GLOBAL_PTR(gi32x4, rb + 16 * c);
        dot = __builtin_amdgcn_sdot4(va.x, vb.x, dot, false);
        dot = __builtin_amdgcn_sdot4(va.y, vb.y, dot, false);
        dot = __builtin_amdgcn_sdot4(va.z, vb.z, dot, false);
        dot = __builtin_amdgcn_sdot4(va.w, vb.w, dot, false);
    }
    return GLOBAL_PTR(int, n8_a)[ka] + GLOBAL_PTR(int, n8_b)[kb] - 2 * dot;
}

__global__ __launch_bounds__(GM_NT) void guided_select_kernel(const GuidedPair* pairs, GuidedArgs ga, mi355_sfpoint* sel_a, mi355_sfpoint* sel_b, int* nsel, int* dist) {
    constexpr unsigned long long NONE = ~0ull;
    __shared__ __attribute__((aligned(16))) unsigned long long s_slab[GM_MAXKP];     // frame i's positions during the walk, the survivors' keys afterwards
    __shared__ unsigned long long s_best[GM_MAXKP];                                  // per keypoint k of frame i: the smallest (d1 << 11 | q) proposed to it
    __shared__ int s_count;
    const int pair = blockIdx.x, tid = threadIdx.x;
    const GuidedPair gp = pairs[pair];
    float2* s_xy = reinterpret_cast<float2*>(s_slab);
    const float qnan = __int_as_float(0x7fc00000);
    for (int k = tid; k < GM_MAXKP; k += GM_NT) {
        gf32x2 v = {qnan, qnan};
        if (k < gp.n_i) v = *GLOBAL_PTR(gf32x2, gp.xy_i + k);
        s_xy[k] = make_float2(v.x, v.y);      // a NaN position is never a candidate
        s_best[k] = NONE;
    }
    if (tid == 0) s_count = 0;
    __syncthreads();
    const int n_even = (gp.n_i + 1) & ~1;
    const float r2 = ga.radius2;
    for (int q = tid; q < gp.n_j; q += GM_NT) {
        const gf32x2 b = *GLOBAL_PTR(gf32x2, gp.xy_j + q);
        float X, Y;
        hm::apply_div9(gp.G, b.x, b.y, X, Y);
        int d1 = 0x7fffffff, d2 = 0x7fffffff, k1 = -1;           // k ascends: a strict < keeps the lowest k among equal d
        auto hit = [&](int k) {
            const int d = desc_dist2(gp.s8_i, gp.n8_i, k, gp.s8_j, gp.n8_j, q);
            if (d < d1) { d2 = d1; d1 = d; k1 = k; }
            else if (d < d2) d2 = d;
        };
        for (int k = 0; k < n_even; k += 2) {
            const float4 a = *reinterpret_cast<const float4*>(&s_xy[k]);
            const float dx0 = a.x - X, dy0 = a.y - Y, dx1 = a.z - X, dy1 = a.w - Y;
            const float e0 = dx0 * dx0 + dy0 * dy0, e1 = dx1 * dx1 + dy1 * dy1;
            const bool h0 = e0 <= r2, h1 = e1 <= r2;
            if (h0 || h1) {
                if (h0) hit(k);
                if (h1) hit(k + 1);
            }
        }
        if (k1 < 0 || d1 > ga.max_dist2) continue;
        const bool lone = d2 == 0x7fffffff;                      // no second candidate (a distance is at most 8 323 200)
        if (lone || !ga.use_ratio || (float)d1 < ga.ratio2 * (float)d2)
            atomicMin(&s_best[k1], ((unsigned long long)(unsigned)d1 << 11) | (unsigned long long)(unsigned)q);
    }
    __syncthreads();
    // the positions are dead: the slab takes the survivors' keys (d1 << 22 | q << 11 | k), compacted in any order -- the sort undoes it
    unsigned long long* key = s_slab;
    for (int k = tid; k < GM_MAXKP; k += GM_NT) {
        const unsigned long long v = s_best[k];
        if (v != NONE) key[atomicAdd(&s_count, 1)] = (v << 11) | (unsigned long long)(unsigned)k;
    }
    __syncthreads();
    const int count = s_count;
    int P = 64;
    while (P < count) P <<= 1;
    for (int i = count + tid; i < P; i += GM_NT) key[i] = NONE;
    __syncthreads();
    if (count > 1) {
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < P; i += GM_NT) {
                    const int ixj = i ^ j;
                    if (ixj > i) {
                        const unsigned long long a = key[i], c = key[ixj];
                        const bool up = (i & k) == 0;
                        if ((a > c) == up) { key[i] = c; key[ixj] = a; }
                    }
                }
                __syncthreads();
            }
        }
    }
    const int n_sel = count < ga.max_selected ? count : ga.max_selected;
    if (tid == 0) nsel[pair] = n_sel;
    const size_t o = (size_t)pair * MI355_MAX_SELECTED;
    for (int t = tid; t < MI355_MAX_SELECTED; t += GM_NT) {
        mi355_sfpoint a = {0.0f, 0.0f, 0}, b = {0.0f, 0.0f, 0};
        int d = 0;
        if (t < n_sel) {
            const unsigned long long v = key[t];
            const int k = (int)(v & 2047u), q = (int)((v >> 11) & 2047u);
            const gf32x2 pa = *GLOBAL_PTR(gf32x2, gp.xy_i + k), pb = *GLOBAL_PTR(gf32x2, gp.xy_j + q);
            a.x = pa.x; a.y = pa.y; a.id = k;
            b.x = pb.x; b.y = pb.y; b.id = q;
            d = (int)(v >> 22);
        }
        sel_a[o + t] = a; sel_b[o + t] = b;
        if (dist) dist[o + t] = d;
    }
}

bool finite_f(float v) { return std::isfinite(v); }

// the checks of every guided entry point, on the host before any launch; fills p (NULL -> defaults) and the pair table
int guided_prepare(mi355_ctx* ctx, const char* who, const int32_t* pairs_ij, int n, const float* guides, const mi355_guided_params* params,
                   mi355_guided_params& p, std::vector<GuidedPair>& table) {
    const std::string w = std::string(who) + ": ";
    if (params) p = *params; else mi355_default_guided_params(&p);
    if (!finite_f(p.radius) || !(p.radius > 0.0f) || p.radius > 64.0f) { ctx->set_error(w + "radius=" + std::to_string(p.radius) + " not finite or outside (0, 64]"); return MI355_ERR_ARG; }
    if (p.max_dist2 < 0 || p.max_dist2 > 8323200) { ctx->set_error(w + "max_dist2=" + std::to_string(p.max_dist2) + " outside [0, 8323200]"); return MI355_ERR_ARG; }
    if (!finite_f(p.ratio) || p.ratio < 0.0f || p.ratio > 1.0f) { ctx->set_error(w + "ratio=" + std::to_string(p.ratio) + " not finite or outside [0, 1]"); return MI355_ERR_ARG; }
    if (p.reserved != 0) { ctx->set_error(w + "reserved=" + std::to_string(p.reserved) + " (must be 0)"); return MI355_ERR_ARG; }
    if (n < 0) { ctx->set_error(w + "n=" + std::to_string(n) + " (not negative)"); return MI355_ERR_ARG; }
    if (n > 0 && (!pairs_ij || !guides)) { ctx->set_error(w + "n=" + std::to_string(n) + " with NULL " + (!pairs_ij ? "pairs_ij" : "guides")); return MI355_ERR_ARG; }
    if (ctx->p.max_selected < 0 || ctx->p.max_selected > MI355_MAX_SELECTED) { ctx->set_error(w + "max_selected=" + std::to_string(ctx->p.max_selected) + " outside [0, 400]"); return MI355_ERR_ARG; }
    table.clear();
    if (n == 0) return MI355_OK;
    for (int k = 0; k < n; k++)
        if (pairs_ij[2 * k] == pairs_ij[2 * k + 1]) { ctx->set_error(w + "pair " + std::to_string(k) + ": i == j == " + std::to_string(pairs_ij[2 * k])); return MI355_ERR_ARG; }
    {                                                       // frames still in flight: wait for those of these pairs only, as match_pairs does
        std::vector<int> ids(pairs_ij, pairs_ij + 2 * (size_t)n);
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        const int rc = mi_resolve_features_of(ctx, ids.data(), (int)ids.size());
        if (rc != MI355_OK) return rc;
    }
    table.resize((size_t)n);
    for (int k = 0; k < n; k++) {
        const int i = pairs_ij[2 * k], j = pairs_ij[2 * k + 1];
        const auto fi = ctx->feats.find(i), fj = ctx->feats.find(j);
        if (fi == ctx->feats.end() || fj == ctx->feats.end()) { ctx->set_error(w + "no resident features for image " + std::to_string(fi == ctx->feats.end() ? i : j)); return MI355_ERR_ARG; }
        const Features &a = fi->second, &b = fj->second;
        if (a.n > GM_MAXKP || b.n > GM_MAXKP) {
            ctx->set_error(w + "image " + std::to_string(a.n > GM_MAXKP ? i : j) + " holds " + std::to_string(a.n > GM_MAXKP ? a.n : b.n) + " keypoints (more than 2048: keep-all frames are out of scope)");
            return MI355_ERR_ARG;
        }
        GuidedPair& g = table[(size_t)k];
        memset(&g, 0, sizeof(g));
        g.xy_i = a.xy.as<float2>(); g.s8_i = a.s8.as<int8_t>(); g.n8_i = a.n8.as<int>(); g.n_i = a.n;
        g.xy_j = b.xy.as<float2>(); g.s8_j = b.s8.as<int8_t>(); g.n8_j = b.n8.as<int>(); g.n_j = b.n;
        memcpy(g.G, guides + (size_t)9 * k, sizeof(g.G));
    }
    return MI355_OK;
}

// the selection of n pairs: one launch on the ctx stream (the table is uploaded first; the host vector is the caller's local, so the copy is waited for)
int guided_select(mi355_ctx* ctx, const std::vector<GuidedPair>& table, const mi355_guided_params& p, mi355_sfpoint* d_a, mi355_sfpoint* d_b, int* d_nsel, int* d_dist) {
    const int n = (int)table.size();
    DevBuf& dt = ctx->buf("guided_pairs");
    MI_HIP(dt.reserve(sizeof(GuidedPair) * (size_t)n));
    MI_HIP(hipMemcpyAsync(dt.p, table.data(), sizeof(GuidedPair) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));
    const GuidedArgs ga{p.radius * p.radius, p.max_dist2, p.ratio * p.ratio, p.ratio > 0.0f ? 1 : 0, ctx->p.max_selected};
    double bytes = 0.0;
    for (const GuidedPair& g : table) bytes += 16.0 * (g.n_i + g.n_j) + 9600.0;
    ProfScope ps(ctx, "guided_select", bytes);
    hipLaunchKernelGGL(guided_select_kernel, dim3((unsigned)n), dim3(GM_NT), 0, ctx->stream, dt.as<GuidedPair>(), ga, d_a, d_b, d_nsel, d_dist);
    MI_HIP(hipGetLastError());
    return MI355_OK;
}

int guided_match_dev(mi355_ctx* ctx, const char* who, const int32_t* pairs_ij, int n, const float* guides, const mi355_guided_params* params, float dist, uint32_t seed,
                     mi355_pair_result* d_out) {
    mi355_guided_params p;
    std::vector<GuidedPair> table;
    { const int rc = guided_prepare(ctx, who, pairs_ij, n, guides, params, p, table); if (rc != MI355_OK) return rc; }
    if (n > 0 && !d_out) { ctx->set_error(std::string(who) + ": n=" + std::to_string(n) + " with NULL records"); return MI355_ERR_ARG; }
    if (n == 0) return MI355_OK;
    DevBuf &sa = ctx->buf("guided_sel_a"), &sb = ctx->buf("guided_sel_b"), &ns = ctx->buf("guided_nsel");
    MI_HIP(sa.reserve(sizeof(mi355_sfpoint) * MI355_MAX_SELECTED * (size_t)n));
    MI_HIP(sb.reserve(sizeof(mi355_sfpoint) * MI355_MAX_SELECTED * (size_t)n));
    MI_HIP(ns.reserve(sizeof(int) * (size_t)n));
    { const int rc = mi_ransac_tables(ctx, seed, nullptr); if (rc != MI355_OK) return rc; }      // a new seed's draw tables are built beside the selection
    { const int rc = guided_select(ctx, table, p, sa.as<mi355_sfpoint>(), sb.as<mi355_sfpoint>(), ns.as<int>(), nullptr); if (rc != MI355_OK) return rc; }
    // the pair stage's tail, unchanged
    { const int rc = mi_ransac_batch(ctx, sa.as<mi355_sfpoint>(), sb.as<mi355_sfpoint>(), ns.as<int>(), nullptr, n, MI355_MAX_SELECTED, dist, ctx->p.sample_times, seed, d_out,
                                     ctx->p.min_inliers); if (rc != MI355_OK) return rc; }
    return mi_finalize_pairs(ctx, pairs_ij, n, ns.as<int>(), d_out);
}

}  // namespace

extern "C" int mi355_guided_select_dev(mi355_ctx* ctx, const int32_t* pairs_ij, int n, const float* guides, const mi355_guided_params* params, mi355_sfpoint* d_a,
                                       mi355_sfpoint* d_b, int32_t* d_nsel, int32_t* d_dist) {
    LOCKED_PROLOGUE
    mi355_guided_params p;
    std::vector<GuidedPair> table;
    { const int rc = guided_prepare(ctx, "guided_select_dev", pairs_ij, n, guides, params, p, table); if (rc != MI355_OK) return rc; }
    if (n > 0 && (!d_a || !d_b || !d_nsel)) { ctx->set_error("guided_select_dev: n=" + std::to_string(n) + " with a NULL output list"); return MI355_ERR_ARG; }
    if (n == 0) return MI355_OK;
    return guided_select(ctx, table, p, d_a, d_b, d_nsel, d_dist);
}

extern "C" int mi355_guided_match_dev(mi355_ctx* ctx, const int32_t* pairs_ij, int n, const float* guides, const mi355_guided_params* params, float ransac_dist, uint32_t seed,
                                      mi355_pair_result* d_out) {
    LOCKED_PROLOGUE
    return guided_match_dev(ctx, "guided_match_dev", pairs_ij, n, guides, params, ransac_dist, seed, d_out);
}

extern "C" int mi355_guided_match(mi355_ctx* ctx, const int32_t* pairs_ij, int n, const float* guides, const mi355_guided_params* params, float ransac_dist, uint32_t seed,
                                  mi355_pair_result* out) {
    LOCKED_PROLOGUE
    DevBuf& dres = ctx->buf("guided_results");
    if (n > 0 && out) MI_HIP(dres.reserve(sizeof(mi355_pair_result) * (size_t)n));
    const int rc = guided_match_dev(ctx, "guided_match", pairs_ij, n, guides, params, ransac_dist, seed, n > 0 && out ? dres.as<mi355_pair_result>() : nullptr);
    if (rc != MI355_OK || n == 0) return rc;
    MI_HIP(hipMemcpyAsync(out, dres.p, sizeof(mi355_pair_result) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}
