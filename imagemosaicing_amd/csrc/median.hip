// csrc/median.hip -- the median render (gfx950): every canvas pixel the per-channel median of its `depth` deepest frames, so that what shows in
// a minority of the looks -- a car, a walker, a drifting shadow -- drops out of the overlaps.  The definition is in include/mi355_mosaic.h
// ("median render"): among the frames that give the pixel a sample the m = min(count, depth) largest in the seamline order (omega_k, k) are
// selected, each channel of their samples is sorted, and the byte is the rounded mean of the two middle values (the median for odd m).  The
// by-products are the coverage count (the seamline render's map) and the spread of the selected samples.
//
//   median_tile_kernel<K, SAMPLE>  one launch over canvas tiles of 128 x 8 RPL pixels (RPL = md_rpl(K)), the lane layout and the per-256 x 256
//                         block candidate lists of the other one-pass renders (mosaic_frame.h: tile_lane).
//                         Phase 1, the selection walk: every frame of the list whose box meets the tile is mapped (frame_src), tested
//                         (src_inside) and weighed (ramp_omega) for each of the lane's pixels, exactly as seamline_tile_kernel does; no texel is
//                         loaded.  A pixel keeps its K largest keys omega << 16 | q, sorted descending, and the number of frames that gave a
//                         sample.  q is the position in the frame table, filled in ascending caller index, so key order is (omega, k) order; keys
//                         are distinct and non-zero, 0 is an empty slot.  A key enters through a max / min chain (hi = max(slot, x); x = min(slot,
//                         x); slot = hi -- 2 K VALU operations, no per-lane branch), whose result does not depend on the walk order.  A depth
//                         below K uses the first `depth` slots of the smallest K >= depth that is built (1, 3, 5, 9): exact, the list is sorted.
//                         Phase 2, in the same kernel (the keys never leave their registers): the m selected frames of a pixel are sampled
//                         (frame_sample3, a per-lane gather of the frame record through the table; xs, ys RECOMPUTED with phase 1's expression,
//                         -ffp-contract=off: the same bits, as seamline.hip does and for its reason), one packed B G R word per sample; per
//                         channel a fixed compare-exchange network (3, 9, 25 exchanges for K = 3, 5, 9; absent slots carry 256 and sort last),
//                         v[(m-1) >> 1] and v[m >> 1] picked by index with selects, the byte and the spread formed.
//                         <K, false>: phase 2 is left out -- the count map alone, or the per-frame "is selected somewhere" flags (the cover call,
//                         and the check that precedes a render some of whose frames came without a pointer).
// Registers, as the compiler reports them when cross-compiling for gfx950 (-Rpass-analysis=kernel-resource-usage); no instantiation uses
// scratch (ScratchSize 0, no SGPR or VGPR spill):
//                         K   RPL   pixels / lane   <K, true>: VGPRs, waves / SIMD    <K, false>: VGPRs, waves / SIMD
//                         1   2     8               60, 8                             60, 8
//                         3   1     4               48, 8                             46, 8
//                         5   1     4               57, 8                             54, 8
//                         9   1     4               93, 5                             70, 7
//                         A lane carries 4 RPL (K + 1) registers of keys and counts through the walk.  With two rows per lane, the seamline
//                         kernel's shape, K = 3 takes 76 VGPRs (6 waves), K = 5 92 (5 waves) and K = 9 124 in the walk alone (4 waves) and 135
//                         plus 304 bytes of scratch with phase 2 (3 waves): one row per lane keeps K = 3 and 5 at the seamline kernel's 8 waves
//                         and K = 9 out of scratch, at the price of paying the workgroup-uniform frame record, ramp and box test once per 4
//                         pixels of a lane instead of once per 8 (-DMD_RPL_V=1 or 2 builds every K with that many rows).  K = 9's phase 2 holds
//                         the 9 sample words of one pixel beside the 27 keys of the lane's other three: 93 VGPRs.
// The host path around the launches -- entry check, frame table, lists, used flags, the host form -- is mosaic_frame.h's.
#include "common.h"
#include "hmath.h"
#include "mosaic_frame.h"
#include "ramp.h"

namespace {

constexpr int MD_W = 128;
#ifdef MD_RPL_V
constexpr int md_rpl(int) { return MD_RPL_V; }          // kernel A/B builds: the same rows per lane for every K
#else
constexpr int md_rpl(int K) { return K <= 1 ? 2 : 1; }  // rows per lane: see the register table in the file head
#endif

// ---- compare-exchange networks, as (a, b) pairs with a < b: after each the smaller value lies at a ----------------------------------------
template <int... P> struct Net {};
using Net1 = Net<>;
using Net3 = Net<0, 2, 0, 1, 1, 2>;
using Net5 = Net<0, 3, 1, 4, 0, 2, 1, 3, 0, 1, 2, 4, 1, 2, 3, 4, 2, 3>;                                   // 9 exchanges (Knuth, TAOCP 3, 5.3.4)
using Net9 = Net<0, 3, 1, 7, 2, 5, 4, 8, 0, 7, 2, 4, 3, 8, 5, 6, 0, 2, 1, 3, 4, 5, 7, 8, 1, 4, 3, 6, 5, 7, 0, 1, 2, 4, 3, 5, 6, 8, 2, 3, 4, 5, 6, 7,
                 1, 2, 3, 4, 5, 6>;                                                                        // 25 exchanges, the optimum for 9
template <int K> struct NetOf;
template <> struct NetOf<1> { using type = Net1; };
template <> struct NetOf<3> { using type = Net3; };
template <> struct NetOf<5> { using type = Net5; };
template <> struct NetOf<9> { using type = Net9; };

// the zero-one principle: a network that sorts every 0 / 1 input sorts every input
template <int... P>
constexpr bool net_sorts(Net<P...>, int K) {
    constexpr int np = sizeof...(P);
    const int p[np + 1] = {P..., 0};
    for (int i = 0; i < np; i += 2) if (!(p[i] >= 0 && p[i] < p[i + 1] && p[i + 1] < K)) return false;
    for (unsigned in = 0; in < (1u << K); in++) {
        unsigned v = in;
        for (int i = 0; i < np; i += 2) {
            const unsigned a = (v >> p[i]) & 1u, b = (v >> p[i + 1]) & 1u;
            if (a > b) v ^= (1u << p[i]) | (1u << p[i + 1]);
        }
        for (int i = 0; i + 1 < K; i++) if (((v >> i) & 1u) > ((v >> (i + 1)) & 1u)) return false;
    }
    return true;
}
static_assert(net_sorts(Net1{}, 1) && net_sorts(Net3{}, 3) && net_sorts(Net5{}, 5) && net_sorts(Net9{}, 9), "a compare-exchange network does not sort");

__device__ __forceinline__ void net_sort(unsigned*, Net<>) {}
template <int A, int B, int... Rest>
__device__ __forceinline__ void net_sort(unsigned* v, Net<A, B, Rest...>) {
    const unsigned lo = v[A] < v[B] ? v[A] : v[B], hi = v[A] < v[B] ? v[B] : v[A];
    v[A] = lo; v[B] = hi;
    net_sort(v, Net<Rest...>{});
}

template <int K, bool SAMPLE>
__global__ __launch_bounds__(256) void median_tile_kernel(const FrameDev* fr, const RampDev* ramps, int n, const uint16_t* lists, const int* counts,
                                                          int bx_n, uint8_t* canvas, uint8_t* spread, uint16_t* count, int* used, int cw, int cws,
                                                          int row0, int row_end, float dGx, float dGy, int depth) {
    constexpr int RPL = md_rpl(K);
    const TileLane t = tile_lane<MD_W, RPL>(lists, counts, n, bx_n, cw, row0, row_end);
    const int xg = t.xg;
    unsigned key[RPL][4][K], cov[RPL][4];                // per pixel: the K largest omega << 16 | q, descending (0: empty), and the number of contributing frames
#pragma unroll
    for (int j = 0; j < RPL; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            cov[j][k] = 0;
#pragma unroll
            for (int i = 0; i < K; i++) key[j][k][i] = 0;
        }
    // ---- phase 1: which frames each pixel selects ----
    for (int e = 0; e < t.cnt; e++) {
        const unsigned q = t.list[e];
        const FrameDev& f = fr[q];                       // uniform over the workgroup: scalar loads
        if (f.begX > t.tx1 || f.endX < t.tx0 || f.begY > t.ty1 || f.endY < t.ty0) continue;
        const RampDev r = ramps[q];
        const float w1 = (float)(f.w - 1), h1 = (float)(f.h - 1);
#pragma unroll
        for (int j = 0; j < RPL; j++) {
            const int yD = t.yB + 8 * j;
            const bool yin = yD >= f.begY && yD <= f.endY;           // the box is clipped to the canvas and to the rows of this call
            const float yf = (float)yD - dGy;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int xD = xg + k;
                const float xf = (float)xD - dGx;
                float xs, ys;
                frame_src(f, xf, yf, xs, ys);
                if (!(yin && xD >= f.begX && xD <= f.endX && src_inside(xs, ys, w1, h1))) continue;
                unsigned x = (ramp_omega(f, r, xs, ys) << 16) | q;
                cov[j][k]++;
#pragma unroll
                for (int i = 0; i < K; i++) {            // the key sinks to its place; what falls off the end is dropped
                    const unsigned s = key[j][k][i], hi = s > x ? s : x;
                    x = s > x ? x : s;
                    key[j][k][i] = hi;
                }
            }
        }
    }
    if (xg >= cw) return;
#pragma unroll
    for (int j = 0; j < RPL; j++) {
        const int yD = t.yB + 8 * j;
        if (yD >= row_end) continue;
        // a pixel at or beyond cw lies in no frame's box: its count stays 0
        if (used) {
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int i = 0; i < K; i++)
                    if (i < depth && key[j][k][i]) used[key[j][k][i] & 0xffffu] = 1;
        }
        if (count) store_map4(count + (size_t)yD * cw, xg, cw, cov[j]);
        if constexpr (SAMPLE) {
            // ---- phase 2: the selected frames' samples, the median of each channel ----
            uint32_t out[3] = {0, 0, 0};                 // 12 bytes: B G R of the 4 pixels
            uint32_t spr = 0;                            // 4 bytes: the spread of the 4 pixels
            const float yf = (float)yD - dGy;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int m = (int)cov[j][k] < depth ? (int)cov[j][k] : depth;
                if (m == 0) continue;                    // no frame covers the pixel
                unsigned s[K];                           // B | G << 8 | R << 16 of the i-th selected frame
#pragma unroll
                for (int i = 0; i < K; i++) {
                    s[i] = 0;
                    if (i >= m) continue;
                    const FrameDev& f = fr[key[j][k][i] & 0xffffu];  // per lane: a gather through the frame table
                    float xs, ys;
                    frame_src(f, (float)(xg + k) - dGx, yf, xs, ys); // phase 1's expression: the same bits
                    unsigned vb, vg, vr;
                    frame_sample3(f, xs, ys, vb, vg, vr);
                    s[i] = vb | (vg << 8) | (vr << 16);
                }
                const int ia = (m - 1) >> 1, ib = m >> 1;
                unsigned widest = 0;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    unsigned v[K];
#pragma unroll
                    for (int i = 0; i < K; i++) v[i] = i < m ? (s[i] >> (8 * c)) & 0xffu : 256u;     // an absent slot sorts last
                    net_sort(v, typename NetOf<K>::type{});
                    unsigned a = v[0], b = v[0], top = v[0];
#pragma unroll
                    for (int i = 1; i < K; i++) {
                        a = i == ia ? v[i] : a;
                        b = i == ib ? v[i] : b;
                        top = i == m - 1 ? v[i] : top;
                    }
                    const unsigned byte = (a + b + 1u) >> 1, d = top - v[0];
                    widest = d > widest ? d : widest;
                    out[(3 * k + c) >> 2] |= byte << (8 * ((3 * k + c) & 3));                        // static positions
                }
                spr |= widest << (8 * k);
            }
            if (canvas) store_row12(canvas, cw, cws, xg, yD, out);
            if (spread) {
                uint8_t* srow = spread + (size_t)yD * cw;
                if (xg + 3 < cw) __builtin_memcpy(srow + xg, &spr, 4);
                else {
#pragma unroll
                    for (int k = 0; k < 3; k++)          // at most 3 pixels
                        if (xg + k < cw) srow[xg + k] = (uint8_t)(spr >> (8 * k));
                }
            }
        }
    }
}

using MedianKernel = void (*)(const FrameDev*, const RampDev*, int, const uint16_t*, const int*, int, uint8_t*, uint8_t*, uint16_t*, int*, int, int, int, int,
                              float, float, int);

// the smallest built K >= depth
template <bool SAMPLE>
MedianKernel median_kernel_of(int depth, int& K) {
    if (depth <= 1) { K = 1; return median_tile_kernel<1, SAMPLE>; }
    if (depth <= 3) { K = 3; return median_tile_kernel<3, SAMPLE>; }
    if (depth <= 5) { K = 5; return median_tile_kernel<5, SAMPLE>; }
    K = 9; return median_tile_kernel<9, SAMPLE>;
}

}  // namespace

static_assert(MI355_MEDIAN_MAX_DEPTH == 9, "the largest instantiation of median_tile_kernel");

// cover_only != NULL (with the three outputs NULL): cover_only[k] = 1 for the frames that are among the selected of at least one pixel of the
// rows; nothing is sampled or stored, and cw, ch, cws are the layout's whatever the caller passes
int mi_mosaic_median_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                         const mi355_median_params* params, uint8_t* d_canvas, int cw, int ch, int cws, uint8_t* d_spread, uint16_t* d_count,
                         int row0, int rows, uint8_t* cover_only) {
    mi355_median_params dp;
    if (!params) { mi355_default_median_params(&dp); params = &dp; }
    if (params->ramp < 0) { ctx->set_error("mosaic_median: ramp=" + std::to_string(params->ramp) + " < 0"); return MI355_ERR_ARG; }
    if (params->depth < 0 || params->depth > MI355_MEDIAN_MAX_DEPTH) {
        ctx->set_error("mosaic_median: depth=" + std::to_string(params->depth) + " outside 0.." + std::to_string(MI355_MEDIAN_MAX_DEPTH));
        return MI355_ERR_ARG;
    }
    const int depth = params->depth ? params->depth : 5;
    const bool sample = d_canvas || d_spread;            // phase 2 runs: the frames are read
    float dG[2]; bool go;
    const int rc = mi_render_entry(ctx, "mosaic_median", w, h, n, h9s, cover_only != nullptr, d_canvas != nullptr, cw, ch, cws, row0, rows, dG, go);     // n <= 65535: 16-bit lists, keys and counts
    if (rc != MI355_OK || !go) return rc;
    FrameTable t;                                        // ascending caller index: (omega, q) orders as (omega, k)
    bool withheld = false;
    for (int k = 0; k < n; k++) {
        FrameDev f;
        if (!mi_frame_dev_setup(h9s + 9 * k, w[k], h[k], dG, cw, ch, row0, rows, f)) continue;
        if (w[k] < 2 || h[k] < 2 || (sample && ws[k] < 3 * w[k]) || w[k] > RAMP_MAX_SIDE || h[k] > RAMP_MAX_SIDE) { ctx->set_error("mosaic_median: bad image geometry"); return MI355_ERR_ARG; }
        f.src = sample ? d_imgs[k] : nullptr; f.w = w[k]; f.h = h[k]; f.ws = sample ? ws[k] : 0;
        if (sample && !f.src) withheld = true;           // fine as long as no pixel of the rows selects the frame: checked below, before any sample
        t.add(f, k);
        t.ramps.push_back(ramp_of_frame(w[k], h[k], params->ramp));
    }
    if (cover_only && t.fr.empty()) return MI355_OK;
    const int rc2 = mi_frame_table_upload(ctx, t, true, false, cw, rows, row0);
    if (rc2 != MI355_OK) return rc2;
    int K;
    const MedianKernel walk = median_kernel_of<false>(depth, K), render = median_kernel_of<true>(depth, K);
    const int th = 8 * md_rpl(K);
    const dim3 grid((cw + MD_W - 1) / MD_W, (rows + th - 1) / th);
    auto launch = [&](MedianKernel kernel, uint8_t* canvas, uint8_t* spread, uint16_t* count, int* used) {
        ProfScope ps(ctx, "median", 0.0);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, t.d_fr, t.d_ramps, t.nf, t.d_lists, t.d_counts, t.bx_n, canvas, spread, count, used,
                           cw, cws, row0, row0 + rows, dG[0], dG[1], depth);
    };
    if (cover_only || withheld) {
        // the selection walk alone, one flag per table entry: the cover call's answer, and what tells a withheld frame that no pixel selects
        // (left out by the caller with reason) from one the render would dereference.  Paid only when a pointer is missing.
        std::vector<int> used;
        int* d_used;
        int rc3 = mi_frame_table_used_begin(ctx, t, &d_used);
        if (rc3 != MI355_OK) return rc3;
        launch(walk, nullptr, nullptr, nullptr, d_used);
        rc3 = mi_frame_table_used_end(ctx, t, used);
        if (rc3 != MI355_OK) return rc3;
        for (int q = 0; q < t.nf; q++) {
            if (!used[q]) continue;
            if (cover_only) cover_only[t.frame_of[q]] = 1;
            else if (!t.fr[q].src) {
                ctx->set_error("mosaic_median: image " + std::to_string(t.frame_of[q]) + " is among the selected frames of these canvas rows but no pointer to it was given");
                return MI355_ERR_ARG;
            }
        }
        if (cover_only) return MI355_OK;
    }
    if (sample) launch(render, d_canvas, d_spread, d_count, nullptr);
    else launch(walk, nullptr, nullptr, d_count, nullptr);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(ctx->stream));           // the table goes out of scope
    return MI355_OK;
}

extern "C" void mi355_default_median_params(mi355_median_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
}

extern "C" int mi355_mosaic_median_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                       const mi355_median_params* params, uint8_t* d_canvas, int cw, int ch, int cws, uint8_t* d_spread,
                                       uint16_t* d_count, int row0, int rows) {
    LOCKED_PROLOGUE
    if (!w || !h || !h9s || n <= 0) return MI355_ERR_ARG;
    if (!d_canvas && !d_spread && !d_count) { ctx->set_error("mosaic_median: d_canvas, d_spread and d_count are all NULL"); return MI355_ERR_ARG; }
    if ((d_canvas || d_spread) && (!d_imgs || !ws)) { ctx->set_error("mosaic_median: a canvas or a spread map is asked for but d_imgs or ws is NULL"); return MI355_ERR_ARG; }
    return mi_mosaic_median_dev(ctx, d_imgs, w, h, ws, n, h9s, params, d_canvas, cw, ch, cws, d_spread, d_count, row0, rows, nullptr);
}

extern "C" int mi355_mosaic_median_cover(mi355_ctx* ctx, const int* w, const int* h, int n, const float* h9s, const mi355_median_params* params,
                                         int row0, int rows, uint8_t* need) {
    LOCKED_PROLOGUE
    if (!w || !h || !h9s || !need || n <= 0) return MI355_ERR_ARG;
    memset(need, 0, (size_t)n);
    return mi_mosaic_median_dev(ctx, nullptr, w, h, nullptr, n, h9s, params, nullptr, 0, 0, 0, nullptr, nullptr, row0, rows, need);
}

// the host form (mi_render_host_begin / _end, frames.hip); the spread map comes back when asked for
extern "C" int mi355_mosaic_median(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                   const mi355_median_params* params, uint8_t** canvas, int* cw, int* ch, int* cws, uint8_t** spread) {
    LOCKED_PROLOGUE
    if (!imgs || !w || !h || !ws || !h9s || !canvas || !cw || !ch || !cws) return MI355_ERR_ARG;
    int lw, lh, lws;
    std::vector<const uint8_t*> d_imgs;
    uint8_t* d_canvas;
    int rc = mi_render_host_begin(ctx, "mosaic_median", imgs, w, h, ws, n, h9s, &lw, &lh, &lws, d_imgs, &d_canvas);
    if (rc != MI355_OK) return rc;
    DevBuf& down = ctx->buf("median_spread");
    const size_t sbytes = (size_t)lw * lh;
    if (spread) MI_HIP(down.reserve(sbytes));
    rc = mi_mosaic_median_dev(ctx, d_imgs.data(), w, h, ws, n, h9s, params, d_canvas, lw, lh, lws, spread ? down.as<uint8_t>() : nullptr, nullptr, 0, lh, nullptr);
    if (rc != MI355_OK) return rc;
    return mi_render_host_end(ctx, lw, lh, lws, canvas, cw, ch, cws, down.p, sbytes, (void**)spread);
}
