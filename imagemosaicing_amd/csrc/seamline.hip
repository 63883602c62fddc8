// csrc/seamline.hip -- the seamline render (gfx950): every canvas pixel from exactly one frame, the frame in which it lies deepest.  The
// definition is in include/mi355_mosaic.h ("seamline render"): among the frames that give the pixel a sample the owner is the argmax of
// (omega_k, k), omega_k the feather weight (ramp.h); the canvas takes the owner's sample, and the walk's by-products are an owner map and a
// coverage count.
//
//   seamline_tile_kernel  one launch over canvas tiles of 128 x 8 SL_RPL pixels, the shape and the per-256 x 256-block candidate lists of
//                         mosaic_tile_kernel (warp.hip) and feather_tile_kernel.
//                         Phase 1, the ownership walk: every frame of the list whose box meets the tile is mapped (frame_src), tested
//                         (src_inside) and weighed (ramp_omega) for each of the lane's pixels; no texel is loaded.  The frame record and its
//                         ramp are uniform over the workgroup (scalar loads).  A lane keeps per pixel one packed key omega << 16 | q as a running
//                         maximum and the number of frames that gave a sample.  q is the frame's position in the compacted frame table, which is
//                         filled in ascending caller index, so that the maximum over keys is the maximum over (omega, k) whatever the walk order;
//                         the caller's k of an entry is carried beside the table (frame_of) for the owner map.
//                         Phase 2, in the same kernel (the keys never leave their registers): one sample per pixel from the winning frame, a
//                         per-lane gather of the frame record through the table.  xs, ys are RECOMPUTED there with phase 1's expression
//                         (-ffp-contract=off: the same bits) rather than kept: keeping them is 2 more live VGPRs per pixel over the whole walk
//                         -- the compiler reports 78 VGPRs (6 waves per SIMD) with them kept against 60 (8 waves) as built -- while the
//                         recomputation is a handful of multiply-adds per pixel, once (-DSL_KEEP_XY_V=1 builds the other form).
//                         <false>: phase 2 is left out -- the maps alone (d_canvas == NULL) or the per-frame "owns a pixel" flags (the cover
//                         call, and the check that precedes a render some of whose frames came without a pointer).
// The lane / tile prologue and the row and map stores (tile_lane, store_row12, store_map4) and the host path around the launches -- entry check, frame table,
// lists, used flags, the host form -- are mosaic_frame.h's, shared with warp.hip and feather.hip; the walk is spelt out here.
#include "common.h"
#include "hmath.h"
#include "mosaic_frame.h"
#include "ramp.h"

namespace {

#ifndef SL_RPL_V
#define SL_RPL_V 2
#endif
#ifndef SL_KEEP_XY_V
#define SL_KEEP_XY_V 0                          // 1: keep the winner's xs, ys from phase 1 (kernel A/B builds)
#endif
constexpr int SL_W = 128, SL_RPL = SL_RPL_V, SL_H = 8 * SL_RPL;   // canvas tile of one workgroup: 256 lanes x 4 pixels x SL_RPL rows

template <bool SAMPLE>
__global__ __launch_bounds__(256) void seamline_tile_kernel(const FrameDev* fr, const RampDev* ramps, const int* frame_of, int n, const uint16_t* lists,
                                                            const int* counts, int bx_n, uint8_t* canvas, uint16_t* owner, uint16_t* count, int* used,
                                                            int cw, int cws, int row0, int row_end, float dGx, float dGy) {
    const TileLane t = tile_lane<SL_W, SL_RPL>(lists, counts, n, bx_n, cw, row0, row_end);
    const int xg = t.xg;
    unsigned key[SL_RPL][4], cov[SL_RPL][4];             // per pixel: max of omega << 16 | q (0: no frame), the number of contributing frames
#if SL_KEEP_XY_V
    float kx[SL_RPL][4], ky[SL_RPL][4];
#endif
#pragma unroll
    for (int j = 0; j < SL_RPL; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) { key[j][k] = 0; cov[j][k] = 0; }
    // ---- phase 1: who owns each pixel ----
    for (int e = 0; e < t.cnt; e++) {
        const unsigned q = t.list[e];
        const FrameDev& f = fr[q];                       // uniform over the workgroup: scalar loads
        if (f.begX > t.tx1 || f.endX < t.tx0 || f.begY > t.ty1 || f.endY < t.ty0) continue;
        const RampDev r = ramps[q];
        const float w1 = (float)(f.w - 1), h1 = (float)(f.h - 1);
#pragma unroll
        for (int j = 0; j < SL_RPL; j++) {
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
                const unsigned kq = (ramp_omega(f, r, xs, ys) << 16) | q;
                cov[j][k]++;
                if (kq > key[j][k]) {
                    key[j][k] = kq;
#if SL_KEEP_XY_V
                    kx[j][k] = xs; ky[j][k] = ys;
#endif
                }
            }
        }
    }
    if (xg >= cw) return;
#pragma unroll
    for (int j = 0; j < SL_RPL; j++) {
        const int yD = t.yB + 8 * j;
        if (yD >= row_end) continue;
        // a pixel at or beyond cw lies in no frame's box: its key stays 0
        if (used) {
#pragma unroll
            for (int k = 0; k < 4; k++) if (key[j][k]) used[key[j][k] & 0xffffu] = 1;
        }
        if (owner) {
            unsigned o[4];
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = key[j][k] ? (unsigned)frame_of[key[j][k] & 0xffffu] + 1u : 0u;
            store_map4(owner + (size_t)yD * cw, xg, cw, o);
        }
        if (count) store_map4(count + (size_t)yD * cw, xg, cw, cov[j]);
        if constexpr (SAMPLE) {
            // ---- phase 2: the owner's sample, once per pixel ----
            uint32_t out[3] = {0, 0, 0};                 // 12 bytes: B G R of the 4 pixels
            const float yf = (float)yD - dGy;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!key[j][k]) continue;                // no frame covers the pixel
                const FrameDev& f = fr[key[j][k] & 0xffffu];         // per lane: a gather through the frame table
                float xs, ys;
#if SL_KEEP_XY_V
                xs = kx[j][k]; ys = ky[j][k];
#else
                frame_src(f, (float)(xg + k) - dGx, yf, xs, ys);     // phase 1's expression: the same bits
#endif
                unsigned v[3];
                frame_sample3(f, xs, ys, v[0], v[1], v[2]);
#pragma unroll
                for (int c = 0; c < 3; c++) out[(3 * k + c) >> 2] |= v[c] << (8 * ((3 * k + c) & 3));      // static positions
            }
            store_row12(canvas, cw, cws, xg, yD, out);
        }
    }
}

}  // namespace

// cover_only != NULL (with the three outputs NULL): cover_only[k] = 1 for the frames that own at least one pixel of the rows; nothing is
// sampled or stored, and cw, ch, cws are the layout's whatever the caller passes
int mi_mosaic_seamline_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                           const mi355_seamline_params* params, uint8_t* d_canvas, int cw, int ch, int cws, uint16_t* d_owner, uint16_t* d_count,
                           int row0, int rows, uint8_t* cover_only) {
    mi355_seamline_params dp;
    if (!params) { mi355_default_seamline_params(&dp); params = &dp; }
    if (params->ramp < 0) { ctx->set_error("mosaic_seamline: ramp=" + std::to_string(params->ramp) + " < 0"); return MI355_ERR_ARG; }
    float dG[2]; bool go;
    const int rc = mi_render_entry(ctx, "mosaic_seamline", w, h, n, h9s, cover_only != nullptr, d_canvas != nullptr, cw, ch, cws, row0, rows, dG, go);     // n <= 65535: 16-bit lists, keys and maps (owner + 1 <= 65535)
    if (rc != MI355_OK || !go) return rc;
    FrameTable t;                                        // frame_of ascending: (omega, q) orders as (omega, k)
    bool withheld = false;
    for (int k = 0; k < n; k++) {
        FrameDev f;
        if (!mi_frame_dev_setup(h9s + 9 * k, w[k], h[k], dG, cw, ch, row0, rows, f)) continue;
        if (w[k] < 2 || h[k] < 2 || (d_canvas && ws[k] < 3 * w[k]) || w[k] > RAMP_MAX_SIDE || h[k] > RAMP_MAX_SIDE) { ctx->set_error("mosaic_seamline: bad image geometry"); return MI355_ERR_ARG; }
        f.src = d_canvas ? d_imgs[k] : nullptr; f.w = w[k]; f.h = h[k]; f.ws = d_canvas ? ws[k] : 0;
        if (d_canvas && !f.src) withheld = true;         // fine as long as the frame owns no pixel of the rows: checked below, before any sample
        t.add(f, k);
        t.ramps.push_back(ramp_of_frame(w[k], h[k], params->ramp));
    }
    if (cover_only && t.fr.empty()) return MI355_OK;
    const int rc2 = mi_frame_table_upload(ctx, t, true, true, cw, rows, row0);
    if (rc2 != MI355_OK) return rc2;
    const dim3 grid((cw + SL_W - 1) / SL_W, (rows + SL_H - 1) / SL_H);
    auto launch = [&](auto kernel, uint8_t* canvas, uint16_t* owner, uint16_t* count, int* used) {
        ProfScope ps(ctx, "seamline", 0.0);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, t.d_fr, t.d_ramps, t.d_frame_of, t.nf, t.d_lists, t.d_counts, t.bx_n, canvas, owner,
                           count, used, cw, cws, row0, row0 + rows, dG[0], dG[1]);
    };
    if (cover_only || withheld) {
        // the ownership walk alone, one flag per table entry: the cover call's answer, and what tells a withheld frame that owns nothing
        // (left out by the caller with reason) from one the render would dereference.  Paid only when a pointer is missing.
        std::vector<int> used;
        int* d_used;
        int rc3 = mi_frame_table_used_begin(ctx, t, &d_used);
        if (rc3 != MI355_OK) return rc3;
        launch(seamline_tile_kernel<false>, nullptr, nullptr, nullptr, d_used);
        rc3 = mi_frame_table_used_end(ctx, t, used);
        if (rc3 != MI355_OK) return rc3;
        for (int q = 0; q < t.nf; q++) {
            if (!used[q]) continue;
            if (cover_only) cover_only[t.frame_of[q]] = 1;
            else if (!t.fr[q].src) {
                ctx->set_error("mosaic_seamline: image " + std::to_string(t.frame_of[q]) + " owns pixels of these canvas rows but no pointer to it was given");
                return MI355_ERR_ARG;
            }
        }
        if (cover_only) return MI355_OK;
    }
    if (d_canvas) launch(seamline_tile_kernel<true>, d_canvas, d_owner, d_count, nullptr);
    else launch(seamline_tile_kernel<false>, nullptr, d_owner, d_count, nullptr);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(ctx->stream));           // the table goes out of scope
    return MI355_OK;
}

extern "C" void mi355_default_seamline_params(mi355_seamline_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
}

extern "C" int mi355_mosaic_seamline_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                         const mi355_seamline_params* params, uint8_t* d_canvas, int cw, int ch, int cws, uint16_t* d_owner,
                                         uint16_t* d_count, int row0, int rows) {
    LOCKED_PROLOGUE
    if (!w || !h || !h9s || n <= 0) return MI355_ERR_ARG;
    if (!d_canvas && !d_owner && !d_count) { ctx->set_error("mosaic_seamline: d_canvas, d_owner and d_count are all NULL"); return MI355_ERR_ARG; }
    if (d_canvas && (!d_imgs || !ws)) { ctx->set_error("mosaic_seamline: a canvas is asked for but d_imgs or ws is NULL"); return MI355_ERR_ARG; }
    return mi_mosaic_seamline_dev(ctx, d_imgs, w, h, ws, n, h9s, params, d_canvas, cw, ch, cws, d_owner, d_count, row0, rows, nullptr);
}

extern "C" int mi355_mosaic_seamline_cover(mi355_ctx* ctx, const int* w, const int* h, int n, const float* h9s, const mi355_seamline_params* params,
                                           int row0, int rows, uint8_t* need) {
    LOCKED_PROLOGUE
    if (!w || !h || !h9s || !need || n <= 0) return MI355_ERR_ARG;
    memset(need, 0, (size_t)n);
    return mi_mosaic_seamline_dev(ctx, nullptr, w, h, nullptr, n, h9s, params, nullptr, 0, 0, 0, nullptr, nullptr, row0, rows, need);
}

// the host form (mi_render_host_begin / _end, frames.hip); the owner map comes back when asked for
extern "C" int mi355_mosaic_seamline(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                     const mi355_seamline_params* params, uint8_t** canvas, int* cw, int* ch, int* cws, uint16_t** owner) {
    LOCKED_PROLOGUE
    if (!imgs || !w || !h || !ws || !h9s || !canvas || !cw || !ch || !cws) return MI355_ERR_ARG;
    int lw, lh, lws;
    std::vector<const uint8_t*> d_imgs;
    uint8_t* d_canvas;
    int rc = mi_render_host_begin(ctx, "mosaic_seamline", imgs, w, h, ws, n, h9s, &lw, &lh, &lws, d_imgs, &d_canvas);
    if (rc != MI355_OK) return rc;
    DevBuf& down = ctx->buf("seamline_owner");
    const size_t obytes = sizeof(uint16_t) * (size_t)lw * lh;
    if (owner) MI_HIP(down.reserve(obytes));
    rc = mi_mosaic_seamline_dev(ctx, d_imgs.data(), w, h, ws, n, h9s, params, d_canvas, lw, lh, lws, owner ? down.as<uint16_t>() : nullptr, nullptr, 0, lh, nullptr);
    if (rc != MI355_OK) return rc;
    return mi_render_host_end(ctx, lw, lh, lws, canvas, cw, ch, cws, down.p, obytes, (void**)owner);
}
