// csrc/feather.hip -- weighted (feather) blending as a one-pass mosaic render (gfx950): UavMatchParam.blending = 1 (MosaicWithoutPos.h:65), the
// mode the reference declares and never implements (MosaicWithoutPos.cpp:4666-4672 falls through to the unblended render).  The definition is
// in include/mi355_mosaic.h ("weighted (feather) blending"): every frame that gives a canvas pixel a sample contributes that sample with an
// integer weight that ramps up from the frame's border, and the pixel is the rounded integer mean.
//
//   feather_tile_kernel   one launch over canvas tiles of 128 x 8 FT_RPL pixels, the shape and the per-256 x 256-block candidate lists of
//                         mosaic_tile_kernel (warp.hip).  The walk has no early exit: every frame of the list whose box meets the tile is
//                         mapped (frame_src), tested (src_inside) and sampled (frame_sample3) for each of the lane's pixels, and the lane keeps
//                         four 32-bit sums per pixel -- weight x B, G, R and the weight.  The weight comes from the sample's own xi, yi: the
//                         border distances of the 2 x 2 texels, each through the ramp quotient (254 min(d, R)) / R by a per-frame multiply-
//                         and-shift that is exact for these operands, then hm::bilin with the sample's p, q.  No weight image exists.  The
//                         frame record, its ramp constants and the box test are uniform over the workgroup (scalar loads).  The epilogue
//                         divides (three exact unsigned divisions per pixel) and stores 12 bytes per row like the unblended render.
//                         Integer sums: the bytes do not depend on the walk order, the tile shape or the stripe cut.
// The lane / tile prologue and the row store (tile_lane, store_row12) and the host path around the launch -- entry check, frame table, lists,
// the host form -- are mosaic_frame.h's, shared with warp.hip and seamline.hip; the walk is spelt out here (mosaic_frame.h says why).
#include "common.h"
#include "hmath.h"
#include "mosaic_frame.h"
#include "ramp.h"

namespace {

#ifndef FT_RPL_V
#define FT_RPL_V 2
#endif
constexpr int FT_W = 128, FT_RPL = FT_RPL_V, FT_H = 8 * FT_RPL;   // canvas tile of one workgroup: 256 lanes x 4 pixels x FT_RPL rows
// (ramp_weight and the weight omega_k itself: ramp.h, shared with seamline.hip)

__global__ __launch_bounds__(256) void feather_tile_kernel(const FrameDev* fr, const RampDev* ramps, int n, const uint16_t* lists, const int* counts, int bx_n,
                                                           uint8_t* canvas, int cw, int cws, int row0, int row_end, float dGx, float dGy) {
    const TileLane t = tile_lane<FT_W, FT_RPL>(lists, counts, n, bx_n, cw, row0, row_end);
    unsigned acc[FT_RPL][4][4];                          // per pixel: sum omega B, sum omega G, sum omega R, sum omega
#pragma unroll
    for (int j = 0; j < FT_RPL; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) { acc[j][k][0] = 0; acc[j][k][1] = 0; acc[j][k][2] = 0; acc[j][k][3] = 0; }
    for (int e = 0; e < t.cnt; e++) {
        const FrameDev& f = fr[t.list[e]];               // uniform over the workgroup: scalar loads
        if (f.begX > t.tx1 || f.endX < t.tx0 || f.begY > t.ty1 || f.endY < t.ty0) continue;
        const RampDev r = ramps[t.list[e]];
        const float w1 = (float)(f.w - 1), h1 = (float)(f.h - 1);
#pragma unroll
        for (int j = 0; j < FT_RPL; j++) {
            const int yD = t.yB + 8 * j;
            const bool yin = yD >= f.begY && yD <= f.endY;           // the box is clipped to the canvas and to the rows of this call
            const float yf = (float)yD - dGy;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int xD = t.xg + k;
                const float xf = (float)xD - dGx;
                float xs, ys;
                frame_src(f, xf, yf, xs, ys);
                if (!(yin && xD >= f.begX && xD <= f.endX && src_inside(xs, ys, w1, h1))) continue;
                unsigned vb, vg, vr;
                frame_sample3(f, xs, ys, vb, vg, vr);
                const unsigned om = ramp_omega(f, r, xs, ys);        // the weight through the sample's own xi, yi, p, q (ramp.h)
                acc[j][k][0] += om * vb; acc[j][k][1] += om * vg; acc[j][k][2] += om * vr; acc[j][k][3] += om;
            }
        }
    }
    if (t.xg >= cw) return;
#pragma unroll
    for (int j = 0; j < FT_RPL; j++) {
        const int yD = t.yB + 8 * j;
        if (yD >= row_end) continue;
        uint32_t out[3] = {0, 0, 0};                     // 12 bytes: B G R of the 4 pixels
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned s = acc[j][k][3];
            if (s == 0) continue;                        // no frame covers the pixel
            const unsigned half = s >> 1;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const unsigned v = (acc[j][k][c] + half) / s;
                out[(3 * k + c) >> 2] |= v << (8 * ((3 * k + c) & 3));      // static positions
            }
        }
        store_row12(canvas, cw, cws, t.xg, yD, out);
    }
}

}  // namespace

int mi_mosaic_feathered_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                            const mi355_feather_params* params, uint8_t* d_canvas, int cw, int ch, int cws, int row0, int rows) {
    mi355_feather_params dp;
    if (!params) { mi355_default_feather_params(&dp); params = &dp; }
    if (params->ramp < 0) { ctx->set_error("mosaic_feathered: ramp=" + std::to_string(params->ramp) + " < 0"); return MI355_ERR_ARG; }
    float dG[2]; bool go;
    const int rc = mi_render_entry(ctx, "mosaic_feathered", w, h, n, h9s, false, true, cw, ch, cws, row0, rows, dG, go);     // n <= 65535: 255 * 255 * 65535 + 255 * 65535 / 2 < 2^32
    if (rc != MI355_OK || !go) return rc;
    FrameTable t;
    for (int k = 0; k < n; k++) {
        FrameDev f;
        if (!mi_frame_dev_setup(h9s + 9 * k, w[k], h[k], dG, cw, ch, row0, rows, f)) continue;
        if (w[k] < 2 || h[k] < 2 || ws[k] < 3 * w[k] || w[k] > RAMP_MAX_SIDE || h[k] > RAMP_MAX_SIDE) { ctx->set_error("mosaic_feathered: bad image geometry"); return MI355_ERR_ARG; }
        // every frame whose box meets the rows is read: there is no "lies under later frames" case here
        if (!d_imgs[k]) { ctx->set_error("mosaic_feathered: the box of image " + std::to_string(k) + " meets these canvas rows but no pointer to it was given"); return MI355_ERR_ARG; }
        f.src = d_imgs[k]; f.w = w[k]; f.h = h[k]; f.ws = ws[k];
        t.add(f, k);
        t.ramps.push_back(ramp_of_frame(w[k], h[k], params->ramp));
    }
    const int rc2 = mi_frame_table_upload(ctx, t, true, false, cw, rows, row0);
    if (rc2 != MI355_OK) return rc2;
    {
        ProfScope ps(ctx, "feather", 0.0);
        hipLaunchKernelGGL(feather_tile_kernel, dim3((cw + FT_W - 1) / FT_W, (rows + FT_H - 1) / FT_H), dim3(256), 0, ctx->stream,
                           t.d_fr, t.d_ramps, t.nf, t.d_lists, t.d_counts, t.bx_n, d_canvas, cw, cws, row0, row0 + rows, dG[0], dG[1]);
    }
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(ctx->stream));           // the table goes out of scope
    return MI355_OK;
}

extern "C" void mi355_default_feather_params(mi355_feather_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
}

extern "C" int mi355_mosaic_feathered_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                          const mi355_feather_params* params, uint8_t* d_canvas, int cw, int ch, int cws, int row0, int rows) {
    LOCKED_PROLOGUE
    if (!d_imgs || !w || !h || !ws || !h9s || !d_canvas || n <= 0) return MI355_ERR_ARG;
    return mi_mosaic_feathered_dev(ctx, d_imgs, w, h, ws, n, h9s, params, d_canvas, cw, ch, cws, row0, rows);
}

// the host form (mi_render_host_begin / _end, frames.hip)
extern "C" int mi355_mosaic_feathered(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                      const mi355_feather_params* params, uint8_t** canvas, int* cw, int* ch, int* cws) {
    LOCKED_PROLOGUE
    if (!imgs || !w || !h || !ws || !h9s || !canvas || !cw || !ch || !cws) return MI355_ERR_ARG;
    int lw, lh, lws;
    std::vector<const uint8_t*> d_imgs;
    uint8_t* d_canvas;
    int rc = mi_render_host_begin(ctx, "mosaic_feathered", imgs, w, h, ws, n, h9s, &lw, &lh, &lws, d_imgs, &d_canvas);
    if (rc == MI355_OK) rc = mi_mosaic_feathered_dev(ctx, d_imgs.data(), w, h, ws, n, h9s, params, d_canvas, lw, lh, lws, 0, lh);
    if (rc != MI355_OK) return rc;
    return mi_render_host_end(ctx, lw, lh, lws, canvas, cw, ch, cws);
}
