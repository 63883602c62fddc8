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
#include "common.h"
#include "hmath.h"
#include "mosaic_frame.h"
#include "ramp.h"

namespace {

#ifndef FT_RPL_V
#define FT_RPL_V 2
#endif
constexpr int FT_W = 128, FT_RPL = FT_RPL_V, FT_H = 8 * FT_RPL;   // canvas tile of one workgroup: 256 lanes x 4 pixels x FT_RPL rows
static_assert(MOSAIC_LIST_BLOCK % FT_W == 0 && MOSAIC_LIST_BLOCK % FT_H == 0, "a tile lies inside one list block");
// (RampDev, ramp_weight and the weight omega_k itself: ramp.h, shared with seamline.hip)

__global__ __launch_bounds__(256) void feather_tile_kernel(const FrameDev* fr, const RampDev* ramps, int n, const uint16_t* lists, const int* counts, int bx_n,
                                                           uint8_t* canvas, int cw, int cws, int row0, int row_end, float dGx, float dGy) {
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * FT_W, ty0 = row0 + blockIdx.y * FT_H;
    // a lane owns 4 adjacent pixels in each of FT_RPL rows (rows ty0 + (tid >> 5) + 8 j), as in mosaic_tile_kernel
    const int xg = tx0 + 4 * (tid & 31), yB = ty0 + (tid >> 5);
    const int cb = ((ty0 - row0) / MOSAIC_LIST_BLOCK) * bx_n + tx0 / MOSAIC_LIST_BLOCK;
    const uint16_t* list = lists + (size_t)cb * n;
    const int cnt = counts[cb];
    unsigned acc[FT_RPL][4][4];                          // per pixel: sum omega B, sum omega G, sum omega R, sum omega
#pragma unroll
    for (int j = 0; j < FT_RPL; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) { acc[j][k][0] = 0; acc[j][k][1] = 0; acc[j][k][2] = 0; acc[j][k][3] = 0; }
    const int tx1 = tx0 + FT_W - 1 < cw - 1 ? tx0 + FT_W - 1 : cw - 1;
    const int ty1 = ty0 + FT_H - 1 < row_end - 1 ? ty0 + FT_H - 1 : row_end - 1;
    for (int e = 0; e < cnt; e++) {
        const FrameDev& f = fr[list[e]];                 // uniform over the workgroup: scalar loads
        if (f.begX > tx1 || f.endX < tx0 || f.begY > ty1 || f.endY < ty0) continue;
        const RampDev r = ramps[list[e]];
        const float w1 = (float)(f.w - 1), h1 = (float)(f.h - 1);
#pragma unroll
        for (int j = 0; j < FT_RPL; j++) {
            const int yD = yB + 8 * j;
            const bool yin = yD >= f.begY && yD <= f.endY;           // the box is clipped to the canvas and to the rows of this call
            const float yf = (float)yD - dGy;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int xD = xg + k;
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
    if (xg >= cw) return;
#pragma unroll
    for (int j = 0; j < FT_RPL; j++) {
        const int yD = yB + 8 * j;
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
        uint8_t* drow = canvas + (size_t)yD * cws + 3 * (size_t)xg;
        if (xg + 3 < cw) {
            uint32_t* d32 = reinterpret_cast<uint32_t*>(drow);
            d32[0] = out[0]; d32[1] = out[1]; d32[2] = out[2];
        } else {
#pragma unroll
            for (int b = 0; b < 9; b++)                  // at most 3 pixels
                if (xg + b / 3 < cw) drow[b] = (uint8_t)(out[b >> 2] >> (8 * (b & 3)));
        }
        // row padding [3 cw, cws): zero, as in the unblended render
        if (xg + 4 >= cw)
            for (int b = 3 * cw; b < cws; b++) canvas[(size_t)yD * cws + b] = 0;
    }
}

}  // namespace

int mi_mosaic_feathered_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                            const mi355_feather_params* params, uint8_t* d_canvas, int cw, int ch, int cws, int row0, int rows) {
    mi355_feather_params dp;
    if (!params) { mi355_default_feather_params(&dp); params = &dp; }
    if (params->ramp < 0) { ctx->set_error("mosaic_feathered: ramp=" + std::to_string(params->ramp) + " < 0"); return MI355_ERR_ARG; }
    int lw, lh, lws; float dG[2];
    int rc = mi355_mosaic_layout(w, h, n, h9s, &lw, &lh, &lws, dG);
    if (rc != MI355_OK) { ctx->set_error("mosaic_feathered: no image with h[8] != 0 / empty canvas"); return rc; }
    if (lw != cw || lh != ch || cws < cw * 3 || (cws & 3)) { ctx->set_error("mosaic_feathered: canvas geometry does not match mi355_mosaic_layout"); return MI355_ERR_ARG; }
    if (row0 < 0) row0 = 0;
    if (rows < 0 || row0 + rows > ch) rows = ch - row0;
    if (rows <= 0) return MI355_OK;
    if (n > 65535) { ctx->set_error("mosaic_feathered: at most 65535 images"); return MI355_ERR_ARG; }      // 16-bit lists; 255 * 255 * 65535 + 255 * 65535 / 2 < 2^32
    std::vector<FrameDev> fr;
    std::vector<RampDev> ramps;
    fr.reserve(n); ramps.reserve(n);
    for (int k = 0; k < n; k++) {
        FrameDev f;
        if (!mi_frame_dev_setup(h9s + 9 * k, w[k], h[k], dG, cw, ch, row0, rows, f)) continue;
        if (w[k] < 2 || h[k] < 2 || ws[k] < 3 * w[k] || w[k] > RAMP_MAX_SIDE || h[k] > RAMP_MAX_SIDE) { ctx->set_error("mosaic_feathered: bad image geometry"); return MI355_ERR_ARG; }
        // every frame whose box meets the rows is read: there is no "lies under later frames" case here
        if (!d_imgs[k]) { ctx->set_error("mosaic_feathered: the box of image " + std::to_string(k) + " meets these canvas rows but no pointer to it was given"); return MI355_ERR_ARG; }
        f.src = d_imgs[k]; f.w = w[k]; f.h = h[k]; f.ws = ws[k];
        fr.push_back(f);
        ramps.push_back(ramp_of_frame(w[k], h[k], params->ramp));
    }
    const int nf = (int)fr.size();
    const int bx_n = (cw + MOSAIC_LIST_BLOCK - 1) / MOSAIC_LIST_BLOCK, by_n = (rows + MOSAIC_LIST_BLOCK - 1) / MOSAIC_LIST_BLOCK;
    DevBuf& dfr = ctx->buf("mosaic_frames");
    DevBuf& dl = ctx->buf("mosaic_lists");
    DevBuf& dc = ctx->buf("mosaic_counts");
    DevBuf& dr = ctx->buf("feather_ramps");
    MI_HIP(dfr.reserve(sizeof(FrameDev) * (size_t)(nf > 0 ? nf : 1)));
    MI_HIP(dr.reserve(sizeof(RampDev) * (size_t)(nf > 0 ? nf : 1)));
    MI_HIP(dl.reserve(sizeof(uint16_t) * (size_t)bx_n * by_n * (size_t)(nf > 0 ? nf : 1)));
    MI_HIP(dc.reserve(sizeof(int) * (size_t)bx_n * by_n));
    if (nf > 0) {
        MI_HIP(hipMemcpyAsync(dfr.p, fr.data(), sizeof(FrameDev) * (size_t)nf, hipMemcpyHostToDevice, ctx->stream));
        MI_HIP(hipMemcpyAsync(dr.p, ramps.data(), sizeof(RampDev) * (size_t)nf, hipMemcpyHostToDevice, ctx->stream));
    }
    mi_mosaic_lists_launch(ctx, dfr.as<FrameDev>(), nf, bx_n, by_n, row0, dl.as<uint16_t>(), dc.as<int>());
    {
        ProfScope ps(ctx, "feather", 0.0);
        hipLaunchKernelGGL(feather_tile_kernel, dim3((cw + FT_W - 1) / FT_W, (rows + FT_H - 1) / FT_H), dim3(256), 0, ctx->stream,
                           dfr.as<FrameDev>(), dr.as<RampDev>(), nf, dl.as<uint16_t>(), dc.as<int>(), bx_n, d_canvas, cw, cws, row0, row0 + rows, dG[0], dG[1]);
    }
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(ctx->stream));           // `fr` and `ramps` go out of scope
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

// the host form: mi355_mosaic_refined's staging, the feathered render in its place
extern "C" int mi355_mosaic_feathered(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                      const mi355_feather_params* params, uint8_t** canvas, int* cw, int* ch, int* cws) {
    LOCKED_PROLOGUE
    if (!imgs || !w || !h || !ws || !h9s || !canvas || !cw || !ch || !cws) return MI355_ERR_ARG;
    if (n <= 1) { ctx->set_error("mosaic_feathered: needs more than one image"); return MI355_ERR_FAILED; }
    int lw, lh, lws;
    int rc = mi355_mosaic_layout(w, h, n, h9s, &lw, &lh, &lws, nullptr);
    if (rc != MI355_OK) { ctx->set_error("mosaic_feathered: empty canvas"); return rc; }
    size_t total = 0;
    std::vector<size_t> off(n, 0);
    for (int k = 0; k < n; k++) { if (h9s[9 * k + 8] == 0.0f) continue; if (!imgs[k] || w[k] < 2 || h[k] < 2 || ws[k] < 3 * w[k]) return MI355_ERR_ARG; off[k] = total; total += ((size_t)ws[k] * h[k] + 255) & ~(size_t)255; }
    DevBuf& dall = ctx->buf("mosaic_srcs");
    DevBuf& dcan = ctx->buf("mosaic_canvas");
    MI_HIP(dall.reserve(total + 16));
    MI_HIP(dcan.reserve((size_t)lws * lh));
    std::vector<const uint8_t*> dptr(n, nullptr);
    for (int k = 0; k < n; k++) {
        if (h9s[9 * k + 8] == 0.0f) continue;
        dptr[k] = dall.as<uint8_t>() + off[k];
        MI_HIP(hipMemcpyAsync((void*)dptr[k], imgs[k], (size_t)ws[k] * h[k], hipMemcpyHostToDevice, ctx->stream));
    }
    rc = mi_mosaic_feathered_dev(ctx, dptr.data(), w, h, ws, n, h9s, params, dcan.as<uint8_t>(), lw, lh, lws, 0, lh);
    if (rc != MI355_OK) return rc;
    uint8_t* out = (uint8_t*)malloc((size_t)lws * lh);
    if (!out) return MI355_ERR_NOMEM;
    hipError_t e = hipMemcpyAsync(out, dcan.p, (size_t)lws * lh, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { free(out); ctx->set_error(hipGetErrorString(e)); return MI355_ERR_DEVICE; }
    *canvas = out; *cw = lw; *ch = lh; *cws = lws;
    return MI355_OK;
}
