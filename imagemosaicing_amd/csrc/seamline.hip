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
static_assert(MOSAIC_LIST_BLOCK % SL_W == 0 && MOSAIC_LIST_BLOCK % SL_H == 0, "a tile lies inside one list block");

// four 16-bit map entries of a lane's pixel group: 8 bytes at once where the group is whole
__device__ __forceinline__ void store_map4(uint16_t* row, int xg, int cw, const unsigned v[4]) {
    if (xg + 3 < cw) {
        const uint32_t two[2] = {v[0] | (v[1] << 16), v[2] | (v[3] << 16)};
        __builtin_memcpy(row + xg, two, 8);
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++)                      // at most 3 pixels
            if (xg + k < cw) row[xg + k] = (uint16_t)v[k];
    }
}

template <bool SAMPLE>
__global__ __launch_bounds__(256) void seamline_tile_kernel(const FrameDev* fr, const RampDev* ramps, const int* frame_of, int n, const uint16_t* lists,
                                                            const int* counts, int bx_n, uint8_t* canvas, uint16_t* owner, uint16_t* count, int* used,
                                                            int cw, int cws, int row0, int row_end, float dGx, float dGy) {
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * SL_W, ty0 = row0 + blockIdx.y * SL_H;
    // a lane owns 4 adjacent pixels in each of SL_RPL rows (rows ty0 + (tid >> 5) + 8 j), as in mosaic_tile_kernel
    const int xg = tx0 + 4 * (tid & 31), yB = ty0 + (tid >> 5);
    const int cb = ((ty0 - row0) / MOSAIC_LIST_BLOCK) * bx_n + tx0 / MOSAIC_LIST_BLOCK;
    const uint16_t* list = lists + (size_t)cb * n;
    const int cnt = counts[cb];
    unsigned key[SL_RPL][4], cov[SL_RPL][4];             // per pixel: max of omega << 16 | q (0: no frame), the number of contributing frames
#if SL_KEEP_XY_V
    float kx[SL_RPL][4], ky[SL_RPL][4];
#endif
#pragma unroll
    for (int j = 0; j < SL_RPL; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) { key[j][k] = 0; cov[j][k] = 0; }
    const int tx1 = tx0 + SL_W - 1 < cw - 1 ? tx0 + SL_W - 1 : cw - 1;
    const int ty1 = ty0 + SL_H - 1 < row_end - 1 ? ty0 + SL_H - 1 : row_end - 1;
    // ---- phase 1: who owns each pixel ----
    for (int e = 0; e < cnt; e++) {
        const unsigned q = list[e];
        const FrameDev& f = fr[q];                       // uniform over the workgroup: scalar loads
        if (f.begX > tx1 || f.endX < tx0 || f.begY > ty1 || f.endY < ty0) continue;
        const RampDev r = ramps[q];
        const float w1 = (float)(f.w - 1), h1 = (float)(f.h - 1);
#pragma unroll
        for (int j = 0; j < SL_RPL; j++) {
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
        const int yD = yB + 8 * j;
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
            uint8_t* drow = canvas + (size_t)yD * cws + 3 * (size_t)xg;
            if (xg + 3 < cw) {
                uint32_t* d32 = reinterpret_cast<uint32_t*>(drow);
                d32[0] = out[0]; d32[1] = out[1]; d32[2] = out[2];
            } else {
#pragma unroll
                for (int b = 0; b < 9; b++)              // at most 3 pixels
                    if (xg + b / 3 < cw) drow[b] = (uint8_t)(out[b >> 2] >> (8 * (b & 3)));
            }
            // row padding [3 cw, cws): zero, as in the unblended render
            if (xg + 4 >= cw)
                for (int b = 3 * cw; b < cws; b++) canvas[(size_t)yD * cws + b] = 0;
        }
    }
}

}  // namespace

// cover_only != NULL: cover_only[k] = 1 for the frames that own at least one pixel of the rows; nothing is sampled or stored (d_imgs, ws and the
// three outputs are not looked at)
int mi_mosaic_seamline_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                           const mi355_seamline_params* params, uint8_t* d_canvas, int cw, int ch, int cws, uint16_t* d_owner, uint16_t* d_count,
                           int row0, int rows, uint8_t* cover_only) {
    mi355_seamline_params dp;
    if (!params) { mi355_default_seamline_params(&dp); params = &dp; }
    if (params->ramp < 0) { ctx->set_error("mosaic_seamline: ramp=" + std::to_string(params->ramp) + " < 0"); return MI355_ERR_ARG; }
    int lw, lh, lws; float dG[2];
    int rc = mi355_mosaic_layout(w, h, n, h9s, &lw, &lh, &lws, dG);
    if (rc != MI355_OK) { ctx->set_error("mosaic_seamline: no image with h[8] != 0 / empty canvas"); return rc; }
    if (cover_only) { cw = lw; ch = lh; cws = lws; d_canvas = nullptr; d_owner = d_count = nullptr; }
    if (lw != cw || lh != ch || (d_canvas && (cws < cw * 3 || (cws & 3)))) { ctx->set_error("mosaic_seamline: canvas geometry does not match mi355_mosaic_layout"); return MI355_ERR_ARG; }
    if (row0 < 0) row0 = 0;
    if (rows < 0 || row0 + rows > ch) rows = ch - row0;
    if (rows <= 0) return MI355_OK;
    if (n > 65535) { ctx->set_error("mosaic_seamline: at most 65535 images"); return MI355_ERR_ARG; }      // 16-bit lists, keys and maps (owner + 1 <= 65535)
    std::vector<FrameDev> fr;
    std::vector<RampDev> ramps;
    std::vector<int> frame_of;                           // the caller's k of table entry q, ascending: (omega, q) orders as (omega, k)
    fr.reserve(n); ramps.reserve(n); frame_of.reserve(n);
    bool withheld = false;
    for (int k = 0; k < n; k++) {
        FrameDev f;
        if (!mi_frame_dev_setup(h9s + 9 * k, w[k], h[k], dG, cw, ch, row0, rows, f)) continue;
        if (w[k] < 2 || h[k] < 2 || (d_canvas && ws[k] < 3 * w[k]) || w[k] > RAMP_MAX_SIDE || h[k] > RAMP_MAX_SIDE) { ctx->set_error("mosaic_seamline: bad image geometry"); return MI355_ERR_ARG; }
        f.src = d_canvas ? d_imgs[k] : nullptr; f.w = w[k]; f.h = h[k]; f.ws = d_canvas ? ws[k] : 0;
        if (d_canvas && !f.src) withheld = true;         // fine as long as the frame owns no pixel of the rows: checked below, before any sample
        fr.push_back(f);
        ramps.push_back(ramp_of_frame(w[k], h[k], params->ramp));
        frame_of.push_back(k);
    }
    const int nf = (int)fr.size();
    if (cover_only && nf == 0) return MI355_OK;
    const int bx_n = (cw + MOSAIC_LIST_BLOCK - 1) / MOSAIC_LIST_BLOCK, by_n = (rows + MOSAIC_LIST_BLOCK - 1) / MOSAIC_LIST_BLOCK;
    const size_t nf1 = (size_t)(nf > 0 ? nf : 1);
    DevBuf& dfr = ctx->buf("mosaic_frames");
    DevBuf& dl = ctx->buf("mosaic_lists");
    DevBuf& dc = ctx->buf("mosaic_counts");
    DevBuf& dr = ctx->buf("feather_ramps");
    DevBuf& dk = ctx->buf("seamline_frame_of");
    MI_HIP(dfr.reserve(sizeof(FrameDev) * nf1));
    MI_HIP(dr.reserve(sizeof(RampDev) * nf1));
    MI_HIP(dk.reserve(sizeof(int) * nf1));
    MI_HIP(dl.reserve(sizeof(uint16_t) * (size_t)bx_n * by_n * nf1));
    MI_HIP(dc.reserve(sizeof(int) * (size_t)bx_n * by_n));
    if (nf > 0) {
        MI_HIP(hipMemcpyAsync(dfr.p, fr.data(), sizeof(FrameDev) * (size_t)nf, hipMemcpyHostToDevice, ctx->stream));
        MI_HIP(hipMemcpyAsync(dr.p, ramps.data(), sizeof(RampDev) * (size_t)nf, hipMemcpyHostToDevice, ctx->stream));
        MI_HIP(hipMemcpyAsync(dk.p, frame_of.data(), sizeof(int) * (size_t)nf, hipMemcpyHostToDevice, ctx->stream));
    }
    mi_mosaic_lists_launch(ctx, dfr.as<FrameDev>(), nf, bx_n, by_n, row0, dl.as<uint16_t>(), dc.as<int>());
    const dim3 grid((cw + SL_W - 1) / SL_W, (rows + SL_H - 1) / SL_H);
    if (cover_only || withheld) {
        // the ownership walk alone, one flag per table entry: the cover call's answer, and what tells a withheld frame that owns nothing
        // (left out by the caller with reason) from one the render would dereference.  Paid only when a pointer is missing.
        DevBuf& du = ctx->buf("mosaic_used");
        MI_HIP(du.reserve(sizeof(int) * nf1));
        MI_HIP(hipMemsetAsync(du.p, 0, sizeof(int) * nf1, ctx->stream));
        {
            ProfScope ps(ctx, "seamline", 0.0);
            hipLaunchKernelGGL(seamline_tile_kernel<false>, grid, dim3(256), 0, ctx->stream, dfr.as<FrameDev>(), dr.as<RampDev>(), dk.as<int>(), nf,
                               dl.as<uint16_t>(), dc.as<int>(), bx_n, (uint8_t*)nullptr, (uint16_t*)nullptr, (uint16_t*)nullptr, du.as<int>(), cw, cws,
                               row0, row0 + rows, dG[0], dG[1]);
        }
        MI_HIP(hipGetLastError());
        std::vector<int> used(nf1, 0);
        MI_HIP(hipMemcpyAsync(used.data(), du.p, sizeof(int) * nf1, hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));
        if (cover_only) {
            for (int q = 0; q < nf; q++) if (used[q]) cover_only[frame_of[q]] = 1;
            return MI355_OK;
        }
        for (int q = 0; q < nf; q++)
            if (used[q] && !fr[q].src) {
                ctx->set_error("mosaic_seamline: image " + std::to_string(frame_of[q]) + " owns pixels of these canvas rows but no pointer to it was given");
                return MI355_ERR_ARG;
            }
    }
    {
        ProfScope ps(ctx, "seamline", 0.0);
        if (d_canvas)
            hipLaunchKernelGGL(seamline_tile_kernel<true>, grid, dim3(256), 0, ctx->stream, dfr.as<FrameDev>(), dr.as<RampDev>(), dk.as<int>(), nf,
                               dl.as<uint16_t>(), dc.as<int>(), bx_n, d_canvas, d_owner, d_count, (int*)nullptr, cw, cws, row0, row0 + rows, dG[0], dG[1]);
        else
            hipLaunchKernelGGL(seamline_tile_kernel<false>, grid, dim3(256), 0, ctx->stream, dfr.as<FrameDev>(), dr.as<RampDev>(), dk.as<int>(), nf,
                               dl.as<uint16_t>(), dc.as<int>(), bx_n, (uint8_t*)nullptr, d_owner, d_count, (int*)nullptr, cw, cws, row0, row0 + rows, dG[0], dG[1]);
    }
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(ctx->stream));           // `fr`, `ramps` and `frame_of` go out of scope
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

// the host form: mi355_mosaic_refined's staging, the seamline render in its place; the owner map comes back when asked for
extern "C" int mi355_mosaic_seamline(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                     const mi355_seamline_params* params, uint8_t** canvas, int* cw, int* ch, int* cws, uint16_t** owner) {
    LOCKED_PROLOGUE
    if (!imgs || !w || !h || !ws || !h9s || !canvas || !cw || !ch || !cws) return MI355_ERR_ARG;
    if (n <= 1) { ctx->set_error("mosaic_seamline: needs more than one image"); return MI355_ERR_FAILED; }
    int lw, lh, lws;
    int rc = mi355_mosaic_layout(w, h, n, h9s, &lw, &lh, &lws, nullptr);
    if (rc != MI355_OK) { ctx->set_error("mosaic_seamline: empty canvas"); return rc; }
    size_t total = 0;
    std::vector<size_t> off(n, 0);
    for (int k = 0; k < n; k++) { if (h9s[9 * k + 8] == 0.0f) continue; if (!imgs[k] || w[k] < 2 || h[k] < 2 || ws[k] < 3 * w[k]) return MI355_ERR_ARG; off[k] = total; total += ((size_t)ws[k] * h[k] + 255) & ~(size_t)255; }
    const size_t cbytes = (size_t)lws * lh, obytes = owner ? sizeof(uint16_t) * (size_t)lw * lh : 0;
    DevBuf& dall = ctx->buf("mosaic_srcs");
    DevBuf& dcan = ctx->buf("mosaic_canvas");
    DevBuf& down = ctx->buf("seamline_owner");
    MI_HIP(dall.reserve(total + 16));
    MI_HIP(dcan.reserve(cbytes));
    if (owner) MI_HIP(down.reserve(obytes));
    std::vector<const uint8_t*> dptr(n, nullptr);
    for (int k = 0; k < n; k++) {
        if (h9s[9 * k + 8] == 0.0f) continue;
        dptr[k] = dall.as<uint8_t>() + off[k];
        MI_HIP(hipMemcpyAsync((void*)dptr[k], imgs[k], (size_t)ws[k] * h[k], hipMemcpyHostToDevice, ctx->stream));
    }
    rc = mi_mosaic_seamline_dev(ctx, dptr.data(), w, h, ws, n, h9s, params, dcan.as<uint8_t>(), lw, lh, lws, owner ? down.as<uint16_t>() : nullptr, nullptr, 0, lh, nullptr);
    if (rc != MI355_OK) return rc;
    uint8_t* out = (uint8_t*)malloc(cbytes);
    uint16_t* own = owner ? (uint16_t*)malloc(obytes) : nullptr;
    if (!out || (owner && !own)) { free(out); free(own); return MI355_ERR_NOMEM; }
    hipError_t e = hipMemcpyAsync(out, dcan.p, cbytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && owner) e = hipMemcpyAsync(own, down.p, obytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { free(out); free(own); ctx->set_error(hipGetErrorString(e)); return MI355_ERR_DEVICE; }
    *canvas = out; *cw = lw; *ch = lh; *cws = lws;
    if (owner) *owner = own;
    return MI355_OK;
}
