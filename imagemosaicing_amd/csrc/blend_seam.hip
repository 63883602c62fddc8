// csrc/blend_seam.hip -- the multiband blend along optimised seams (gfx950): the seam finder of seamcut.hip in front of the multiband blender.
// The definition is in include/mi355_mosaic.h ("multiband blend along optimised seams"); tests/blend_seam_ref.py restates it in numpy.
//
// The cell map of mi355_seam_cells_dev lives on mi355_mosaic_layout's canvas under the seamline's sample rule and feather weights; the blend
// has a canvas of its own (it always contains the origin), chips with sub-pixel shifts, and the normalised-distance arg-max of
// FindMasksByDistMap for a seam.  So stage 1 is made again in the blend's geometry and the ownership learns to follow a map; the label stage
// (mi_seam_labels_dev) and the blender (blend.hip) are used as they are.
//
//   blend_seam_candidates_kernel  one wave per cell.  A cell lies inside one 256 x 256 ownership block (the cell side divides 256): its chips
//                           come from that block's list.  Phase 1, the probe: the lanes share out the list, each computes for its chips the
//                           value owner_kernel computes at the probe pixel -- quad_min_dist over the chip's maximum, the same operations, so the
//                           same bits -- where the chip's validity byte is set, and keeps its own sorted top 8 of the 64-bit keys
//                           d_bits << 16 | (0xffff - position).  d > 0, so the float order is the bit order, and among equal d the lower
//                           position is the larger key: slot 0 is the pixel's FindMasksByDistMap owner.  `depth` rounds of a wave-wide maximum
//                           draw the slots, the lane that held the winner popping it.  Phase 2, the signatures: for each drawn chip the lanes
//                           walk the cell's pixels (clipped to the canvas) and add gray << 11 | 1 of the chip's own bytes where its validity
//                           byte is set: sum (<= 255 * 1024 < 2^18) and count (<= 1024 < 2^11) in one word, one butterfly.
//                           It runs after distmax_kernel (the maxima) and before any ownership rewrite of the masks (validity).
//   owner_cells_kernel      owner_kernel with one more input.  A thread's four rows start at a multiple of 4 and the cell side is >= 4: one map
//                           load per thread.  A candidate whose image the cell names and whose byte is set takes the lead with bd = +inf; no
//                           later d > bd can pass, and a NaN or 0 distance does not matter to it.  Everything else is owner_kernel's walk.
// Registers, as the compiler reports them for gfx950 with the library's flags (-Rpass-analysis=kernel-resource-usage; neither kernel uses
// scratch): blend_seam_candidates_kernel 71 VGPRs (7 waves per SIMD, as seam_candidates_kernel), owner_cells_kernel 56 (8 waves per SIMD).
// The host side of both kernels is warp.hip's ChipStage (chips.h: the SEAM forms); this file has the launches, the entry checks and the C ABI.
#include "common.h"
#include "chips.h"
#include "chip_own.h"

static_assert(MI355_SEAMCUT_MAX_DEPTH == 8, "a lane's top 8 keys");

namespace {

constexpr int BS_SLOTS = MI355_SEAMCUT_MAX_DEPTH;

__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64);
        const unsigned long long t = ((unsigned long long)hi << 32) | lo;
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ unsigned wave_sum32(unsigned v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void blend_seam_candidates_kernel(const ChipDev* chips, uint8_t* const* masks, const uint8_t* const* pixels, const int* img,
                                                                    const unsigned* maxbits, const LineSet* lines, const int* list_off, const int* list, int bx_n,
                                                                    mi355_seam_cell* out, int gw, int gh, int cw, int ch, int level, int depth) {
    const int lane = threadIdx.x & 63;
    const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= (long long)gw * gh) return;              // the whole wave
    const int cy = (int)(cell / gw), cx = (int)(cell - (long long)cy * gw);
    const int s = 1 << level, x0 = cx << level, y0 = cy << level;
    const int px = x0 + s / 2 < cw - 1 ? x0 + s / 2 : cw - 1, py = y0 + s / 2 < ch - 1 ? y0 + s / 2 : ch - 1;
    const int blk = (y0 / OWN_BLK) * bx_n + x0 / OWN_BLK;                        // a cell lies inside one ownership block: s divides 256
    const int l0 = list_off[blk], l1 = list_off[blk + 1];
    // ---- phase 1: the lane's own top 8 at the probe, then the wave's top `depth` ----
    unsigned long long key[BS_SLOTS];
#pragma unroll
    for (int i = 0; i < BS_SLOTS; i++) key[i] = 0;
    for (int e = l0 + lane; e < l1; e += 64) {
        const int q = list[e];
        const ChipDev cd = chips[q];
        const int xC = px - cd.x0, yC = py - cd.y0;
        if (xC < 0 || xC >= cd.w || yC < 0 || yC >= cd.h) continue;
        if (masks[q][(size_t)yC * cd.mws + xC] == 0) continue;
        const float d = quad_min_dist(lines[q], xC, yC) / __uint_as_float(maxbits[q]);      // owner_kernel's value: the same operations
        if (!(d > 0.0f)) continue;                                                           // 0 and NaN own nothing there either
        unsigned long long x = ((unsigned long long)__float_as_uint(d) << 16) | (unsigned long long)(0xffffu - (unsigned)q);
#pragma unroll
        for (int i = 0; i < BS_SLOTS; i++) {             // the key sinks to its place; what falls off the end is dropped
            const unsigned long long sl = key[i], hi = sl > x ? sl : x;
            x = sl > x ? x : sl;
            key[i] = hi;
        }
    }
    mi355_seam_cell rec;
    memset(&rec, 0, sizeof(rec));
#pragma unroll
    for (int i = 0; i < BS_SLOTS; i++) {
        if (i >= depth) break;
        const unsigned long long best = wave_max64(key[0]);
        if (!best) break;                                // uniform: fewer candidates than depth
        if (key[0] == best) {                            // one lane: keys are distinct
#pragma unroll
            for (int j = 0; j + 1 < BS_SLOTS; j++) key[j] = key[j + 1];
            key[BS_SLOTS - 1] = 0;
        }
        // ---- phase 2: the chip's gray over the cell's pixels where it has a sample ----
        const int q = (int)(0xffffu - (unsigned)(best & 0xffffu));              // uniform over the wave
        const ChipDev cd = chips[q];
        const uint8_t* mask = masks[q];
        const uint8_t* pix = pixels[q];
        const int cws = (cd.w * 3 + 3) & ~3;
        unsigned acc = 0;                                // gray sum << 11 | samples
        for (int idx = lane; idx < s * s; idx += 64) {
            const int xD = x0 + (idx & (s - 1)), yD = y0 + (idx >> level);
            const int xC = xD - cd.x0, yC = yD - cd.y0;
            if (xD >= cw || yD >= ch || xC < 0 || xC >= cd.w || yC < 0 || yC >= cd.h) continue;
            if (mask[(size_t)yC * cd.mws + xC] == 0) continue;
            const uint8_t* p = pix + (size_t)yC * cws + 3 * xC;
            acc += (((1868u * p[0] + 9617u * p[1] + 4899u * p[2] + 8192u) >> 14) << 11) | 1u;
        }
        acc = wave_sum32(acc);
        const unsigned tot = acc >> 11, num = acc & 0x7ffu;                    // num >= 1: the probe is one of the pixels
        const float d = __uint_as_float((unsigned)(best >> 16));
        rec.frame[i] = (uint16_t)(img[q] + 1);
        rec.omega[i] = (uint8_t)(1 + (int)fminf(d * 254.0f, 254.0f));
        rec.gray[i] = (uint8_t)((tot + num / 2) / (num ? num : 1u));
    }
    if (lane == 0) out[cell] = rec;
}

// owner_kernel (warp.hip) with the cell map: see there for the walk, the staging and the one-pass mask rewrite
__global__ __launch_bounds__(256) void owner_cells_kernel(const ChipDev* chips, const LineSet* lines, const unsigned* maxbits, const int* list_off, const int* list,
                                                          int bx_n, int rectW, int rectH, uint8_t* const* masks, const int* img, const uint16_t* cells, int gw,
                                                          int level) {
    constexpr int NE = 32;
    __shared__ OwnEntry s_e[NE];
    __shared__ int s_img[NE];
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = (blockIdx.y * blockDim.y + threadIdx.y) * OWN_ROWS;                                  // first of the thread's rows
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    const bool inside = c < rectW && r < rectH;
    const int rb = (blockIdx.y * blockDim.y * OWN_ROWS) / OWN_BLK, cb = (blockIdx.x * blockDim.x) / OWN_BLK;      // the workgroup (64 x 16 pixels) lies inside one block
    const int blk = rb * bx_n + cb;
    const int l0 = list_off[blk], l1 = list_off[blk + 1];
    // the image the cell of the thread's four pixels names, -1: none (r is a multiple of 4 <= the cell side: the rows share a cell row)
    const int want = inside ? (int)cells[(size_t)(r >> level) * gw + (c >> level)] - 1 : -1;
    float bd[OWN_ROWS];
    uint8_t* lead[OWN_ROWS];                                      // the leader's mask byte
#pragma unroll
    for (int j = 0; j < OWN_ROWS; j++) { bd[j] = 0.0f; lead[j] = nullptr; }
    for (int base = l0; base < l1; base += NE) {
        const int ne = l1 - base < NE ? l1 - base : NE;
        __syncthreads();
        if (tid < ne) {
            const int k = list[base + tid];
            const ChipDev cd = chips[k];
            OwnEntry e;
            e.x0 = cd.x0; e.y0 = cd.y0; e.w = cd.w; e.h = cd.h; e.mws = cd.mws; e.k = k; e.maxv = __uint_as_float(maxbits[k]); e.pad = 0;
            e.mask = masks[k]; e.L = lines[k];
            s_e[tid] = e;
            s_img[tid] = img[k];
        }
        __syncthreads();
        if (!inside) continue;
        uint8_t nxt[OWN_ROWS];
        auto fetch = [&](int q, uint8_t* out) {
            const OwnEntry& e = s_e[q];
            const int xC = c - e.x0, yC0 = r - e.y0;
            const bool xin = xC >= 0 && xC < e.w;
#pragma unroll
            for (int j = 0; j < OWN_ROWS; j++) {
                const int yC = yC0 + j;
                out[j] = (xin && yC >= 0 && yC < e.h && r + j < rectH) ? e.mask[(size_t)yC * e.mws + xC] : (uint8_t)0;
            }
        };
        fetch(0, nxt);
        for (int q = 0; q < ne; q++) {
            const OwnEntry& e = s_e[q];
            uint8_t cur[OWN_ROWS];
#pragma unroll
            for (int j = 0; j < OWN_ROWS; j++) cur[j] = nxt[j];
            if (q + 1 < ne) fetch(q + 1, nxt);
            const int xC = c - e.x0, yC0 = r - e.y0;
            if (xC < 0 || xC >= e.w || yC0 + OWN_ROWS - 1 < 0 || yC0 >= e.h) continue;
            const bool wanted = s_img[q] == want;                   // (want = -1 names nobody: image indices are >= 0)
            float ac[4];
#pragma unroll
            for (int i = 0; i < 4; i++) ac[i] = e.L.A[i] * (float)xC;      // the first product of quad_min_dist's expression
#pragma unroll
            for (int j = 0; j < OWN_ROWS; j++) {
                const int yC = yC0 + j;
                if (yC < 0 || yC >= e.h || r + j >= rectH) continue;
                uint8_t* m = e.mask + (size_t)yC * e.mws + xC;
                if (cur[j] != 0) {
                    float minDist = (float)(1 << 29);                       // quad_min_dist(e.L, xC, yC), same operations
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const float dd = fabsf(ac[i] + e.L.B[i] * (float)yC + e.L.C[i]) * e.L.inv[i];
                        if (dd < minDist) minDist = dd;
                    }
                    const float d = wanted ? __builtin_inff() : minDist / e.maxv;      // validity is enough for the named chip
                    if (d > bd[j]) { bd[j] = d; if (lead[j]) *lead[j] = 0; lead[j] = m; }
                    else *m = 0;
                }
            }
        }
    }
}

// the blend's layout at this level, the grid against it, and a pointer for every frame that gives a chip
int seam_entry(mi355_ctx* ctx, const char* who, const uint8_t* const* imgs, const int* w, const int* h, int n, const float* h9s, const uint8_t* keep,
               const mi355_seamcut_params* params, int gw, int gh, int* cw, int* ch) {
    const std::string me(who);
    int rc = mi_seamcut_params_check(ctx, who, params);
    if (rc != MI355_OK) return rc;
    if (params->ramp != 0) { ctx->set_error(me + ": ramp=" + std::to_string(params->ramp) + " has no meaning for the blend's seams and must be 0"); return MI355_ERR_ARG; }
    if (n > 65535) { ctx->set_error(me + ": at most 65535 images"); return MI355_ERR_ARG; }      // 16-bit positions in the keys, 16-bit frame ids
    rc = mi_blend_layout(w, h, n, h9s, keep, cw, ch);
    if (rc != MI355_OK) return rc;
    if (*cw <= 0 || *ch <= 0) { ctx->set_error(me + ": empty canvas"); return MI355_ERR_FAILED; }
    const int s = 1 << params->level, lgw = (*cw + s - 1) / s, lgh = (*ch + s - 1) / s;
    if (gw != lgw || gh != lgh) {
        ctx->set_error(me + ": grid " + std::to_string(gw) + "x" + std::to_string(gh) + ", the blend's layout at this level has " + std::to_string(lgw) + "x" + std::to_string(lgh));
        return MI355_ERR_ARG;
    }
    for (int k = 0; imgs && k < n; k++) {               // (imgs NULL: the host forms, whose sources are checked where they are staged)
        if ((keep && !keep[k]) || h9s[9 * k + 8] == 0.0f) continue;
        if (!imgs[k]) { ctx->set_error(me + ": image " + std::to_string(k) + " takes part but no pointer to it was given"); return MI355_ERR_ARG; }
    }
    return MI355_OK;
}

}  // namespace

#define BS_PARAMS                                                                             \
    mi355_seamcut_params dp_;                                                                 \
    if (!params) { mi355_default_seamcut_params(&dp_); params = &dp_; }

int mi_blend_seam_candidates_launch(mi355_ctx* ctx, const chips::OwnTables& t, const mi355_seamcut_params* params, mi355_seam_cell* d_cand, int gw, int gh) {
    const long long cells = (long long)gw * gh;
    ProfScope ps(ctx, "blend_seam_candidates", 0.0);
    hipLaunchKernelGGL(blend_seam_candidates_kernel, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, ctx->stream, static_cast<const ChipDev*>(t.chips), t.masks, t.pixels,
                       t.img, t.maxbits, static_cast<const LineSet*>(t.lines), t.list_off, t.list, t.bx_n, d_cand, gw, gh, t.W, t.H, params->level, params->depth);
    MI_HIP(hipGetLastError());
    return MI355_OK;
}

int mi_owner_cells_launch(mi355_ctx* ctx, const chips::OwnTables& t, const uint16_t* d_cells, int gw, int level) {
    ProfScope ps(ctx, "owner", (double)t.W * t.H);
    hipLaunchKernelGGL(owner_cells_kernel, dim3((t.W + 63) / 64, (t.H + 4 * OWN_ROWS - 1) / (4 * OWN_ROWS)), dim3(64, 4), 0, ctx->stream,
                       static_cast<const ChipDev*>(t.chips), static_cast<const LineSet*>(t.lines), t.maxbits, t.list_off, t.list, t.bx_n, t.W, t.H, t.masks, t.img, d_cells, gw,
                       level);
    MI_HIP(hipGetLastError());
    return MI355_OK;
}

extern "C" int mi355_blend_seam_cells_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                          const uint8_t* keep, const mi355_seamcut_params* params, uint16_t* d_cells, int gw, int gh, mi355_seam_report* report,
                                          mi355_seam_cell* d_cand) {
    LOCKED_PROLOGUE
    if (!d_imgs || !w || !h || !ws || !h9s || !d_cells || n <= 0) { ctx->set_error("blend_seam_cells: bad arguments"); return MI355_ERR_ARG; }
    BS_PARAMS
    int cw, ch;
    const int rc = seam_entry(ctx, "blend_seam_cells", d_imgs, w, h, n, h9s, keep, params, gw, gh, &cw, &ch);
    if (rc != MI355_OK) return rc;
    chips::Request req{chips::Request::SEAM_DEVICE};
    req.seam.params = params; req.seam.d_cells = d_cells; req.seam.gw = gw; req.seam.gh = gh;
    req.seam.make_cells = true; req.seam.stop_after_cells = true; req.seam.d_cand = d_cand; req.seam.report = report;
    chips::ChipSet set;
    return mi_chips_and_masks_dev(ctx, d_imgs, w, h, ws, n, h9s, keep, req, set);
}

extern "C" int mi355_chips_and_masks_seam(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                          const uint8_t* keep, const mi355_seamcut_params* params, const uint16_t* cells, int gw, int gh, int* n_chips,
                                          mi355_chip_info** chips, uint8_t*** chip_imgs, uint8_t*** masks, int* canvas_w, int* canvas_h) {
    LOCKED_PROLOGUE
    if (!imgs || !w || !h || !ws || !h9s || n <= 0 || !n_chips || !chips || !chip_imgs || !masks) { ctx->set_error("chips_and_masks_seam: bad arguments"); return MI355_ERR_ARG; }
    BS_PARAMS
    int cw, ch;
    const int rc = seam_entry(ctx, "chips_and_masks_seam", imgs, w, h, n, h9s, keep, params, gw, gh, &cw, &ch);
    if (rc != MI355_OK) return rc;
    DevBuf& dcells = ctx->buf("blend_seam_cells");
    const size_t cbytes = sizeof(uint16_t) * (size_t)gw * gh;
    MI_HIP(dcells.reserve(cbytes));
    if (cells) {
        MI_HIP(hipMemcpyAsync(dcells.p, cells, cbytes, hipMemcpyHostToDevice, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));       // the caller's map may go once the call returns; nothing below waits before the first use of it otherwise
    }
    chips::Request req{chips::Request::SEAM_HOST};
    req.seam.params = params; req.seam.d_cells = dcells.as<uint16_t>(); req.seam.gw = gw; req.seam.gh = gh; req.seam.make_cells = cells == nullptr;
    return mi_chips_and_masks_host(ctx, imgs, w, h, ws, n, h9s, keep, req, n_chips, chips, chip_imgs, masks, canvas_w, canvas_h);
}

extern "C" int mi355_mosaic_blended_seam_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                             const uint8_t* keep, int band, const mi355_seamcut_params* params, const uint16_t* d_cells, int gw, int gh,
                                             uint8_t* d_canvas, int cw, int ch, int cws) {
    LOCKED_PROLOGUE
    if (!d_imgs || !w || !h || !ws || !h9s || !d_canvas || n <= 0) { ctx->set_error("mosaic_blended_seam_dev: bad arguments"); return MI355_ERR_ARG; }
    BS_PARAMS
    int lw, lh;
    const int rc = seam_entry(ctx, "mosaic_blended_seam_dev", d_imgs, w, h, n, h9s, keep, params, gw, gh, &lw, &lh);
    if (rc != MI355_OK) return rc;
    if (lw != cw || lh != ch) { ctx->set_error("mosaic_blended_seam_dev: canvas geometry does not match mi355_blend_layout"); return MI355_ERR_ARG; }
    return mi_mosaic_blended_seam_dev(ctx, d_imgs, w, h, ws, n, h9s, keep, band, params, d_cells, gw, gh, d_canvas, cw, ch, cws);
}

// the check the host forms (frames.hip) make before they stage anything: parameters and the layout; the grid is the layout's own
int mi_blend_seam_host_entry(mi355_ctx* ctx, const char* who, const int* w, const int* h, int n, const float* h9s, const uint8_t* keep,
                             const mi355_seamcut_params* params, int* cw, int* ch, int* gw, int* gh) {
    int rc = mi_seamcut_params_check(ctx, who, params);
    if (rc != MI355_OK) return rc;
    rc = mi_blend_layout(w, h, n, h9s, keep, cw, ch);
    if (rc != MI355_OK) return rc;
    const int s = 1 << params->level;
    *gw = (*cw + s - 1) / s; *gh = (*ch + s - 1) / s;
    return seam_entry(ctx, who, nullptr, w, h, n, h9s, keep, params, *gw, *gh, cw, ch);
}
