// csrc/overview.hip -- the overview levels of a rendered canvas (gfx950): levels 1 .. 7 of a BGR u8 canvas, or of one stripe of it, in one launch,
// averaging only the pixels that hold data.  The definition is in include/mi355_mosaic.h ("overview levels"): pixel (X, Y) of level l is
// (S[c] + n / 2) / n over the n valid level-0 pixels of its 2^l x 2^l block, every level defined on level 0 directly.
//
//   overview_kernel<NODATA>  one workgroup per canvas tile of 128 x 128 pixels, whose origin is a multiple of 2^levels in both directions, so
//                            that every output pixel of every level lies inside one workgroup: no atomics, nothing re-read from HBM.
//                            Four passes of 32 rows.  In a pass a lane owns 4 adjacent pixels in each of 4 adjacent rows: 12 canvas bytes
//                            per row as one 4-byte-aligned load (a row pointer and the pitch are multiples of 4, and so is 3 * 4 pixels: no
//                            head to peel; the lanes of a wave read 384 contiguous bytes of a row), plus 8 map bytes; the group that
//                            crosses cw is read byte by byte with clipping -- the one tail of a row, and the same code for odd cw / ch.
//                            From these 16 pixels the lane forms, in registers, the sums and counts of its 2 x 2 level-1 cells and of its one
//                            level-2 cell, writes both levels and leaves the level-2 cell {S_B, S_G, S_R, n} in LDS (32 x 32 cells, 16 KB).
//                            Levels 3 .. levels then halve that table in LDS: level l has (128 >> l)^2 cells, one per lane, each the sum of
//                            four cells of level l - 1 (5.3 KB more for all of them).  Integer sums: the order of the additions is immaterial.
//                            Rows at or beyond row0 + rows and columns at or beyond cw count as invalid, which is the clipping of the definition:
//                            a stripe that ends inside the canvas ends on a multiple of 2^levels.
//   Division: level 1 has n <= 4, a multiply by ceil(2^16 / n) and a shift (exact for S + n / 2 <= 1022); the higher levels take the float
//   quotient of two integers below 2^23 and correct it by at most one step either way, which makes it the integer quotient.
#include "common.h"

namespace {

constexpr int OV_T = 128;                       // tile side in level-0 pixels = 2^7: a multiple of every block size
constexpr int OV_MAX_LEVELS = 7;
// LDS tables of {S_B, S_G, S_R, n}: level 2 at 0 (32 x 32), level 3 (16 x 16), ... level 7 (1 x 1)
constexpr int OV_LDS_CELLS = 1024 + 256 + 64 + 16 + 4 + 1;

struct OverviewArgs {
    const uint8_t* rows;                        // canvas row row0
    const uint16_t* valid;                      // map row row0 (NODATA_MAP)
    uint8_t* level[OV_MAX_LEVELS];              // whole buffers; NULL: the level is not stored
    uint16_t* cover[OV_MAX_LEVELS];
    int cw, cws, row0, row_end, levels;
};

struct Px12 { uint32_t d[3]; };                 // 4 BGR pixels
struct Map4 { uint16_t v[4]; };

// a / n for 0 < n <= 16384, a < 2^23: both exact as floats, the product is within one of the quotient
__device__ __forceinline__ unsigned div_exact(unsigned a, unsigned n) {
    unsigned q = (unsigned)((float)a * (1.0f / (float)n));
    int r = (int)a - (int)(q * n);
    if (r < 0) { q--; r += (int)n; }
    if (r >= (int)n) q++;
    return q;
}

// one output pixel of level l (1-based) at (X, Y): its 3 bytes, its cover value and, behind the last pixel of a row, the row's padding
__device__ __forceinline__ void store_px(const OverviewArgs& a, int l, int X, int Y, unsigned b, unsigned g, unsigned r, unsigned n) {
    const int ow = (a.cw + (1 << l) - 1) >> l, ows = (3 * ow + 3) & ~3;
    if (uint8_t* out = a.level[l - 1]) {
        uint8_t* p = out + (size_t)Y * ows + 3 * (size_t)X;
        p[0] = (uint8_t)b; p[1] = (uint8_t)g; p[2] = (uint8_t)r;
        if (X == ow - 1)
            for (int k = 3 * ow; k < ows; k++) out[(size_t)Y * ows + k] = 0;
    }
    if (uint16_t* cv = a.cover[l - 1]) cv[(size_t)Y * ow + X] = (uint16_t)n;
}

template <int NODATA>
__global__ __launch_bounds__(256) void overview_kernel(const OverviewArgs a) {
    __shared__ uint4 cells[OV_LDS_CELLS];
    const int tid = threadIdx.x, lx = tid & 31, ly = tid >> 5;
    const int tx0 = blockIdx.x * OV_T, ty0 = a.row0 + blockIdx.y * OV_T;
    const int xg = tx0 + 4 * lx;
    const int ow1 = (a.cw + 1) >> 1, ows1 = (3 * ow1 + 3) & ~3;
    for (int pass = 0; pass < 4; pass++) {
        const int yg = ty0 + 32 * pass + 4 * ly;             // the lane's 4 rows
        unsigned S[2][2][3], N[2][2];                         // level-1 cells [row pair][column pair]
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) { S[i][j][0] = S[i][j][1] = S[i][j][2] = 0; N[i][j] = 0; }
        if (xg < a.cw && yg < a.row_end) {
            Px12 px[4];
            Map4 mp[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                px[r].d[0] = px[r].d[1] = px[r].d[2] = 0;
                mp[r].v[0] = mp[r].v[1] = mp[r].v[2] = mp[r].v[3] = 0;
                const int y = yg + r;
                if (y >= a.row_end) continue;
                const uint8_t* src = a.rows + (size_t)(y - a.row0) * a.cws + 3 * (size_t)xg;
                const uint16_t* vsrc = NODATA == MI355_NODATA_MAP ? a.valid + (size_t)(y - a.row0) * a.cw + xg : nullptr;
                if (xg + 3 < a.cw) {
                    __builtin_memcpy(&px[r], __builtin_assume_aligned(src, 4), 12);
                    if (NODATA == MI355_NODATA_MAP) __builtin_memcpy(&mp[r], vsrc, 8);
                } else {
                    const int np = a.cw - xg;                 // 1 .. 3 pixels
#pragma unroll
                    for (int k = 0; k < 9; k++)               // static positions: the registers stay registers
                        if (k < 3 * np) px[r].d[k >> 2] |= (uint32_t)src[k] << (8 * (k & 3));
                    if (NODATA == MI355_NODATA_MAP) {
#pragma unroll
                        for (int k = 0; k < 3; k++)
                            if (k < np) mp[r].v[k] = vsrc[k];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const bool yin = yg + r < a.row_end;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    unsigned c[3];
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) c[ch] = (px[r].d[(3 * k + ch) >> 2] >> (8 * ((3 * k + ch) & 3))) & 255u;
                    bool v = yin && xg + k < a.cw;
                    if (NODATA == MI355_NODATA_ZERO) v = v && (c[0] | c[1] | c[2]) != 0;
                    if (NODATA == MI355_NODATA_MAP) v = v && mp[r].v[k] != 0;
                    if (v) {
                        S[r >> 1][k >> 1][0] += c[0]; S[r >> 1][k >> 1][1] += c[1]; S[r >> 1][k >> 1][2] += c[2];
                        N[r >> 1][k >> 1]++;
                    }
                }
            }
            // ---- level 1: the lane's 2 x 2 cells, 6 bytes per row ----
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int y = yg + 2 * i;
                if (y >= a.row_end) continue;
                const int Y = y >> 1, X = xg >> 1;
                unsigned o[2][3];
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const unsigned n = N[i][j], m = n == 1 ? 65536u : n == 2 ? 32768u : n == 3 ? 21846u : 16384u;
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) o[j][ch] = ((S[i][j][ch] + (n >> 1)) * m) >> 16;      // S = 0 where n = 0
                }
                const bool two = xg + 2 < a.cw;               // the second cell exists
                if (uint8_t* out = a.level[0]) {
                    uint8_t* p = out + (size_t)Y * ows1 + 3 * (size_t)X;
                    if (two) {
                        const uint8_t b6[6] = {(uint8_t)o[0][0], (uint8_t)o[0][1], (uint8_t)o[0][2], (uint8_t)o[1][0], (uint8_t)o[1][1], (uint8_t)o[1][2]};
                        __builtin_memcpy(p, b6, 6);
                    } else {
                        p[0] = (uint8_t)o[0][0]; p[1] = (uint8_t)o[0][1]; p[2] = (uint8_t)o[0][2];
                    }
                    if (X + (two ? 1 : 0) == ow1 - 1)
                        for (int k = 3 * ow1; k < ows1; k++) out[(size_t)Y * ows1 + k] = 0;
                }
                if (uint16_t* cv = a.cover[0]) {
                    cv[(size_t)Y * ow1 + X] = (uint16_t)N[i][0];
                    if (two) cv[(size_t)Y * ow1 + X + 1] = (uint16_t)N[i][1];
                }
            }
        }
        if (a.levels >= 2) {                                  // uniform
            // ---- level 2: the lane's one cell ----
            uint4 c2;
            c2.x = S[0][0][0] + S[0][1][0] + S[1][0][0] + S[1][1][0];
            c2.y = S[0][0][1] + S[0][1][1] + S[1][0][1] + S[1][1][1];
            c2.z = S[0][0][2] + S[0][1][2] + S[1][0][2] + S[1][1][2];
            c2.w = N[0][0] + N[0][1] + N[1][0] + N[1][1];
            if (xg < a.cw && yg < a.row_end) {
                const unsigned n = c2.w, h = n >> 1;
                store_px(a, 2, xg >> 2, yg >> 2, n ? div_exact(c2.x + h, n) : 0, n ? div_exact(c2.y + h, n) : 0, n ? div_exact(c2.z + h, n) : 0, n);
            }
            cells[(8 * pass + ly) * 32 + lx] = c2;            // cells outside the canvas or the rows: zeros
        }
    }
    // ---- levels 3 .. levels: the table halves in LDS ----
    int from = 0, side = 32;                                  // level l - 1: offset and cells per side
    for (int l = 3; l <= a.levels; l++) {
        __syncthreads();
        const int hs = side >> 1, to = from + side * side;
        if (tid < hs * hs) {
            const int cx = tid % hs, cy = tid / hs;
            const uint4 p = cells[from + (2 * cy) * side + 2 * cx], q = cells[from + (2 * cy) * side + 2 * cx + 1];
            const uint4 r = cells[from + (2 * cy + 1) * side + 2 * cx], s = cells[from + (2 * cy + 1) * side + 2 * cx + 1];
            uint4 c;
            c.x = p.x + q.x + r.x + s.x; c.y = p.y + q.y + r.y + s.y; c.z = p.z + q.z + r.z + s.z; c.w = p.w + q.w + r.w + s.w;
            cells[to + cy * hs + cx] = c;
            const int x0 = tx0 + (cx << l), y0 = ty0 + (cy << l);      // the block's first level-0 pixel
            if (x0 < a.cw && y0 < a.row_end) {
                const unsigned n = c.w, h = n >> 1;
                store_px(a, l, x0 >> l, y0 >> l, n ? div_exact(c.x + h, n) : 0, n ? div_exact(c.y + h, n) : 0, n ? div_exact(c.z + h, n) : 0, n);
            }
        }
        from = to; side = hs;
    }
}

}  // namespace

extern "C" int mi355_overview_layout(int cw, int ch, int levels, int* ow, int* oh, int* ows) {
    if (cw < 1 || ch < 1 || levels < 1 || levels > OV_MAX_LEVELS) { mi_set_host_error("overview_layout: cw, ch >= 1 and 1 <= levels <= 7"); return MI355_ERR_ARG; }
    for (int l = 1; l <= levels; l++) {
        const int w = (cw + (1 << l) - 1) >> l, h = (ch + (1 << l) - 1) >> l;
        if (ow) ow[l - 1] = w;
        if (oh) oh[l - 1] = h;
        if (ows) ows[l - 1] = (3 * w + 3) & ~3;
    }
    return MI355_OK;
}

int mi_mosaic_overview_dev(mi355_ctx* ctx, const uint8_t* d_rows, int cw, int ch, int cws, const uint16_t* d_valid_rows, int nodata, int levels,
                           uint8_t* const* d_levels, uint16_t* const* d_covers, int row0, int rows, int only_level) {
    if (levels < 1 || levels > OV_MAX_LEVELS) { ctx->set_error("mosaic_overview: levels=" + std::to_string(levels) + " outside 1..7"); return MI355_ERR_ARG; }
    if (nodata < 0 || nodata > 2) { ctx->set_error("mosaic_overview: nodata=" + std::to_string(nodata) + " outside 0..2"); return MI355_ERR_ARG; }
    if (nodata == MI355_NODATA_MAP && !d_valid_rows) { ctx->set_error("mosaic_overview: MI355_NODATA_MAP without a map"); return MI355_ERR_ARG; }
    if (!d_rows || !d_levels) { ctx->set_error("mosaic_overview: d_rows or d_levels is NULL"); return MI355_ERR_ARG; }
    if (cw < 1 || ch < 1 || (long)cws < 3L * cw || (cws & 3) || ((uintptr_t)d_rows & 3)) {
        ctx->set_error("mosaic_overview: canvas geometry (cw, ch >= 1, cws >= 3 cw, cws and the row pointer multiples of 4)");
        return MI355_ERR_ARG;
    }
    if (rows < 0) rows = ch - row0;
    const int align = (1 << levels) - 1;
    if (row0 < 0 || rows <= 0 || row0 + rows > ch || (row0 & align) || ((rows & align) && row0 + rows != ch)) {
        ctx->set_error("mosaic_overview: rows [" + std::to_string(row0) + ", " + std::to_string(row0 + rows) + ") of " + std::to_string(ch) +
                       ": row0 and rows must be multiples of 2^levels = " + std::to_string(align + 1) + " (rows need not where the stripe ends the canvas)");
        return MI355_ERR_ARG;
    }
    OverviewArgs a;
    memset(&a, 0, sizeof(a));
    double bytes = (3.0 + (nodata == MI355_NODATA_MAP ? 2.0 : 0.0)) * cw * (double)rows;       // level 0 read once, every level written once
    for (int l = 1; l <= levels; l++) {
        if (!d_levels[l - 1] && only_level != l) {
            if (only_level) continue;
            ctx->set_error("mosaic_overview: d_levels[" + std::to_string(l - 1) + "] is NULL");
            return MI355_ERR_ARG;
        }
        a.level[l - 1] = d_levels[l - 1];
        a.cover[l - 1] = d_covers ? d_covers[l - 1] : nullptr;
        const double ow = (cw + (1 << l) - 1) >> l, orows = ((row0 + rows + (1 << l) - 1) >> l) - (row0 >> l);
        if (a.level[l - 1]) bytes += (double)(((int)ow * 3 + 3) & ~3) * orows;
        if (a.cover[l - 1]) bytes += 2.0 * ow * orows;
    }
    a.rows = d_rows; a.valid = d_valid_rows; a.cw = cw; a.cws = cws; a.row0 = row0; a.row_end = row0 + rows; a.levels = levels;
    const dim3 grid((cw + OV_T - 1) / OV_T, (rows + OV_T - 1) / OV_T);
    {
        ProfScope ps(ctx, "overview", bytes);
        if (nodata == MI355_NODATA_NONE) hipLaunchKernelGGL(overview_kernel<MI355_NODATA_NONE>, grid, dim3(256), 0, ctx->stream, a);
        else if (nodata == MI355_NODATA_ZERO) hipLaunchKernelGGL(overview_kernel<MI355_NODATA_ZERO>, grid, dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL(overview_kernel<MI355_NODATA_MAP>, grid, dim3(256), 0, ctx->stream, a);
    }
    MI_HIP(hipGetLastError());
    return MI355_OK;
}

extern "C" int mi355_mosaic_overview_dev(mi355_ctx* ctx, const uint8_t* d_rows, int cw, int ch, int cws, const uint16_t* d_valid_rows, int nodata,
                                         int levels, uint8_t* const* d_levels, uint16_t* const* d_covers, int row0, int rows) {
    LOCKED_PROLOGUE
    return mi_mosaic_overview_dev(ctx, d_rows, cw, ch, cws, d_valid_rows, nodata, levels, d_levels, d_covers, row0, rows, 0);
}

// the host form: canvas and map staged in HBM, every level (and cover) back in buffers of its own
extern "C" int mi355_mosaic_overview(mi355_ctx* ctx, const uint8_t* canvas, int cw, int ch, int cws, const uint16_t* valid, int nodata, int levels,
                                     uint8_t*** out_levels, uint16_t*** out_covers) {
    LOCKED_PROLOGUE
    if (!canvas || !out_levels) { ctx->set_error("mosaic_overview: canvas or out_levels is NULL"); return MI355_ERR_ARG; }
    int ow[OV_MAX_LEVELS], oh[OV_MAX_LEVELS], ows[OV_MAX_LEVELS];
    if (mi355_overview_layout(cw, ch, levels, ow, oh, ows) != MI355_OK) { ctx->set_error("mosaic_overview: cw, ch >= 1 and 1 <= levels <= 7"); return MI355_ERR_ARG; }
    if (nodata < 0 || nodata > 2 || (nodata == MI355_NODATA_MAP && !valid) || (long)cws < 3L * cw || (cws & 3)) {
        ctx->set_error("mosaic_overview: nodata outside 0..2, MI355_NODATA_MAP without a map, or cws < 3 cw / not a multiple of 4");
        return MI355_ERR_ARG;
    }
    const bool use_map = nodata == MI355_NODATA_MAP;
    size_t lev_off[OV_MAX_LEVELS], cov_off[OV_MAX_LEVELS], total = 0;
    for (int l = 0; l < levels; l++) { lev_off[l] = total; total += ((size_t)ows[l] * oh[l] + 255) & ~(size_t)255; }
    for (int l = 0; l < levels; l++) { cov_off[l] = total; if (out_covers) total += (2 * (size_t)ow[l] * oh[l] + 255) & ~(size_t)255; }
    DevBuf& dcan = ctx->buf("overview_canvas");
    DevBuf& dmap = ctx->buf("overview_map");
    DevBuf& dout = ctx->buf("overview_out");
    MI_HIP(dcan.reserve((size_t)cws * ch));
    if (use_map) MI_HIP(dmap.reserve(2 * (size_t)cw * ch));
    MI_HIP(dout.reserve(total));
    MI_HIP(hipMemcpyAsync(dcan.p, canvas, (size_t)cws * ch, hipMemcpyHostToDevice, ctx->stream));
    if (use_map) MI_HIP(hipMemcpyAsync(dmap.p, valid, 2 * (size_t)cw * ch, hipMemcpyHostToDevice, ctx->stream));
    uint8_t* dl[OV_MAX_LEVELS];
    uint16_t* dc[OV_MAX_LEVELS];
    for (int l = 0; l < levels; l++) { dl[l] = dout.as<uint8_t>() + lev_off[l]; dc[l] = (uint16_t*)(dout.as<uint8_t>() + cov_off[l]); }
    int rc = mi_mosaic_overview_dev(ctx, dcan.as<uint8_t>(), cw, ch, cws, use_map ? dmap.as<uint16_t>() : nullptr, nodata, levels, dl, out_covers ? dc : nullptr, 0, ch, 0);
    if (rc != MI355_OK) return rc;
    uint8_t** lv = (uint8_t**)calloc((size_t)levels, sizeof(uint8_t*));
    uint16_t** cv = out_covers ? (uint16_t**)calloc((size_t)levels, sizeof(uint16_t*)) : nullptr;
    bool ok = lv && (!out_covers || cv);
    hipError_t e = hipSuccess;
    for (int l = 0; ok && e == hipSuccess && l < levels; l++) {
        lv[l] = (uint8_t*)malloc((size_t)ows[l] * oh[l]);
        if (cv) cv[l] = (uint16_t*)malloc(2 * (size_t)ow[l] * oh[l]);
        ok = lv[l] && (!cv || cv[l]);
        if (!ok) break;
        e = hipMemcpyAsync(lv[l], dl[l], (size_t)ows[l] * oh[l], hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && cv) e = hipMemcpyAsync(cv[l], dc[l], 2 * (size_t)ow[l] * oh[l], hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);      // also before anything is freed below
    if (e == hipSuccess) e = e2;
    if (!ok || e != hipSuccess) {
        for (int l = 0; l < levels; l++) { if (lv) free(lv[l]); if (cv) free(cv[l]); }
        free(lv); free(cv);
        if (!ok) return MI355_ERR_NOMEM;
        ctx->set_error(hipGetErrorString(e));
        return MI355_ERR_DEVICE;
    }
    *out_levels = lv;
    if (out_covers) *out_covers = cv;
    return MI355_OK;
}

extern "C" void mi355_default_preview_params(mi355_preview_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->level = 3;
    p->nodata = MI355_NODATA_MAP;
}
