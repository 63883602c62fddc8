// csrc/tie_refine.hip -- tie-point refinement by patch correlation in the resident frames (include/mi355_mosaic.h, "tie-point refinement").
// For every inlier (a, b) of every accepted pair record the position a in image i is replaced by the peak of the zero-mean normalised
// cross-correlation of the gray patch around b in image j with the neighbourhood of a, searched over (2S+1)^2 whole-pixel shifts and refined
// by a parabola per axis.  Compiled with -ffp-contract=off: the float and double chains are the header's, one rounding per operation; the
// correlation sums are integers, so their order is free.
//
//   tie_refine_kernel   one workgroup (4 waves) per record, a wave per tie, four ties in flight.  The record's two lists are copied to LDS
//                       first and nothing of the record is read from memory afterwards, so d_out == d_in is safe.  Per tie the lanes sample
//                       the (2R+1)^2 template and the (2(R+S)+1)^2 window once into LDS as bytes (every position is tested on its floats
//                       before the cast, and every texel address follows from an accepted position), then lane s owns shift s (a second
//                       pass above 64 shifts): three 32-bit sums over the template, four columns per v_dot4_u32_u8 on dword-padded rows
//                       (template dwords are LDS broadcasts, the window's aligned dwords are shifted into place by the lane's dx & 3 with
//                       v_alignbyte_b32; 3.1 x faster on C4's records than byte reads and multiply-adds), the score in double, a wave
//                       argmax on (score, smallest index).  Lane 0 leaves the tie's new position, status and score in LDS.
//                       After the last tie the workgroup compacts the lists by a ballot prefix over the keep flags (stable), writes the
//                       record, the per-tie outputs at the original indices and the report, whose counts were summed in LDS: one writer.
//                       Records that are not processed are decided in the first instructions and copied word by word.
#include "common.h"
#include "hmath.h"

#include <cmath>

int mi_frame_sources(mi355_ctx* ctx, const char* who, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h, const int* ws,
                     int n, const uint8_t* need, const char* staging, std::vector<const uint8_t*>& dptr);      // frames.hip

namespace {

// patch rows are padded to dwords for the packed u8 dot product: at the limits (R = 10, S = 4) 21 template rows of 24 bytes, 29 window rows of 36
constexpr int TR_T_BYTES = 21 * 24;
constexpr int TR_W_BYTES = 29 * 36 + 4;
constexpr int TR_SCORES = 88;          // (2 * 4 + 1)^2 = 81 scores
constexpr int TR_WAVES = 4;
constexpr int TR_TIES = MI355_MAX_SELECTED;
constexpr int TR_CHUNKS = (TR_TIES + 63) / 64;

struct TieFrame { const uint8_t* p; int32_t w, h, ws, _pad; };
struct TieArgs { int32_t R, S, drop_mask, min_inliers, n_images, _pad; double min2; };

__device__ __forceinline__ bool tie_inside(float x, float y, float w1, float h1) { return x >= 0.0f && x < w1 && y >= 0.0f && y < h1; }

__device__ __forceinline__ unsigned tie_gray(unsigned b, unsigned g, unsigned r) { return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14; }

// the gray sample at a position tie_inside accepted: 0 <= xi <= w - 2, 0 <= yi <= h - 2, so the 2 x 2 texels are pixels of the frame.  Six
// bytes per row; the 8-byte load only where all 8 are pixels of the row (xi + 3 <= w, texel_sample3's rule), else 4 + 2.
__device__ __forceinline__ unsigned tie_sample(const uint8_t* src, int w, int ws, float x, float y) {
    const int xi = (int)x, yi = (int)y;
    const float q = x - (float)xi, p = y - (float)yi;
    const uint8_t* s0 = src + (size_t)yi * (size_t)ws + 3 * (size_t)xi;
    const uint8_t* s1 = s0 + ws;
    uint64_t r0, r1;
    if (xi + 3 <= w) {
        __builtin_memcpy(&r0, s0, 8);
        __builtin_memcpy(&r1, s1, 8);
    } else {
        uint32_t lo; uint16_t hi;
        __builtin_memcpy(&lo, s0, 4); __builtin_memcpy(&hi, s0 + 4, 2);
        r0 = (uint64_t)lo | ((uint64_t)hi << 32);
        __builtin_memcpy(&lo, s1, 4); __builtin_memcpy(&hi, s1 + 4, 2);
        r1 = (uint64_t)lo | ((uint64_t)hi << 32);
    }
    const unsigned a0 = (unsigned)r0, a1 = (unsigned)(r0 >> 24), c0 = (unsigned)r1, c1 = (unsigned)(r1 >> 24);
    const unsigned g00 = tie_gray(a0 & 0xff, (a0 >> 8) & 0xff, (a0 >> 16) & 0xff), g01 = tie_gray(a1 & 0xff, (a1 >> 8) & 0xff, (a1 >> 16) & 0xff);
    const unsigned g10 = tie_gray(c0 & 0xff, (c0 >> 8) & 0xff, (c0 >> 16) & 0xff), g11 = tie_gray(c1 & 0xff, (c1 >> 8) & 0xff, (c1 >> 16) & 0xff);
    return hm::bilin((float)g00, (float)g01, (float)g10, (float)g11, p, q);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(64 * TR_WAVES) void tie_refine_kernel(const mi355_pair_result* in, int n, const TieFrame* frames, TieArgs g, mi355_pair_result* out,
                                                                   uint8_t* status, float* ncc2, mi355_tie_report* report) {
    __shared__ mi355_sfpoint la[TR_TIES], lb[TR_TIES];
    __shared__ float nax[TR_TIES], nay[TR_TIES], nsc[TR_TIES];
    __shared__ uint8_t nst[TR_TIES];
    __shared__ __align__(8) uint8_t pT[TR_WAVES][TR_T_BYTES], pW[TR_WAVES][TR_W_BYTES];
    __shared__ double psc[TR_WAVES][TR_SCORES];
    __shared__ int cnt_st[8], chunk_keep[TR_CHUNKS + 1];
    __shared__ unsigned long long qsum;

    const int rec = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, t = tid & 63;
    if (rec >= n) return;
    const mi355_pair_result& e = in[rec];
    const int pi = e.i, pj = e.j, nin = e.n_in, nsel = e.n_selected, ok = e.ok, acc = e.accepted, pad = e._pad;
    float H[9];
#pragma unroll
    for (int q = 0; q < 9; q++) H[q] = e.H[q];

    int flags = 0;
    TieFrame fi = {nullptr, 0, 0, 0, 0}, fj = fi;
    if (acc == 0) flags = 1;
    else if (nin < 1 || nin > TR_TIES || pi < 0 || pj < 0 || pi >= g.n_images || pj >= g.n_images || pi == pj) flags = 4;
    else {
        fi = frames[pi]; fj = frames[pj];
        if (!fi.p || !fj.p) flags = 2;
    }
    const size_t tie0 = (size_t)rec * TR_TIES;
    if (flags) {                                           // not processed: the record bit for bit, no tie outputs, the reason in the report
        if (out != in) {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(&e);
            uint32_t* d = reinterpret_cast<uint32_t*>(&out[rec]);
            for (int q = tid; q < (int)(sizeof(mi355_pair_result) / 4); q += 64 * TR_WAVES) d[q] = s[q];
        }
        for (int k = tid; k < TR_TIES; k += 64 * TR_WAVES) {
            if (status) status[tie0 + k] = 0;
            if (ncc2) ncc2[tie0 + k] = 0.0f;
        }
        if (report && tid == 0) {
            mi355_tie_report r;
            r.i = pi; r.j = pj; r.n_in = nin; r.n_out = nin; r.flags = flags; r._pad = 0; r.ncc_q_sum = 0;
            for (int q = 0; q < 8; q++) r.count[q] = 0;
            report[rec] = r;
        }
        return;
    }

    const int cnt = nin;
    for (int k = tid; k < TR_TIES; k += 64 * TR_WAVES) {
        const bool in = k < cnt;
        la[k].x = in ? e.a[k].x : 0.0f; la[k].y = in ? e.a[k].y : 0.0f; la[k].id = in ? e.a[k].id : 0;
        lb[k].x = in ? e.b[k].x : 0.0f; lb[k].y = in ? e.b[k].y : 0.0f; lb[k].id = in ? e.b[k].id : 0;
        nst[k] = 0; nsc[k] = 0.0f;
    }
    if (tid < 8) cnt_st[tid] = 0;
    if (tid == 0) qsum = 0ull;
    __syncthreads();                                       // from here on the input record is not read again

    const float h8 = H[8];
    H[8] = 1.0f;                                           // M: H[8] carries Ransac2D's residual
    const int R = g.R, S = g.S, TW = 2 * R + 1, WW = 2 * (R + S) + 1, SS = 2 * S + 1, NS = SS * SS, NT = TW * TW;
    const float fR = (float)R;
    const float wi1 = (float)(fi.w - 1), hi1 = (float)(fi.h - 1), wj1 = (float)(fj.w - 1), hj1 = (float)(fj.h - 1);
    uint8_t* T = pT[wv];
    uint8_t* W = pW[wv];
    // row strides: a shifted row read of the window ends at most 7 bytes past its last column ((dx >> 2) * 4 + TS + 4 <= WW + 7 <= WS)
    const int TS = (TW + 3) & ~3, WS = (WW + 10) & ~3;
    for (int q = t; q < TR_T_BYTES; q += 64) T[q] = 0;     // the template's row padding stays zero: it multiplies whatever lies beside the window
    for (int q = t; q < TR_W_BYTES; q += 64) W[q] = 0;
    double* sc = psc[wv];

    for (int k0 = 0; k0 < cnt; k0 += TR_WAVES) {
        const int k = k0 + wv;
        const bool active = k < cnt;
        bool edge = false;
        float ax = 0.0f, ay = 0.0f, bx = 0.0f, by = 0.0f, X0 = 0.0f, Y0 = 0.0f;
        if (active) {
            ax = la[k].x; ay = la[k].y; bx = lb[k].x; by = lb[k].y;
            edge = !(tie_inside(bx - fR, by - fR, wj1, hj1) && tie_inside(bx + fR, by + fR, wj1, hj1));
            if (!edge) {
                hm::apply_div9(H, bx, by, X0, Y0);
                int bad = 0;
                for (int idx = t; idx < WW * WW; idx += 64) {
                    const int v = idx / WW - (R + S), u = idx - (idx / WW) * WW - (R + S);
                    float X, Y;
                    hm::apply_div9(H, bx + (float)u, by + (float)v, X, Y);
                    const float xs = (X - X0) + ax, ys = (Y - Y0) + ay;
                    if (tie_inside(xs, ys, wi1, hi1)) W[(v + R + S) * WS + (u + R + S)] = (uint8_t)tie_sample(fi.p, fi.w, fi.ws, xs, ys);
                    else bad = 1;
                }
                edge = __any(bad) != 0;
            }
            if (!edge) {
                int bad = 0;
                for (int idx = t; idx < NT; idx += 64) {
                    const int v = idx / TW - R, u = idx - (idx / TW) * TW - R;
                    const float xs = bx + (float)u, ys = by + (float)v;
                    // inside by the corner test above and the monotony of a rounded sum; tested all the same before the address is formed
                    if (tie_inside(xs, ys, wj1, hj1)) T[(v + R) * TS + (u + R)] = (uint8_t)tie_sample(fj.p, fj.w, fj.ws, xs, ys);
                    else bad = 1;
                }
                edge = __any(bad) != 0;
            }
        }
        __syncthreads();                                   // the wave's patches are in LDS
        bool flat = false;
        double best = -1.0;
        int besti = 0x7fffffff;
        if (active && !edge) {
            int st = 0, stt = 0;
            for (int idx = t; idx < TW * TS; idx += 64) { const int tv = T[idx]; st += tv; stt += tv * tv; }      // padding is zero
            st = wave_sum(st); stt = wave_sum(stt);
            const int64_t nn = NT, St = st, Stt = stt;
            const int64_t vt = nn * Stt - St * St;
            flat = vt == 0;
            if (!flat) {
                for (int s = t; s < NS; s += 64) {
                    const int dy = s / SS, dx = s - dy * SS;                       // shift + S
                    // four columns per instruction: aligned dwords of the window row, shifted into place by the lane's dx & 3
                    unsigned sw = 0, sww = 0, stw = 0;
                    const int sh = dx & 3, nc = TS >> 2;
                    const unsigned last = (TW & 3) ? (0xffffffffu >> (8 * (4 - (TW & 3)))) : 0xffffffffu;
                    for (int v = 0; v < TW; v++) {
                        const uint32_t* tr = reinterpret_cast<const uint32_t*>(T + v * TS);
                        const uint32_t* wr = reinterpret_cast<const uint32_t*>(W + (v + dy) * WS) + (dx >> 2);
                        unsigned lo = wr[0];
                        for (int c = 0; c < nc; c++) {
                            const unsigned hi = wr[c + 1];
                            unsigned w4 = __builtin_amdgcn_alignbyte(hi, lo, sh);
                            lo = hi;
                            if (c == nc - 1) w4 &= last;
                            sw = __builtin_amdgcn_udot4(w4, 0x01010101u, sw, false);
                            sww = __builtin_amdgcn_udot4(w4, w4, sww, false);
                            stw = __builtin_amdgcn_udot4(tr[c], w4, stw, false);
                        }
                    }
                    const int64_t Sw = sw, Sww = sww, Stw = stw;
                    const int64_t vw = nn * Sww - Sw * Sw, num = nn * Stw - St * Sw;
                    const double score = (num > 0 && vw > 0) ? ((double)num * (double)num) / ((double)vt * (double)vw) : 0.0;
                    sc[s] = score;
                    if (score > best) { best = score; besti = s; }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double ob = __shfl_xor(best, o);
                    const int oi = __shfl_xor(besti, o);
                    if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
                }
            }
        }
        __syncthreads();                                   // the wave's scores are in LDS
        if (active) {
            int stv;
            double peak = 0.0;
            float nx = ax, ny = ay;
            if (edge) stv = 2;
            else if (flat) stv = 3;
            else {
                peak = best;
                const int dy = besti / SS - S, dx = besti - (besti / SS) * SS - S;
                if (peak == 0.0 || peak < g.min2) stv = 4;
                else if (dx == S || dx == -S || dy == S || dy == -S) stv = 5;
                else {
                    const double s0 = peak;
                    double sm = sc[besti - 1], sp = sc[besti + 1];
                    double den = (sm - s0) + (sp - s0);
                    const double offx = den < 0.0 ? (0.5 * (sm - sp)) / den : 0.0;
                    sm = sc[besti - SS]; sp = sc[besti + SS];
                    den = (sm - s0) + (sp - s0);
                    const double offy = den < 0.0 ? (0.5 * (sm - sp)) / den : 0.0;
                    const float ex = (float)((double)dx + offx), ey = (float)((double)dy + offy);
                    float X1, Y1;
                    hm::apply_div9(H, bx + ex, by + ey, X1, Y1);
                    nx = ax + (X1 - X0); ny = ay + (Y1 - Y0);
                    stv = 1;
                }
            }
            if (t == 0) {
                nax[k] = nx; nay[k] = ny; nst[k] = (uint8_t)stv; nsc[k] = (float)peak;
                atomicAdd(&cnt_st[stv], 1);
                if (stv == 1) atomicAdd(&qsum, (unsigned long long)(int64_t)(peak * 1048576.0));
            }
        }
    }
    __syncthreads();

    // stable compaction: chunk c of 64 ties belongs to wave c mod 4
    unsigned long long ball[2] = {0ull, 0ull};
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int c = wv + TR_WAVES * q, k = 64 * c + t;
        const bool keep = c < TR_CHUNKS && k < cnt && !((g.drop_mask >> nst[k < TR_TIES ? k : 0]) & 1);
        ball[q] = __ballot(keep);
        if (t == 0 && c < TR_CHUNKS) chunk_keep[c] = __popcll(ball[q]);
    }
    __syncthreads();
    int nout = 0;
    for (int c = 0; c < TR_CHUNKS; c++) nout += chunk_keep[c];
    const bool demote = nout < cnt && nout <= g.min_inliers;
    mi355_pair_result& o = out[rec];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int c = wv + TR_WAVES * q, k = 64 * c + t;
        if (!((ball[q] >> t) & 1ull)) continue;
        int pos = __popcll(ball[q] & ((1ull << t) - 1ull));
        for (int cc = 0; cc < c; cc++) pos += chunk_keep[cc];
        mi355_sfpoint pa = {nax[k], nay[k], la[k].id};
        o.a[pos] = pa;
        o.b[pos] = lb[k];
    }
    for (int k = nout + tid; k < TR_TIES; k += 64 * TR_WAVES) {
        const mi355_sfpoint z = {0.0f, 0.0f, 0};
        o.a[k] = z; o.b[k] = z;
    }
    for (int k = tid; k < TR_TIES; k += 64 * TR_WAVES) {
        if (status) status[tie0 + k] = nst[k];
        if (ncc2) ncc2[tie0 + k] = nsc[k];
    }
    if (tid == 0) {
        o.i = pi; o.j = pj; o.n_in = nout; o.n_selected = nsel; o.ok = demote ? 0 : ok; o.accepted = demote ? 0 : acc; o._pad = pad;
        H[8] = h8;
#pragma unroll
        for (int q = 0; q < 9; q++) o.H[q] = demote ? 0.0f : H[q];
        if (report) {
            mi355_tie_report r;
            r.i = pi; r.j = pj; r.n_in = cnt; r.n_out = nout; r.flags = demote ? 8 : 0; r._pad = 0; r.ncc_q_sum = (int64_t)qsum;
            for (int q = 0; q < 8; q++) r.count[q] = cnt_st[q];
            report[rec] = r;
        }
    }
}
static_assert(sizeof(mi355_tie_report) == 64 && sizeof(mi355_tie_params) == 20 && sizeof(TieFrame) == 24, "tie records");

bool tie_params_ok(const mi355_tie_params& p, std::string& err) {
    if (p.radius < 1 || p.radius > 10) { err = "radius=" + std::to_string(p.radius) + " outside [1, 10]"; return false; }
    if (p.search < 1 || p.search > 4) { err = "search=" + std::to_string(p.search) + " outside [1, 4]"; return false; }
    if (!std::isfinite(p.min_ncc) || p.min_ncc < 0.0f || p.min_ncc > 1.0f) { err = "min_ncc=" + std::to_string(p.min_ncc) + " outside [0, 1]"; return false; }
    if (p.drop_mask & ~0x3c) { err = "drop_mask=" + std::to_string(p.drop_mask) + " has bits outside 2..5"; return false; }
    if (p.reserved != 0) { err = "reserved=" + std::to_string(p.reserved) + " must be 0"; return false; }
    return true;
}

// caller holds the ctx lock and has checked n > 0 and the parameters: the frame table to the device (through pinned memory: the caller's
// arrays may be gone before the copy runs), one launch
int launch_ties(mi355_ctx* ctx, const mi355_pair_result* d_in, int n, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n_images,
                const mi355_tie_params& p, mi355_pair_result* d_out, uint8_t* d_status, float* d_ncc2, mi355_tie_report* d_report) {
    for (int k = 0; k < n_images; k++) {
        if (!d_imgs[k]) continue;
        if (w[k] < 2 || h[k] < 2 || w[k] > (1 << 20) || h[k] > (1 << 20) || ws[k] < 3 * w[k]) {
            ctx->set_error("refine_ties: image " + std::to_string(k) + ": bad geometry " + std::to_string(w[k]) + "x" + std::to_string(h[k]) + " (width_step " + std::to_string(ws[k]) + ")");
            return MI355_ERR_ARG;
        }
    }
    const size_t bytes = sizeof(TieFrame) * (size_t)n_images;
    HostBuf& stage = ctx->hbuf("tie_frames_host");
    DevBuf& dtab = ctx->buf("tie_frames");
    MI_HIP(stage.reserve(bytes));
    MI_HIP(dtab.reserve(bytes));
    MI_HIP(hipStreamSynchronize(ctx->stream));            // the previous call's upload has left the staging area
    TieFrame* tab = stage.as<TieFrame>();
    for (int k = 0; k < n_images; k++) { tab[k].p = d_imgs[k]; tab[k].w = d_imgs[k] ? w[k] : 0; tab[k].h = d_imgs[k] ? h[k] : 0; tab[k].ws = d_imgs[k] ? ws[k] : 0; tab[k]._pad = 0; }
    MI_HIP(hipMemcpyAsync(dtab.p, stage.p, bytes, hipMemcpyHostToDevice, ctx->stream));
    TieArgs g;
    g.R = p.radius; g.S = p.search; g.drop_mask = p.drop_mask; g.min_inliers = ctx->p.min_inliers; g.n_images = n_images; g._pad = 0;
    g.min2 = (double)p.min_ncc * (double)p.min_ncc;
    {
        ProfScope ps(ctx, "tie_refine", 2.0 * (double)sizeof(mi355_pair_result) * (double)n);
        hipLaunchKernelGGL(tie_refine_kernel, dim3(n), dim3(64 * TR_WAVES), 0, ctx->stream, d_in, n, dtab.as<TieFrame>(), g, d_out, d_status, d_ncc2, d_report);
    }
    MI_HIP(hipGetLastError());
    return MI355_OK;
}

int tie_common_checks(mi355_ctx* ctx, const char* who, int n, int n_images, const void* imgs, const int* w, const int* h, const int* ws,
                      const mi355_tie_params* params, mi355_tie_params& p) {
    if (params) p = *params; else mi355_default_tie_params(&p);
    std::string err;
    if (!tie_params_ok(p, err)) { ctx->set_error(std::string(who) + ": " + err); return MI355_ERR_ARG; }
    if (n < 0 || n_images < 1 || !imgs || !w || !h || !ws) { ctx->set_error(std::string(who) + ": bad arguments (n, n_images or a NULL pointer)"); return MI355_ERR_ARG; }
    return MI355_OK;
}

}  // namespace

extern "C" void mi355_default_tie_params(mi355_tie_params* p) {
    if (!p) return;
    p->radius = 7; p->search = 3; p->drop_mask = 0; p->reserved = 0; p->min_ncc = 0.7f;
}

extern "C" int mi355_refine_ties_dev(mi355_ctx* ctx, const mi355_pair_result* d_in, int n, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws,
                                     int n_images, const mi355_tie_params* params, mi355_pair_result* d_out, uint8_t* d_status, float* d_ncc2,
                                     mi355_tie_report* d_report) {
    LOCKED_PROLOGUE
    mi355_tie_params p;
    { const int rc = tie_common_checks(ctx, "refine_ties_dev", n, n_images, d_imgs, w, h, ws, params, p); if (rc != MI355_OK) return rc; }
    if (n > 0 && (!d_in || !d_out)) { ctx->set_error("refine_ties_dev: NULL records"); return MI355_ERR_ARG; }
    if (n == 0) return MI355_OK;
    return launch_ties(ctx, d_in, n, d_imgs, w, h, ws, n_images, p, d_out, d_status, d_ncc2, d_report);
}

extern "C" int mi355_refine_ties(mi355_ctx* ctx, const mi355_pair_result* in, int n, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h,
                                 const int* ws, int n_images, const mi355_tie_params* params, mi355_pair_result* out, uint8_t* status, float* ncc2,
                                 mi355_tie_report* report) {
    LOCKED_PROLOGUE
    mi355_tie_params p;
    const void* some = imgs ? (const void*)imgs : (const void*)img_ids;
    { const int rc = tie_common_checks(ctx, "refine_ties", n, n_images, some, w, h, ws, params, p); if (rc != MI355_OK) return rc; }
    if (n > 0 && (!in || !out)) { ctx->set_error("refine_ties: NULL records"); return MI355_ERR_ARG; }
    if (n == 0) return MI355_OK;
    // the images that a record to be processed names and that have a source: only those are read or uploaded
    std::vector<uint8_t> need((size_t)n_images, 0);
    for (int r = 0; r < n; r++) {
        const mi355_pair_result& e = in[r];
        if (!e.accepted) continue;
        if (e.n_in < 1 || e.n_in > MI355_MAX_SELECTED || e.i < 0 || e.j < 0 || e.i >= n_images || e.j >= n_images || e.i == e.j) {
            ctx->set_error("refine_ties: record " + std::to_string(r) + ": n_in=" + std::to_string(e.n_in) + ", i=" + std::to_string(e.i) + ", j=" + std::to_string(e.j) +
                           " (n_in outside [1, 400], an index outside [0, " + std::to_string(n_images) + ") or i == j)");
            return MI355_ERR_ARG;
        }
        const int ij[2] = {e.i, e.j};
        bool both = true;
        for (int q = 0; q < 2; q++) both = both && ((img_ids && img_ids[ij[q]] >= 0) || (imgs && imgs[ij[q]]));
        if (both) need[e.i] = need[e.j] = 1;
    }
    std::vector<const uint8_t*> dptr;
    { const int rc = mi_frame_sources(ctx, "refine_ties", imgs, img_ids, w, h, ws, n_images, need.data(), "tie_srcs", dptr); if (rc != MI355_OK) return rc; }
    const size_t rb = sizeof(mi355_pair_result) * (size_t)n, sb = (size_t)MI355_MAX_SELECTED * (size_t)n, fb = sizeof(float) * sb, pb = sizeof(mi355_tie_report) * (size_t)n;
    DevBuf& drec = ctx->buf("tie_records");
    DevBuf& dout = ctx->buf("tie_outputs");
    MI_HIP(drec.reserve(rb));
    MI_HIP(dout.reserve(fb + pb + sb));
    float* d_ncc2 = dout.as<float>();
    mi355_tie_report* d_rep = reinterpret_cast<mi355_tie_report*>(dout.as<uint8_t>() + fb);
    uint8_t* d_st = dout.as<uint8_t>() + fb + pb;
    MI_HIP(hipMemcpyAsync(drec.p, in, rb, hipMemcpyHostToDevice, ctx->stream));
    { const int rc = launch_ties(ctx, drec.as<mi355_pair_result>(), n, dptr.data(), w, h, ws, n_images, p, drec.as<mi355_pair_result>(), d_st, d_ncc2, d_rep); if (rc != MI355_OK) return rc; }
    MI_HIP(hipMemcpyAsync(out, drec.p, rb, hipMemcpyDeviceToHost, ctx->stream));
    if (status) MI_HIP(hipMemcpyAsync(status, d_st, sb, hipMemcpyDeviceToHost, ctx->stream));
    if (ncc2) MI_HIP(hipMemcpyAsync(ncc2, d_ncc2, fb, hipMemcpyDeviceToHost, ctx->stream));
    if (report) MI_HIP(hipMemcpyAsync(report, d_rep, pb, hipMemcpyDeviceToHost, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}
