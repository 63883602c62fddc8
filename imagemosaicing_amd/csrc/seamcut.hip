// csrc/seamcut.hip -- optimised seamlines (gfx950): a cost-aware owner map on a coarse grid of canvas cells and the render that follows it.
// The definition is in include/mi355_mosaic.h ("optimised seamlines"); tests/seamcut_ref.py restates every stage in numpy.
//
//   seam_candidates_kernel  one wave per cell.  Phase 1, the probe: the lanes share out the frames of the cell's list block (the per-256 x 256
//                           candidate lists of the one-pass renders), each maps, tests and weighs its frames at the probe pixel exactly as
//                           seamline_tile_kernel does and keeps its own sorted top 8 of the keys omega << 16 | q (median_tile_kernel's max / min
//                           chain); the cell's top `depth` are then drawn by `depth` rounds of a wave-wide maximum over the lanes' heads, the
//                           lane that held the winner popping it.  Keys are distinct, so the order is (omega, k) whatever the share-out.
//                           Phase 2, the signatures: for each selected frame the lanes walk the cell's pixels (clipped to the canvas), sample
//                           where the frame gives a sample (frame_sample3), form the integer gray and add gray << 11 | 1 -- sum and number of
//                           samples in one word (at most 1024 pixels of at most 255) -- which a butterfly sums over the wave.
//   seam_path_kernel        one direction of the aggregation: one wave per scanline, lane (a, b) = (lane >> 3, lane & 7) holds the pair
//                           "slot a of this cell, slot b of the cell before".  Per step: ONE frame-id compare and one ballot give every lane
//                           both "frame of b is a candidate of this cell, at which slot" (the ballot's column b) and "frame of a is a
//                           candidate of the cell before, at which slot" (its row a); the gray bytes of either cell are one 64-bit word per
//                           lane, indexed by shifts.  min over b: three xor-butterflies inside the groups of eight (they never leave the
//                           group); L(p, b) for the next step comes from lane 8 b (one bpermute).  The next cell's loads are issued before
//                           the step's arithmetic.  L <= D + V <= 16 * 254 + 255 + 16 * 510 = 12479, and the sum over four directions fits
//                           the uint16 it is accumulated in (the first direction stores, the others add; a cell slot belongs to one lane).
//                           The four directions are four launches that differ in base, step and line stride only.
//   seam_argmin_kernel, seam_energy_kernel, seam_finish_kernel   per cell: the label, both energies (64-bit atomics on integers: the sum
//                           does not depend on the order), the fallback and the cell map.
//   seamcut_tile_kernel     seamline_tile_kernel with one more input: a lane's four pixels lie in one cell (level >= 2), so each of its rows
//                           carries the cell's wanted frame; a walked frame that is the wanted one gets bit 24 of its key set, above every
//                           omega, so the running maximum prefers it wherever it gives a sample and is the seamline owner elsewhere.
// Registers, as the compiler reports them for gfx950 with the library's flags (build.py; -Rpass-analysis=kernel-resource-usage; no kernel uses
// scratch): seam_candidates_kernel 71 VGPRs (7 waves per SIMD), seam_path_kernel 48, seamcut_tile_kernel 64 in both forms -- four more than
// seamline_tile_kernel's 60, still 8 waves per SIMD (without -ffp-contract=off the two report 60 and 56) --, the per-cell passes 6 to 26.
// The host path of the render -- entry check, frame table, lists, used flags, the host form -- is mosaic_frame.h's.
#include "common.h"
#include "hmath.h"
#include "mosaic_frame.h"
#include "ramp.h"

static_assert(sizeof(mi355_seam_cell) == 32 && offsetof(mi355_seam_cell, omega) == 16 && offsetof(mi355_seam_cell, gray) == 24, "cell record layout");
static_assert(sizeof(mi355_seamcut_params) == 32 && sizeof(mi355_seam_report) == 24, "seamcut parameter / report layout");
static_assert(MI355_SEAMCUT_MAX_DEPTH == 8, "the 8 x 8 slot pairs of a step are one wave64");

namespace {

constexpr int SC_SLOTS = MI355_SEAMCUT_MAX_DEPTH;
constexpr int SC_INF = 1 << 28;
struct SeamCosts { int data_weight, diff_weight, seam_penalty, miss_cost; };

__host__ __device__ inline unsigned sc_gray(unsigned b, unsigned g, unsigned r) { return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14; }

// V between slot a of cell p and slot b of cell q (both slots hold a frame): the header's smoothness term
__host__ __device__ inline int sc_pair_cost(const mi355_seam_cell& p, int a, const mi355_seam_cell& q, int b, const SeamCosts& c) {
    const unsigned k = p.frame[a], l = q.frame[b];
    if (k == l) return 0;
    int dp = c.miss_cost, dq = c.miss_cost;
    for (int i = 0; i < SC_SLOTS; i++) {
        if (p.frame[i] == l) { const int d = (int)p.gray[a] - (int)p.gray[i]; dp = d < 0 ? -d : d; }
        if (q.frame[i] == k) { const int d = (int)q.gray[i] - (int)q.gray[b]; dq = d < 0 ? -d : d; }
    }
    return c.seam_penalty + c.diff_weight * (dp + dq);
}

__host__ __device__ inline int sc_data_cost(const mi355_seam_cell& p, int a, const SeamCosts& c) { return c.data_weight * ((int)p.omega[0] - (int)p.omega[a]); }

// D + V to the right and lower neighbours of cell (cx, cy) under the labelling lab (NULL: all slot 0)
__host__ __device__ inline long long sc_cell_energy(const mi355_seam_cell* cand, const uint8_t* lab, int gw, int gh, int cx, int cy, const SeamCosts& c) {
    const size_t i = (size_t)cy * gw + cx;
    const mi355_seam_cell& p = cand[i];
    if (!p.frame[0]) return 0;
    const int a = lab ? lab[i] : 0;
    long long e = sc_data_cost(p, a, c);
    if (cx + 1 < gw && cand[i + 1].frame[0]) e += sc_pair_cost(p, a, cand[i + 1], lab ? lab[i + 1] : 0, c);
    if (cy + 1 < gh && cand[i + gw].frame[0]) e += sc_pair_cost(p, a, cand[i + gw], lab ? lab[i + gw] : 0, c);
    return e;
}

// argmin over the slots that hold a frame of (S, slot): the lower slot wins a tie; 0 for a cell without candidates
__host__ __device__ inline int sc_argmin(const mi355_seam_cell& p, const uint16_t* S) {
    int best = 0;
    for (int a = 1; a < SC_SLOTS; a++)
        if (p.frame[a] && S[a] < S[best]) best = a;
    return best;
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)v, o, 64); v = t > v ? t : v; }
    return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}
__device__ __forceinline__ int group8_min(int v) {
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) { const int t = __shfl_xor(v, o, 64); v = t < v ? t : v; }
    return v;
}

// ---- stage 1 ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seam_candidates_kernel(const FrameDev* fr, const RampDev* ramps, const int* frame_of, int n, const uint16_t* lists,
                                                              const int* counts, int bx_n, mi355_seam_cell* out, int gw, int gh, int cw, int ch, int level,
                                                              int depth, float dGx, float dGy) {
    const int lane = threadIdx.x & 63;
    const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= (long long)gw * gh) return;              // the whole wave
    const int cy = (int)(cell / gw), cx = (int)(cell - (long long)cy * gw);
    const int s = 1 << level, x0 = cx << level, y0 = cy << level;
    const int px = x0 + s / 2 < cw - 1 ? x0 + s / 2 : cw - 1, py = y0 + s / 2 < ch - 1 ? y0 + s / 2 : ch - 1;
    const int cb = (y0 / MOSAIC_LIST_BLOCK) * bx_n + x0 / MOSAIC_LIST_BLOCK;     // a cell lies inside one list block: s divides 256
    const uint16_t* list = lists + (size_t)cb * n;
    const int cnt = counts[cb];
    // ---- phase 1: the lane's own top 8 at the probe, then the wave's top `depth` ----
    unsigned key[SC_SLOTS];
#pragma unroll
    for (int i = 0; i < SC_SLOTS; i++) key[i] = 0;
    const float xf = (float)px - dGx, yf = (float)py - dGy;
    for (int e = lane; e < cnt; e += 64) {
        const unsigned q = list[e];
        const FrameDev& f = fr[q];
        if (px < f.begX || px > f.endX || py < f.begY || py > f.endY) continue;
        float xs, ys;
        frame_src(f, xf, yf, xs, ys);
        if (!src_inside(xs, ys, (float)(f.w - 1), (float)(f.h - 1))) continue;
        unsigned x = (ramp_omega(f, ramps[q], xs, ys) << 16) | q;
#pragma unroll
        for (int i = 0; i < SC_SLOTS; i++) {             // the key sinks to its place; what falls off the end is dropped
            const unsigned sl = key[i], hi = sl > x ? sl : x;
            x = sl > x ? x : sl;
            key[i] = hi;
        }
    }
    mi355_seam_cell rec;
    memset(&rec, 0, sizeof(rec));
#pragma unroll
    for (int i = 0; i < SC_SLOTS; i++) {
        if (i >= depth) break;
        const unsigned best = wave_max(key[0]);
        if (!best) break;                                // uniform: fewer contributors than depth
        if (key[0] == best) {                            // one lane: keys are distinct
#pragma unroll
            for (int j = 0; j + 1 < SC_SLOTS; j++) key[j] = key[j + 1];
            key[SC_SLOTS - 1] = 0;
        }
        // ---- phase 2: the frame's gray over the cell's pixels it gives a sample ----
        const unsigned q = best & 0xffffu;
        const FrameDev& f = fr[q];                       // uniform over the wave
        const float w1 = (float)(f.w - 1), h1 = (float)(f.h - 1);
        unsigned acc = 0;                                // gray sum << 11 | samples
        for (int idx = lane; idx < s * s; idx += 64) {
            const int xD = x0 + (idx & (s - 1)), yD = y0 + (idx >> level);
            if (xD >= cw || yD >= ch || xD < f.begX || xD > f.endX || yD < f.begY || yD > f.endY) continue;
            float xs, ys;
            frame_src(f, (float)xD - dGx, (float)yD - dGy, xs, ys);
            if (!src_inside(xs, ys, w1, h1)) continue;
            unsigned vb, vg, vr;
            frame_sample3(f, xs, ys, vb, vg, vr);
            acc += (sc_gray(vb, vg, vr) << 11) | 1u;
        }
        acc = wave_sum(acc);
        const unsigned tot = acc >> 11, num = acc & 0x7ffu;                  // num >= 1: the probe is one of the pixels
        rec.frame[i] = (uint16_t)(frame_of[q] + 1);
        rec.omega[i] = (uint8_t)(best >> 16);
        rec.gray[i] = (uint8_t)((tot + num / 2) / (num ? num : 1u));
    }
    if (lane == 0) out[cell] = rec;
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------------------
struct PathCell { unsigned fa, fb, ga, gb, oa, o0; unsigned long long g8; };

__device__ __forceinline__ PathCell path_load(const mi355_seam_cell* rec, int a, int b) {
    PathCell c;
    c.fa = rec->frame[a]; c.fb = rec->frame[b]; c.ga = rec->gray[a]; c.gb = rec->gray[b]; c.oa = rec->omega[a]; c.o0 = rec->omega[0];
    __builtin_memcpy(&c.g8, rec->gray, 8);
    return c;
}

// cell i of line l: base + l * line_stride + i * step
__global__ __launch_bounds__(256) void seam_path_kernel(const mi355_seam_cell* cand, uint16_t* S, int nlines, int len, long long base, long long line_stride,
                                                        long long step, int first, SeamCosts c) {
    const int lane = threadIdx.x & 63, a = lane >> 3, b = lane & 7;
    const int line = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (line >= nlines) return;                          // the whole wave
    long long idx = base + (long long)line * line_stride;
    unsigned fq = 0, gq = 0;                             // slot b of the cell before: frame (0: none, also before the first cell), gray
    unsigned long long gq8 = 0;
    int Lq = 0;                                          // L(cell before, b)
    PathCell cur = path_load(cand + idx, a, b);
    for (int i = 0; i < len; i++) {
        PathCell nxt = cur;
        if (i + 1 < len) nxt = path_load(cand + idx + step, a, b);          // in flight during the step
        const bool match = cur.fa != 0 && cur.fa == fq;
        const unsigned long long m64 = __ballot(match);
        const unsigned long long col = (m64 >> b) & 0x0101010101010101ull;  // rows a' with frame(p, a') == frame(q, b)
        const unsigned row = (unsigned)(m64 >> (8 * a)) & 0xffu;            // columns b' with frame(q, b') == frame(p, a)
        int dp = c.miss_cost, dq = c.miss_cost;
        if (col) { const int d = (int)cur.ga - (int)((cur.g8 >> (__builtin_ctzll(col) & 56)) & 0xffu); dp = d < 0 ? -d : d; }
        if (row) { const int d = (int)((gq8 >> (8 * __builtin_ctz(row))) & 0xffu) - (int)gq; dq = d < 0 ? -d : d; }
        const int V = match ? 0 : c.seam_penalty + c.diff_weight * (dp + dq);
        const int mn = group8_min(fq ? Lq + V : SC_INF), mp = group8_min(fq ? Lq : SC_INF);
        const int D = c.data_weight * ((int)cur.o0 - (int)cur.oa);
        const int L = cur.fa ? (mp < SC_INF ? D + mn - mp : D) : 0;
        if (b == 0) {
            uint16_t* s = S + (size_t)idx * SC_SLOTS + a;
            *s = (uint16_t)(first ? L : *s + L);
        }
        Lq = __shfl(L, 8 * b, 64);
        fq = cur.fb; gq = cur.gb; gq8 = cur.g8;
        cur = nxt;
        idx += step;
    }
}

__global__ __launch_bounds__(256) void seam_argmin_kernel(const mi355_seam_cell* cand, const uint16_t* S, uint8_t* lab, long long cells) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    uint16_t s[SC_SLOTS];
    __builtin_memcpy(s, S + (size_t)i * SC_SLOTS, sizeof(s));
    lab[i] = (uint8_t)sc_argmin(cand[i], s);
}

// acc[0] += energy of the all-slot-0 labelling, acc[1] += energy of lab, acc[2] += cells with lab != 0
__global__ __launch_bounds__(256) void seam_energy_kernel(const mi355_seam_cell* cand, const uint8_t* lab, int gw, int gh, SeamCosts c, unsigned long long* acc) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long e0 = 0, e1 = 0, ch = 0;
    if (i < (long long)gw * gh) {
        const int cy = (int)(i / gw), cx = (int)(i - (long long)cy * gw);
        e0 = (unsigned long long)sc_cell_energy(cand, nullptr, gw, gh, cx, cy, c);
        e1 = (unsigned long long)sc_cell_energy(cand, lab, gw, gh, cx, cy, c);
        ch = lab[i] != 0;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) { e0 += __shfl_xor(e0, o, 64); e1 += __shfl_xor(e1, o, 64); ch += __shfl_xor(ch, o, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (e0) atomicAdd(acc, e0);
        if (e1) atomicAdd(acc + 1, e1);
        if (ch) atomicAdd(acc + 2, ch);
    }
}

__global__ __launch_bounds__(256) void seam_finish_kernel(const mi355_seam_cell* cand, const uint8_t* lab, const unsigned long long* acc, uint16_t* cells, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int a = acc[1] > acc[0] ? 0 : lab[i];          // the fallback: never worse than the seamline labelling by the energy
    cells[i] = a ? cand[i].frame[a] : (uint16_t)0;
}

// ---- stage 3 ---------------------------------------------------------------------------------------------------------------------
constexpr int SCT_W = 128, SCT_RPL = 2, SCT_H = 8 * SCT_RPL;
constexpr unsigned SCT_WANTED = 1u << 24;                // above omega << 16 (omega <= 255)

template <bool SAMPLE>
__global__ __launch_bounds__(256) void seamcut_tile_kernel(const FrameDev* fr, const RampDev* ramps, const int* frame_of, int n, const uint16_t* lists,
                                                           const int* counts, int bx_n, const uint16_t* cells, int gw, int level, uint8_t* canvas,
                                                           uint16_t* owner, uint16_t* count, int* used, int cw, int cws, int row0, int row_end, float dGx,
                                                           float dGy) {
    const TileLane t = tile_lane<SCT_W, SCT_RPL>(lists, counts, n, bx_n, cw, row0, row_end);
    const int xg = t.xg;
    unsigned key[SCT_RPL][4], cov[SCT_RPL][4];           // per pixel: max of wanted << 24 | omega << 16 | q (0: no frame), the number of contributing frames
    int want[SCT_RPL];                                   // per row: the frame the cell of the lane's four pixels names, -1: none (xg is a multiple of 4 <= the cell side)
#pragma unroll
    for (int j = 0; j < SCT_RPL; j++) {
        const int yD = t.yB + 8 * j;
        want[j] = xg < cw && yD < row_end ? (int)cells[(size_t)(yD >> level) * gw + (xg >> level)] - 1 : -1;
#pragma unroll
        for (int k = 0; k < 4; k++) { key[j][k] = 0; cov[j][k] = 0; }
    }
    // ---- phase 1: who owns each pixel ----
    for (int e = 0; e < t.cnt; e++) {
        const unsigned q = t.list[e];
        const FrameDev& f = fr[q];                       // uniform over the workgroup: scalar loads
        if (f.begX > t.tx1 || f.endX < t.tx0 || f.begY > t.ty1 || f.endY < t.ty0) continue;
        const RampDev r = ramps[q];
        const int kq = frame_of[q];
        const float w1 = (float)(f.w - 1), h1 = (float)(f.h - 1);
#pragma unroll
        for (int j = 0; j < SCT_RPL; j++) {
            const int yD = t.yB + 8 * j;
            const bool yin = yD >= f.begY && yD <= f.endY;           // the box is clipped to the canvas and to the rows of this call
            const float yf = (float)yD - dGy;
            const unsigned boost = want[j] == kq ? SCT_WANTED : 0u;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int xD = xg + k;
                const float xf = (float)xD - dGx;
                float xs, ys;
                frame_src(f, xf, yf, xs, ys);
                if (!(yin && xD >= f.begX && xD <= f.endX && src_inside(xs, ys, w1, h1))) continue;
                const unsigned key1 = boost | (ramp_omega(f, r, xs, ys) << 16) | q;
                cov[j][k]++;
                if (key1 > key[j][k]) key[j][k] = key1;
            }
        }
    }
    if (xg >= cw) return;
#pragma unroll
    for (int j = 0; j < SCT_RPL; j++) {
        const int yD = t.yB + 8 * j;
        if (yD >= row_end) continue;
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
                frame_src(f, (float)(xg + k) - dGx, yf, xs, ys);     // phase 1's expression: the same bits
                unsigned v[3];
                frame_sample3(f, xs, ys, v[0], v[1], v[2]);
#pragma unroll
                for (int c = 0; c < 3; c++) out[(3 * k + c) >> 2] |= v[c] << (8 * ((3 * k + c) & 3));      // static positions
            }
            store_row12(canvas, cw, cws, xg, yD, out);
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
bool sc_params_ok(const mi355_seamcut_params* p, std::string& err) {
    struct { const char* name; int v, lo, hi; } f[] = {{"ramp", p->ramp, 0, INT32_MAX}, {"level", p->level, 2, 5}, {"depth", p->depth, 1, MI355_SEAMCUT_MAX_DEPTH},
                                                      {"data_weight", p->data_weight, 0, 16}, {"diff_weight", p->diff_weight, 0, 16},
                                                      {"seam_penalty", p->seam_penalty, 0, 255}, {"miss_cost", p->miss_cost, 0, 255}};
    for (const auto& e : f)
        if (e.v < e.lo || e.v > e.hi) {
            err = std::string(e.name) + "=" + std::to_string(e.v) + " outside " + std::to_string(e.lo) + ".." + (e.hi == INT32_MAX ? std::string("") : std::to_string(e.hi));
            return false;
        }
    return true;
}

SeamCosts sc_costs(const mi355_seamcut_params* p) { return SeamCosts{p->data_weight, p->diff_weight, p->seam_penalty, p->miss_cost}; }

bool sc_grid_ok(int gw, int gh, std::string& err) {
    if (gw < 1 || gh < 1 || gw > (1 << 20) || gh > (1 << 20)) { err = "grid " + std::to_string(gw) + "x" + std::to_string(gh) + " outside 1..2^20 a side"; return false; }
    return true;
}

}  // namespace

#define SC_PARAMS(who)                                                                        \
    mi355_seamcut_params dp_;                                                                 \
    if (!params) { mi355_default_seamcut_params(&dp_); params = &dp_; }                       \
    { std::string e_; if (!sc_params_ok(params, e_)) { ctx->set_error(std::string(who) + ": " + e_); return MI355_ERR_ARG; } }

// the range check for the callers outside this file (blend_seam.hip)
int mi_seamcut_params_check(mi355_ctx* ctx, const char* who, const mi355_seamcut_params* params) {
    std::string e;
    if (sc_params_ok(params, e)) return MI355_OK;
    ctx->set_error(std::string(who) + ": " + e);
    return MI355_ERR_ARG;
}

extern "C" void mi355_default_seamcut_params(mi355_seamcut_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->level = 3; p->depth = 4; p->data_weight = 1; p->diff_weight = 2; p->seam_penalty = 2; p->miss_cost = 32;
}

int mi_seam_candidates_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                           const mi355_seamcut_params* params, mi355_seam_cell* d_cand, int gw, int gh) {
    SC_PARAMS("seam_candidates")
    int cw = 0, ch = 0, cws = 0, row0 = 0, rows = -1;
    float dG[2]; bool go;
    const int rc = mi_render_entry(ctx, "seam_candidates", w, h, n, h9s, true, false, cw, ch, cws, row0, rows, dG, go);
    if (rc != MI355_OK) return rc;
    const int s = 1 << params->level;
    if (gw != (cw + s - 1) / s || gh != (ch + s - 1) / s) {
        ctx->set_error("seam_candidates: grid " + std::to_string(gw) + "x" + std::to_string(gh) + ", the layout at this level has " + std::to_string((cw + s - 1) / s) + "x" + std::to_string((ch + s - 1) / s));
        return MI355_ERR_ARG;
    }
    if (!go) return MI355_OK;
    FrameTable t;                                        // frame_of ascending: (omega, q) orders as (omega, k)
    for (int k = 0; k < n; k++) {
        FrameDev f;
        if (!mi_frame_dev_setup(h9s + 9 * k, w[k], h[k], dG, cw, ch, 0, ch, f)) continue;
        if (w[k] < 2 || h[k] < 2 || ws[k] < 3 * w[k] || w[k] > RAMP_MAX_SIDE || h[k] > RAMP_MAX_SIDE) { ctx->set_error("seam_candidates: bad image geometry"); return MI355_ERR_ARG; }
        if (!d_imgs[k]) { ctx->set_error("seam_candidates: image " + std::to_string(k) + " takes part but no pointer to it was given"); return MI355_ERR_ARG; }
        f.src = d_imgs[k]; f.w = w[k]; f.h = h[k]; f.ws = ws[k];
        t.add(f, k);
        t.ramps.push_back(ramp_of_frame(w[k], h[k], params->ramp));
    }
    const int rc2 = mi_frame_table_upload(ctx, t, true, true, cw, ch, 0);
    if (rc2 != MI355_OK) return rc2;
    const long long cells = (long long)gw * gh;
    {
        ProfScope ps(ctx, "seam_candidates", 0.0);
        hipLaunchKernelGGL(seam_candidates_kernel, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, ctx->stream, t.d_fr, t.d_ramps, t.d_frame_of, t.nf, t.d_lists,
                           t.d_counts, t.bx_n, d_cand, gw, gh, cw, ch, params->level, params->depth, dG[0], dG[1]);
    }
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(ctx->stream));           // the table goes out of scope
    return MI355_OK;
}

int mi_seam_labels_dev(mi355_ctx* ctx, const mi355_seam_cell* d_cand, int gw, int gh, const mi355_seamcut_params* params, uint16_t* d_cells,
                       mi355_seam_report* report) {
    SC_PARAMS("seam_labels")
    { std::string e; if (!sc_grid_ok(gw, gh, e)) { ctx->set_error("seam_labels: " + e); return MI355_ERR_ARG; } }
    const long long cells = (long long)gw * gh;
    DevBuf& dS = ctx->buf("seamcut_sums");
    DevBuf& dlab = ctx->buf("seamcut_labels");
    DevBuf& dacc = ctx->buf("seamcut_energy");
    MI_HIP(dS.reserve(sizeof(uint16_t) * SC_SLOTS * (size_t)cells));
    MI_HIP(dlab.reserve((size_t)cells));
    MI_HIP(dacc.reserve(3 * sizeof(unsigned long long)));
    MI_HIP(hipMemsetAsync(dacc.p, 0, 3 * sizeof(unsigned long long), ctx->stream));
    const SeamCosts c = sc_costs(params);
    const unsigned blocks = (unsigned)((cells + 255) / 256);
    unsigned long long acc[3];
    {
        ProfScope ps(ctx, "seam_labels", 0.0);
        const struct { int nlines, len; long long base, line_stride, step; } dir[4] = {
            {gh, gw, 0, gw, 1}, {gh, gw, gw - 1, gw, -1}, {gw, gh, 0, 1, gw}, {gw, gh, (long long)(gh - 1) * gw, 1, -(long long)gw}};
        for (int r = 0; r < 4; r++)
            hipLaunchKernelGGL(seam_path_kernel, dim3((unsigned)((dir[r].nlines + 3) / 4)), dim3(256), 0, ctx->stream, d_cand, dS.as<uint16_t>(), dir[r].nlines,
                               dir[r].len, dir[r].base, dir[r].line_stride, dir[r].step, r == 0, c);
        hipLaunchKernelGGL(seam_argmin_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_cand, dS.as<uint16_t>(), dlab.as<uint8_t>(), cells);
        hipLaunchKernelGGL(seam_energy_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_cand, dlab.as<uint8_t>(), gw, gh, c, dacc.as<unsigned long long>());
        hipLaunchKernelGGL(seam_finish_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_cand, dlab.as<uint8_t>(), dacc.as<unsigned long long>(), d_cells, cells);
    }
    MI_HIP(hipGetLastError());
    MI_HIP(hipMemcpyAsync(acc, dacc.p, sizeof(acc), hipMemcpyDeviceToHost, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));
    if (report) {
        report->energy_before = (int64_t)acc[0]; report->energy_after = (int64_t)acc[1];
        report->fallback = acc[1] > acc[0];
        report->changed = report->fallback ? 0 : (int32_t)acc[2];
    }
    return MI355_OK;
}

// d_cells == NULL: stages 1 and 2 first, into the ctx's own cell map
int mi_mosaic_seamcut_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                          const mi355_seamcut_params* params, const uint16_t* d_cells, uint8_t* d_canvas, int cw, int ch, int cws, uint16_t* d_owner,
                          uint16_t* d_count, int row0, int rows, uint8_t* cover_only) {
    SC_PARAMS("mosaic_seamcut")
    float dG[2]; bool go;
    const int rc = mi_render_entry(ctx, "mosaic_seamcut", w, h, n, h9s, cover_only != nullptr, d_canvas != nullptr, cw, ch, cws, row0, rows, dG, go);     // n <= 65535: 16-bit lists, keys and maps
    if (rc != MI355_OK || !go) return rc;
    const int s = 1 << params->level, gw = (cw + s - 1) / s, gh = (ch + s - 1) / s;
    if (!d_cells) {
        if (!d_imgs || !ws) { ctx->set_error("mosaic_seamcut: no cell map and no frames to make one from"); return MI355_ERR_ARG; }
        DevBuf& dcand = ctx->buf("seamcut_candidates");
        DevBuf& dcells = ctx->buf("seamcut_cells");
        MI_HIP(dcand.reserve(sizeof(mi355_seam_cell) * (size_t)gw * gh));
        MI_HIP(dcells.reserve(sizeof(uint16_t) * (size_t)gw * gh));
        int rcs = mi_seam_candidates_dev(ctx, d_imgs, w, h, ws, n, h9s, params, dcand.as<mi355_seam_cell>(), gw, gh);
        if (rcs == MI355_OK) rcs = mi_seam_labels_dev(ctx, dcand.as<mi355_seam_cell>(), gw, gh, params, dcells.as<uint16_t>(), nullptr);
        if (rcs != MI355_OK) return rcs;
        d_cells = dcells.as<uint16_t>();
    }
    FrameTable t;                                        // frame_of ascending: (omega, q) orders as (omega, k)
    bool withheld = false;
    for (int k = 0; k < n; k++) {
        FrameDev f;
        if (!mi_frame_dev_setup(h9s + 9 * k, w[k], h[k], dG, cw, ch, row0, rows, f)) continue;
        if (w[k] < 2 || h[k] < 2 || (d_canvas && ws[k] < 3 * w[k]) || w[k] > RAMP_MAX_SIDE || h[k] > RAMP_MAX_SIDE) { ctx->set_error("mosaic_seamcut: bad image geometry"); return MI355_ERR_ARG; }
        f.src = d_canvas ? d_imgs[k] : nullptr; f.w = w[k]; f.h = h[k]; f.ws = d_canvas ? ws[k] : 0;
        if (d_canvas && !f.src) withheld = true;         // fine as long as the frame owns no pixel of the rows: checked below, before any sample
        t.add(f, k);
        t.ramps.push_back(ramp_of_frame(w[k], h[k], params->ramp));
    }
    if (cover_only && t.fr.empty()) return MI355_OK;
    const int rc2 = mi_frame_table_upload(ctx, t, true, true, cw, rows, row0);
    if (rc2 != MI355_OK) return rc2;
    const dim3 grid((cw + SCT_W - 1) / SCT_W, (rows + SCT_H - 1) / SCT_H);
    auto launch = [&](auto kernel, uint8_t* canvas, uint16_t* owner, uint16_t* count, int* used) {
        ProfScope ps(ctx, "seamcut", 0.0);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, t.d_fr, t.d_ramps, t.d_frame_of, t.nf, t.d_lists, t.d_counts, t.bx_n, d_cells, gw, params->level,
                           canvas, owner, count, used, cw, cws, row0, row0 + rows, dG[0], dG[1]);
    };
    if (cover_only || withheld) {
        // the ownership walk alone, one flag per table entry: the cover call's answer, and what tells a withheld frame that owns nothing
        // from one the render would dereference.  Paid only when a pointer is missing.
        std::vector<int> used;
        int* d_used;
        int rc3 = mi_frame_table_used_begin(ctx, t, &d_used);
        if (rc3 != MI355_OK) return rc3;
        launch(seamcut_tile_kernel<false>, nullptr, nullptr, nullptr, d_used);
        rc3 = mi_frame_table_used_end(ctx, t, used);
        if (rc3 != MI355_OK) return rc3;
        for (int q = 0; q < t.nf; q++) {
            if (!used[q]) continue;
            if (cover_only) cover_only[t.frame_of[q]] = 1;
            else if (!t.fr[q].src) {
                ctx->set_error("mosaic_seamcut: image " + std::to_string(t.frame_of[q]) + " owns pixels of these canvas rows but no pointer to it was given");
                return MI355_ERR_ARG;
            }
        }
        if (cover_only) return MI355_OK;
    }
    if (d_canvas) launch(seamcut_tile_kernel<true>, d_canvas, d_owner, d_count, nullptr);
    else launch(seamcut_tile_kernel<false>, nullptr, d_owner, d_count, nullptr);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(ctx->stream));           // the table goes out of scope
    return MI355_OK;
}

extern "C" int mi355_seam_candidates_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                         const mi355_seamcut_params* params, mi355_seam_cell* d_cand, int gw, int gh) {
    LOCKED_PROLOGUE
    if (!d_imgs || !w || !h || !ws || !h9s || !d_cand || n <= 0) return MI355_ERR_ARG;
    return mi_seam_candidates_dev(ctx, d_imgs, w, h, ws, n, h9s, params, d_cand, gw, gh);
}

extern "C" int mi355_seam_labels_dev(mi355_ctx* ctx, const mi355_seam_cell* d_cand, int gw, int gh, const mi355_seamcut_params* params, uint16_t* d_cells,
                                     mi355_seam_report* report) {
    LOCKED_PROLOGUE
    if (!d_cand || !d_cells) return MI355_ERR_ARG;
    return mi_seam_labels_dev(ctx, d_cand, gw, gh, params, d_cells, report);
}

extern "C" int mi355_seam_cells_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                    const mi355_seamcut_params* params, uint16_t* d_cells, int gw, int gh, mi355_seam_report* report) {
    LOCKED_PROLOGUE
    if (!d_imgs || !w || !h || !ws || !h9s || !d_cells || n <= 0) return MI355_ERR_ARG;
    SC_PARAMS("seam_cells")
    {
        // the grid against the layout before anything is reserved for gw x gh cells
        int lw, lh, lws;
        float dG[2];
        if (mi355_mosaic_layout(w, h, n, h9s, &lw, &lh, &lws, dG) != MI355_OK) { ctx->set_error("seam_cells: no image with h[8] != 0 / empty canvas"); return MI355_ERR_ARG; }
        const int s = 1 << params->level;
        if (gw != (lw + s - 1) / s || gh != (lh + s - 1) / s) {
            ctx->set_error("seam_cells: grid " + std::to_string(gw) + "x" + std::to_string(gh) + ", the layout at this level has " + std::to_string((lw + s - 1) / s) + "x" + std::to_string((lh + s - 1) / s));
            return MI355_ERR_ARG;
        }
    }
    DevBuf& dcand = ctx->buf("seamcut_candidates");
    MI_HIP(dcand.reserve(sizeof(mi355_seam_cell) * (size_t)gw * gh));
    const int rc = mi_seam_candidates_dev(ctx, d_imgs, w, h, ws, n, h9s, params, dcand.as<mi355_seam_cell>(), gw, gh);
    if (rc != MI355_OK) return rc;
    return mi_seam_labels_dev(ctx, dcand.as<mi355_seam_cell>(), gw, gh, params, d_cells, report);
}

// the host twin of the label stage: the same integers through the same sc_pair_cost / sc_argmin / sc_cell_energy
extern "C" int mi355_seam_labels_host(const mi355_seam_cell* cand, int gw, int gh, const mi355_seamcut_params* params, uint16_t* cells, mi355_seam_report* report) {
    mi355_seamcut_params dp;
    if (!params) { mi355_default_seamcut_params(&dp); params = &dp; }
    std::string err;
    if (!cand || !cells || !sc_params_ok(params, err) || !sc_grid_ok(gw, gh, err)) return MI355_ERR_ARG;
    const SeamCosts c = sc_costs(params);
    const size_t n = (size_t)gw * gh;
    std::vector<uint16_t> S(n * SC_SLOTS, 0);
    const struct { int nlines, len; long long base, line_stride, step; } dir[4] = {
        {gh, gw, 0, gw, 1}, {gh, gw, gw - 1, gw, -1}, {gw, gh, 0, 1, gw}, {gw, gh, (long long)(gh - 1) * gw, 1, -(long long)gw}};
    for (const auto& d : dir)
        for (int line = 0; line < d.nlines; line++) {
            long long idx = d.base + line * d.line_stride;
            const mi355_seam_cell* q = nullptr;          // the cell before, when it has a candidate
            int Lq[SC_SLOTS] = {0};
            for (int i = 0; i < d.len; i++, idx += d.step) {
                const mi355_seam_cell& p = cand[idx];
                int L[SC_SLOTS] = {0};
                int mp = SC_INF;
                if (q)
                    for (int b = 0; b < SC_SLOTS; b++) if (q->frame[b] && Lq[b] < mp) mp = Lq[b];
                for (int a = 0; a < SC_SLOTS && p.frame[a]; a++) {
                    L[a] = sc_data_cost(p, a, c);
                    if (!q) continue;
                    int mn = SC_INF;
                    for (int b = 0; b < SC_SLOTS && q->frame[b]; b++) { const int v = Lq[b] + sc_pair_cost(p, a, *q, b, c); if (v < mn) mn = v; }
                    L[a] += mn - mp;
                }
                for (int a = 0; a < SC_SLOTS; a++) { S[(size_t)idx * SC_SLOTS + a] += (uint16_t)L[a]; Lq[a] = L[a]; }
                q = p.frame[0] ? &p : nullptr;
            }
        }
    std::vector<uint8_t> lab(n);
    for (size_t i = 0; i < n; i++) lab[i] = (uint8_t)sc_argmin(cand[i], &S[i * SC_SLOTS]);
    long long e0 = 0, e1 = 0, changed = 0;
    for (int cy = 0; cy < gh; cy++)
        for (int cx = 0; cx < gw; cx++) {
            e0 += sc_cell_energy(cand, nullptr, gw, gh, cx, cy, c);
            e1 += sc_cell_energy(cand, lab.data(), gw, gh, cx, cy, c);
            changed += lab[(size_t)cy * gw + cx] != 0;
        }
    const bool fallback = e1 > e0;
    for (size_t i = 0; i < n; i++) cells[i] = !fallback && lab[i] ? cand[i].frame[lab[i]] : (uint16_t)0;
    if (report) { report->energy_before = e0; report->energy_after = e1; report->fallback = fallback; report->changed = fallback ? 0 : (int32_t)changed; }
    return MI355_OK;
}

extern "C" int mi355_mosaic_seamcut_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                        const mi355_seamcut_params* params, const uint16_t* d_cells, uint8_t* d_canvas, int cw, int ch, int cws,
                                        uint16_t* d_owner, uint16_t* d_count, int row0, int rows) {
    LOCKED_PROLOGUE
    if (!w || !h || !h9s || n <= 0) return MI355_ERR_ARG;
    if (!d_canvas && !d_owner && !d_count) { ctx->set_error("mosaic_seamcut: d_canvas, d_owner and d_count are all NULL"); return MI355_ERR_ARG; }
    if (d_canvas && (!d_imgs || !ws)) { ctx->set_error("mosaic_seamcut: a canvas is asked for but d_imgs or ws is NULL"); return MI355_ERR_ARG; }
    return mi_mosaic_seamcut_dev(ctx, d_imgs, w, h, ws, n, h9s, params, d_cells, d_canvas, cw, ch, cws, d_owner, d_count, row0, rows, nullptr);
}

extern "C" int mi355_mosaic_seamcut_cover(mi355_ctx* ctx, const int* w, const int* h, int n, const float* h9s, const mi355_seamcut_params* params,
                                          const uint16_t* d_cells, int row0, int rows, uint8_t* need) {
    LOCKED_PROLOGUE
    if (!w || !h || !h9s || !need || !d_cells || n <= 0) return MI355_ERR_ARG;
    memset(need, 0, (size_t)n);
    return mi_mosaic_seamcut_dev(ctx, nullptr, w, h, nullptr, n, h9s, params, d_cells, nullptr, 0, 0, 0, nullptr, nullptr, row0, rows, need);
}

// the host form (mi_render_host_begin / _end, frames.hip): all three stages on the staged frames; the owner map comes back when asked for
extern "C" int mi355_mosaic_seamcut(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                    const mi355_seamcut_params* params, uint8_t** canvas, int* cw, int* ch, int* cws, uint16_t** owner) {
    LOCKED_PROLOGUE
    if (!imgs || !w || !h || !ws || !h9s || !canvas || !cw || !ch || !cws) return MI355_ERR_ARG;
    SC_PARAMS("mosaic_seamcut")
    int lw, lh, lws;
    std::vector<const uint8_t*> d_imgs;
    uint8_t* d_canvas;
    int rc = mi_render_host_begin(ctx, "mosaic_seamcut", imgs, w, h, ws, n, h9s, &lw, &lh, &lws, d_imgs, &d_canvas);
    if (rc != MI355_OK) return rc;
    DevBuf& down = ctx->buf("seamline_owner");
    const size_t obytes = sizeof(uint16_t) * (size_t)lw * lh;
    if (owner) MI_HIP(down.reserve(obytes));
    rc = mi_mosaic_seamcut_dev(ctx, d_imgs.data(), w, h, ws, n, h9s, params, nullptr, d_canvas, lw, lh, lws, owner ? down.as<uint16_t>() : nullptr, nullptr, 0, lh, nullptr);
    if (rc != MI355_OK) return rc;
    return mi_render_host_end(ctx, lw, lh, lws, canvas, cw, ch, cws, down.p, obytes, (void**)owner);
}
