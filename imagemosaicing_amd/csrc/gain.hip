// csrc/gain.hip -- exposure gain compensation (gfx950): per-frame, per-channel gains from the frames' overlaps, applied to the texels before a
// render (include/mi355_mosaic.h, "exposure gain compensation").  OpenCV's detail::GainCompensator restricted to the listed pairs, with the
// overlap means measured on a lattice of canvas pixels through the refined render's own map and sample (mosaic_frame.h).
//
//   gain_stats_kernel   the hot path.  The work list is built on the host: tiles of 64 x 16 lattice points, over each listed pair's
//                       canvas-box intersection (pair tiles) and over each frame's own box (cover tiles, for N_k).  One launch for all of
//                       them; one lane per lattice point column, 4 lattice rows per lane.  A pair tile maps the point into both frames and,
//                       where both have a sample, gathers both 2 x 2 neighbourhoods (load_quad3, the render's loads) and sums the bytes; a
//                       cover tile only maps and counts (no texel loads).  The sums are reduced in 32-bit registers (at most 256 x 4 x 255
//                       per field and workgroup) and land with one 64-bit vector atomic per field per workgroup in a device record array:
//                       integer sums, so the result does not depend on the order the workgroups run in.
//   gain_apply_kernel   a row-streaming LUT pass over every frame in one launch: a workgroup builds its frame's 3 x 256 table in LDS from
//                       the gains (in double) and streams 16 rows, 16 B in and 16 B out per lane where the row is aligned, bytes at the ends.
//                       Its roofline is HBM: 2 x 3 w h bytes per frame.
// Block gains (a gain map per frame on a grid of cells; header section "block gain compensation") follow further down with their own kernels.
// The two apply kernels are one row streamer (stream_rows) around different middles: how a byte becomes an output byte (a LUT read, or the
// Q12 interpolation).  The two stats kernels keep their sample walk inline (see the note above gain_stats_kernel).  On the host the stages
// share the stats' checks, frame table and work list (stats_setup and the tile builder: stats_tiles.h, which sharp.hip uses as well), the
// apply's frame check and launch (check_apply_frames, launch_apply) and the compensate calls' choice of frames (NonUnit).  The parameter
// checks and both solves are host-only: gain_solve.cpp (gain.h).
#include "common.h"
#include "gain.h"
#include "hmath.h"
#include "mosaic_frame.h"
#include "stats_tiles.h"
#include <algorithm>
#include <cmath>
#include <cstddef>

namespace {

using namespace mi_gain;

constexpr int AP_NT = 256, AP_ROWS = 16;      // apply: lanes and frame rows per workgroup

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The two stats kernels carry the same walk over a tile's samples (lane to lattice point, frame_src, src_inside, frame_sample3) spelled out
// twice.  A shared walk that hands each sample to a callable was tried, as one function and as a cover and a pair walk: with it the compiler
// schedules the unrolled rows differently and block_gain_stats_kernel grows from 3235 to 3540 instructions (v_pk_* 114 -> 71).  So, as with
// mosaic_tile_kernel in mosaic_frame.h, the walk stays inline: a fix to one copy goes into the other as well.
__global__ __launch_bounds__(256) void gain_stats_kernel(const FrameDev* fr, const GainTile* tiles, int step, float dGx, float dGy,
                                                         unsigned long long* pair_acc, unsigned long long* cover_acc) {
    const GainTile t = tiles[blockIdx.x];
    const int lx = t.lx0 + (threadIdx.x & 63), ly0 = t.ly0 + (threadIdx.x >> 6);
    const FrameDev& fa = fr[t.a];
    const float wa1 = (float)(fa.w - 1), ha1 = (float)(fa.h - 1);
    const float xf = (float)(lx * step) - dGx;                   // the render's xf = (float)xD - dGx
    const bool col = lx <= t.lx1;
    int v[7] = {0, 0, 0, 0, 0, 0, 0};                            // count, sum_a[3], sum_b[3]
    if (t.b < 0) {
#pragma unroll
        for (int r = 0; r < GT_Y / 4; r++) {
            const int ly = ly0 + 4 * r;
            const float yf = (float)(ly * step) - dGy;
            float xs, ys;
            frame_src(fa, xf, yf, xs, ys);
            v[0] += (col && ly <= t.ly1 && src_inside(xs, ys, wa1, ha1)) ? 1 : 0;
        }
    } else {
        const FrameDev& fb = fr[t.b];
        const float wb1 = (float)(fb.w - 1), hb1 = (float)(fb.h - 1);
#pragma unroll
        for (int r = 0; r < GT_Y / 4; r++) {
            const int ly = ly0 + 4 * r;
            const float yf = (float)(ly * step) - dGy;
            float xa, ya, xb, yb;
            frame_src(fa, xf, yf, xa, ya);
            frame_src(fb, xf, yf, xb, yb);
            if (col && ly <= t.ly1 && src_inside(xa, ya, wa1, ha1) && src_inside(xb, yb, wb1, hb1)) {
                unsigned b0, g0, r0, b1, g1, r1;
                frame_sample3(fa, xa, ya, b0, g0, r0);
                frame_sample3(fb, xb, yb, b1, g1, r1);
                v[0] += 1; v[1] += (int)b0; v[2] += (int)g0; v[3] += (int)r0; v[4] += (int)b1; v[5] += (int)g1; v[6] += (int)r1;
            }
        }
    }
    __shared__ int s_v[4][7];
    const int nv = t.b < 0 ? 1 : 7;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = 0; i < nv; i++) {
        const int s = wave_sum(v[i]);
        if (lane == 0) s_v[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < nv) {
        const int i = threadIdx.x;
        const long long s = (long long)s_v[0][i] + s_v[1][i] + s_v[2][i] + s_v[3][i];
        if (s != 0) {
            unsigned long long* dst = t.b < 0 ? cover_acc + t.rec : pair_acc + 7 * (size_t)t.rec + i;
            atomicAdd(dst, (unsigned long long)s);
        }
    }
}

// One record per frame an apply launch works on.  Both forms begin alike: frame_of_block, stream_rows and launch_apply read that part.
struct ApplyHead { const uint8_t* src; uint8_t* dst; int w, h, ws, first_block; };
struct ApplyFrame : ApplyHead { float g[3]; int _pad; };
struct BlockApplyFrame : ApplyHead { int q_off; int _pad; };
static_assert(offsetof(ApplyHead, first_block) == 28 && sizeof(ApplyHead) == 32 && sizeof(ApplyFrame) == 48 && sizeof(BlockApplyFrame) == 40, "apply record layout");

// the record of this workgroup's frame: the last k with first_block <= blockIdx.x (first_block ascends).  Ends in a barrier.
template <class Rec>
__device__ __forceinline__ const Rec& frame_of_block(const Rec* frames, int nf) {
    __shared__ int s_k;
    if (threadIdx.x == 0) {
        int lo = 0, hi = nf - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (frames[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
        s_k = lo;
    }
    __syncthreads();
    return frames[s_k];
}

// Rows y0 .. y0 + AP_ROWS - 1 of frame f from src to dst: 16 B in and 16 B out per lane where the row is aligned, bytes at its ends.  What a
// byte becomes is the cursor's business: cursor_of_row(y - y0) gives a row's cursor, seek(off) puts it at byte offset off of the row, map(v)
// is the output byte for input byte v there, next() moves it one byte on.
template <class RowCursor>
__device__ __forceinline__ void stream_rows(const ApplyHead& f, int y0, RowCursor cursor_of_row) {
    const int nb = 3 * f.w;
    for (int y = y0; y < y0 + AP_ROWS && y < f.h; y++) {
        auto cur = cursor_of_row(y - y0);
        const uint8_t* srow = f.src + (size_t)y * f.ws;
        uint8_t* drow = f.dst + (size_t)y * f.ws;
        int head = (int)((16 - ((uintptr_t)srow & 15)) & 15);
        if (head > nb) head = nb;
        const bool vec = (((uintptr_t)(drow + head)) & 15) == 0;
        const int nvec = vec ? (nb - head) >> 4 : 0;
        const int tail = head + 16 * nvec;
        for (int i = threadIdx.x; i < nvec; i += AP_NT) {
            const int off = head + 16 * i;
            const uint4 in = *reinterpret_cast<const uint4*>(srow + off);
            const unsigned w4[4] = {in.x, in.y, in.z, in.w};
            unsigned o4[4];
            cur.seek(off);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                unsigned o = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    o |= cur.map((w4[q] >> (8 * j)) & 0xffu) << (8 * j);
                    cur.next();
                }
                o4[q] = o;
            }
            *reinterpret_cast<uint4*>(drow + off) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
        }
        // the row's ends (or the whole row where src and dst are not aligned alike): bytes
        const int nhead = vec ? head : nb;
        for (int i = threadIdx.x; i < nhead; i += AP_NT) { cur.seek(i); drow[i] = (uint8_t)cur.map(srow[i]); }
        if (vec)
            for (int i = tail + (int)threadIdx.x; i < nb; i += AP_NT) { cur.seek(i); drow[i] = (uint8_t)cur.map(srow[i]); }
    }
}

struct LutCursor {
    const uint8_t* lut; int c;                                  // the 3 x 256 table; the channel of the byte the cursor is at
    __device__ __forceinline__ void seek(int off) { c = off % 3; }
    __device__ __forceinline__ unsigned map(unsigned v) const { return lut[c * 256 + v]; }
    __device__ __forceinline__ void next() { c = c == 2 ? 0 : c + 1; }
};

__global__ __launch_bounds__(AP_NT) void gain_apply_kernel(const ApplyFrame* frames, int nf) {
    __shared__ uint8_t lut[3 * 256];
    const ApplyFrame& f = frame_of_block(frames, nf);
    {
        const int v = threadIdx.x;                                  // AP_NT == 256: one table entry per lane and channel
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double o = floor((double)f.g[c] * (double)v + 0.5);
            o = o < 0.0 ? 0.0 : (o > 255.0 ? 255.0 : o);
            lut[c * 256 + v] = (uint8_t)(int)o;
        }
    }
    __syncthreads();
    stream_rows(f, ((int)blockIdx.x - f.first_block) * AP_ROWS, [&](int) __attribute__((always_inline)) { return LutCursor{lut, 0}; });
}

int gain_stats(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
               const int32_t* pairs_ab, int n_pairs, int step, mi355_gain_pair_stats* pair_stats, int64_t* frame_cover) {
    if (n_pairs > 0 && !pair_stats) { ctx->set_error("gain_stats: NULL argument or n_pairs < 0"); return MI355_ERR_ARG; }
    StatsFrames s;
    { const int rc = stats_setup(ctx, "gain_stats: ", d_imgs, w, h, ws, n, h9s, pairs_ab, n_pairs, step, nullptr, s); if (rc != MI355_OK) return rc; }
    std::vector<GainTile> tiles;
    s.push_cover_tiles(tiles, step);
    for (int p = 0; p < n_pairs; p++) s.push_pair_tiles(tiles, pairs_ab[2 * p], pairs_ab[2 * p + 1], p, step);
    const size_t n_acc = (size_t)n_pairs * 7 + (size_t)n;
    DevBuf& dt = ctx->buf("gain_tiles"); DevBuf& dacc = ctx->buf("gain_acc");
    MI_HIP(dt.reserve(sizeof(GainTile) * std::max<size_t>(tiles.size(), 1)));
    MI_HIP(dacc.reserve(sizeof(unsigned long long) * n_acc));
    if (!tiles.empty()) MI_HIP(hipMemcpyAsync(dt.p, tiles.data(), sizeof(GainTile) * tiles.size(), hipMemcpyHostToDevice, ctx->stream));
    MI_HIP(hipMemsetAsync(dacc.p, 0, sizeof(unsigned long long) * n_acc, ctx->stream));
    unsigned long long* pair_acc = dacc.as<unsigned long long>();
    unsigned long long* cover_acc = pair_acc + (size_t)n_pairs * 7;
    for (size_t t0 = 0; t0 < tiles.size(); t0 += (size_t)1 << 30) {     // grid.x < 2^31
        const size_t nt = std::min(tiles.size() - t0, (size_t)1 << 30);
        ProfScope ps(ctx, "gain_stats", 0.0);
        hipLaunchKernelGGL(gain_stats_kernel, dim3((unsigned)nt), dim3(256), 0, ctx->stream, s.d_fr, dt.as<GainTile>() + t0, step, s.dG[0], s.dG[1], pair_acc,
                           cover_acc);
        MI_HIP(hipGetLastError());
    }
    std::vector<unsigned long long> acc(n_acc);
    MI_HIP(hipMemcpyAsync(acc.data(), dacc.p, sizeof(unsigned long long) * n_acc, hipMemcpyDeviceToHost, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));                 // s.fr / tiles are locals
    for (int p = 0; p < n_pairs; p++) {
        mi355_gain_pair_stats& st = pair_stats[p];
        st.a = pairs_ab[2 * p]; st.b = pairs_ab[2 * p + 1];
        st.n = (int64_t)acc[7 * (size_t)p];
        for (int c = 0; c < 3; c++) { st.sum_a[c] = (int64_t)acc[7 * (size_t)p + 1 + c]; st.sum_b[c] = (int64_t)acc[7 * (size_t)p + 4 + c]; }
    }
    if (frame_cover)
        for (int k = 0; k < n; k++) frame_cover[k] = (int64_t)acc[(size_t)n_pairs * 7 + k];
    return MI355_OK;
}

// What mi355_apply_gains_dev and mi355_apply_block_gains_dev ask of their frames (who prefixes the messages): pointers, geometry, finite gains
// (per_frame values each), and a dst range that meets no other range but its own src range exactly.
int check_apply_frames(mi355_ctx* ctx, const std::string& who, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws,
                       int n, const float* gains, int per_frame) {
    struct Span { uintptr_t lo, hi; int k; };
    std::vector<Span> dsts, srcs;
    for (int k = 0; k < n; k++) {
        const std::string fk = who + ": frame " + std::to_string(k);
        if (!d_src[k] || !d_dst[k]) { ctx->set_error(fk + ": NULL pointer"); return MI355_ERR_ARG; }
        if (w[k] < 1 || h[k] < 1 || ws[k] < 3 * w[k]) { ctx->set_error(fk + ": bad geometry w=" + std::to_string(w[k]) + " h=" + std::to_string(h[k]) + " ws=" + std::to_string(ws[k])); return MI355_ERR_ARG; }
        for (int c = 0; c < per_frame; c++)
            if (!std::isfinite(gains[(size_t)per_frame * k + c])) { ctx->set_error(fk + ": gain[" + std::to_string(c) + "] is not finite"); return MI355_ERR_ARG; }
        const size_t bytes = (size_t)ws[k] * (size_t)(h[k] - 1) + 3 * (size_t)w[k];
        dsts.push_back({(uintptr_t)d_dst[k], (uintptr_t)d_dst[k] + bytes, k});
        srcs.push_back({(uintptr_t)d_src[k], (uintptr_t)d_src[k] + bytes, k});
    }
    // a dst range may meet no other range but its own src range exactly
    std::sort(dsts.begin(), dsts.end(), [](const Span& x, const Span& y) { return x.lo < y.lo; });
    for (size_t i = 1; i < dsts.size(); i++)
        if (dsts[i].lo < dsts[i - 1].hi) { ctx->set_error(who + ": dst of frame " + std::to_string(dsts[i].k) + " overlaps dst of frame " + std::to_string(dsts[i - 1].k)); return MI355_ERR_ARG; }
    for (const Span& s : srcs) {
        auto it = std::lower_bound(dsts.begin(), dsts.end(), s.hi, [](const Span& x, uintptr_t v) { return x.lo < v; });   // first dst starting at or after s.hi
        if (it == dsts.begin()) continue;
        --it;                                                                                                              // the last dst starting before s.hi
        if (it->hi <= s.lo) continue;
        if (it->k == s.k && it->lo == s.lo) continue;                                                                      // in place
        ctx->set_error(who + ": dst of frame " + std::to_string(it->k) + " overlaps src of frame " + std::to_string(s.k) + " without being equal to it");
        return MI355_ERR_ARG;
    }
    return MI355_OK;
}

bool all_one(const float* g, int per) {
    bool unit = true;
    for (int i = 0; i < per; i++) unit = unit && g[i] == 1.0f;
    return unit;
}

// One apply launch over checked frames with `per` gains each: a record for every frame but those in place with gains all 1 (their bytes stay
// as they are), AP_ROWS rows per workgroup, the records in ctx buffer buf, the kernel's time under scope.  fill(rec, gains of the frame) sets
// the form's own fields; launch(records on the device, their number, workgroups) uploads what else the form needs and starts its kernel.
template <class Rec, class Fill, class Launch>
int launch_apply(mi355_ctx* ctx, const char* buf, const char* scope, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws,
                 int n, const float* gains, int per, Fill fill, Launch launch) {
    std::vector<Rec> af;
    int blocks = 0;
    double bytes = 0.0;
    for (int k = 0; k < n; k++) {
        const float* g = gains + (size_t)per * k;
        if (all_one(g, per) && d_src[k] == d_dst[k]) continue;
        Rec f;
        f.src = d_src[k]; f.dst = d_dst[k]; f.w = w[k]; f.h = h[k]; f.ws = ws[k]; f.first_block = blocks; f._pad = 0;
        fill(f, g);
        af.push_back(f);
        blocks += (h[k] + AP_ROWS - 1) / AP_ROWS;
        bytes += 6.0 * (double)w[k] * h[k];
    }
    if (af.empty()) return MI355_OK;
    DevBuf& daf = ctx->buf(buf);
    MI_HIP(daf.reserve(sizeof(Rec) * af.size()));
    MI_HIP(hipMemcpyAsync(daf.p, af.data(), sizeof(Rec) * af.size(), hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, scope, bytes);
        MI_HIP(launch(daf.as<Rec>(), (int)af.size(), blocks));
        MI_HIP(hipGetLastError());
    }
    MI_HIP(hipStreamSynchronize(ctx->stream));                 // af and what fill gathered are locals
    return MI355_OK;
}

int apply_gains(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws, int n, const float* gains) {
    std::string err;
    if (!d_src || !d_dst || !w || !h || !ws || !gains) { ctx->set_error("apply_gains: NULL argument"); return MI355_ERR_ARG; }
    if (!check_frames_n(n, err)) { ctx->set_error("apply_gains: " + err); return MI355_ERR_ARG; }
    { const int rc = check_apply_frames(ctx, "apply_gains", d_src, d_dst, w, h, ws, n, gains, 3); if (rc != MI355_OK) return rc; }
    return launch_apply<ApplyFrame>(ctx, "gain_apply_frames", "gain_apply", d_src, d_dst, w, h, ws, n, gains, 3,
        [](ApplyFrame& f, const float* g) { for (int c = 0; c < 3; c++) f.g[c] = g[c]; },
        [&](const ApplyFrame* d_af, int nf, int blocks) {
            hipLaunchKernelGGL(gain_apply_kernel, dim3(blocks), dim3(AP_NT), 0, ctx->stream, d_af, nf);
            return hipSuccess;
        });
}

// the frames whose `per` gains are not all 1: what a compensate call applies in place.  The others (the frames the render skips; their
// pointers may be NULL) are left out and so not touched.
struct NonUnit {
    std::vector<uint8_t*> img;
    std::vector<int> w, h, ws;
    std::vector<float> g;
    NonUnit(uint8_t* const* d_imgs, const int* w_, const int* h_, const int* ws_, int n, const float* gains, int per) {
        for (int k = 0; k < n; k++) {
            if (all_one(gains + (size_t)per * k, per)) continue;
            img.push_back(d_imgs[k]); w.push_back(w_[k]); h.push_back(h_[k]); ws.push_back(ws_[k]);
            g.insert(g.end(), gains + (size_t)per * k, gains + (size_t)per * (k + 1));
        }
    }
    const uint8_t* const* src() const { return (const uint8_t* const*)img.data(); }
};

// ---- block gains: a gain map per frame (include/mi355_mosaic.h, "block gain compensation") ------------------------------------------------
//   block_gain_stats_kernel    gain_stats_kernel's work list and walk; the sums are binned by (cell_a, cell_b).  A lane adds up its four
//                              points in registers while their key stays the same; a wave whose lanes all end with one and the same key (the
//                              usual tile: a cell is hundreds of canvas pixels wide) reduces with shuffles as gain_stats_kernel does, every
//                              other lane adds its run to an LDS table keyed by hashing (BG_SLOTS = 1024 slots for at most 1024 points of a
//                              tile, so a key always finds a slot), and the occupied slots land with one 64-bit vector atomic per field in the
//                              batch's dense table: 7 planes of pairs x cells^2 accumulators.  Pairs go in batches whose table fits
//                              BG_TABLE_BYTES.  Integer sums: the order of the workgroups does not matter.
//   block_gain_compact_kernel  the table's entries with n > 0 become records (order arbitrary: the host sorts them).  The record buffer holds
//                              sum over the batch's pairs of min(cells^2, lattice points of the pair's tiles), which no batch can exceed;
//                              the kernel checks the slot all the same and the launcher fails on the flag.
//   block_gain_apply_kernel    gain_apply_kernel's stream_rows with the header's integer interpolation in the LUT's place: per workgroup the
//                              16 rows' R_i (grid_x x 3 each) and the columns' (i0, fx) in LDS, so the divisions happen once per 16 rows.
constexpr int BG_SLOTS = 1024;
constexpr size_t BG_TABLE_BYTES = (size_t)32 << 20;
constexpr int BA_COLS = 8192;                   // widest frame whose column table fits; wider frames compute (i0, fx) per pixel

// (xi * g) / w for 0 <= xi < w <= 2^20 and g <= 16: the product is below 2^24, exact in float; the float quotient is off by at most one
__device__ __forceinline__ int bg_cell(int xi, int g, int w, float rw) {
    const int num = xi * g;
    int q = (int)((float)num * rw);
    const int r = num - q * w;
    q += r >= w ? 1 : (r < 0 ? -1 : 0);
    return q;
}

// a lane's run v (NV fields) into key's slot of the LDS table
template <int NV>
__device__ __forceinline__ void bg_flush(int* s_key, int (*s_val)[BG_SLOTS], int key, const int (&v)[7]) {
    unsigned s = ((unsigned)key * 2654435761u) >> 22;                    // 10 bits
    for (;;) {
        const int old = atomicCAS(&s_key[s], -1, key);
        if (old == -1 || old == key) break;
        s = (s + 1) & (BG_SLOTS - 1);                                    // at most 1024 keys for 1024 slots: ends
    }
#pragma unroll
    for (int i = 0; i < NV; i++)
        if (v[i]) atomicAdd(&s_val[i][s], v[i]);
}

// the lanes' runs into the LDS table: whole waves with one key through shuffles, the rest lane by lane
template <int NV>
__device__ __forceinline__ void bg_finish(int* s_key, int (*s_val)[BG_SLOTS], int cur, bool flushed, int (&v)[7]) {
    if (!__any(flushed)) {
        const unsigned long long m = __ballot(cur >= 0);
        if (m) {
            const int k0 = __shfl(cur, __ffsll((long long)m) - 1);
            if (__all(cur < 0 || cur == k0)) {
#pragma unroll
                for (int i = 0; i < NV; i++) v[i] = wave_sum(v[i]);
                if ((threadIdx.x & 63) == 0) bg_flush<NV>(s_key, s_val, k0, v);
                cur = -1;
            }
        }
    }
    if (cur >= 0) bg_flush<NV>(s_key, s_val, cur, v);
}

__global__ __launch_bounds__(256) void block_gain_stats_kernel(const FrameDev* fr, const GainTile* tiles, int step, float dGx, float dGy, int gx, int gy,
                                                               unsigned long long* pair_acc, size_t plane, unsigned long long* cover_acc) {
    __shared__ int s_key[BG_SLOTS];
    __shared__ int s_val[7][BG_SLOTS];
    for (int i = threadIdx.x; i < BG_SLOTS; i += 256) {
        s_key[i] = -1;
#pragma unroll
        for (int f = 0; f < 7; f++) s_val[f][i] = 0;
    }
    __syncthreads();
    const GainTile t = tiles[blockIdx.x];
    const int lx = t.lx0 + (threadIdx.x & 63), ly0 = t.ly0 + (threadIdx.x >> 6);
    const FrameDev& fa = fr[t.a];
    const float wa1 = (float)(fa.w - 1), ha1 = (float)(fa.h - 1);
    const float rwa = 1.0f / (float)fa.w, rha = 1.0f / (float)fa.h;
    const float xf = (float)(lx * step) - dGx;                   // the render's xf = (float)xD - dGx
    const bool col = lx <= t.lx1;
    const int cells = gx * gy;
    int v[7] = {0, 0, 0, 0, 0, 0, 0};                            // count, sum_a[3], sum_b[3] of the lane's current key
    int cur = -1;
    bool flushed = false;
    if (t.b < 0) {
#pragma unroll
        for (int r = 0; r < GT_Y / 4; r++) {
            const int ly = ly0 + 4 * r;
            const float yf = (float)(ly * step) - dGy;
            float xs, ys;
            frame_src(fa, xf, yf, xs, ys);
            if (col && ly <= t.ly1 && src_inside(xs, ys, wa1, ha1)) {
                const int key = bg_cell((int)ys, gy, fa.h, rha) * gx + bg_cell((int)xs, gx, fa.w, rwa);
                if (cur >= 0 && key != cur) { bg_flush<1>(s_key, s_val, cur, v); v[0] = 0; flushed = true; }
                cur = key;
                v[0] += 1;
            }
        }
        bg_finish<1>(s_key, s_val, cur, flushed, v);
    } else {
        const FrameDev& fb = fr[t.b];
        const float wb1 = (float)(fb.w - 1), hb1 = (float)(fb.h - 1);
        const float rwb = 1.0f / (float)fb.w, rhb = 1.0f / (float)fb.h;
#pragma unroll
        for (int r = 0; r < GT_Y / 4; r++) {
            const int ly = ly0 + 4 * r;
            const float yf = (float)(ly * step) - dGy;
            float xa, ya, xb, yb;
            frame_src(fa, xf, yf, xa, ya);
            frame_src(fb, xf, yf, xb, yb);
            if (col && ly <= t.ly1 && src_inside(xa, ya, wa1, ha1) && src_inside(xb, yb, wb1, hb1)) {
                unsigned b0, g0, r0, b1, g1, r1;
                frame_sample3(fa, xa, ya, b0, g0, r0);
                frame_sample3(fb, xb, yb, b1, g1, r1);
                const int ca = bg_cell((int)ya, gy, fa.h, rha) * gx + bg_cell((int)xa, gx, fa.w, rwa);
                const int cb = bg_cell((int)yb, gy, fb.h, rhb) * gx + bg_cell((int)xb, gx, fb.w, rwb);
                const int key = ca * cells + cb;
                if (cur >= 0 && key != cur) {
                    bg_flush<7>(s_key, s_val, cur, v);
#pragma unroll
                    for (int i = 0; i < 7; i++) v[i] = 0;
                    flushed = true;
                }
                cur = key;
                v[0] += 1; v[1] += (int)b0; v[2] += (int)g0; v[3] += (int)r0; v[4] += (int)b1; v[5] += (int)g1; v[6] += (int)r1;
            }
        }
        bg_finish<7>(s_key, s_val, cur, flushed, v);
    }
    __syncthreads();
    const int nv = t.b < 0 ? 1 : 7;
    for (int s = threadIdx.x; s < BG_SLOTS; s += 256) {
        const int key = s_key[s];
        if (key < 0) continue;
        if (t.b < 0) { atomicAdd(cover_acc + (size_t)t.a * cells + key, (unsigned long long)s_val[0][s]); continue; }
        unsigned long long* dst = pair_acc + (size_t)t.rec * cells * cells + key;
        for (int i = 0; i < nv; i++) {
            const int x = s_val[i][s];
            if (x) atomicAdd(dst + (size_t)i * plane, (unsigned long long)x);
        }
    }
}

// counter[0]: records written (or wanted), counter[1]: a record found no room
__global__ __launch_bounds__(256) void block_gain_compact_kernel(const unsigned long long* acc, size_t plane, int cells, int pair0, mi355_block_gain_stats* out,
                                                                 unsigned cap, unsigned* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool has = i < plane && acc[i] != 0;
    const unsigned long long m = __ballot(has);
    if (!m) return;
    const int lane = threadIdx.x & 63, lead = __ffsll((long long)m) - 1;
    unsigned base = 0;
    if (lane == lead) base = atomicAdd(counter, (unsigned)__popcll(m));
    base = __shfl(base, lead);
    if (!has) return;
    const unsigned slot = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (slot >= cap) { counter[1] = 1u; return; }
    const size_t c2 = (size_t)cells * cells;
    const int key = (int)(i % c2);
    mi355_block_gain_stats r;
    r.pair = pair0 + (int)(i / c2); r.cell_a = key / cells; r.cell_b = key % cells; r.reserved = 0;
    r.n = (int64_t)acc[i];
    for (int c = 0; c < 3; c++) { r.sum_a[c] = (int64_t)acc[(size_t)(1 + c) * plane + i]; r.sum_b[c] = (int64_t)acc[(size_t)(4 + c) * plane + i]; }
    out[slot] = r;
}

// the header's i0 and fx (or j0 and fy) of pixel x along an axis of w pixels and g cells
__device__ __forceinline__ void bg_axis(int x, int g, int w, unsigned& i0, unsigned& f) {
    int num = (2 * x + 1) * g - w;
    const int top = 2 * w * (g - 1);
    num = num < 0 ? 0 : (num > top ? top : num);
    const unsigned d = 2u * (unsigned)w;
    i0 = (unsigned)num / d;
    f = (((unsigned)num - i0 * d) * 256u) / d;
}

// the block form's cursor: pixel x and channel c of the current byte, and the pixel's column (offsets of R_i0, R_i1 in the row's R, and fx),
// loaded anew whenever x changes
struct BlockCursor {
    const uint32_t* R; const uint16_t* cols; bool table; int w, gx;       // the row's R_i; the column table (i0 << 8 | fx) where table
    int x, c; unsigned o0, o1, fx;
    __device__ __forceinline__ void column() {
        const int xc = x < w ? x : w - 1;
        unsigned i0;
        if (table) { const unsigned e = cols[xc]; i0 = e >> 8; fx = e & 255u; }
        else bg_axis(xc, gx, w, i0, fx);
        o0 = 3u * i0; o1 = 3u * min(i0 + 1u, (unsigned)gx - 1u);
    }
    __device__ __forceinline__ void seek(int off) { x = off / 3; c = off - 3 * x; column(); }
    __device__ __forceinline__ unsigned map(unsigned v) const {
        const unsigned G = (256u - fx) * R[o0 + c] + fx * R[o1 + c];
        const unsigned o = (((G + 128u) >> 8) * v + (1u << 19)) >> 20;
        return o > 255u ? 255u : o;
    }
    __device__ __forceinline__ void next() { if (c == 2) { c = 0; x++; column(); } else c++; }
};

__global__ __launch_bounds__(AP_NT) void block_gain_apply_kernel(const BlockApplyFrame* frames, int nf, const uint16_t* qs, int gx, int gy) {
    __shared__ uint16_t s_col[BA_COLS];                         // i0 << 8 | fx
    __shared__ uint32_t s_R[AP_ROWS][MAX_GRID * 3];             // R_i of the workgroup's rows, [i][channel]
    const BlockApplyFrame& f = frame_of_block(frames, nf);
    const int y0 = ((int)blockIdx.x - f.first_block) * AP_ROWS;
    const int g3 = gx * 3;
    for (int e = threadIdx.x; e < AP_ROWS * g3; e += AP_NT) {
        const int r = e / g3, ic = e - r * g3;
        if (y0 + r >= f.h) break;
        unsigned j0, fy;
        bg_axis(y0 + r, gy, f.h, j0, fy);
        const unsigned j1 = min(j0 + 1u, (unsigned)gy - 1u);
        const uint16_t* q = qs + f.q_off;
        s_R[r][ic] = (256u - fy) * q[j0 * g3 + ic] + fy * q[j1 * g3 + ic];
    }
    const bool table = f.w <= BA_COLS;
    if (table)
        for (int x = threadIdx.x; x < f.w; x += AP_NT) {
            unsigned i0, fx;
            bg_axis(x, gx, f.w, i0, fx);
            s_col[x] = (uint16_t)(i0 << 8 | fx);
        }
    __syncthreads();
    stream_rows(f, y0, [&](int r) __attribute__((always_inline)) { return BlockCursor{s_R[r], s_col, table, f.w, gx, 0, 0, 0u, 0u, 0u}; });
}

int block_gain_stats(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s, const int32_t* pairs_ab,
                     int n_pairs, int step, int gx, int gy, std::vector<mi355_block_gain_stats>& recs, int64_t* cell_cover) {
    const std::string who = "block_gain_stats: ";
    recs.clear();
    StatsFrames s;
    const int grid[2] = {gx, gy};
    { const int rc = stats_setup(ctx, who, d_imgs, w, h, ws, n, h9s, pairs_ab, n_pairs, step, grid, s); if (rc != MI355_OK) return rc; }
    const int cells = gx * gy;
    const size_t c2 = (size_t)cells * cells;
    const int per_batch = (int)std::max<size_t>(1, BG_TABLE_BYTES / (c2 * 7 * sizeof(unsigned long long)));
    const size_t n_cover = (size_t)n * cells;
    DevBuf& dt = ctx->buf("gain_tiles"); DevBuf& dacc = ctx->buf("block_gain_acc");
    DevBuf& dcov = ctx->buf("block_gain_cover"); DevBuf& dout = ctx->buf("block_gain_records"); DevBuf& dcnt = ctx->buf("block_gain_count");
    MI_HIP(dcov.reserve(sizeof(unsigned long long) * n_cover));
    MI_HIP(dcnt.reserve(2 * sizeof(unsigned)));
    MI_HIP(hipMemsetAsync(dcov.p, 0, sizeof(unsigned long long) * n_cover, ctx->stream));
    std::vector<GainTile> tiles;
    for (int p0 = 0; p0 == 0 || p0 < n_pairs; p0 += per_batch) {
        const int np = std::min(per_batch, n_pairs - p0);
        const size_t plane = (size_t)std::max(np, 0) * c2;
        tiles.clear();
        if (p0 == 0) s.push_cover_tiles(tiles, step);
        size_t cap = 0;                                                // records this batch can give
        for (int p = p0; p < p0 + np; p++) {
            const size_t t0 = tiles.size();
            s.push_pair_tiles(tiles, pairs_ab[2 * p], pairs_ab[2 * p + 1], p - p0, step);
            size_t pts = 0;
            for (size_t t = t0; t < tiles.size(); t++) pts += (size_t)(tiles[t].lx1 - tiles[t].lx0 + 1) * (size_t)(tiles[t].ly1 - tiles[t].ly0 + 1);
            cap += std::min(pts, c2);
        }
        if (tiles.empty()) continue;
        if (tiles.size() >= ((size_t)1 << 31) || cap >= ((size_t)1 << 32)) { ctx->set_error(who + "too many tiles or records in one batch"); return MI355_ERR_FAILED; }
        MI_HIP(dt.reserve(sizeof(GainTile) * tiles.size()));
        MI_HIP(dacc.reserve(sizeof(unsigned long long) * std::max<size_t>(7 * plane, 1)));
        MI_HIP(dout.reserve(sizeof(mi355_block_gain_stats) * std::max<size_t>(cap, 1)));
        MI_HIP(hipMemcpyAsync(dt.p, tiles.data(), sizeof(GainTile) * tiles.size(), hipMemcpyHostToDevice, ctx->stream));
        if (plane) MI_HIP(hipMemsetAsync(dacc.p, 0, sizeof(unsigned long long) * 7 * plane, ctx->stream));
        MI_HIP(hipMemsetAsync(dcnt.p, 0, 2 * sizeof(unsigned), ctx->stream));
        {
            ProfScope ps(ctx, "block_gain_stats", 0.0);
            hipLaunchKernelGGL(block_gain_stats_kernel, dim3((unsigned)tiles.size()), dim3(256), 0, ctx->stream, s.d_fr, dt.as<GainTile>(), step, s.dG[0], s.dG[1],
                               gx, gy, dacc.as<unsigned long long>(), plane, dcov.as<unsigned long long>());
            MI_HIP(hipGetLastError());
        }
        unsigned cnt[2] = {0, 0};
        if (plane && cap) {
            ProfScope ps(ctx, "block_gain_compact", (double)plane * 8.0);
            hipLaunchKernelGGL(block_gain_compact_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, ctx->stream, dacc.as<unsigned long long>(), plane,
                               cells, p0, dout.as<mi355_block_gain_stats>(), (unsigned)cap, dcnt.as<unsigned>());
            MI_HIP(hipGetLastError());
        }
        MI_HIP(hipMemcpyAsync(cnt, dcnt.p, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));                 // tiles is reused by the next batch
        if (cnt[1] || cnt[0] > cap) { ctx->set_error(who + "record buffer too small (" + std::to_string(cnt[0]) + " records for " + std::to_string(cap) + ")"); return MI355_ERR_FAILED; }
        if (cnt[0]) {
            const size_t at = recs.size();
            recs.resize(at + cnt[0]);
            MI_HIP(hipMemcpyAsync(recs.data() + at, dout.p, sizeof(mi355_block_gain_stats) * cnt[0], hipMemcpyDeviceToHost, ctx->stream));
            MI_HIP(hipStreamSynchronize(ctx->stream));
        }
    }
    std::sort(recs.begin(), recs.end(), [](const mi355_block_gain_stats& x, const mi355_block_gain_stats& y) {
        return x.pair != y.pair ? x.pair < y.pair : (x.cell_a != y.cell_a ? x.cell_a < y.cell_a : x.cell_b < y.cell_b);
    });
    if (cell_cover) {
        std::vector<unsigned long long> cov(n_cover);
        MI_HIP(hipMemcpyAsync(cov.data(), dcov.p, sizeof(unsigned long long) * n_cover, hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < n_cover; i++) cell_cover[i] = (int64_t)cov[i];
    } else MI_HIP(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}

int apply_block_gains(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws, int n, int gx, int gy,
                      const float* gains) {
    const std::string who = "apply_block_gains";
    std::string err;
    if (!d_src || !d_dst || !w || !h || !ws || !gains) { ctx->set_error(who + ": NULL argument"); return MI355_ERR_ARG; }
    if (!check_frames_n(n, err) || !check_grid(gx, gy, err)) { ctx->set_error(who + ": " + err); return MI355_ERR_ARG; }
    const int per = gx * gy * 3;
    { const int rc = check_apply_frames(ctx, who, d_src, d_dst, w, h, ws, n, gains, per); if (rc != MI355_OK) return rc; }
    for (int k = 0; k < n; k++)
        if (w[k] > BG_MAX_DIM || h[k] > BG_MAX_DIM) { ctx->set_error(who + ": frame " + std::to_string(k) + ": w=" + std::to_string(w[k]) + " h=" + std::to_string(h[k]) + " above 2^20"); return MI355_ERR_ARG; }
    std::vector<uint16_t> qs;                                          // the Q12 maps of the frames that get a record
    return launch_apply<BlockApplyFrame>(ctx, "block_gain_apply_frames", "block_gain_apply", d_src, d_dst, w, h, ws, n, gains, per,
        [&](BlockApplyFrame& f, const float* g) {
            f.q_off = (int)qs.size();
            for (int i = 0; i < per; i++) {
                double q = std::floor((double)g[i] * 4096.0 + 0.5);
                q = q < 0.0 ? 0.0 : (q > 32767.0 ? 32767.0 : q);
                qs.push_back((uint16_t)(int)q);
            }
        },
        [&](const BlockApplyFrame* d_af, int nf, int blocks) {
            DevBuf& dq = ctx->buf("block_gain_apply_q");
            hipError_t e = dq.reserve(sizeof(uint16_t) * qs.size());
            if (e == hipSuccess) e = hipMemcpyAsync(dq.p, qs.data(), sizeof(uint16_t) * qs.size(), hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess) hipLaunchKernelGGL(block_gain_apply_kernel, dim3(blocks), dim3(AP_NT), 0, ctx->stream, d_af, nf, dq.as<uint16_t>(), gx, gy);
            return e;
        });
}

}  // namespace

extern "C" int mi355_gain_stats_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                    const int32_t* pairs_ab, int n_pairs, int step, mi355_gain_pair_stats* pair_stats, int64_t* frame_cover) {
    LOCKED_PROLOGUE
    return gain_stats(ctx, d_imgs, w, h, ws, n, h9s, pairs_ab, n_pairs, step, pair_stats, frame_cover);
}

extern "C" int mi355_apply_gains_dev(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws, int n,
                                     const float* gains) {
    LOCKED_PROLOGUE
    return apply_gains(ctx, d_src, d_dst, w, h, ws, n, gains);
}

extern "C" int mi355_gain_compensate_dev(mi355_ctx* ctx, uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                         const int32_t* pairs_ab, int n_pairs, const mi355_gain_params* p, float* gains_out) {
    LOCKED_PROLOGUE
    mi355_gain_params dp;
    if (!p) { mi355_default_gain_params(&dp); p = &dp; }
    std::string err;
    if (!check_params(p->sigma_n, p->sigma_g, p->channels, &p->step, err)) { ctx->set_error("gain_compensate: " + err); return MI355_ERR_ARG; }
    if (!check_frames_n(n, err)) { ctx->set_error("gain_compensate: " + err); return MI355_ERR_ARG; }
    std::vector<mi355_gain_pair_stats> st((size_t)std::max(n_pairs, 1));
    std::vector<int64_t> cover((size_t)n);
    int rc = gain_stats(ctx, (const uint8_t* const*)d_imgs, w, h, ws, n, h9s, pairs_ab, n_pairs, p->step, st.data(), cover.data());
    if (rc != MI355_OK) return rc;
    std::vector<float> g((size_t)n * 3);
    rc = solve_gains(st.data(), n_pairs, cover.data(), n, *p, g.data(), err);
    if (rc != MI355_OK) { ctx->set_error("gain_compensate: " + err); return rc; }
    const NonUnit nu(d_imgs, w, h, ws, n, g.data(), 3);
    if (!nu.img.empty()) rc = apply_gains(ctx, nu.src(), nu.img.data(), nu.w.data(), nu.h.data(), nu.ws.data(), (int)nu.img.size(), nu.g.data());
    if (rc != MI355_OK) return rc;
    if (gains_out) std::copy(g.begin(), g.end(), gains_out);
    return MI355_OK;
}

extern "C" int mi355_block_gain_stats_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                          const int32_t* pairs_ab, int n_pairs, int step, int grid_x, int grid_y, mi355_block_gain_stats** records,
                                          int64_t* n_records, int64_t* cell_cover) {
    LOCKED_PROLOGUE
    if (!records || !n_records) { ctx->set_error("block_gain_stats: NULL argument or n_pairs < 0"); return MI355_ERR_ARG; }
    *records = nullptr; *n_records = 0;
    std::vector<mi355_block_gain_stats> recs;
    const int rc = block_gain_stats(ctx, d_imgs, w, h, ws, n, h9s, pairs_ab, n_pairs, step, grid_x, grid_y, recs, cell_cover);
    if (rc != MI355_OK || recs.empty()) return rc;
    mi355_block_gain_stats* out = (mi355_block_gain_stats*)malloc(sizeof(mi355_block_gain_stats) * recs.size());
    if (!out) { ctx->set_error("block_gain_stats: out of host memory"); return MI355_ERR_FAILED; }
    std::copy(recs.begin(), recs.end(), out);
    *records = out; *n_records = (int64_t)recs.size();
    return MI355_OK;
}

extern "C" int mi355_apply_block_gains_dev(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws, int n,
                                           int grid_x, int grid_y, const float* gains) {
    LOCKED_PROLOGUE
    return apply_block_gains(ctx, d_src, d_dst, w, h, ws, n, grid_x, grid_y, gains);
}

extern "C" int mi355_block_gain_compensate_dev(mi355_ctx* ctx, uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                               const int32_t* pairs_ab, int n_pairs, const mi355_block_gain_params* p, float* gains_out) {
    LOCKED_PROLOGUE
    mi355_block_gain_params dp;
    if (!p) { mi355_default_block_gain_params(&dp); p = &dp; }
    std::string err;
    if (!check_block_params(*p, true, err) || !check_frames_n(n, err)) { ctx->set_error("block_gain_compensate: " + err); return MI355_ERR_ARG; }
    const int per = p->grid_x * p->grid_y * 3;
    std::vector<mi355_block_gain_stats> recs;
    std::vector<int64_t> cover((size_t)n * (per / 3));
    int rc = block_gain_stats(ctx, (const uint8_t* const*)d_imgs, w, h, ws, n, h9s, pairs_ab, n_pairs, p->step, p->grid_x, p->grid_y, recs, cover.data());
    if (rc != MI355_OK) return rc;
    std::vector<float> g((size_t)n * per);
    rc = solve_block_gains(recs.data(), (int64_t)recs.size(), pairs_ab, n_pairs, cover.data(), n, *p, g.data(), err);
    if (rc != MI355_OK) { ctx->set_error("block_gain_compensate: " + err); return rc; }
    const NonUnit nu(d_imgs, w, h, ws, n, g.data(), per);
    if (!nu.img.empty()) rc = apply_block_gains(ctx, nu.src(), nu.img.data(), nu.w.data(), nu.h.data(), nu.ws.data(), (int)nu.img.size(), p->grid_x, p->grid_y, nu.g.data());
    if (rc != MI355_OK) return rc;
    if (gains_out) std::copy(g.begin(), g.end(), gains_out);
    return MI355_OK;
}
