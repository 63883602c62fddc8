// csrc/cover.hip -- cover depth (gfx950): how many kept frames cover each point of the canvas lattice, and per frame how many of its points lie
// at each depth (include/mi355_mosaic.h, "cover depth"; mosaic_frame.h).  Geometry only: no image pointer is taken and no texel is loaded.
//
//   cover_depth_kernel   the hot path.  Every lattice point needs ALL kept frames at that point, so the work is cut by canvas area: the
//                        renders' candidate lists (mi_frame_table_upload: per 256 x 256 canvas block the kept frames whose box meets it) and,
//                        inside each list block, tiles of 64 x 16 lattice points, so that a tile's points never straddle two lists whatever the
//                        step.  One lane per lattice column, 4 lattice rows per lane.  Pass 1 walks the block's list (uniform over the
//                        workgroup: scalar loads) and counts the depth d of the lane's 4 points with frame_src / src_inside on the integer
//                        pixel inside the frame's clipped box; where the list has at most 64 entries it keeps the cover bits in a register
//                        pair per point.  Pass 2 credits each point to the frames that cover it, from the bits or, for longer lists, by
//                        evaluating the map again, in chunks of CV_CHUNK list entries with one 32-bit LDS counter per (entry, depth bucket): a
//                        wave adds the popcount of a ballot per distinct bucket among its lanes, never one add per point.  After a chunk the
//                        nonzero counters land with one 64-bit vector atomic per (frame, bucket, workgroup) in the device record array, the
//                        depth histogram with one per bin: integer sums, so the result does not depend on the order the workgroups run in.
// The parameter checks and the selection loop are host-only: cover_select.cpp (cover.h).  This file gives that loop the survey's boxes
// (frame_boxes) and, in mi355_cover_select_dev, the kernel as its statistics function.
#include "common.h"
#include "cover.h"
#include "gain.h"
#include "hmath.h"
#include "mosaic_frame.h"
#include <algorithm>
#include <cstddef>

namespace {

using namespace mi_cover;

constexpr int CV_X = 64, CV_Y = 16;            // lattice columns x rows of a tile (256 lanes: 64 x 4, 4 rows each)
constexpr int CV_CHUNK = 64;                   // list entries that share one set of LDS counters in pass 2

// counters[b] += the number of lanes of this wave with ok and bucket b, one LDS add per distinct bucket among them.  Every lane of the wave
// must call it (ballots); b is read only where ok.
__device__ __forceinline__ void tally(bool ok, int b, unsigned* counters) {
    unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
    while (m) {                                                  // uniform: m is a ballot
        const int b0 = __builtin_amdgcn_readlane(b, __builtin_ctzll(m));
        const unsigned long long mb = __builtin_amdgcn_ballot_w64(ok && b == b0);
        if ((threadIdx.x & 63) == 0) atomicAdd(&counters[b0], (unsigned)__builtin_popcountll(mb));
        m &= ~mb;
    }
}

// frame f covers the lane's point in lattice row r: the pixel inside the clipped box and the render's map of it inside the frame
__device__ __forceinline__ bool covers(const FrameDev& f, float w1, float h1, bool xin, int y, float xf, float dGy) {
    float xs, ys;
    frame_src(f, xf, (float)y - dGy, xs, ys);
    return xin && y >= f.begY && y <= f.endY && src_inside(xs, ys, w1, h1);
}

// Tile t of the launch: list block t / (sub_x sub_y), inside it tile (sx, sy) of the block's lattice points.  frame_acc: 8 accumulators per
// caller frame (frame_of maps a table entry to it), hist_acc: MI355_COVER_BINS.
__global__ __launch_bounds__(256) void cover_depth_kernel(const FrameDev* fr, const int* frame_of, const uint16_t* lists, const int* counts, int nf, int bx_n,
                                                          int sub_x, int sub_y, long long tile0, int step, int cw, int ch, float dGx, float dGy,
                                                          unsigned long long* frame_acc, unsigned long long* hist_acc) {
    __shared__ unsigned s_cnt[CV_CHUNK][8];                      // a workgroup holds 1024 points: every counter stays below 2^11
    __shared__ unsigned s_hist[MI355_COVER_BINS];                // likewise
    const int tid = threadIdx.x;
    const long long t = tile0 + blockIdx.x;
    const int per_block = sub_x * sub_y;
    const int cb = (int)(t / per_block), sub = (int)(t - (long long)cb * per_block);
    const int by = cb / bx_n, bx = cb - by * bx_n;
    const int sy = sub / sub_x, sx = sub - sy * sub_x;
    // the block's lattice points, then the tile's
    const int px0 = bx * MOSAIC_LIST_BLOCK, py0 = by * MOSAIC_LIST_BLOCK;
    const int px1 = min(px0 + MOSAIC_LIST_BLOCK - 1, cw - 1), py1 = min(py0 + MOSAIC_LIST_BLOCK - 1, ch - 1);
    const int lx0 = (px0 + step - 1) / step + CV_X * sx, ly0 = (py0 + step - 1) / step + CV_Y * sy;
    const int lxb1 = px1 / step, lyb1 = py1 / step;
    if (lx0 > lxb1 || ly0 > lyb1) return;                        // uniform over the workgroup, before any barrier
    const int lx1 = min(lx0 + CV_X - 1, lxb1), ly1 = min(ly0 + CV_Y - 1, lyb1);
    const int tx0 = lx0 * step, tx1 = lx1 * step, ty0 = ly0 * step, ty1 = ly1 * step;
    const int lx = lx0 + (tid & 63), lyB = ly0 + (tid >> 6);
    const int x = lx * step;
    const bool col = lx <= lx1;
    const float xf = (float)x - dGx;                             // the render's xf = (float)xD - dGx
    const int cnt = counts[cb];
    const uint16_t* list = lists + (size_t)cb * nf;
    const bool small = cnt <= 64;
    if (tid < MI355_COVER_BINS) s_hist[tid] = 0u;
    int d[4] = {0, 0, 0, 0};
    unsigned long long bits[4] = {0ull, 0ull, 0ull, 0ull};
    for (int e = 0; e < cnt; e++) {
        const FrameDev& f = fr[list[e]];                         // uniform over the workgroup: scalar loads
        if (f.begX > tx1 || f.endX < tx0 || f.begY > ty1 || f.endY < ty0) continue;
        const float w1 = (float)(f.w - 1), h1 = (float)(f.h - 1);
        const bool xin = col && x >= f.begX && x <= f.endX;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int ly = lyB + 4 * r;
            const bool ok = ly <= ly1 && covers(f, w1, h1, xin, ly * step, xf, dGy);
            d[r] += ok ? 1 : 0;
            if (small) bits[r] |= (unsigned long long)(ok ? 1 : 0) << e;
        }
    }
    __syncthreads();                                             // s_hist is zero
#pragma unroll
    for (int r = 0; r < 4; r++) tally(col && lyB + 4 * r <= ly1, min(d[r], 8), s_hist);
    for (int e0 = 0; e0 < cnt; e0 += CV_CHUNK) {
        const int e1 = min(cnt, e0 + CV_CHUNK);
        for (int i = tid; i < CV_CHUNK * 8; i += 256) s_cnt[i >> 3][i & 7] = 0u;
        __syncthreads();
        for (int e = e0; e < e1; e++) {
            const FrameDev& f = fr[list[e]];
            if (f.begX > tx1 || f.endX < tx0 || f.begY > ty1 || f.endY < ty0) continue;
            const float w1 = (float)(f.w - 1), h1 = (float)(f.h - 1);
            const bool xin = col && x >= f.begX && x <= f.endX;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int ly = lyB + 4 * r;
                const bool ok = small ? ((bits[r] >> e) & 1ull) != 0 : (ly <= ly1 && covers(f, w1, h1, xin, ly * step, xf, dGy));
                tally(ok, min(d[r], 8) - 1, s_cnt[e - e0]);      // ok: this frame covers the point, so d >= 1
            }
        }
        __syncthreads();
        for (int i = tid; i < (e1 - e0) * 8; i += 256) {
            const unsigned v = s_cnt[i >> 3][i & 7];
            if (v != 0u) atomicAdd(frame_acc + 8 * (size_t)frame_of[list[e0 + (i >> 3)]] + (i & 7), (unsigned long long)v);
        }
        __syncthreads();                                         // before the next chunk zeroes the counters
    }
    __syncthreads();
    if (tid < MI355_COVER_BINS && s_hist[tid] != 0u) atomicAdd(hist_acc + tid, (unsigned long long)s_hist[tid]);
}

// What the launcher keeps between the rounds of a selection: the layout for h9s as passed and every frame's FrameDev (src stays NULL).
struct CoverFrames {
    int n = 0, cw = 0, ch = 0;
    float dG[2] = {0.0f, 0.0f};
    std::vector<FrameDev> fr;
    std::vector<char> part;
};

// n is checked by the caller
int cover_frames(const int* w, const int* h, int n, const float* h9s, CoverFrames& s, std::string& err) {
    int cws;
    if (mi355_mosaic_layout(w, h, n, h9s, &s.cw, &s.ch, &cws, s.dG) != MI355_OK) { err = "no image with h[8] != 0 / empty canvas"; return MI355_ERR_FAILED; }
    s.n = n;
    s.fr.assign((size_t)n, FrameDev());
    s.part.assign((size_t)n, 0);
    for (int k = 0; k < n; k++) {
        if (!mi_frame_dev_setup(h9s + 9 * k, w[k], h[k], s.dG, s.cw, s.ch, 0, s.ch, s.fr[k])) continue;
        if (w[k] < 2 || h[k] < 2) { err = "frame " + std::to_string(k) + ": bad geometry w=" + std::to_string(w[k]) + " h=" + std::to_string(h[k]); return MI355_ERR_ARG; }
        s.fr[k].w = w[k]; s.fr[k].h = h[k];
        s.part[k] = 1;
    }
    return MI355_OK;
}

// one launch (more only past 2^30 tiles) under keep; complete on return
int cover_launch(mi355_ctx* ctx, const CoverFrames& s, const uint8_t* keep, int step, mi355_cover_frame_stats* frame_stats, int64_t* hist) {
    const int n = s.n;
    FrameTable t;
    for (int k = 0; k < n; k++)
        if (s.part[k] && (!keep || keep[k])) t.add(s.fr[k], k);
    { const int rc = mi_frame_table_upload(ctx, t, false, true, s.cw, s.ch, 0); if (rc != MI355_OK) return rc; }
    const size_t n_acc = (size_t)n * 8 + MI355_COVER_BINS;
    DevBuf& dacc = ctx->buf("cover_acc");
    MI_HIP(dacc.reserve(sizeof(unsigned long long) * n_acc));
    MI_HIP(hipMemsetAsync(dacc.p, 0, sizeof(unsigned long long) * n_acc, ctx->stream));
    unsigned long long* frame_acc = dacc.as<unsigned long long>();
    unsigned long long* hist_acc = frame_acc + (size_t)n * 8;
    const int per_axis = (MOSAIC_LIST_BLOCK + step - 1) / step;   // the most lattice points a list block holds along an axis
    const int sub_x = (per_axis + CV_X - 1) / CV_X, sub_y = (per_axis + CV_Y - 1) / CV_Y;
    const int by_n = (s.ch + MOSAIC_LIST_BLOCK - 1) / MOSAIC_LIST_BLOCK;
    const size_t tiles = (size_t)t.bx_n * by_n * sub_x * sub_y;
    for (size_t t0 = 0; t0 < tiles; t0 += (size_t)1 << 30) {       // grid.x < 2^31
        const size_t nt = std::min(tiles - t0, (size_t)1 << 30);
        ProfScope ps(ctx, "cover_depth", 0.0);
        hipLaunchKernelGGL(cover_depth_kernel, dim3((unsigned)nt), dim3(256), 0, ctx->stream, t.d_fr, t.d_frame_of, t.d_lists, t.d_counts, t.nf, t.bx_n, sub_x,
                           sub_y, (long long)t0, step, s.cw, s.ch, s.dG[0], s.dG[1], frame_acc, hist_acc);
        MI_HIP(hipGetLastError());
    }
    std::vector<unsigned long long> acc(n_acc);
    MI_HIP(hipMemcpyAsync(acc.data(), dacc.p, sizeof(unsigned long long) * n_acc, hipMemcpyDeviceToHost, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));                 // the table's host vectors are locals
    if (frame_stats)
        for (int k = 0; k < n; k++)
            for (int j = 0; j < 8; j++) frame_stats[k].at_depth[j] = (int64_t)acc[8 * (size_t)k + j];
    if (hist)
        for (int j = 0; j < MI355_COVER_BINS; j++) hist[j] = (int64_t)acc[(size_t)n * 8 + j];
    return MI355_OK;
}

int cover_setup(mi355_ctx* ctx, const char* who, const int* w, const int* h, int n, const float* h9s, CoverFrames& s) {
    std::string err;
    if (!w || !h || !h9s) { ctx->set_error(std::string(who) + "NULL argument or a count < 0"); return MI355_ERR_ARG; }
    if (!mi_gain::check_frames_n(n, err)) { ctx->set_error(who + err); return MI355_ERR_ARG; }
    const int rc = cover_frames(w, h, n, h9s, s, err);
    if (rc != MI355_OK) ctx->set_error(who + err);
    return rc;
}

}  // namespace

int mi_cover::frame_boxes(const int* w, const int* h, int n, const float* h9s, Box* box, char* part, std::string& err) {
    CoverFrames s;
    const int rc = cover_frames(w, h, n, h9s, s, err);
    if (rc != MI355_OK) return rc;
    for (int k = 0; k < n; k++) {
        part[k] = s.part[k];
        box[k] = Box{s.fr[k].begX, s.fr[k].endX, s.fr[k].begY, s.fr[k].endY};
    }
    return MI355_OK;
}

extern "C" int mi355_cover_stats_dev(mi355_ctx* ctx, const int* w, const int* h, int n, const float* h9s, const uint8_t* keep, int step,
                                     mi355_cover_frame_stats* frame_stats, int64_t* hist) {
    LOCKED_PROLOGUE
    if (step < 1 || step > 64) { ctx->set_error("cover_stats: step=" + std::to_string(step) + " outside [1, 64]"); return MI355_ERR_ARG; }
    CoverFrames s;
    { const int rc = cover_setup(ctx, "cover_stats: ", w, h, n, h9s, s); if (rc != MI355_OK) return rc; }
    return cover_launch(ctx, s, keep, step, frame_stats, hist);
}

extern "C" int mi355_cover_select_dev(mi355_ctx* ctx, const int* w, const int* h, int n, const float* h9s, const uint8_t* keep, const int32_t* order,
                                      int n_order, const int32_t* pairs_ab, int n_pairs, const mi355_cover_params* p, uint8_t* status, uint8_t* keep_out,
                                      int32_t* rounds, int64_t* lost, mi355_cover_frame_stats* frame_stats, int64_t* hist) {
    LOCKED_PROLOGUE
    mi355_cover_params dp;
    if (!p) { mi355_default_cover_params(&dp); p = &dp; }
    std::string err;
    if (!check_cover_params(*p, err)) { ctx->set_error("cover_select: " + err); return MI355_ERR_ARG; }
    CoverFrames s;
    { const int rc = cover_setup(ctx, "cover_select: ", w, h, n, h9s, s); if (rc != MI355_OK) return rc; }
    std::vector<Box> box((size_t)n);
    for (int k = 0; k < n; k++) box[k] = Box{s.fr[k].begX, s.fr[k].endX, s.fr[k].begY, s.fr[k].endY};
    bool launch_failed = false;                                  // then the message is the launcher's own
    const int rc = select(n, box.data(), s.part.data(), keep, order, n_order, pairs_ab, n_pairs, *p,
                          [&](const uint8_t* kp, mi355_cover_frame_stats* fs, std::string&) {
                              const int r = cover_launch(ctx, s, kp, p->step, fs, nullptr);
                              launch_failed = r != MI355_OK;
                              return r;
                          },
                          status, keep_out, rounds, lost, err);
    if (rc != MI355_OK) { if (!launch_failed) ctx->set_error("cover_select: " + err); return rc; }
    if (frame_stats || hist) return cover_launch(ctx, s, keep_out, p->step, frame_stats, hist);
    return MI355_OK;
}
