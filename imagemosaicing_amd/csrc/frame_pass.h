// csrc/frame_pass.h -- the host path of a per-frame resampling pass over device BGR frames, shared by the lens undistortion (undistort.hip)
// and the local registration's apply (local_warp.hip): the argument and overlap checks of mi355_undistort_frames_dev, the frame table with
// its first_block prefix, one launch over frames of mixed sizes, in-place frames through a ctx scratch buffer in groups, the per-frame
// 64-bit counters.  The kernels stay in their own files; a pass hands its launch in as a callable.
#pragma once
#include "common.h"
#include <algorithm>

namespace {

constexpr int FP_NT = 256, FP_PX = 4, FP_ROWS = 8;      // lanes, adjacent pixels per lane, rows per lane
constexpr int FP_BW = FP_NT * FP_PX;                    // output columns of a workgroup
constexpr int FP_MAX_DIM = 1 << 20, FP_MAX_FRAMES = 65535;
constexpr size_t FP_SCRATCH_BYTES = (size_t)512 << 20;  // in-place frames per group: as many as this holds, at least one
constexpr int FP_MAX_BLOCKS = 1 << 30;                  // workgroups per launch

struct PassFrame { const uint8_t* src; uint8_t* dst; int w, h, ws_src, ws_dst; int first_block, bx_n, k, _pad; };
static_assert(sizeof(PassFrame) == 48, "frame pass record layout");

inline bool fp_check_size(int w, int h, std::string& err) {
    if (w < 2 || w > FP_MAX_DIM) { err = "w=" + std::to_string(w) + " outside [2, 2^20]"; return false; }
    if (h < 2 || h > FP_MAX_DIM) { err = "h=" + std::to_string(h) + " outside [2, 2^20]"; return false; }
    return true;
}

// One or more launches over a frame list (first_block, bx_n are filled in here; a launch takes at most FP_MAX_BLOCKS workgroups), complete
// on return: the list is the caller's local.  launch(table, nf, blocks, bytes) enqueues the pass's kernel on the ctx stream.
template <class Launch>
int fp_launch_frames(mi355_ctx* ctx, const std::string& prefix, std::vector<PassFrame>& fr, Launch&& launch) {
    DevBuf& dfr = ctx->buf(prefix + "_frames");
    for (size_t i0 = 0; i0 < fr.size();) {
        int blocks = 0;
        double bytes = 0.0;
        size_t i1 = i0;
        for (; i1 < fr.size(); i1++) {
            PassFrame& f = fr[i1];
            f.bx_n = (f.w + FP_BW - 1) / FP_BW;
            const int nb = f.bx_n * ((f.h + FP_ROWS - 1) / FP_ROWS);            // at most 2^10 * 2^17
            if (i1 > i0 && blocks > FP_MAX_BLOCKS - nb) break;
            f.first_block = blocks;
            blocks += nb;
            bytes += 6.0 * (double)f.w * f.h;
        }
        const size_t nf = i1 - i0;
        MI_HIP(dfr.reserve(sizeof(PassFrame) * nf));
        MI_HIP(hipMemcpyAsync(dfr.p, fr.data() + i0, sizeof(PassFrame) * nf, hipMemcpyHostToDevice, ctx->stream));
        launch(dfr.as<PassFrame>(), (int)nf, blocks, bytes);
        MI_HIP(hipGetLastError());
        MI_HIP(hipStreamSynchronize(ctx->stream));                  // the table is rewritten by the next launch
        i0 = i1;
    }
    return MI355_OK;
}

// The frames of a call through `launch`, after the checks (MI355_ERR_ARG before any launch; `who` ends in ": ").  prepare(d_counts) runs
// after the checks and before the first launch (the pass's own uploads); counts: HOST, n values, may be NULL.
template <class Prepare, class Launch>
int fp_run_frames(mi355_ctx* ctx, const std::string& who, const std::string& prefix, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h,
                  const int* ws_src, const int* ws_dst, int n, int64_t* counts, Prepare&& prepare, Launch&& launch) {
    std::string err;
    if (!d_src || !d_dst || !w || !h || !ws_src || !ws_dst) {
        ctx->set_error(who + (!d_src ? "d_src" : !d_dst ? "d_dst" : !w ? "w" : !h ? "h" : !ws_src ? "ws_src" : "ws_dst") + " is NULL");
        return MI355_ERR_ARG;
    }
    // a destination range may meet no other range of the call; a frame in place (same pointer, same pitch) is one range
    struct Span { uintptr_t lo, hi; int k; bool dst; };
    std::vector<Span> spans;
    std::vector<char> in_place((size_t)n, 0);
    for (int k = 0; k < n; k++) {
        const std::string fk = who + "frame " + std::to_string(k) + ": ";
        if (!d_src[k]) { ctx->set_error(fk + "d_src is NULL"); return MI355_ERR_ARG; }
        if (!d_dst[k]) { ctx->set_error(fk + "d_dst is NULL"); return MI355_ERR_ARG; }
        if (!fp_check_size(w[k], h[k], err)) { ctx->set_error(fk + err); return MI355_ERR_ARG; }
        if (ws_src[k] < 3 * w[k]) { ctx->set_error(fk + "ws_src=" + std::to_string(ws_src[k]) + " < 3 w=" + std::to_string(3 * w[k])); return MI355_ERR_ARG; }
        if (ws_dst[k] < 3 * w[k]) { ctx->set_error(fk + "ws_dst=" + std::to_string(ws_dst[k]) + " < 3 w=" + std::to_string(3 * w[k])); return MI355_ERR_ARG; }
        in_place[k] = d_dst[k] == d_src[k] && ws_dst[k] == ws_src[k];
        const size_t sb = (size_t)ws_src[k] * (size_t)(h[k] - 1) + 3 * (size_t)w[k], db = (size_t)ws_dst[k] * (size_t)(h[k] - 1) + 3 * (size_t)w[k];
        if (!in_place[k]) spans.push_back({(uintptr_t)d_src[k], (uintptr_t)d_src[k] + sb, k, false});
        spans.push_back({(uintptr_t)d_dst[k], (uintptr_t)d_dst[k] + db, k, true});
    }
    std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
    {
        uintptr_t hi_dst = 0, hi_src = 0;                           // the furthest end of the destination / source ranges that start earlier
        int k_dst = -1, k_src = -1;
        for (const Span& s : spans) {
            if (hi_dst > s.lo) {
                ctx->set_error(who + "d_dst of frame " + std::to_string(k_dst) + " overlaps " + (s.dst ? "d_dst" : "d_src") + " of frame " + std::to_string(s.k));
                return MI355_ERR_ARG;
            }
            if (s.dst && hi_src > s.lo) {
                ctx->set_error(who + "d_dst of frame " + std::to_string(s.k) + " overlaps d_src of frame " + std::to_string(k_src) + " without being in place");
                return MI355_ERR_ARG;
            }
            if (s.dst) { if (s.hi > hi_dst) { hi_dst = s.hi; k_dst = s.k; } }
            else if (s.hi > hi_src) { hi_src = s.hi; k_src = s.k; }
        }
    }
    DevBuf& dout = ctx->buf(prefix + "_outside");
    MI_HIP(dout.reserve(sizeof(unsigned long long) * (size_t)n));
    MI_HIP(hipMemsetAsync(dout.p, 0, sizeof(unsigned long long) * (size_t)n, ctx->stream));
    { const int rc = prepare(); if (rc != MI355_OK) return rc; }
    auto record = [&](int k, uint8_t* dst, int dst_pitch) {
        PassFrame f;
        f.src = d_src[k]; f.dst = dst; f.w = w[k]; f.h = h[k]; f.ws_src = ws_src[k]; f.ws_dst = dst_pitch; f.first_block = 0; f.bx_n = 0; f.k = k; f._pad = 0;
        return f;
    };
    std::vector<PassFrame> fr;
    for (int k = 0; k < n; k++)
        if (!in_place[k]) fr.push_back(record(k, d_dst[k], ws_dst[k]));
    if (!fr.empty()) { const int rc = fp_launch_frames(ctx, prefix, fr, launch); if (rc != MI355_OK) return rc; }
    // in place: through the scratch buffer (rows of 3w bytes rounded up to 4, frames 256 bytes apart), group by group
    auto scratch_bytes = [&](int k) { return ((((size_t)3 * w[k] + 3) & ~(size_t)3) * (size_t)h[k] + 255) & ~(size_t)255; };
    for (int k0 = 0; k0 < n;) {
        if (!in_place[k0]) { k0++; continue; }
        size_t total = 0;
        int k1 = k0;
        fr.clear();
        std::vector<size_t> off;
        for (; k1 < n; k1++) {
            if (!in_place[k1]) continue;
            const size_t sb = scratch_bytes(k1);
            if (!fr.empty() && total + sb > FP_SCRATCH_BYTES) break;
            off.push_back(total);
            fr.push_back(record(k1, nullptr, (3 * w[k1] + 3) & ~3));
            total += sb;
        }
        DevBuf& ds = ctx->buf(prefix + "_scratch");
        MI_HIP(ds.reserve(total));
        for (size_t i = 0; i < fr.size(); i++) fr[i].dst = ds.as<uint8_t>() + off[i];
        { const int rc = fp_launch_frames(ctx, prefix, fr, launch); if (rc != MI355_OK) return rc; }
        for (const PassFrame& f : fr)
            MI_HIP(hipMemcpy2DAsync(d_dst[f.k], (size_t)ws_dst[f.k], f.dst, (size_t)f.ws_dst, 3 * (size_t)f.w, (size_t)f.h, hipMemcpyDeviceToDevice, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));                  // the scratch is refilled by the next group
        k0 = k1;
    }
    if (counts) {
        std::vector<unsigned long long> cnt((size_t)n);
        MI_HIP(hipMemcpyAsync(cnt.data(), dout.p, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));
        for (int k = 0; k < n; k++) counts[k] = (int64_t)cnt[k];
    }
    return MI355_OK;
}

}  // namespace
