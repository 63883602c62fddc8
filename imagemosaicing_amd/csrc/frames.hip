// csrc/frames.hip -- where the renders' inputs come from and how their canvas reaches the caller.  Host code only: the canvases come from the
// kernels of warp.hip / feather.hip / seamline.hip / median.hip / blend.hip.  Host frames kept in HBM after their extraction (option "keep_frames");
// render_sources, the staging every form shares; the host forms of the one-pass renders (mi_render_host_begin / _end: a malloc'd canvas) and the calls
// that write straight into caller memory (render_into: mi355_mosaic_refined_into / _feathered_into / _seamline_into / _median_into / _blended_into).
// Last, mi355_mosaic_preview_into: the same sources, rendered stripe by stripe and reduced by overview.hip, one overview level reaching the
// caller.
#include "common.h"
#include "mosaic_frame.h"
#include <thread>

// ---- kept frames ------------------------------------------------------------------------------------------------------
// The kept buffer of img_id made ready to take a new frame of this geometry.  A SIFT batch may still read the old frame (it was parked
// with the kept frame's event, which the batch records when it finishes): a batch still collecting frames is launched first, then the ctx
// stream waits for the event before the caller uploads into the same buffer -- or, when the buffer must grow, the host waits before the
// old one is freed.  Renders and _dev calls that read the frame run on the ctx stream, so the upload is ordered after them too.
int mi_kept_frame_slot(mi355_ctx* ctx, int img_id, int w, int h, int ws, const char* who, uint8_t** d_frame) {
    KeptFrame& f = ctx->kept_frames[img_id];
    const size_t bytes = (size_t)ws * h + 16;
    if (!f.ev) {
        MI_HIP(hipEventCreateWithFlags(&f.ev, hipEventDisableTiming));
    } else {
        int rc = mi_sift_flush_if_parked(ctx, f.ev);
        if (rc != MI355_OK) return rc;
        if (bytes > f.cap && f.p) {
            MI_HIP(hipEventSynchronize(f.ev));
            MI_HIP(hipStreamSynchronize(ctx->stream));
        } else {
            MI_HIP(hipStreamWaitEvent(ctx->stream, f.ev, 0));
        }
    }
    if (bytes > f.cap) {
        if (f.p) { MI_HIP(hipFree(f.p)); f.p = nullptr; f.cap = 0; }
        const hipError_t e = hipMalloc(&f.p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)hipEventDestroy(f.ev);
            ctx->kept_frames.erase(img_id);
            ctx->set_error(std::string(who) + ": no device memory to keep the frame of image " + std::to_string(img_id) + " (" +
                           std::to_string(bytes) + " bytes, option keep_frames): " + hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? MI355_ERR_NOMEM : MI355_ERR_DEVICE;
        }
        f.cap = bytes;
    }
    f.w = w; f.h = h; f.ws = ws;
    *d_frame = (uint8_t*)f.p;
    return MI355_OK;
}

// every reader of the frame done: a batch still collecting it is launched and waited for, and the ctx stream is drained
static int kept_frame_idle(mi355_ctx* ctx, KeptFrame& f) {
    if (!f.ev) return MI355_OK;
    int rc = mi_sift_flush_if_parked(ctx, f.ev);
    if (rc != MI355_OK) return rc;
    MI_HIP(hipEventSynchronize(f.ev));
    MI_HIP(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}

static void kept_frame_free(KeptFrame& f) {
    if (f.p) (void)hipFree(f.p);
    if (f.ev) (void)hipEventDestroy(f.ev);
    f = KeptFrame();
}

// mi355_destroy (the streams are idle by then)
void mi_frames_release(mi355_ctx* ctx) {
    for (auto& kv : ctx->kept_frames) { if (kv.second.ev) (void)hipEventSynchronize(kv.second.ev); kept_frame_free(kv.second); }
    ctx->kept_frames.clear();
    for (int i = 0; i < 2; i++) ctx->hbuf(i ? "download_1" : "download_0").release();
    for (hipEvent_t& e : ctx->dl_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    if (ctx->dl_stream) { (void)hipStreamDestroy(ctx->dl_stream); ctx->dl_stream = nullptr; }
}

extern "C" int mi355_drop_frames(mi355_ctx* ctx, int img_id) {
    LOCKED_PROLOGUE
    if (img_id >= 0) {
        auto it = ctx->kept_frames.find(img_id);
        if (it == ctx->kept_frames.end()) return MI355_OK;
        const int rc = kept_frame_idle(ctx, it->second);
        if (rc != MI355_OK) return rc;
        kept_frame_free(it->second);
        ctx->kept_frames.erase(it);
        return MI355_OK;
    }
    for (auto& kv : ctx->kept_frames) { const int rc = kept_frame_idle(ctx, kv.second); if (rc != MI355_OK) return rc; }
    for (auto& kv : ctx->kept_frames) kept_frame_free(kv.second);
    ctx->kept_frames.clear();
    return MI355_OK;
}

extern "C" int mi355_get_frame_dev(mi355_ctx* ctx, int img_id, const uint8_t** d_frame, int* w, int* h, int* ws) {
    LOCKED_PROLOGUE
    if (!d_frame) { ctx->set_error("get_frame_dev: d_frame is NULL"); return MI355_ERR_ARG; }
    *d_frame = nullptr;
    auto it = ctx->kept_frames.find(img_id);
    if (img_id < 0 || it == ctx->kept_frames.end()) {
        ctx->set_error("get_frame_dev: image " + std::to_string(img_id) + " holds no kept frame" + (ctx->keep_frames ? "" : " (option keep_frames is 0)"));
        return MI355_ERR_ARG;
    }
    MI_HIP(hipStreamSynchronize(ctx->stream));     // the upload is complete: the pointer may be read on any stream
    *d_frame = (const uint8_t*)it->second.p;
    if (w) *w = it->second.w;
    if (h) *h = it->second.h;
    if (ws) *ws = it->second.ws;
    return MI355_OK;
}

// ---- the render calls' sources --------------------------------------------------------------------------------------------
// n <= 1 and the layout of the one-pass renders' host-image forms (MergeImagesRefined's convention, MosaicWithoutPos.cpp:2164-2167)
static int render_layout(mi355_ctx* ctx, const char* who, const int* w, const int* h, int n, const float* h9s, int* lw, int* lh, int* lws) {
    if (n <= 1) { ctx->set_error(std::string(who) + ": needs more than one image"); return MI355_ERR_FAILED; }
    const int rc = mi355_mosaic_layout(w, h, n, h9s, lw, lh, lws, nullptr);
    if (rc != MI355_OK) ctx->set_error(std::string(who) + ": empty canvas");
    return rc;
}

// Device pointers of the images a render reads: kept frames where img_ids (may be NULL) names one, the host images staged in the ctx buffer
// `staging` otherwise.  Images the render skips (h9[8] == 0, or keep[k] == 0 where keep is given) are neither read nor checked.
static int render_sources(mi355_ctx* ctx, const char* who, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h,
                          const int* ws, int n, const float* h9s, const uint8_t* keep, const char* staging, std::vector<const uint8_t*>& dptr) {
    std::vector<char> skip((size_t)n);
    for (int k = 0; k < n; k++) skip[k] = (keep && !keep[k]) || h9s[9 * k + 8] == 0.0f;
    dptr.assign((size_t)n, nullptr);
    std::vector<size_t> off((size_t)n, 0);
    size_t total = 0;
    for (int k = 0; k < n; k++) {
        if (skip[k]) continue;
        if (img_ids && img_ids[k] >= 0) {
            auto it = ctx->kept_frames.find(img_ids[k]);
            if (it == ctx->kept_frames.end()) {
                ctx->set_error(std::string(who) + ": image " + std::to_string(k) + ": id " + std::to_string(img_ids[k]) + " holds no kept frame");
                return MI355_ERR_ARG;
            }
            const KeptFrame& f = it->second;
            if (f.w != w[k] || f.h != h[k] || f.ws != ws[k]) {
                ctx->set_error(std::string(who) + ": image " + std::to_string(k) + ": the kept frame of id " + std::to_string(img_ids[k]) + " is " +
                               std::to_string(f.w) + "x" + std::to_string(f.h) + " (width_step " + std::to_string(f.ws) + "), the call says " +
                               std::to_string(w[k]) + "x" + std::to_string(h[k]) + " (width_step " + std::to_string(ws[k]) + ")");
                return MI355_ERR_ARG;
            }
            dptr[k] = (const uint8_t*)f.p;
            continue;
        }
        if (!imgs || !imgs[k] || w[k] < 2 || h[k] < 2 || ws[k] < 3 * w[k]) {
            ctx->set_error(std::string(who) + ": image " + std::to_string(k) + ": no host image or bad geometry");
            return MI355_ERR_ARG;
        }
        off[k] = total;
        total += ((size_t)ws[k] * h[k] + 255) & ~(size_t)255;
    }
    if (total == 0) return MI355_OK;
    DevBuf& dall = ctx->buf(staging);
    MI_HIP(dall.reserve(total + 16));
    for (int k = 0; k < n; k++) {
        if (skip[k] || dptr[k]) continue;
        dptr[k] = dall.as<uint8_t>() + off[k];
        MI_HIP(hipMemcpyAsync((void*)dptr[k], imgs[k], (size_t)ws[k] * h[k], hipMemcpyHostToDevice, ctx->stream));
    }
    return MI355_OK;
}

// The same sources for a caller that reads frames without rendering them (tie_refine.hip): image k is wanted iff need[k] != 0.
int mi_frame_sources(mi355_ctx* ctx, const char* who, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h, const int* ws,
                     int n, const uint8_t* need, const char* staging, std::vector<const uint8_t*>& dptr) {
    const std::vector<float> h9s((size_t)9 * (size_t)n, 1.0f);
    return render_sources(ctx, who, imgs, img_ids, w, h, ws, n, h9s.data(), need, staging, dptr);
}

// ---- canvas download ------------------------------------------------------------------------------------------------------
// rows of row_bytes from the device canvas (pitch src_pitch) into the caller's host rows (pitch dst_pitch); the bytes past row_bytes of
// every destination row are left as they are.  Default: chunks of whole rows go device -> pinned on the copy stream into two halves in
// turn, and the host copies chunk k out of one half while chunk k + 1 lands in the other.
static void copy_rows(uint8_t* dst, size_t dst_pitch, const uint8_t* src, size_t src_pitch, size_t row_bytes, int rows, int threads) {
    auto part = [&](int r0, int r1) { for (int r = r0; r < r1; r++) memcpy(dst + (size_t)r * dst_pitch, src + (size_t)r * src_pitch, row_bytes); };
    if (threads <= 1 || (size_t)rows * row_bytes < ((size_t)4 << 20)) { part(0, rows); return; }
    if (threads > rows) threads = rows;
    std::vector<std::thread> th;
    for (int t = 1; t < threads; t++) th.emplace_back(part, (int)((long)rows * t / threads), (int)((long)rows * (t + 1) / threads));
    part(0, (int)((long)rows / threads));
    for (auto& x : th) x.join();
}

static int download_rows(mi355_ctx* ctx, const uint8_t* d_src, size_t src_pitch, uint8_t* dst, size_t dst_pitch, size_t row_bytes, int rows) {
    if (!ctx->dl_stream) MI_HIP(hipStreamCreateWithFlags(&ctx->dl_stream, hipStreamNonBlocking));
    for (hipEvent_t& e : ctx->dl_ev) if (!e) MI_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    MI_HIP(hipEventRecord(ctx->dl_ev[2], ctx->stream));
    MI_HIP(hipStreamWaitEvent(ctx->dl_stream, ctx->dl_ev[2], 0));
    if (ctx->download_mode == 1 || ctx->download_mode == 2) {
        const bool reg = ctx->download_mode == 2;
        if (reg) MI_HIP(hipHostRegister(dst, dst_pitch * (size_t)(rows - 1) + row_bytes, hipHostRegisterDefault));
        hipError_t e = hipMemcpy2DAsync(dst, dst_pitch, d_src, src_pitch, row_bytes, (size_t)rows, hipMemcpyDeviceToHost, ctx->dl_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->dl_stream);
        if (reg) (void)hipHostUnregister(dst);
        if (e != hipSuccess) { ctx->set_error(std::string("download: ") + hipGetErrorString(e)); return MI355_ERR_DEVICE; }
        return MI355_OK;
    }
    int chunk_rows = (int)(ctx->download_chunk / src_pitch);
    if (chunk_rows < 1) chunk_rows = 1;
    if (chunk_rows > rows) chunk_rows = rows;
    HostBuf* pb[2] = {&ctx->hbuf("download_0"), &ctx->hbuf("download_1")};
    const int nchunks = (rows + chunk_rows - 1) / chunk_rows;
    for (int i = 0; i < (nchunks > 1 ? 2 : 1); i++) MI_HIP(pb[i]->reserve((size_t)chunk_rows * src_pitch));
    auto issue = [&](int c) -> hipError_t {
        const int r0 = c * chunk_rows, nr = rows - r0 < chunk_rows ? rows - r0 : chunk_rows;
        hipError_t e = hipMemcpyAsync(pb[c & 1]->p, d_src + (size_t)r0 * src_pitch, (size_t)nr * src_pitch, hipMemcpyDeviceToHost, ctx->dl_stream);
        return e == hipSuccess ? hipEventRecord(ctx->dl_ev[c & 1], ctx->dl_stream) : e;
    };
    MI_HIP(issue(0));
    if (nchunks > 1) MI_HIP(issue(1));
    for (int c = 0; c < nchunks; c++) {
        MI_HIP(hipEventSynchronize(ctx->dl_ev[c & 1]));
        const int r0 = c * chunk_rows, nr = rows - r0 < chunk_rows ? rows - r0 : chunk_rows;
        copy_rows(dst + (size_t)r0 * dst_pitch, dst_pitch, pb[c & 1]->as<uint8_t>(), src_pitch, row_bytes, nr, ctx->download_threads);
        if (c + 2 < nchunks) MI_HIP(issue(c + 2));
    }
    return MI355_OK;
}

static int check_dst(mi355_ctx* ctx, const char* who, const uint8_t* dst, int dst_pitch, int cw, int ch, int lw, int lh) {
    if (cw != lw || ch != lh) {
        ctx->set_error(std::string(who) + ": cw x ch = " + std::to_string(cw) + "x" + std::to_string(ch) + ", the layout is " + std::to_string(lw) + "x" + std::to_string(lh));
        return MI355_ERR_ARG;
    }
    if (!dst) { ctx->set_error(std::string(who) + ": dst is NULL"); return MI355_ERR_ARG; }
    if ((long)dst_pitch < 3L * cw) { ctx->set_error(std::string(who) + ": dst_pitch " + std::to_string(dst_pitch) + " < 3 * cw = " + std::to_string(3L * cw)); return MI355_ERR_ARG; }
    return MI355_OK;
}

// ---- the host forms: host images in, a malloc'd canvas out ---------------------------------------------------------------------
int mi_render_host_begin(mi355_ctx* ctx, const char* who, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                         int* lw, int* lh, int* lws, std::vector<const uint8_t*>& d_imgs, uint8_t** d_canvas) {
    int rc = render_layout(ctx, who, w, h, n, h9s, lw, lh, lws);
    if (rc != MI355_OK) return rc;
    rc = render_sources(ctx, who, imgs, nullptr, w, h, ws, n, h9s, nullptr, "mosaic_srcs", d_imgs);     // every contributing image staged in HBM (frames stay resident: 288 GB)
    if (rc != MI355_OK) return rc;
    DevBuf& dcan = ctx->buf("mosaic_canvas");
    MI_HIP(dcan.reserve((size_t)*lws * *lh));
    *d_canvas = dcan.as<uint8_t>();
    return MI355_OK;
}

int mi_render_host_end(mi355_ctx* ctx, int lw, int lh, int lws, uint8_t** canvas, int* cw, int* ch, int* cws, const void* d_map, size_t map_bytes, void** map) {
    const size_t cbytes = (size_t)lws * lh;
    void* out = malloc(cbytes);
    void* m = map ? malloc(map_bytes) : nullptr;
    if (!out || (map && !m)) { free(out); free(m); return MI355_ERR_NOMEM; }
    hipError_t e = hipMemcpyAsync(out, ctx->buf("mosaic_canvas").p, cbytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && map) e = hipMemcpyAsync(m, d_map, map_bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { free(out); free(m); ctx->set_error(hipGetErrorString(e)); return MI355_ERR_DEVICE; }
    *canvas = (uint8_t*)out; *cw = lw; *ch = lh; *cws = lws;
    if (map) *map = m;
    return MI355_OK;
}

// ---- render into caller memory --------------------------------------------------------------------------------------------
// sources (kept frames / "into_srcs"), render(d_imgs, d_canvas) into "into_canvas", the canvas's rows into dst
template <class Render>
static int render_into(mi355_ctx* ctx, const char* who, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h, const int* ws,
                       int n, const float* h9s, const uint8_t* keep, uint8_t* dst, int dst_pitch, int cw, int ch, int lw, int lh, int lws, Render render) {
    int rc = check_dst(ctx, who, dst, dst_pitch, cw, ch, lw, lh);
    if (rc != MI355_OK) return rc;
    std::vector<const uint8_t*> dptr;
    rc = render_sources(ctx, who, imgs, img_ids, w, h, ws, n, h9s, keep, "into_srcs", dptr);
    if (rc != MI355_OK) return rc;
    DevBuf& dcan = ctx->buf("into_canvas");
    MI_HIP(dcan.reserve((size_t)lws * lh));
    rc = render(dptr.data(), dcan.as<uint8_t>());
    if (rc != MI355_OK) return rc;
    return download_rows(ctx, dcan.as<uint8_t>(), (size_t)lws, dst, (size_t)dst_pitch, (size_t)3 * lw, lh);
}

extern "C" int mi355_mosaic_refined_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h,
                                         const int* ws, int n, const float* h9s, uint8_t* dst, int dst_pitch, int cw, int ch) {
    LOCKED_PROLOGUE
    if (!w || !h || !ws || !h9s || (!imgs && !img_ids)) { ctx->set_error("mosaic_refined_into: bad arguments"); return MI355_ERR_ARG; }
    int lw, lh, lws;
    const int rc = render_layout(ctx, "mosaic_refined_into", w, h, n, h9s, &lw, &lh, &lws);
    if (rc != MI355_OK) return rc;
    return render_into(ctx, "mosaic_refined_into", imgs, img_ids, w, h, ws, n, h9s, nullptr, dst, dst_pitch, cw, ch, lw, lh, lws,
                       [&](const uint8_t* const* d, uint8_t* dc) { return mi_mosaic_refined_dev(ctx, d, w, h, ws, n, h9s, dc, lw, lh, lws, 0, lh); });
}

extern "C" int mi355_mosaic_feathered_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h,
                                           const int* ws, int n, const float* h9s, const mi355_feather_params* params, uint8_t* dst, int dst_pitch,
                                           int cw, int ch) {
    LOCKED_PROLOGUE
    if (!w || !h || !ws || !h9s || (!imgs && !img_ids)) { ctx->set_error("mosaic_feathered_into: bad arguments"); return MI355_ERR_ARG; }
    int lw, lh, lws;
    const int rc = render_layout(ctx, "mosaic_feathered_into", w, h, n, h9s, &lw, &lh, &lws);
    if (rc != MI355_OK) return rc;
    return render_into(ctx, "mosaic_feathered_into", imgs, img_ids, w, h, ws, n, h9s, nullptr, dst, dst_pitch, cw, ch, lw, lh, lws,
                       [&](const uint8_t* const* d, uint8_t* dc) { return mi_mosaic_feathered_dev(ctx, d, w, h, ws, n, h9s, params, dc, lw, lh, lws, 0, lh); });
}

extern "C" int mi355_mosaic_seamline_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h,
                                           const int* ws, int n, const float* h9s, const mi355_seamline_params* params, uint8_t* dst, int dst_pitch,
                                           int cw, int ch) {
    LOCKED_PROLOGUE
    if (!w || !h || !ws || !h9s || (!imgs && !img_ids)) { ctx->set_error("mosaic_seamline_into: bad arguments"); return MI355_ERR_ARG; }
    int lw, lh, lws;
    const int rc = render_layout(ctx, "mosaic_seamline_into", w, h, n, h9s, &lw, &lh, &lws);
    if (rc != MI355_OK) return rc;
    return render_into(ctx, "mosaic_seamline_into", imgs, img_ids, w, h, ws, n, h9s, nullptr, dst, dst_pitch, cw, ch, lw, lh, lws, [&](const uint8_t* const* d, uint8_t* dc) {
        return mi_mosaic_seamline_dev(ctx, d, w, h, ws, n, h9s, params, dc, lw, lh, lws, nullptr, nullptr, 0, lh, nullptr);
    });
}

extern "C" int mi355_mosaic_median_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h,
                                         const int* ws, int n, const float* h9s, const mi355_median_params* params, uint8_t* dst, int dst_pitch,
                                         int cw, int ch) {
    LOCKED_PROLOGUE
    if (!w || !h || !ws || !h9s || (!imgs && !img_ids)) { ctx->set_error("mosaic_median_into: bad arguments"); return MI355_ERR_ARG; }
    int lw, lh, lws;
    const int rc = render_layout(ctx, "mosaic_median_into", w, h, n, h9s, &lw, &lh, &lws);
    if (rc != MI355_OK) return rc;
    return render_into(ctx, "mosaic_median_into", imgs, img_ids, w, h, ws, n, h9s, nullptr, dst, dst_pitch, cw, ch, lw, lh, lws, [&](const uint8_t* const* d, uint8_t* dc) {
        return mi_mosaic_median_dev(ctx, d, w, h, ws, n, h9s, params, dc, lw, lh, lws, nullptr, nullptr, 0, lh, nullptr);
    });
}

extern "C" int mi355_mosaic_seamcut_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h,
                                          const int* ws, int n, const float* h9s, const mi355_seamcut_params* params, uint8_t* dst, int dst_pitch,
                                          int cw, int ch) {
    LOCKED_PROLOGUE
    if (!w || !h || !ws || !h9s || (!imgs && !img_ids)) { ctx->set_error("mosaic_seamcut_into: bad arguments"); return MI355_ERR_ARG; }
    int lw, lh, lws;
    const int rc = render_layout(ctx, "mosaic_seamcut_into", w, h, n, h9s, &lw, &lh, &lws);
    if (rc != MI355_OK) return rc;
    return render_into(ctx, "mosaic_seamcut_into", imgs, img_ids, w, h, ws, n, h9s, nullptr, dst, dst_pitch, cw, ch, lw, lh, lws, [&](const uint8_t* const* d, uint8_t* dc) {
        return mi_mosaic_seamcut_dev(ctx, d, w, h, ws, n, h9s, params, nullptr, dc, lw, lh, lws, nullptr, nullptr, 0, lh, nullptr);
    });
}

extern "C" int mi355_mosaic_blended_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h,
                                         const int* ws, int n, const float* h9s, const uint8_t* keep, int band, uint8_t* dst, int dst_pitch,
                                         int cw, int ch) {
    LOCKED_PROLOGUE
    if (!w || !h || !ws || !h9s || n <= 0 || (!imgs && !img_ids)) { ctx->set_error("mosaic_blended_into: bad arguments"); return MI355_ERR_ARG; }
    int lw = 0, lh = 0;
    const int rc = mi_blend_layout(w, h, n, h9s, keep, &lw, &lh);
    if (rc != MI355_OK) return rc;
    const int lws = (lw * 3 + 3) & ~3;
    return render_into(ctx, "mosaic_blended_into", imgs, img_ids, w, h, ws, n, h9s, keep, dst, dst_pitch, cw, ch, lw, lh, lws,
                       [&](const uint8_t* const* d, uint8_t* dc) { return mi_mosaic_blended_dev(ctx, d, w, h, ws, n, h9s, keep, band, dc, lw, lh, lws); });
}

// The blend along optimised seams (blend_seam.hip) with mi355_mosaic_blended_into's sources and download: all three stages in the call.
int mi_blend_seam_host_entry(mi355_ctx*, const char* who, const int* w, const int* h, int n, const float* h9s, const uint8_t* keep,
                             const mi355_seamcut_params* params, int* cw, int* ch, int* gw, int* gh);      // blend_seam.hip
extern "C" int mi355_mosaic_blended_seam_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h,
                                              const int* ws, int n, const float* h9s, const uint8_t* keep, int band, const mi355_seamcut_params* params,
                                              uint8_t* dst, int dst_pitch, int cw, int ch) {
    LOCKED_PROLOGUE
    if (!w || !h || !ws || !h9s || n <= 0 || (!imgs && !img_ids)) { ctx->set_error("mosaic_blended_seam_into: bad arguments"); return MI355_ERR_ARG; }
    mi355_seamcut_params dp;
    if (!params) { mi355_default_seamcut_params(&dp); params = &dp; }
    int lw = 0, lh = 0, gw = 0, gh = 0;
    const int rc = mi_blend_seam_host_entry(ctx, "mosaic_blended_seam_into", w, h, n, h9s, keep, params, &lw, &lh, &gw, &gh);
    if (rc != MI355_OK) return rc;
    const int lws = (lw * 3 + 3) & ~3;
    return render_into(ctx, "mosaic_blended_seam_into", imgs, img_ids, w, h, ws, n, h9s, keep, dst, dst_pitch, cw, ch, lw, lh, lws, [&](const uint8_t* const* d, uint8_t* dc) {
        return mi_mosaic_blended_seam_dev(ctx, d, w, h, ws, n, h9s, keep, band, params, nullptr, gw, gh, dc, lw, lh, lws);
    });
}

// ... into a malloc'd canvas of the layout's own pitch
extern "C" int mi355_mosaic_blended_seam(mi355_ctx* ctx, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                         const uint8_t* keep, int band, const mi355_seamcut_params* params, uint8_t** out, int* out_w, int* out_h, int* out_ws) {
    if (!ctx) return MI355_ERR_ARG;
    if (!out || !w || !h || !h9s || n <= 0) { std::lock_guard<std::mutex> lk(ctx->mu); ctx->set_error("mosaic_blended_seam: bad arguments"); return MI355_ERR_ARG; }
    int lw = 0, lh = 0;
    if (mi_blend_layout(w, h, n, h9s, keep, &lw, &lh) != MI355_OK || lw <= 0 || lh <= 0) { std::lock_guard<std::mutex> lk(ctx->mu); ctx->set_error("mosaic_blended_seam: empty canvas"); return MI355_ERR_FAILED; }
    const int lws = (lw * 3 + 3) & ~3;
    uint8_t* host = (uint8_t*)calloc((size_t)lws, (size_t)lh);       // the row padding stays zero
    if (!host) return MI355_ERR_NOMEM;
    const int rc = mi355_mosaic_blended_seam_into(ctx, imgs, nullptr, w, h, ws, n, h9s, keep, band, params, host, lws, lw, lh);      // (takes the lock)
    if (rc != MI355_OK) { free(host); return rc; }
    *out = host;
    if (out_w) *out_w = lw;
    if (out_h) *out_h = lh;
    if (out_ws) *out_ws = lws;
    return MI355_OK;
}

// ---- striped preview ------------------------------------------------------------------------------------------------------
// Level `level` of a render's canvas without that canvas: the survey is rendered stripe by stripe into ONE stripe buffer, each stripe is
// reduced by the overview kernel (overview.hip) into the level's buffer, and only that level comes back.  The render launchers address the
// canvas as base + y * pitch with y a row of the whole canvas, so a stripe buffer is handed to them as the base the whole canvas would have
// had: buffer - row0 * pitch.  Only rows [row0, row0 + rows) are ever touched through it.
template <class T> static T* stripe_base(T* buf, int row0, size_t pitch_elems) {
    return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(buf) - (uintptr_t)row0 * pitch_elems * sizeof(T));
}

extern "C" int mi355_mosaic_preview_into(mi355_ctx* ctx, const uint8_t* const* imgs, const int32_t* img_ids, const int* w, const int* h,
                                         const int* ws, int n, const float* h9s, const mi355_preview_params* params, uint8_t* dst, int dst_pitch,
                                         uint16_t* cover, int ow, int oh) {
    LOCKED_PROLOGUE
    if (!w || !h || !ws || !h9s || (!imgs && !img_ids)) { ctx->set_error("mosaic_preview_into: bad arguments"); return MI355_ERR_ARG; }
    mi355_preview_params dp;
    if (!params) { mi355_default_preview_params(&dp); params = &dp; }
    if (params->render < 0 || params->render > 2) { ctx->set_error("mosaic_preview_into: render=" + std::to_string(params->render) + " outside 0..2"); return MI355_ERR_ARG; }
    if (params->level < 1 || params->level > 7) { ctx->set_error("mosaic_preview_into: level=" + std::to_string(params->level) + " outside 1..7"); return MI355_ERR_ARG; }
    if (params->nodata < 0 || params->nodata > 2) { ctx->set_error("mosaic_preview_into: nodata=" + std::to_string(params->nodata) + " outside 0..2"); return MI355_ERR_ARG; }
    if (params->ramp < 0) { ctx->set_error("mosaic_preview_into: ramp=" + std::to_string(params->ramp) + " < 0"); return MI355_ERR_ARG; }
    const int level = params->level;
    int lw, lh, lws;
    int rc = render_layout(ctx, "mosaic_preview_into", w, h, n, h9s, &lw, &lh, &lws);
    if (rc != MI355_OK) return rc;
    int aw[7], ah[7], aws[7];
    mi355_overview_layout(lw, lh, level, aw, ah, aws);
    const int low = aw[level - 1], loh = ah[level - 1], lows = aws[level - 1];
    rc = check_dst(ctx, "mosaic_preview_into", dst, dst_pitch, ow, oh, low, loh);
    if (rc != MI355_OK) return rc;
    std::vector<const uint8_t*> dptr;
    rc = render_sources(ctx, "mosaic_preview_into", imgs, img_ids, w, h, ws, n, h9s, nullptr, "into_srcs", dptr);
    if (rc != MI355_OK) return rc;
    const int unit = 1 << level;
    long srows = ctx->preview_stripe_rows > 0 ? ((long)ctx->preview_stripe_rows + unit - 1) / unit * unit : lh;
    if (srows > lh) srows = lh;                            // one stripe: it ends the canvas
    const bool use_map = params->nodata == MI355_NODATA_MAP;
    DevBuf& dstripe = ctx->buf("preview_stripe");
    DevBuf& dmap = ctx->buf("preview_map");
    DevBuf& dlev = ctx->buf("preview_level");
    DevBuf& dcov = ctx->buf("preview_cover");
    MI_HIP(dstripe.reserve((size_t)lws * srows));
    if (use_map) MI_HIP(dmap.reserve(sizeof(uint16_t) * (size_t)lw * srows));
    MI_HIP(dlev.reserve((size_t)lows * loh));
    if (cover) MI_HIP(dcov.reserve(sizeof(uint16_t) * (size_t)low * loh));
    uint8_t* d_lv[7] = {nullptr};
    uint16_t* d_cv[7] = {nullptr};
    d_lv[level - 1] = dlev.as<uint8_t>();
    d_cv[level - 1] = cover ? dcov.as<uint16_t>() : nullptr;
    mi355_feather_params fp;
    mi355_seamline_params sp;
    mi355_default_feather_params(&fp); fp.ramp = params->ramp;
    mi355_default_seamline_params(&sp); sp.ramp = params->ramp;
    for (int row0 = 0; row0 < lh; row0 += (int)srows) {
        const int rows = lh - row0 < srows ? lh - row0 : (int)srows;
        uint8_t* base = stripe_base(dstripe.as<uint8_t>(), row0, (size_t)lws);
        uint16_t* mbase = use_map ? stripe_base(dmap.as<uint16_t>(), row0, (size_t)lw) : nullptr;
        if (params->render == 0) rc = mi_mosaic_refined_dev(ctx, dptr.data(), w, h, ws, n, h9s, base, lw, lh, lws, row0, rows);
        else if (params->render == 1) rc = mi_mosaic_feathered_dev(ctx, dptr.data(), w, h, ws, n, h9s, &fp, base, lw, lh, lws, row0, rows);
        else rc = mi_mosaic_seamline_dev(ctx, dptr.data(), w, h, ws, n, h9s, &sp, base, lw, lh, lws, nullptr, mbase, row0, rows, nullptr);
        // exact coverage of the refined and feathered renders: the seamline ownership walk's count, nothing sampled
        if (rc == MI355_OK && use_map && params->render != 2)
            rc = mi_mosaic_seamline_dev(ctx, nullptr, w, h, nullptr, n, h9s, &sp, nullptr, lw, lh, lws, nullptr, mbase, row0, rows, nullptr);
        if (rc != MI355_OK) return rc;
        rc = mi_mosaic_overview_dev(ctx, dstripe.as<uint8_t>(), lw, lh, lws, use_map ? dmap.as<uint16_t>() : nullptr, params->nodata, level, d_lv, d_cv,
                                    row0, rows, level);
        if (rc != MI355_OK) return rc;
    }
    rc = download_rows(ctx, dlev.as<uint8_t>(), (size_t)lows, dst, (size_t)dst_pitch, (size_t)3 * low, loh);
    if (rc != MI355_OK || !cover) return rc;
    return download_rows(ctx, dcov.as<uint8_t>(), sizeof(uint16_t) * (size_t)low, (uint8_t*)cover, sizeof(uint16_t) * (size_t)low, sizeof(uint16_t) * (size_t)low, loh);
}
