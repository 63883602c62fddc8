// csrc/undistort.hip -- lens undistortion (gfx950): BGR frames of a camera with Brown-Conrady distortion resampled to an ideal pinhole
// camera (include/mi355_mosaic.h, "lens undistortion").  The mapping itself lives in lens.h, for the kernel and the two host-only calls
// (mi355_undistort_fit, mi355_undistort_map) alike.
//
//   undistort_kernel   one launch over all frames of a call (or of an in-place group): a frame table with a first_block prefix, as the gain
//                      apply has (gain.hip: ApplyHead), found by a wave-uniform binary search -- no LDS, no barrier.  A workgroup of 256
//                      lanes works on UD_BW = 1024 output columns x UD_ROWS rows; a lane owns 4 adjacent pixels in each of the rows, so that
//                      x, x * x and the store address's column part are formed once per lane and only the y terms per row.  Per pixel: the
//                      map (about 40 f32 operations, no division), the inside test, then -- only for a pixel that has a sample, so no address
//                      is formed from a coordinate that failed the test -- the 2 x 2 texels through load_quad3 and hm::bilin
//                      (mosaic_frame.h: texel_sample3).  The lanes of a wave read nearly contiguous runs of two source rows, which L1 / L2
//                      serve (the renders measured that staging such a footprint in LDS loses to that).  A lane's 12 bytes leave as three
//                      dwords where the destination's base and pitch are multiples of 4 and its 4 pixels lie inside the row, bytewise
//                      otherwise.  Pixels without a sample are counted per wave (ballot / popcount into a scalar) and land with one 64-bit
//                      vector atomic per wave that has any.
//   Its floor is HBM: 3 w h bytes read and 3 w h written per frame.
#include "common.h"
#include "lens.h"
#include "frame_pass.h"
#include "mosaic_frame.h"
#include <cmath>

namespace {

// the workgroup shape and the frame record are the shared host path's (frame_pass.h)
constexpr int UD_NT = FP_NT, UD_PX = FP_PX, UD_ROWS = FP_ROWS, UD_BW = FP_BW;
constexpr int UD_MAX_FRAMES = FP_MAX_FRAMES;
using UdFrame = PassFrame;

__global__ __launch_bounds__(UD_NT) void undistort_kernel(const UdFrame* frames, int nf, lens::Consts c, unsigned fill, unsigned long long* n_outside) {
    // the record of this workgroup's frame: the last one with first_block <= blockIdx.x (first_block ascends); the same in every lane
    int lo = 0, hi = nf - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (frames[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
    const UdFrame f = frames[lo];
    const int b = (int)blockIdx.x - f.first_block;
    const int by = b / f.bx_n, bx = b - by * f.bx_n;
    const int u0 = bx * UD_BW + UD_PX * (int)threadIdx.x, v0 = by * UD_ROWS;
    const float w1 = (float)(f.w - 1), h1 = (float)(f.h - 1);
    float x[UD_PX], xx[UD_PX];
#pragma unroll
    for (int i = 0; i < UD_PX; i++) { x[i] = lens::norm_x(c, u0 + i); xx[i] = x[i] * x[i]; }
    const bool whole = u0 + UD_PX - 1 < f.w;
    const bool dwords = whole && (((uintptr_t)f.dst | (uintptr_t)(unsigned)f.ws_dst) & 3) == 0;
    const size_t col = 3 * (size_t)u0;
    int cnt = 0;                                                 // pixels of the wave without a sample (wave-uniform)
    for (int v = v0; v < v0 + UD_ROWS && v < f.h; v++) {
        const float y = lens::norm_y(c, v), yy = y * y;
        uint32_t out[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < UD_PX; i++) {
            float xs, ys;
            lens::distort(c, x[i], xx[i], y, yy, xs, ys);
            const bool mine = u0 + i < f.w;
            const bool has = lens::inside(xs, ys, w1, h1);
            cnt += __popcll(__ballot(mine && !has));
            unsigned vb = fill, vg = fill, vr = fill;
            if (mine && has) {                                   // the inside test comes before any address is formed
                const int xi = min((int)xs, f.w - 2), yi = min((int)ys, f.h - 2);
                texel_sample3(f.src, f.w, f.ws_src, xi, yi, ys - (float)yi, xs - (float)xi, vb, vg, vr);
            }
            out[(3 * i) >> 2] |= vb << (8 * ((3 * i) & 3));
            out[(3 * i + 1) >> 2] |= vg << (8 * ((3 * i + 1) & 3));
            out[(3 * i + 2) >> 2] |= vr << (8 * ((3 * i + 2) & 3));
        }
        uint8_t* drow = f.dst + (size_t)v * f.ws_dst + col;
        if (dwords) {
            uint32_t* d32 = reinterpret_cast<uint32_t*>(drow);
            d32[0] = out[0]; d32[1] = out[1]; d32[2] = out[2];
        } else {
#pragma unroll
            for (int j = 0; j < 3 * UD_PX; j++)
                if (u0 + j / 3 < f.w) drow[j] = (uint8_t)(out[j >> 2] >> (8 * (j & 3)));
        }
    }
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_outside + f.k, (unsigned long long)cnt);
}

bool finite_all(const double* v, int n) {
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

const char* const CAM_NAMES[9] = {"fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3"};

// the camera's checks; err names the value
bool check_camera(const mi355_camera* cam, std::string& err) {
    if (!cam) { err = "camera is NULL"; return false; }
    const double* v = &cam->fx;
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(v[i])) { err = std::string("camera.") + CAM_NAMES[i] + " is not finite"; return false; }
    if (cam->fx <= 0.0) { err = "camera.fx=" + std::to_string(cam->fx) + " <= 0"; return false; }
    if (cam->fy <= 0.0) { err = "camera.fy=" + std::to_string(cam->fy) + " <= 0"; return false; }
    return true;
}

bool check_size(int w, int h, std::string& err) { return fp_check_size(w, h, err); }

// The constants of a call from a checked camera and the parameters (NULL: defaults), and the fill byte; the parameters' own checks.
bool lens_consts(const mi355_camera& cam, const mi355_undistort_params* p, lens::Consts& c, int& fill, std::string& err) {
    mi355_undistort_params dp;
    if (!p) { mi355_default_undistort_params(&dp); p = &dp; }
    const double o[4] = {p->out_fx, p->out_fy, p->out_cx, p->out_cy};
    static const char* const names[4] = {"out_fx", "out_fy", "out_cx", "out_cy"};
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(o[i])) { err = std::string("params.") + names[i] + " is not finite"; return false; }
    const bool own = o[0] == 0.0 && o[1] == 0.0 && o[2] == 0.0 && o[3] == 0.0;
    const double ofx = own ? cam.fx : o[0], ofy = own ? cam.fy : o[1], ocx = own ? cam.cx : o[2], ocy = own ? cam.cy : o[3];
    if (ofx <= 0.0) { err = "params.out_fx=" + std::to_string(ofx) + " <= 0"; return false; }
    if (ofy <= 0.0) { err = "params.out_fy=" + std::to_string(ofy) + " <= 0"; return false; }
    if (p->fill < 0 || p->fill > 255) { err = "params.fill=" + std::to_string(p->fill) + " outside 0..255"; return false; }
    c.fx = (float)cam.fx; c.fy = (float)cam.fy; c.cx = (float)cam.cx; c.cy = (float)cam.cy;
    c.k1 = (float)cam.k1; c.k2 = (float)cam.k2; c.p1 = (float)cam.p1; c.p2 = (float)cam.p2; c.k3 = (float)cam.k3;
    c.ocx = (float)ocx; c.ocy = (float)ocy;
    c.ifx = (float)(1.0 / ofx); c.ify = (float)(1.0 / ofy);
    fill = p->fill;
    return true;
}

// all 2 (w + h) - 4 border pixels of the output have a sample
bool border_inside(const lens::Consts& c, int w, int h) {
    const float w1 = (float)(w - 1), h1 = (float)(h - 1);
    auto ok = [&](int u, int v) {
        const float x = lens::norm_x(c, u), y = lens::norm_y(c, v);
        float xs, ys;
        lens::distort(c, x, x * x, y, y * y, xs, ys);
        return lens::inside(xs, ys, w1, h1);
    };
    for (int u = 0; u < w; u++)
        if (!ok(u, 0) || !ok(u, h - 1)) return false;
    for (int v = 1; v < h - 1; v++)
        if (!ok(0, v) || !ok(w - 1, v)) return false;
    return true;
}

int undistort_frames(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws_src, const int* ws_dst,
                     int n, const mi355_camera* cam, const mi355_undistort_params* p, int64_t* n_outside) {
    const std::string who = "undistort_frames: ";
    std::string err;
    if (n < 0 || n > UD_MAX_FRAMES) { ctx->set_error(who + "n=" + std::to_string(n) + " outside [0, 65535]"); return MI355_ERR_ARG; }
    lens::Consts c; int fill;
    if (!check_camera(cam, err) || !lens_consts(*cam, p, c, fill, err)) { ctx->set_error(who + err); return MI355_ERR_ARG; }
    if (n == 0) return MI355_OK;
    unsigned long long* d_outside = nullptr;
    return fp_run_frames(ctx, who, "undistort", d_src, d_dst, w, h, ws_src, ws_dst, n, n_outside,
                         [&]() { d_outside = ctx->buf("undistort_outside").as<unsigned long long>(); return MI355_OK; },
                         [&](const UdFrame* table, int nf, int blocks, double bytes) {
                             ProfScope ps(ctx, "undistort", bytes);
                             hipLaunchKernelGGL(undistort_kernel, dim3((unsigned)blocks), dim3(UD_NT), 0, ctx->stream, table, nf, c, (unsigned)fill, d_outside);
                         });
}

}  // namespace

extern "C" void mi355_default_undistort_params(mi355_undistort_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
}

extern "C" int mi355_undistort_fit(const mi355_camera* cam, int w, int h, mi355_undistort_params* out) {
    const std::string who = "undistort_fit: ";
    std::string err;
    if (!out) { mi_set_host_error(who + "out is NULL"); return MI355_ERR_ARG; }
    if (!check_camera(cam, err) || !check_size(w, h, err)) { mi_set_host_error(who + err); return MI355_ERR_ARG; }
    mi355_undistort_params p;
    mi355_default_undistort_params(&p);
    p.out_cx = cam->cx; p.out_cy = cam->cy;
    for (int j = 128; j <= 1024; j++) {
        const double s = (double)j / 256.0;
        p.out_fx = s * (double)(float)cam->fx; p.out_fy = s * (double)(float)cam->fy;
        lens::Consts c; int fill;
        if (!lens_consts(*cam, &p, c, fill, err)) { mi_set_host_error(who + err); return MI355_ERR_ARG; }
        if (border_inside(c, w, h)) { *out = p; return MI355_OK; }
    }
    mi_set_host_error(who + "no scale j / 256 with j in 128..1024 puts every border pixel inside the source");
    return MI355_ERR_FAILED;
}

extern "C" int mi355_undistort_map(const mi355_camera* cam, const mi355_undistort_params* p, int w, int h, float* xs, float* ys) {
    const std::string who = "undistort_map: ";
    std::string err;
    lens::Consts c; int fill;
    if (!check_camera(cam, err) || !lens_consts(*cam, p, c, fill, err) || !check_size(w, h, err)) { mi_set_host_error(who + err); return MI355_ERR_ARG; }
    if (!xs || !ys) { mi_set_host_error(who + (!xs ? "xs" : "ys") + " is NULL"); return MI355_ERR_ARG; }
    std::vector<float> x((size_t)w), xx((size_t)w);
    for (int u = 0; u < w; u++) { x[u] = lens::norm_x(c, u); xx[u] = x[u] * x[u]; }
    for (int v = 0; v < h; v++) {
        const float y = lens::norm_y(c, v), yy = y * y;
        for (int u = 0; u < w; u++) lens::distort(c, x[u], xx[u], y, yy, xs[(size_t)v * w + u], ys[(size_t)v * w + u]);
    }
    return MI355_OK;
}

extern "C" int mi355_undistort_frames_dev(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws_src,
                                          const int* ws_dst, int n, const mi355_camera* cam, const mi355_undistort_params* p, int64_t* n_outside) {
    LOCKED_PROLOGUE
    return undistort_frames(ctx, d_src, d_dst, w, h, ws_src, ws_dst, n, cam, p, n_outside);
}

extern "C" int mi355_undistort_image(mi355_ctx* ctx, const uint8_t* src, int w, int h, int ws, uint8_t* dst, int dst_ws, const mi355_camera* cam,
                                     const mi355_undistort_params* p, int64_t* n_outside) {
    LOCKED_PROLOGUE
    const std::string who = "undistort_image: ";
    std::string err;
    if (!src || !dst) { ctx->set_error(who + (!src ? "src" : "dst") + " is NULL"); return MI355_ERR_ARG; }
    if (!check_size(w, h, err)) { ctx->set_error(who + err); return MI355_ERR_ARG; }
    if (ws < 3 * w) { ctx->set_error(who + "ws=" + std::to_string(ws) + " < 3 w=" + std::to_string(3 * w)); return MI355_ERR_ARG; }
    if (dst_ws < 3 * w) { ctx->set_error(who + "dst_ws=" + std::to_string(dst_ws) + " < 3 w=" + std::to_string(3 * w)); return MI355_ERR_ARG; }
    { lens::Consts c; int fill; if (!check_camera(cam, err) || !lens_consts(*cam, p, c, fill, err)) { ctx->set_error(who + err); return MI355_ERR_ARG; } }   // before the upload
    const int dws = (3 * w + 3) & ~3;
    const size_t bytes = (size_t)dws * (size_t)h;
    DevBuf& ds = ctx->buf("undistort_host_src"); DevBuf& dd = ctx->buf("undistort_host_dst");
    MI_HIP(ds.reserve(bytes));
    MI_HIP(dd.reserve(bytes));
    MI_HIP(hipMemcpy2DAsync(ds.p, (size_t)dws, src, (size_t)ws, 3 * (size_t)w, (size_t)h, hipMemcpyHostToDevice, ctx->stream));
    const uint8_t* sp = ds.as<uint8_t>(); uint8_t* dp = dd.as<uint8_t>();
    const int rc = undistort_frames(ctx, &sp, &dp, &w, &h, &dws, &dws, 1, cam, p, n_outside);
    if (rc != MI355_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }   // the upload reads the caller's rows
    MI_HIP(hipMemcpy2DAsync(dst, (size_t)dst_ws, dd.p, (size_t)dws, 3 * (size_t)w, (size_t)h, hipMemcpyDeviceToHost, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}
