// csrc/mosaic_frame.h -- what the one-pass canvas renders (refined: warp.hip, feathered: feather.hip, seamline: seamline.hip, median: median.hip) share.
// Host side: the FrameDev record and its setup (the clipped canvas box and the inverse), the entry check of the _dev launchers, the frame
// table with its upload and candidate lists, the "which table entries were used" pass (all warp.hip), and the host forms' staging and
// download (frames.hip).  Device side: the 2 x 2 texel loads, "frame f gives canvas pixel (x, y) this sample" (also gain.hip), and the
// lane / tile prologue and 12-byte row store of feather_tile_kernel, seamline_tile_kernel and median_tile_kernel.  mosaic_tile_kernel spells the same
// map / bounds / hm::bilin / store steps inline, so that its registers stay what they are: 63 VGPRs, 8 waves per SIMD, one register below the
// 64 at which it loses a wave (72 and 7 waves while load_quad3 took its bytes out of a 64-bit integer).  Issuing the loads of a row's four
// pixels together before the arithmetic was tried on top: 96 to 104 VGPRs, or 120 bytes of scratch at a forced 64, and a slower kernel
// (CHANGELOG.md).  tests/test_gpu_gain.py pins the helpers against the render (per-frame samples and cover equal the oracle's refined
// canvas); tests/test_gpu_sample_paths.py pins the two load forms and the byte positions in every kernel that samples.
#pragma once
#include "common.h"
#include "hmath.h"

struct FrameDev {
    const uint8_t* src; int w, h, ws;
    int begX, endX, begY, endY;                 // clipped canvas bounding box the reference visits for this image (MosaicWithoutPos.cpp:2276-2306)
    float inv[9];
    int unit_den;                               // affine with m8 = 1: the two divisions are by exactly 1.0f
};

// frame k's FrameDev for the canvas rows [row0, row0 + rows) of a cw x ch canvas with shift dG (mi355_mosaic_layout): 0 when the render skips
// the frame (h9[8] == 0, no inverse, or a clipped box that misses the rows), 1 otherwise.  src / w / h / ws are left to the caller.
int mi_frame_dev_setup(const float* h9, int w, int h, const float dG[2], int cw, int ch, int row0, int rows, FrameDev& f);

// a frame's feather ramp (ramp.h: ramp_of_frame, ramp_weight)
struct RampDev { uint32_t R, mul, shift, _pad; };

// ---- the host path of the one-pass renders ------------------------------------------------------------------------------------------
// The entry check of a _dev launcher (`who` prefixes its messages): the layout of the survey must be the caller's cw x ch (and, where a canvas
// is written, cws a multiple of 4 that holds a row) -- a cover call (cover) has no canvas and takes the layout's; row0 / rows are clamped to
// the canvas, dG is the layout's shift.  go = 0: no rows, nothing to do.
int mi_render_entry(mi355_ctx* ctx, const char* who, const int* w, const int* h, int n, const float* h9s, bool cover, bool want_canvas,
                    int& cw, int& ch, int& cws, int& row0, int& rows, float dG[2], bool& go);

// The frames a render walks: fr[q] is the caller's image frame_of[q] (ascending), ramps[q] its ramp where the render weighs.  Which frames
// enter, and what a withheld pointer means, is the render's own loop over mi_frame_dev_setup.
constexpr int MOSAIC_LIST_BLOCK = 256;
struct FrameTable {
    std::vector<FrameDev> fr;
    std::vector<int> frame_of;
    std::vector<RampDev> ramps;
    void add(const FrameDev& f, int k) { fr.push_back(f); frame_of.push_back(k); }
    // filled by mi_frame_table_upload
    int nf = 0, bx_n = 0;
    const FrameDev* d_fr = nullptr; const RampDev* d_ramps = nullptr; const int* d_frame_of = nullptr;
    const uint16_t* d_lists = nullptr; const int* d_counts = nullptr;
};

// The table into the ctx buffers "mosaic_frames" (with_ramps: "feather_ramps", with_frame_of: "seamline_frame_of") and its per-block candidate
// lists (mosaic_lists_kernel into "mosaic_lists" / "mosaic_counts"), enqueued on the ctx stream: for every MOSAIC_LIST_BLOCK x MOSAIC_LIST_BLOCK
// block of the canvas rows from row0 on (bx_n blocks a row, row-major) the frames whose box meets it, highest index first, at d_lists[block *
// nf ..], their number in d_counts[block].  The host vectors must outlive the copies (the renders end with a stream synchronise).
int mi_frame_table_upload(mi355_ctx* ctx, FrameTable& t, bool with_ramps, bool with_frame_of, int cw, int rows, int row0);

// used[q] != 0 for the table entries a pass marked: _begin zeroes "mosaic_used" and hands it out, the caller enqueues the pass that sets
// d_used[q] on the ctx stream, _end copies the flags back (complete on return).
int mi_frame_table_used_begin(mi355_ctx* ctx, const FrameTable& t, int** d_used);
int mi_frame_table_used_end(mi355_ctx* ctx, const FrameTable& t, std::vector<int>& used);

// The host form of a render (frames.hip).  _begin: n <= 1 and the layout, the images with h9[8] != 0 staged in "mosaic_srcs" (d_imgs), and
// "mosaic_canvas" sized for the layout.  The caller renders.  _end: the canvas -- and d_map, map_bytes of a second output where asked for --
// handed back in malloc'd memory, complete on return; on failure no output is touched.
int mi_render_host_begin(mi355_ctx* ctx, const char* who, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                         int* lw, int* lh, int* lws, std::vector<const uint8_t*>& d_imgs, uint8_t** d_canvas);
int mi_render_host_end(mi355_ctx* ctx, int lw, int lh, int lws, uint8_t** canvas, int* cw, int* ch, int* cws, const void* d_map = nullptr,
                       size_t map_bytes = 0, void** map = nullptr);

namespace {

// Texel addresses come out of a table in memory (FrameDev::src), so to the compiler they are generic pointers: flat loads.  Frames are
// device allocations; through the global address space the same loads are global_load_* (the idiom of match.hip, guided.hip, blend.hip).
#define GLOBAL_PTR(T, p) ((const __attribute__((address_space(1))) T*)(p))

template <int CH>
__device__ __forceinline__ void load_pair(const uint8_t* s, uint32_t& lo, uint32_t& hi);

// 6 bytes (two BGR pixels) as the words {bytes 0..3, bytes 4..5}: one dword + one ushort load; the device handles unaligned addresses.
template <>
__device__ __forceinline__ void load_pair<3>(const uint8_t* s, uint32_t& lo, uint32_t& hi) {
    uint16_t h;
    __builtin_memcpy(&lo, GLOBAL_PTR(void, s), 4);
    __builtin_memcpy(&h, GLOBAL_PTR(void, s + 4), 2);
    hi = h;
}

// the same two words out of ONE 8-byte load: the 8 bytes stay one object and are split by value into their 32-bit halves.  (Copied into two
// addressable words, the compiler split some of the loads into two dword loads; the load count is one of the canvas kernel's two bounds.)
__device__ __forceinline__ void load_wide3(const uint8_t* s, uint32_t& lo, uint32_t& hi) {
    uint64_t q;
    __builtin_memcpy(&q, GLOBAL_PTR(void, s), 8);
    lo = (uint32_t)q; hi = (uint32_t)(q >> 32);
}

// the six bytes of two BGR pixels in {lo, hi} as floats: each one v_cvt_f32_ubyteN of a 32-bit register.  (Taken with shifts of the uint64_t
// itself, every byte was the generic u64 -> f32 conversion, six instructions: 73 of the 183 vector instructions of a sampled pixel.)  One
// spelling after the wide / narrow choice, so that neither form's knowledge of the upper bits of hi turns a byte into a shift and a u32 convert.
__device__ __forceinline__ void bytes6(uint32_t lo, uint32_t hi, float& b0, float& g0, float& r0, float& b1, float& g1, float& r1) {
    b0 = (float)(lo & 0xff); g0 = (float)((lo >> 8) & 0xff); r0 = (float)((lo >> 16) & 0xff);
    b1 = (float)(lo >> 24);  g1 = (float)(hi & 0xff);        r1 = (float)((hi >> 8) & 0xff);
}

// the two BGR pixel pairs of a 2 x 2 neighbourhood (rows s and s + ws): one 8-byte load per row where 8 bytes from s still lie inside the row's
// pitch (6 are used), else the 4 + 2 byte form -- half the load instructions of a sample (the canvas kernel is bound by their number)
__device__ __forceinline__ void load_quad3(const uint8_t* s, int ws, bool wide, float& b00, float& g00, float& r00, float& b01, float& g01, float& r01,
                                           float& b10, float& g10, float& r10, float& b11, float& g11, float& r11) {
    uint32_t lo0, hi0, lo1, hi1;
    if (wide) { load_wide3(s, lo0, hi0); load_wide3(s + ws, lo1, hi1); }
    else { load_pair<3>(s, lo0, hi0); load_pair<3>(s + ws, lo1, hi1); }
    bytes6(lo0, hi0, b00, g00, r00, b01, g01, r01);
    bytes6(lo1, hi1, b10, g10, r10, b11, g11, r11);
}

// canvas pixel (xD, yD) -> source coordinate of frame f (xf = xD - dGx, yf = yD - dGy)
__device__ __forceinline__ void frame_src(const FrameDev& f, float xf, float yf, float& xs, float& ys) {
    if (f.unit_den) { xs = f.inv[0] * xf + f.inv[1] * yf + f.inv[2]; ys = f.inv[3] * xf + f.inv[4] * yf + f.inv[5]; }
    else hm::apply_div9(f.inv, xf, yf, xs, ys);
}

// the frame has a sample at that source coordinate: inside [0, w - 1) x [0, h - 1) (w1 = w - 1, h1 = h - 1), which also rejects NaN.  Together
// with the pixel lying inside the frame's canvas box, this is "frame f gives the canvas pixel a sample".
__device__ __forceinline__ bool src_inside(float xs, float ys, float w1, float h1) {
    return xs >= 0.0f && xs < w1 && ys >= 0.0f && ys < h1;
}

// the B, G, R bytes of frame f at a source coordinate frame_src accepted
__device__ __forceinline__ void frame_sample3(const FrameDev& f, float xs, float ys, unsigned& vb, unsigned& vg, unsigned& vr) {
    const int xi = (int)xs, yi = (int)ys;
    const float p = ys - (float)yi, q = xs - (float)xi;
    float b00, g00, r00, b01, g01, r01, b10, g10, r10, b11, g11, r11;
    // the 2 x 2 neighbourhood straight from the image: the lanes of a wave walk two nearly contiguous runs of the two
    // source rows, so the 6-byte loads share their cache lines (staging the tile's footprint in LDS first was measured
    // slower: 11.4 ms against 8.5 ms for the C3 canvas -- its barriers and 24 KB per workgroup cost more than the
    // L1 / L2 hits they replace)
    const uint8_t* g0 = f.src + (size_t)yi * f.ws + 3 * (size_t)xi;
    load_quad3(g0, f.ws, 3 * xi + 8 <= f.ws, b00, g00, r00, b01, g01, r01, b10, g10, r10, b11, g11, r11);
    vb = hm::bilin(b00, b01, b10, b11, p, q); vg = hm::bilin(g00, g01, g10, g11, p, q); vr = hm::bilin(r00, r01, r10, r11, p, q);
}

// The same sample for a caller that chose the texel itself (undistort.hip: xi, yi clamped to w - 2, h - 2, so p or q may be exactly 1): the
// B, G, R bytes from the 2 x 2 texels at (xi, yi) of a w-pixel-wide image with rows ws bytes apart.  The 8-byte form only where its 8 bytes
// are pixels of the row (xi <= w - 3): no byte outside the image's pixels is read.  frame_sample3 stays as it is, and with it the code objects
// of the kernels that call it.
__device__ __forceinline__ void texel_sample3(const uint8_t* src, int w, int ws, int xi, int yi, float p, float q, unsigned& vb, unsigned& vg, unsigned& vr) {
    float b00, g00, r00, b01, g01, r01, b10, g10, r10, b11, g11, r11;
    const uint8_t* g0 = src + (size_t)yi * ws + 3 * (size_t)xi;
    load_quad3(g0, ws, xi + 3 <= w, b00, g00, r00, b01, g01, r01, b10, g10, r10, b11, g11, r11);
    vb = hm::bilin(b00, b01, b10, b11, p, q); vg = hm::bilin(g00, g01, g10, g11, p, q); vr = hm::bilin(r00, r01, r10, r11, p, q);
}

// ---- the tile prologue and row store of feather_tile_kernel / seamline_tile_kernel ----------------------------------------------------
// (mosaic_tile_kernel keeps its own spelling, see the file head.  The walk between the two stays spelt out in both kernels: as a helper
// taking the per-sample step as a functor it cost feather_tile_kernel 16 VGPRs, 99 against 83, and with them a wave per SIMD.)
// What a lane of the 256-lane workgroup of a TW x 8 RPL canvas tile (TW = 128) works on: 4 adjacent pixels from column xg in each of the RPL rows
// yB + 8 j, the candidate list of the tile's block, and the tile's corners clipped to the canvas and the rows of the call.
struct TileLane { int tx0, ty0, tx1, ty1, xg, yB, cnt; const uint16_t* list; };

template <int TW, int RPL>
__device__ __forceinline__ TileLane tile_lane(const uint16_t* lists, const int* counts, int n, int bx_n, int cw, int row0, int row_end) {
    constexpr int TH = 8 * RPL;
    static_assert(MOSAIC_LIST_BLOCK % TW == 0 && MOSAIC_LIST_BLOCK % TH == 0, "a tile lies inside one list block");
    const int tid = threadIdx.x;
    TileLane t;
    t.tx0 = blockIdx.x * TW; t.ty0 = row0 + blockIdx.y * TH;
    t.xg = t.tx0 + 4 * (tid & 31); t.yB = t.ty0 + (tid >> 5);
    const int cb = ((t.ty0 - row0) / MOSAIC_LIST_BLOCK) * bx_n + t.tx0 / MOSAIC_LIST_BLOCK;
    t.list = lists + (size_t)cb * n;
    t.cnt = counts[cb];
    t.tx1 = t.tx0 + TW - 1 < cw - 1 ? t.tx0 + TW - 1 : cw - 1;
    t.ty1 = t.ty0 + TH - 1 < row_end - 1 ? t.ty0 + TH - 1 : row_end - 1;
    return t;
}

// The 12 bytes (B G R of 4 pixels) of a lane's group in canvas row yD: three dwords where the group is whole, bytes where the row ends inside
// it; the lane that owns the row's last group clears the padding [3 cw, cws), as the unblended render does.
__device__ __forceinline__ void store_row12(uint8_t* canvas, int cw, int cws, int xg, int yD, const uint32_t out[3]) {
    uint8_t* drow = canvas + (size_t)yD * cws + 3 * (size_t)xg;
    if (xg + 3 < cw) {
        uint32_t* d32 = reinterpret_cast<uint32_t*>(drow);
        d32[0] = out[0]; d32[1] = out[1]; d32[2] = out[2];
    } else {
#pragma unroll
        for (int b = 0; b < 9; b++)                      // at most 3 pixels
            if (xg + b / 3 < cw) drow[b] = (uint8_t)(out[b >> 2] >> (8 * (b & 3)));
    }
    if (xg + 4 >= cw)
        for (int b = 3 * cw; b < cws; b++) canvas[(size_t)yD * cws + b] = 0;
}

// four 16-bit map entries of a lane's pixel group (seamline.hip: owner, count; median.hip: count): 8 bytes at once where the group is whole
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

}  // namespace
