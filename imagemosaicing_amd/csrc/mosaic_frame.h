// csrc/mosaic_frame.h -- one frame of the refined render as its kernels see it: the FrameDev record and its host setup (the clipped canvas box
// and the inverse, warp.hip: mi_frame_dev_setup), the 2 x 2 texel loads, and "frame f gives canvas pixel (x, y) this sample" as device helpers
// (gain.hip).  mosaic_tile_kernel spells the same map / bounds / hm::bilin steps inline, unchanged, so that its code object stays what it
// was; tests/test_gpu_gain.py pins the helpers against the render (per-frame samples and cover equal the oracle's refined canvas).
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

// The per-block candidate lists of the one-pass renders (warp.hip: mosaic_lists_kernel), enqueued on the ctx stream: for every MOSAIC_LIST_BLOCK x
// MOSAIC_LIST_BLOCK block of the canvas rows from row0 on (bx_n x by_n blocks, row-major) the frames of d_fr[0 .. nf) whose box meets it, highest
// index first, at d_lists[block * nf ..], their number in d_counts[block].
constexpr int MOSAIC_LIST_BLOCK = 256;
void mi_mosaic_lists_launch(mi355_ctx* ctx, const FrameDev* d_fr, int nf, int bx_n, int by_n, int row0, uint16_t* d_lists, int* d_counts);

namespace {

template <int CH>
__device__ __forceinline__ void load_pair(const uint8_t* s, float& a, float& b, float& c, float& a1, float& b1, float& c1);

// 6 bytes (two BGR pixels) with one dword + one ushort load; the device handles unaligned addresses.
template <>
__device__ __forceinline__ void load_pair<3>(const uint8_t* s, float& b0, float& g0, float& r0, float& b1, float& g1, float& r1) {
    uint32_t lo; uint16_t hi;
    __builtin_memcpy(&lo, s, 4);
    __builtin_memcpy(&hi, s + 4, 2);
    b0 = (float)(lo & 0xff); g0 = (float)((lo >> 8) & 0xff); r0 = (float)((lo >> 16) & 0xff);
    b1 = (float)(lo >> 24);  g1 = (float)(hi & 0xff);        r1 = (float)(hi >> 8);
}

// the two BGR pixel pairs of a 2 x 2 neighbourhood (rows s and s + ws): one 8-byte load per row where 8 bytes from s still lie inside the row's
// pitch (6 are used), else the 4 + 2 byte form -- half the load instructions of a sample (the canvas kernel is bound by their number)
__device__ __forceinline__ void load_quad3(const uint8_t* s, int ws, bool wide, float& b00, float& g00, float& r00, float& b01, float& g01, float& r01,
                                           float& b10, float& g10, float& r10, float& b11, float& g11, float& r11) {
    if (wide) {
        uint64_t q0, q1;
        __builtin_memcpy(&q0, s, 8);
        __builtin_memcpy(&q1, s + ws, 8);
        b00 = (float)(q0 & 0xff); g00 = (float)((q0 >> 8) & 0xff); r00 = (float)((q0 >> 16) & 0xff);
        b01 = (float)((q0 >> 24) & 0xff); g01 = (float)((q0 >> 32) & 0xff); r01 = (float)((q0 >> 40) & 0xff);
        b10 = (float)(q1 & 0xff); g10 = (float)((q1 >> 8) & 0xff); r10 = (float)((q1 >> 16) & 0xff);
        b11 = (float)((q1 >> 24) & 0xff); g11 = (float)((q1 >> 32) & 0xff); r11 = (float)((q1 >> 40) & 0xff);
    } else {
        load_pair<3>(s, b00, g00, r00, b01, g01, r01);
        load_pair<3>(s + ws, b10, g10, r10, b11, g11, r11);
    }
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

}  // namespace
