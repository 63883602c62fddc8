// csrc/ramp.h -- the border-distance weight omega_k of include/mi355_mosaic.h ("weighted (feather) blending"), shared by the renders that
// weigh a frame's sample by how deep it lies inside the frame: feather.hip (the weight of a mean) and seamline.hip (the depth that decides
// which frame owns a pixel).  Exact integers and one hm::bilin; no weight image exists.
#pragma once
#include "common.h"
#include "hmath.h"
#include "mosaic_frame.h"

constexpr int RAMP_MAX_SIDE = 1 << 20;          // frames up to 2^20 a side: 254 * (border distance) < 2^28, the range ramp_weight's quotient is exact on

// frame k's ramp: R and the constants of n / R for 0 <= n < 2^28 (Granlund & Montgomery 1994, theorem 4.2: with l = ceil(log2 R) and
// mul = ceil(2^(28 + l) / R), floor(n mul / 2^(28 + l)) = floor(n / R) for every n < 2^28; mul <= 2^29)
// (struct RampDev { R, mul, shift }: mosaic_frame.h, beside the frame record it travels with)

inline RampDev ramp_setup(uint32_t R) {
    uint32_t l = 0;
    while (((uint64_t)1 << l) < R) l++;
    RampDev r;
    r.R = R; r.shift = 28 + l; r._pad = 0;
    r.mul = (uint32_t)((((uint64_t)1 << r.shift) + R - 1) / R);
    return r;
}

// R of a w x h frame: params.ramp, or a full tent for ramp == 0
inline RampDev ramp_of_frame(int w, int h, int ramp) {
    const int side = w < h ? w : h;
    return ramp_setup((uint32_t)(ramp > 0 ? ramp : (side + 1) / 2));
}

namespace {

// Wk along one axis: (254 min(d, R)) / R for the border distance d of a texel row or column
__device__ __forceinline__ unsigned ramp_weight(int d, const RampDev& r) {
    const unsigned m = (unsigned)d < r.R ? (unsigned)d : r.R;
    return (unsigned)(((unsigned long long)(254u * m) * r.mul) >> r.shift);
}

// omega_k in [1, 255] at a source coordinate frame_src accepted, through the sample's own xi, yi, p, q: Wk of a texel = min over the two
// axes of the axis ramp (the quotient is monotone in d), then hm::bilin over the 2 x 2 texels
__device__ __forceinline__ unsigned ramp_omega(const FrameDev& f, const RampDev& r, float xs, float ys) {
    const int xi = (int)xs, yi = (int)ys;
    const float p = ys - (float)yi, q = xs - (float)xi;
    const int ax = f.w - 1 - xi, ay = f.h - 1 - yi;
    const unsigned wx0 = ramp_weight(xi < ax ? xi : ax, r), wx1 = ramp_weight(xi + 1 < ax - 1 ? xi + 1 : ax - 1, r);
    const unsigned wy0 = ramp_weight(yi < ay ? yi : ay, r), wy1 = ramp_weight(yi + 1 < ay - 1 ? yi + 1 : ay - 1, r);
    const float W00 = (float)(wx0 < wy0 ? wx0 : wy0), W01 = (float)(wx1 < wy0 ? wx1 : wy0);
    const float W10 = (float)(wx0 < wy1 ? wx0 : wy1), W11 = (float)(wx1 < wy1 ? wx1 : wy1);
    return 1u + hm::bilin(W00, W01, W10, W11, p, q);
}

}  // namespace
