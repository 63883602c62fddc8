// csrc/lens.h -- the Brown-Conrady mapping of the lens undistortion (include/mi355_mosaic.h, "lens undistortion"), once: the kernel of
// undistort.hip, mi355_undistort_fit and mi355_undistort_map all call these functions, so host and device cannot drift apart.  Every
// operation is a separately rounded f32 operation in the header's order (the build's -ffp-contract=off is part of the contract); nothing
// here divides.
#pragma once
#include "hmath.h"

namespace lens {

// the constants of a call, formed once on the host (lens_consts in undistort.hip): the nine camera values and the output principal point
// cast to float, and the reciprocals of the output focal lengths, each quotient taken in double
struct Consts { float fx, fy, cx, cy, k1, k2, p1, p2, k3, ocx, ocy, ifx, ify; };

// normalised coordinates of output column u / row v
HD float norm_x(const Consts& c, int u) { return ((float)u - c.ocx) * c.ifx; }
HD float norm_y(const Consts& c, int v) { return ((float)v - c.ocy) * c.ify; }

// source coordinate of the output pixel with normalised coordinates (x, y); xx = x * x and yy = y * y come from the caller, who forms the
// column terms once per column and the row terms once per row
HD void distort(const Consts& c, float x, float xx, float y, float yy, float& xs, float& ys) {
    const float xy = x * y, r2 = xx + yy, a1 = xy + xy;
    float t = r2 * c.k3;
    t = c.k2 + t; t = r2 * t; t = c.k1 + t; t = r2 * t;
    const float rad = 1.0f + t;
    const float tx = (c.p1 * a1) + (c.p2 * (r2 + (xx + xx)));
    const float ty = (c.p1 * (r2 + (yy + yy))) + (c.p2 * a1);
    const float xd = (x * rad) + tx, yd = (y * rad) + ty;
    xs = (c.fx * xd) + c.cx;
    ys = (c.fy * yd) + c.cy;
}

// the pixel has a sample: the closed interval [0, w - 1] x [0, h - 1] (w1 = w - 1, h1 = h - 1), so that an undistorted camera gives back its
// last row and column -- on purpose not the renders' [0, w - 1) (mosaic_frame.h: src_inside).  Rejects NaN and infinities.
HD bool inside(float xs, float ys, float w1, float h1) { return xs >= 0.0f && xs <= w1 && ys >= 0.0f && ys <= h1; }

}  // namespace lens
