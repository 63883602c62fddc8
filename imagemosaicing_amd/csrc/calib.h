// csrc/calib.h -- what the lens self-calibration's host loop (calib_solve.cpp) and its device half (calib.hip) share: the chain of one tie
// (include/mi355_mosaic.h, "lens self-calibration"), written once for both compilers, and the loop's interface to whoever forms the blocks.
// Every operation is a separately rounded double operation in the header's order (the build's -ffp-contract=off is part of the contract).
#pragma once
#include "tie_blocks.h"

constexpr int MI_CAL_ROW = 14;                   // a tie's row [d rx / d (h0..h7, k1, k2, p1, p2, k3) | -rx] (and the same of ry)

// one side of a tie: the undistorted point U_theta(xo, yo) in normalised coordinates, dU/dtheta, and whether the point is good
struct CalSide { double x, y, gx[5], gy[5]; bool good; };

// lens::distort's terms at (x, y), in double
MI_TIE_HD inline void mi_cal_terms(const mi355_camera& c, double x, double y, double& xx, double& yy, double& xy, double& r2, double& a1, double& rad,
                                   double& tx, double& ty) {
    xx = x * x; yy = y * y; xy = x * y; r2 = xx + yy; a1 = xy + xy;
    double t = r2 * c.k3;
    t = c.k2 + t; t = r2 * t; t = c.k1 + t; t = r2 * t;
    rad = 1.0 + t;
    tx = (c.p1 * a1) + (c.p2 * (r2 + (xx + xx)));
    ty = (c.p1 * (r2 + (yy + yy))) + (c.p2 * a1);
}

MI_TIE_HD inline void mi_cal_undistort(const mi355_camera& c, double xo, double yo, CalSide& s) {
    const double xd = (xo - c.cx) / c.fx, yd = (yo - c.cy) / c.fy;
    double x = xd, y = yd, dx = 0.0, dy = 0.0, xx, yy, xy, r2, a1, rad, tx, ty;
    for (int it = 0; it < MI355_CALIB_STEPS; it++) {
        mi_cal_terms(c, x, y, xx, yy, xy, r2, a1, rad, tx, ty);
        const double inv = 1.0 / rad;
        const double xn = (xd - tx) * inv, yn = (yd - ty) * inv;
        dx = xn - x; dy = yn - y;
        x = xn; y = yn;
    }
    mi_cal_terms(c, x, y, xx, yy, xy, r2, a1, rad, tx, ty);
    double dr = r2 * c.k3;
    dr = 3.0 * dr; dr = (c.k2 + c.k2) + dr; dr = r2 * dr; dr = c.k1 + dr;
    const double d2 = dr + dr, x2 = x + x, y2 = y + y;
    const double a11 = (rad + d2 * xx) + ((c.p1 * y2) + (c.p2 * (6.0 * x)));
    const double a12 = (d2 * xy) + ((c.p1 * x2) + (c.p2 * y2));
    const double a22 = (rad + d2 * yy) + ((c.p1 * (6.0 * y)) + (c.p2 * x2));
    const double det = a11 * a22 - a12 * a12;
    const double idet = 1.0 / det;
    const double r4 = r2 * r2, r6 = r4 * r2;
    const double ex[5] = {x * r2, x * r4, a1, r2 + (xx + xx), x * r6};
    const double ey[5] = {y * r2, y * r4, r2 + (yy + yy), a1, y * r6};
    for (int m = 0; m < 5; m++) {
        s.gx[m] = -((a22 * ex[m] - a12 * ey[m]) * idet);
        s.gy[m] = -((a11 * ey[m] - a12 * ex[m]) * idet);
    }
    s.x = x; s.y = y;
    s.good = mi_finite(x) && mi_finite(y) && mi_finite(idet) && (dx < 0.0 ? -dx : dx) <= MI355_CALIB_TOL && (dy < 0.0 ? -dy : dy) <= MI355_CALIB_TOL;
}

// image j's side through the state h: columns 0..7 of the two rows, the projected point, and dU_b/dtheta chained through the homography
struct CalChain { double X[8], Y[8], px, py, cx[5], cy[5]; bool good; };

MI_TIE_HD inline void mi_cal_chain(const mi355_camera& c, const double* h, const CalSide& b, CalChain& o) {
    const double w = (h[6] * b.x + h[7] * b.y) + 1.0;
    const double u = (h[0] * b.x + h[1] * b.y) + h[2];
    const double v = (h[3] * b.x + h[4] * b.y) + h[5];
    const double q1 = 1.0 / w;
    const double qx = b.x * q1, qy = b.y * q1, px = u * q1, py = v * q1;
    o.X[0] = -(c.fx * qx); o.X[1] = -(c.fx * qy); o.X[2] = -(c.fx * q1); o.X[3] = 0.0; o.X[4] = 0.0; o.X[5] = 0.0; o.X[6] = c.fx * (px * qx); o.X[7] = c.fx * (px * qy);
    o.Y[0] = 0.0; o.Y[1] = 0.0; o.Y[2] = 0.0; o.Y[3] = -(c.fy * qx); o.Y[4] = -(c.fy * qy); o.Y[5] = -(c.fy * q1); o.Y[6] = c.fy * (py * qx); o.Y[7] = c.fy * (py * qy);
    const double dxu = (h[0] - px * h[6]) * q1, dxv = (h[1] - px * h[7]) * q1;
    const double dyu = (h[3] - py * h[6]) * q1, dyv = (h[4] - py * h[7]) * q1;
    for (int m = 0; m < 5; m++) {
        o.cx[m] = dxu * b.gx[m] + dxv * b.gy[m];
        o.cy[m] = dyu * b.gx[m] + dyv * b.gy[m];
    }
    o.px = px; o.py = py;
    o.good = b.good && mi_finite(px) && mi_finite(py);
}

// image i's side closes the rows: columns 8..12 and the negated residual (X and Y point at columns 8..13)
MI_TIE_HD inline void mi_cal_close(const mi355_camera& c, const CalSide& a, double px, double py, const double* cx, const double* cy, double* X, double* Y) {
    for (int m = 0; m < 5; m++) {
        X[m] = c.fx * (a.gx[m] - cx[m]);
        Y[m] = c.fy * (a.gy[m] - cy[m]);
    }
    X[5] = c.fx * (px - a.x);
    Y[5] = c.fy * (py - a.y);
}

// is the record used, as far as a block entry point can tell (h: the record's eight state values)
MI_TIE_HD inline bool mi_cal_used(int accepted, int n_in, int i, int j, int min_ties, const double* h) {
    if (!accepted || n_in < min_ties || n_in > MI355_MAX_SELECTED || i == j || i < 0 || j < 0) return false;
    for (int k = 0; k < 8; k++) if (!mi_finite(h[k])) return false;
    return true;
}

// what the loop reads of a record itself: the rest is the block former's business
struct CalibHead { int32_t i, j, n_in; float H[9]; };

// whoever holds the records of the loop: the accepted ones, in record order
struct CalibSource {
    virtual ~CalibSource() {}
    virtual int count() = 0;
    virtual int heads(CalibHead* out, std::string& err) = 0;                          // count() heads
    virtual int blocks(const double* h8, const mi355_camera& cam, int min_ties, const mi355_pair_calib_block** out, std::string& err) = 0;     // count() blocks
    virtual int record(int p, mi355_pair_result* out, std::string& err) = 0;          // a copy of record p (to name a bad tie)
};
int mi_calibrate_lens(CalibSource& src, const mi355_camera* start, const mi355_calib_params* params, mi355_camera* out, mi355_calib_report* report,
                      std::string& err);
// argument checks that need no records (shared by the three forms; the dev form runs them before it touches the device)
int mi_calib_check(const char* who, const mi355_camera* cam, const mi355_calib_params* params, std::string& err);
int mi_calib_check_blocks(const char* who, int n, const void* records, const double* h8, const mi355_camera* cam, int min_ties, const void* out, std::string& err);
