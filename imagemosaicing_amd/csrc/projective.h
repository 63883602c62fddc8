// csrc/projective.h -- what the projective refinement's host loop (projective_solve.cpp) and its device half (projective.hip) share: the
// arithmetic of one side of a point, written once for both compilers, and the loop's interface to whoever forms the blocks.
#pragma once
#include "tie_blocks.h"

constexpr int MI_PROJ_ROW = 17;                  // a point's row [Rx | rx] (and [Ry | ry]): the 153 sums of a block are the lower triangle of X X^T + Y Y^T

// one side of a point under the parameters h (include/mi355_mosaic.h, "Side of a point"): the eight entries of Jx and Jy times `sign`
// (+1 for image i's side, -1 for image j's: a negation is exact), and U, V
MI_TIE_HD inline void mi_proj_side(const double* h, double x, double y, double sign, double* jx, double* jy, double& U, double& V) {
    const double w = (h[6] * x + h[7] * y) + 1.0;
    const double u = (h[0] * x + h[1] * y) + h[2];
    const double v = (h[3] * x + h[4] * y) + h[5];
    const double qx = x / w, qy = y / w, q1 = 1.0 / w;
    U = u / w; V = v / w;
    jx[0] = sign * qx; jx[1] = sign * qy; jx[2] = sign * q1; jx[3] = 0.0; jx[4] = 0.0; jx[5] = 0.0; jx[6] = sign * -(U * qx); jx[7] = sign * -(U * qy);
    jy[0] = 0.0; jy[1] = 0.0; jy[2] = 0.0; jy[3] = sign * qx; jy[4] = sign * qy; jy[5] = sign * q1; jy[6] = sign * -(V * qx); jy[7] = sign * -(V * qy);
}

// is the record used, as far as a block entry point can tell (part: 0 no part, 1 takes part, 2 takes part and is fixed)?  *keep_n = the n_in
// the block carries: the record's own for a used record and for a malformed accepted one, else 0
MI_TIE_HD inline bool mi_proj_used(int accepted, int n_in, int i, int j, const uint8_t* part, int n_images, int* keep_n) {
    *keep_n = 0;
    if (!accepted || n_in < 1) return false;
    if (n_in > MI355_MAX_SELECTED || i < 0 || i >= n_images || j < 0 || j >= n_images) { *keep_n = n_in; return false; }
    if (i == j || !part[i] || !part[j] || (part[i] == 2 && part[j] == 2)) return false;
    *keep_n = n_in;
    return true;
}

// whoever forms the blocks for the loop: blocks of its records (accepted ones, in record order) at the parameters h8
struct ProjectiveSource {
    virtual ~ProjectiveSource() {}
    virtual int blocks(const double* h8, const uint8_t* part, int n_images, const mi355_pair_normal_block** out, int* n, std::string& err) = 0;
};
// the loop of include/mi355_mosaic.h on such a source; err receives the message of an error return
int mi_projective_refine(ProjectiveSource& src, int n_images, const int32_t* w, const int32_t* h, const int32_t* fixed, const int32_t* label,
                         const mi355_image_transform* start, const mi355_projective_params* params, mi355_image_transform* out,
                         mi355_projective_report* report, std::string& err);
// argument checks that need no records (shared by the three forms; the dev form runs them before it touches the device)
int mi_projective_check(int n_images, const int32_t* w, const int32_t* h, const mi355_image_transform* start, const mi355_projective_params* params,
                        mi355_image_transform* out, std::string& err);
