// csrc/verify.h -- what pair verification's kernels, their host twins (verify.hip) and its host loop (verify_loop.cpp) share
// (include/mi355_mosaic.h, "pair verification"): the arithmetic of an edge, of a triangle and of a tie's residual, written once for both
// compilers, and the loop's interface to whoever forms the records.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include "../../include/mi355_mosaic.h"

#ifdef __HIP__
#define VF_HD __host__ __device__ inline
#else
#define VF_HD inline
#endif

constexpr int VF_MAX_IMAGES = 65535;
constexpr double VF_DBL_MAX = 1.79769313486231570815e308;

VF_HD bool vf_finite(double v) { return v >= -VF_DBL_MAX && v <= VF_DBL_MAX; }          // false for NaN
VF_HD bool vf_den_ok(double d) { return d > 0.0 && d <= VF_DBL_MAX; }

VF_HD bool vf_usable(int accepted, int n_in, int i, int j, int n_images) {
    return accepted != 0 && n_in >= 1 && n_in <= MI355_MAX_SELECTED && i >= 0 && j >= 0 && i < n_images && j < n_images && i != j;
}

// P(M, x, y) of the header; false on a den failure
VF_HD bool vf_map(const double* M, double x, double y, double& X, double& Y) {
    const double den = (M[6] * x + M[7] * y) + M[8];
    X = ((M[0] * x + M[1] * y) + M[2]) / den;
    Y = ((M[3] * x + M[4] * y) + M[5]) / den;
    return vf_den_ok(den);
}

// the total order of float bit patterns as unsigned keys (-0 below +0): minimum and maximum by it do not depend on the order of the values
VF_HD uint32_t vf_key(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
VF_HD float vf_unkey(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// what is stored of a NaN: the one quiet NaN 0x7ff8000000000000 (sign and payload of an arithmetic NaN differ between processors)
VF_HD double vf_canon(double v) {
    if (v == v) return v;
    const uint64_t q = 0x7ff8000000000000ull;
    double r;
    __builtin_memcpy(&r, &q, 8);
    return r;
}

// F, B and the TESTABLE bit of a usable record's edge from its H (local registration's adjugate formula applied to F)
VF_HD void vf_edge_matrices(const float* H, mi355_pair_edge& o) {
    for (int q = 0; q < 8; q++) o.F[q] = vf_canon((double)H[q]);
    o.F[8] = 1.0;
    const double a = o.F[0], b = o.F[1], c = o.F[2], d = o.F[3], e = o.F[4], f = o.F[5], g = o.F[6], h = o.F[7], i = o.F[8];
    double A[9];
    A[0] = e * i - f * h;  A[1] = c * h - b * i;  A[2] = b * f - c * e;
    A[3] = f * g - d * i;  A[4] = a * i - c * g;  A[5] = c * d - a * f;
    A[6] = d * h - e * g;  A[7] = b * g - a * h;  A[8] = a * e - b * d;
    const double det = (a * A[0] + b * A[3]) + c * A[6];
    bool fin = true;
    for (int q = 0; q < 9; q++) {
        o.B[q] = vf_canon(A[q] / det);
        fin = fin && vf_finite(o.F[q]) && vf_finite(o.B[q]);
    }
    o.flags = MI355_EDGE_USABLE | (fin ? MI355_EDGE_TESTABLE : 0);
}

// one triangle of edge e: Mkj maps e's frame j to k, Mik maps k to e's frame i.  false: a den failure (E is then not formed)
VF_HD bool vf_triangle(const mi355_pair_edge& e, const double* Mkj, const double* Mik, double& E) {
    const double x0 = (double)e.box[0], y0 = (double)e.box[1], x1 = (double)e.box[2], y1 = (double)e.box[3];
    const double xm = (x0 + x1) * 0.5, ym = (y0 + y1) * 0.5;
    bool ok = true;
    E = 0.0;
    for (int q = 0; q < 9; q++) {
        const int qx = q % 3, qy = q / 3;
        const double x = qx == 0 ? x0 : (qx == 1 ? xm : x1), y = qy == 0 ? y0 : (qy == 1 ? ym : y1);
        double dx, dy, tx, ty, lx, ly;
        ok = vf_map(e.F, x, y, dx, dy) && ok;
        ok = vf_map(Mkj, x, y, tx, ty) && ok;
        ok = vf_map(Mik, tx, ty, lx, ly) && ok;
        const double ex = lx - dx, ey = ly - dy;
        const double e2 = ex * ex + ey * ey;
        if (q == 0 || e2 > E || e2 != e2) E = e2;             // the largest; a NaN stays
    }
    return ok;
}

// a triangle's verdict into the edge's three results
VF_HD void vf_count(bool den_ok, double E, double tol2, int& n_ok, int& n_bad, double& min_e2) {
    if (!den_ok) { n_bad++; return; }
    if (E < min_e2) min_e2 = E;
    if (vf_finite(E) && E <= tol2) n_ok++; else n_bad++;
}

// an adjacency entry: the neighbour frame, and the edge index with the bit "the list's frame is the edge's i"
struct VfAdj { int32_t nbr; uint32_t edge2; };

// r2 of one tie under the doubles Hi, Hj of two frames' transforms; -1.0 marks a den failure (an r2 is never negative)
VF_HD double vf_tie_r2(const double* Hi, const double* Hj, double ax, double ay, double bx, double by) {
    double cix, ciy, cjx, cjy;
    const bool oi = vf_map(Hi, ax, ay, cix, ciy), oj = vf_map(Hj, bx, by, cjx, cjy);
    if (!(oi && oj)) return -1.0;
    const double rx = cjx - cix, ry = cjy - ciy;
    return rx * rx + ry * ry;
}
VF_HD bool vf_measured(int accepted, int n_in, int i, int j, int n_images, const float* h9s, const int32_t* label) {
    if (!vf_usable(accepted, n_in, i, j, n_images)) return false;
    if (label && !(label[i] != 0 && label[j] != 0)) return false;
    return h9s[9 * (size_t)i + 8] != 0.0f && h9s[9 * (size_t)j + 8] != 0.0f;
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
#include <vector>
// the CSR adjacency of the testable edges (row: n_images + 1 offsets); MI355_ERR_ARG with a message for two usable records of one frame pair
int mi_verify_adjacency(const mi355_pair_edge* edges, int n, int n_images, std::vector<int32_t>& row, std::vector<VfAdj>& adj, std::string& err);
// the checks that need no records
int mi_verify_check(int n_pairs, int n_images, const mi355_verify_params* params, mi355_verify_params& p, std::string& err);

// whoever forms the records for the loop (n records each, in record order; the arrays stay valid until the next call of the same member)
struct VerifySource {
    virtual ~VerifySource() {}
    virtual int moments(const mi355_pair_moments** out, std::string& err) = 0;
    virtual int edges(const mi355_pair_edge** out, std::string& err) = 0;
    virtual int cycles(const mi355_pair_edge* edges, const std::vector<int32_t>& row, const std::vector<VfAdj>& adj, double cycle_tol,
                       const mi355_pair_cycle** out, std::string& err) = 0;
    virtual int residuals(const float* h9s, const int32_t* label, const mi355_pair_residual** out, std::string& err) = 0;
};
// stages 1 to 3 on such a source; demote[p] = 1 for the records stage 4 demotes
int mi_verify_loop(VerifySource& src, int n_pairs, int n_images, const int32_t* fixed, const mi355_verify_params& p, uint8_t* demote,
                   int32_t* label_out, mi355_image_transform* transforms_out, mi355_verify_report* report, mi355_verify_summary* summary,
                   std::string& err);
