// csrc/guided_host.cpp -- the host-only pieces of guided matching (include/mi355_mosaic.h, section "guided matching"): the defaults, the candidate
// pairs an alignment proposes (mi355_guided_candidates) and the merge of two record sets (mi355_merge_pair_results).  No ctx, no device.
// Every double operation is a separate operation in the order written (-ffp-contract=off); tests/guided_ref.py holds the numpy twins.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "../../include/mi355_mosaic.h"
#include "host_error.h"

extern "C" void mi355_default_guided_params(mi355_guided_params* p) {
    if (!p) return;
    p->radius = 4.0f; p->max_dist2 = 90000; p->ratio = 0.8f; p->reserved = 0;
}

namespace {

// adjugate (row-major) and determinant of a 3 x 3 matrix
void adj3(const double* t, double* A, double& det) {
    A[0] = t[4] * t[8] - t[5] * t[7]; A[1] = t[2] * t[7] - t[1] * t[8]; A[2] = t[1] * t[5] - t[2] * t[4];
    A[3] = t[5] * t[6] - t[3] * t[8]; A[4] = t[0] * t[8] - t[2] * t[6]; A[5] = t[2] * t[3] - t[0] * t[5];
    A[6] = t[3] * t[7] - t[4] * t[6]; A[7] = t[1] * t[6] - t[0] * t[7]; A[8] = t[0] * t[4] - t[1] * t[3];
    det = t[0] * A[0] + t[1] * A[3] + t[2] * A[6];
}

// points of the 3 x 3 control grid that M carries into [0, w-1] x [0, h-1]
int grid_hits(const double* M, double w1, double h1) {
    const double xs[3] = {0.0, w1 / 2.0, w1}, ys[3] = {0.0, h1 / 2.0, h1};
    int cnt = 0;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const double x = xs[c], y = ys[r];
            const double den = M[6] * x + M[7] * y + M[8];
            const double X = (M[0] * x + M[1] * y + M[2]) / den, Y = (M[3] * x + M[4] * y + M[5]) / den;
            if (X >= 0.0 && X <= w1 && Y >= 0.0 && Y <= h1) cnt++;
        }
    return cnt;
}

// the guide of (i, j) and its control-point count; false: the pair is skipped
bool guide_of(const float* Ti, const float* Tj, double w1, double h1, float* G, int& count) {
    double t[9], u[9], A[9], det;
    for (int k = 0; k < 9; k++) { t[k] = (double)Ti[k]; u[k] = (double)Tj[k]; }
    adj3(t, A, det);
    if (det == 0.0 || !std::isfinite(det)) return false;
    double P[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) P[3 * r + c] = (A[3 * r] * u[c] + A[3 * r + 1] * u[3 + c] + A[3 * r + 2] * u[6 + c]) / det;
    if (P[8] == 0.0 || !std::isfinite(P[8])) return false;
    double g[9], gi[9], A2[9], det2;
    for (int k = 0; k < 9; k++) { G[k] = (float)(P[k] / P[8]); g[k] = (double)G[k]; }
    adj3(g, A2, det2);
    for (int k = 0; k < 9; k++) gi[k] = A2[k] / det2;        // det2 == 0: nothing of frame i lands anywhere (inf / NaN fail the test)
    count = grid_hits(g, w1, h1) + grid_hits(gi, w1, h1);
    return true;
}

}  // namespace

extern "C" int mi355_guided_candidates(int w, int h, int n_images, const float* transforms, const int32_t* have_ij, int n_have, int min_points, int32_t* pairs_ij, float* guides,
                                       int max_pairs, int* n_pairs) {
    if (w < 1 || h < 1) { mi_set_host_error("guided_candidates: frame size " + std::to_string(w) + "x" + std::to_string(h) + " (at least 1x1)"); return MI355_ERR_ARG; }
    if (n_images < 0 || (n_images > 0 && !transforms)) { mi_set_host_error("guided_candidates: n_images=" + std::to_string(n_images) + (n_images < 0 ? " (not negative)" : " with NULL transforms")); return MI355_ERR_ARG; }
    if (n_have < 0 || (n_have > 0 && !have_ij)) { mi_set_host_error("guided_candidates: n_have=" + std::to_string(n_have) + (n_have < 0 ? " (not negative)" : " with a NULL list")); return MI355_ERR_ARG; }
    if (!n_pairs) { mi_set_host_error("guided_candidates: NULL n_pairs"); return MI355_ERR_ARG; }
    if (pairs_ij && max_pairs < 0) { mi_set_host_error("guided_candidates: max_pairs=" + std::to_string(max_pairs) + " (not negative)"); return MI355_ERR_ARG; }
    if (min_points <= 0) min_points = 2;
    std::map<std::pair<int, int>, int> have;
    for (int k = 0; k < n_have; k++) {
        const int a = have_ij[2 * k], b = have_ij[2 * k + 1];
        have[a < b ? std::make_pair(a, b) : std::make_pair(b, a)] = 1;
    }
    const double w1 = (double)(w - 1), h1 = (double)(h - 1);
    std::vector<int32_t> ij;
    std::vector<float> gs;
    for (int i = 0; i < n_images; i++) {
        if (transforms[9 * (size_t)i + 8] == 0.0f) continue;
        for (int j = i + 1; j < n_images; j++) {
            if (transforms[9 * (size_t)j + 8] == 0.0f || have.count(std::make_pair(i, j))) continue;
            float G[9];
            int count = 0;
            if (!guide_of(transforms + 9 * (size_t)i, transforms + 9 * (size_t)j, w1, h1, G, count) || count < min_points) continue;
            ij.push_back(i); ij.push_back(j);
            gs.insert(gs.end(), G, G + 9);
        }
    }
    const int cnt = (int)(ij.size() / 2);
    *n_pairs = cnt;
    if (!pairs_ij) return MI355_OK;
    if (max_pairs < cnt) { mi_set_host_error("guided_candidates: max_pairs=" + std::to_string(max_pairs) + " (the alignment proposes " + std::to_string(cnt) + " pairs)"); return MI355_ERR_ARG; }
    if (cnt > 0) {
        memcpy(pairs_ij, ij.data(), sizeof(int32_t) * ij.size());
        if (guides) memcpy(guides, gs.data(), sizeof(float) * gs.size());
    }
    return MI355_OK;
}

extern "C" int mi355_merge_pair_results(const mi355_pair_result* base, int n_base, const mi355_pair_result* extra, int n_extra, mi355_pair_result* out, int* n_out) {
    if (n_base < 0 || n_extra < 0 || (n_base > 0 && !base) || (n_extra > 0 && !extra) || !n_out || (n_base + n_extra > 0 && !out)) {
        mi_set_host_error("merge_pair_results: n_base=" + std::to_string(n_base) + ", n_extra=" + std::to_string(n_extra) + " (negative, or with a NULL array)");
        return MI355_ERR_ARG;
    }
    if (out != base && n_base > 0) memmove(out, base, sizeof(mi355_pair_result) * (size_t)n_base);
    std::map<std::pair<int, int>, int> at;                  // (i, j) as written -> the record's place in out (the first one of equal pairs)
    for (int k = 0; k < n_base; k++) at.insert(std::make_pair(std::make_pair(out[k].i, out[k].j), k));
    int n = n_base;
    for (int e = 0; e < n_extra; e++) {
        const auto key = std::make_pair(extra[e].i, extra[e].j);
        const auto it = at.find(key);
        if (it == at.end()) { at.insert(std::make_pair(key, n)); out[n++] = extra[e]; }
        else if (extra[e].n_in > out[it->second].n_in) out[it->second] = extra[e];      // equal n_in: the record already there stays
    }
    *n_out = n;
    return MI355_OK;
}
