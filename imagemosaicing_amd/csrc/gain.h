// csrc/gain.h -- what gain.hip (kernels and launchers) takes from gain_solve.cpp (host only: parameter and pair-list checks, the two solves).
// err receives the refusal without a prefix; the caller names itself in front of it.
#pragma once
#include "../../include/mi355_mosaic.h"
#include <functional>
#include <string>
#include <utility>
#include <vector>

namespace mi_gain {

constexpr int MAX_FRAMES = 65535;
constexpr int MAX_GRID = 16;                  // block gains: cells per axis

// A symmetric positive definite system on a graph, A = diag(diag) + off[q] at (u_q, v_q) and (v_q, u_q) for the edges in list order, solved as
// the gain solves need it: reverse Cuthill-McKee order, envelope Cholesky, one step of iterative refinement; single-threaded double in a
// fixed order, so the same bits on every call.  build once per graph, solve per right-hand side and set of values.
struct EnvelopeGraph {
    int m = 0;
    double work = 0.0;                          // multiply-adds of one factorisation
    std::vector<std::pair<int, int>> edges;
    std::vector<int> order, pos, fst;
    std::vector<size_t> rp;
    std::vector<double> E, r, d, xp;
    void build(int m, const std::vector<std::pair<int, int>>& edges);
    // x (m values, unknown order) or, where a pivot is not positive, the unknown it belongs to; -1: solved
    int solve(const std::vector<double>& diag, const std::vector<double>& off, const std::vector<double>& rhs, std::vector<double>& x);
};

bool check_frames_n(int n, std::string& err);
bool check_pairs(const std::function<void(int, int&, int&)>& pair_at, int n_pairs, int n, std::string& err);   // pair_at(p, a, b) gives pair p
inline auto flat_pairs(const int32_t* ab) { return [ab](int p, int& a, int& b) { a = ab[2 * p]; b = ab[2 * p + 1]; }; }        // a, b, a, b, ...
bool check_params(float sigma_n, float sigma_g, int channels, const int* step, std::string& err);   // step == NULL: a call that takes no step
bool check_grid(int gx, int gy, std::string& err);
bool check_block_params(const mi355_block_gain_params& p, bool need_step, std::string& err);
int solve_gains(const mi355_gain_pair_stats* ps, int n_pairs, const int64_t* cover, int n, const mi355_gain_params& prm, float* gains, std::string& err);
int solve_block_gains(const mi355_block_gain_stats* rs, int64_t n_recs, const int32_t* pairs_ab, int n_pairs, const int64_t* cell_cover, int n,
                      const mi355_block_gain_params& prm, float* gains, std::string& err);

}  // namespace mi_gain
