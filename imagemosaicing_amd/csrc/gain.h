// csrc/gain.h -- what gain.hip (kernels and launchers) takes from gain_solve.cpp (host only: parameter and pair-list checks, the two solves).
// err receives the refusal without a prefix; the caller names itself in front of it.
#pragma once
#include "../../include/mi355_mosaic.h"
#include <functional>
#include <string>

namespace mi_gain {

constexpr int MAX_FRAMES = 65535;
constexpr int MAX_GRID = 16;                  // block gains: cells per axis

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
