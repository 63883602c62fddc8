// csrc/sharp.h -- what sharp.hip (kernel and launchers) takes from sharp_solve.cpp (host only: parameter checks, the solve, flag and select).
// err receives the refusal without a prefix; the caller names itself in front of it.
#pragma once
#include "../../include/mi355_mosaic.h"
#include <string>

namespace mi_sharp {

bool check_sharp_params(const mi355_sharp_params& p, bool need_step, std::string& err);
// l (n doubles; 0 for a frame in no usable pair), rel (n doubles) and usable (n_pairs flags); any of the three may be NULL
int solve_sharpness(const mi355_sharp_pair_stats* ps, int n_pairs, int n, const mi355_sharp_params& prm, double* l, double* rel, char* usable, std::string& err);
int select_sharp_frames(const mi355_sharp_pair_stats* ps, int n_pairs, int n, const mi355_sharp_params& prm, uint8_t* status, float* sharp, std::string& err);

}  // namespace mi_sharp
