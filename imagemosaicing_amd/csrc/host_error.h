// csrc/host_error.h -- the one declaration of mi_set_host_error, for units with (common.h) and without HIP (gain_solve.cpp)
#pragma once
#include <string>
void mi_set_host_error(const std::string& s);       // api.hip: what mi355_last_error(NULL) returns (calls without a ctx)
