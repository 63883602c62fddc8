// csrc/tie_blocks.h -- what the tie-driven refinements (projective.*, calib.*) share on the host and with their device halves: the lower
// triangle of X X^T + Y Y^T that a block is made of, the runner of host blocks, the flat list's run splitter, and the Levenberg-Marquardt
// schedule with its driver.  Plain C++ (host units include it without HIP); the device skeleton of the blocks is tie_blocks_dev.h.
#pragma once
#include "../../include/mi355_mosaic.h"
#include "envelope_chol.h"
#include <cmath>
#include <string>

#ifdef __HIP__
#define MI_TIE_HD __host__ __device__
#else
#define MI_TIE_HD
#endif

MI_TIE_HD inline bool mi_finite(double v) { return __builtin_isfinite(v); }

// A block's sums are the lower triangle of X X^T + Y Y^T over its ties' rows X[ROW], Y[ROW]: sum s = r (r + 1) / 2 + c, c <= r.  The first
// ROW (ROW - 1) / 2 are the block's N, the next ROW - 1 its g (row ROW - 1), the last one its cost.
MI_TIE_HD inline void mi_tri_rc(int s, int& r, int& c) {
    r = 0;
    while ((r + 1) * (r + 2) / 2 <= s) r++;
    c = s - r * (r + 1) / 2;
}
template <int ROW, class Block> MI_TIE_HD inline void mi_tri_store(Block& o, int s, double v) {
    constexpr int NN = ROW * (ROW - 1) / 2, NG = ROW - 1;
    if (s < NN) o.N[s] = v; else if (s < NN + NG) o.g[s - NN] = v; else o.cost = v;
}
// the host's sums: every sum takes its ties in order, two separately rounded products per tie (the device kernel's chain, the same bits)
// (inlined into the caller's loop over the ties, where S, X and Y are its own arrays: out of line the stores to S would make it reload X and Y)
template <int ROW> __attribute__((always_inline)) inline void mi_tri_add(double* S, const double* X, const double* Y) {
    int s = 0;
    for (int r = 0; r < ROW; r++)
        for (int c = 0; c <= r; c++, s++) {
            double v = S[s];
            v = v + X[r] * X[c];
            v = v + Y[r] * Y[c];
            S[s] = v;
        }
}
template <int ROW, class Block> inline void mi_tri_split(const double* S, Block& o) {
    constexpr int NN = ROW * (ROW - 1) / 2, NG = ROW - 1;
    memcpy(o.N, S, sizeof(double) * NN);
    memcpy(o.g, S + NN, sizeof(double) * NG);
    o.cost = S[NN + NG];
}

// host blocks of n records, one(p) each, on up to 8 threads once the records' weights add up to more than `threshold`: a thread owns whole
// records, so every sum keeps its order
template <class Weight, class One> void mi_host_blocks(size_t n, size_t threshold, Weight&& weight, One&& one) {
    size_t total = 0;
    for (size_t p = 0; p < n; p++) total += weight(p);
    parallel_chunks(n, total > threshold ? (host_threads() < 8 ? host_threads() : 8) : 1, [&](size_t lo, size_t hi) { for (size_t p = lo; p < hi; p++) one(p); });
}

// the flat list: the entries of one image pair are consecutive (mi355_results_to_match_pairs); fn(p, q) for every run [p, q) of equal
// (ptA_i, ptB_i), cut after `cap` entries (cap <= 0: never cut)
template <class F> void mi_flat_runs(const mi355_match_point_pairs* v, int n, int cap, F&& fn) {
    for (int p = 0; p < n;) {
        int q = p;
        while (q < n && (cap <= 0 || q - p < cap) && v[q].ptA_i == v[p].ptA_i && v[q].ptB_i == v[p].ptB_i) q++;
        fn(p, q);
        p = q;
    }
}

// the Levenberg-Marquardt schedule of both loops (the fields of that name in mi355_projective_params and mi355_calib_params)
struct LmSchedule { int max_iters; double lambda0, lambda_up, lambda_down, min_rel_decrease; };
template <class P> LmSchedule mi_lm_schedule(const P& p) { return LmSchedule{p.max_iters, p.lambda0, p.lambda_up, p.lambda_down, p.min_rel_decrease}; }

inline int mi_lm_check(const char* who, const LmSchedule& s, std::string& err) {
    auto bad = [&](const char* name, double v, const char* rule) { err = std::string(who) + ": " + name + " = " + std::to_string(v) + " (" + rule + ")"; return MI355_ERR_ARG; };
    if (s.max_iters < 0) { err = std::string(who) + ": max_iters = " + std::to_string(s.max_iters) + " (not negative)"; return MI355_ERR_ARG; }
    if (!mi_finite(s.lambda0) || s.lambda0 < 0.0) return bad("lambda0", s.lambda0, "finite, not negative");
    if (!mi_finite(s.lambda_up) || s.lambda_up <= 1.0) return bad("lambda_up", s.lambda_up, "finite, above 1");
    if (!mi_finite(s.lambda_down) || s.lambda_down <= 1.0) return bad("lambda_down", s.lambda_down, "finite, above 1");
    if (!mi_finite(s.min_rel_decrease) || s.min_rel_decrease < 0.0) return bad("min_rel_decrease", s.min_rel_decrease, "finite, not negative");
    return MI355_OK;
}

// The loop from the cost c0 at lambda0.  A trial: try_step(lambda, c, c2, rc) forms the damped step and the cost c2 after it; false: no
// step (a failed factorisation, a trial that may not be taken); rc other than MI355_OK ends the loop with that code.  A step is accepted
// when c2 is finite and below c: accept() makes the trial state the current one and lambda goes down, else lambda goes up.  The loop ends
// after max_iters trials, at a zero cost, at lambda above 1e16, or after an accepted step whose relative decrease is below min_rel_decrease.
struct LmState { int trials = 0, accepted = 0; double lambda = 0.0, c = 0.0; };
template <class Try, class Accept> int mi_lm_run(const LmSchedule& s, double c0, LmState& st, Try&& try_step, Accept&& accept) {
    st.lambda = s.lambda0; st.c = c0;
    double &lambda = st.lambda, &c = st.c;
    while (st.trials < s.max_iters && c != 0.0 && lambda <= 1e16) {
        st.trials++;
        double c2 = 0.0;
        int rc = MI355_OK;
        const bool ok = try_step(lambda, c, c2, rc);
        if (rc != MI355_OK) return rc;
        if (ok && mi_finite(c2) && c2 < c) {
            st.accepted++;
            accept();
            lambda = lambda / s.lambda_down;
            const double rel = (c - c2) / c;
            c = c2;
            if (rel < s.min_rel_decrease) break;
        } else lambda = lambda * s.lambda_up;
    }
    return MI355_OK;
}
