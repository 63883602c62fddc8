// csrc/sharp_solve.cpp -- the host half of frame sharpness (include/mi355_mosaic.h, "frame sharpness"): the parameter and record checks, the
// solve that turns pairwise energy ratios into one log sharpness per frame, and the flag-and-select step.  Host-only code, no device work;
// sharp.hip holds the kernel and its launchers and takes what it needs from here through sharp.h.
//
//   mi355_solve_sharpness      single-threaded double: the normal equations of the header over the frames in a usable pair, in pair-list
//                              order, solved by gain_solve.cpp's EnvelopeGraph (reverse Cuthill-McKee, envelope Cholesky, one step of
//                              iterative refinement).  Fixed order throughout: the same bits every call.
//   mi355_select_sharp_frames  the solve, then rel against the partners' lower median, the blurred frames by ascending (rel, index), and
//                              per candidate one breadth-first walk over the kept frames of its component without it.
#include "sharp.h"
#include "gain.h"
#include "host_error.h"
#include "kept_graph.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace mi_sharp {

using mi_gain::check_frames_n;
using mi_gain::check_pairs;
using mi_gain::EnvelopeGraph;

bool check_sharp_params(const mi355_sharp_params& p, bool need_step, std::string& err) {
    if (need_step && (p.step < 1 || p.step > 64)) { err = "step=" + std::to_string(p.step) + " outside [1, 64]"; return false; }
    if (!(p.prior > 0.0f) || !std::isfinite(p.prior)) { err = "prior=" + std::to_string(p.prior) + " must be > 0"; return false; }
    if (!(p.blur_ratio > 0.0f) || !(p.blur_ratio <= 1.0f)) { err = "blur_ratio=" + std::to_string(p.blur_ratio) + " outside (0, 1]"; return false; }
    return true;
}

namespace {

bool check_records(const mi355_sharp_pair_stats* ps, int n_pairs, int n, std::string& err) {
    if (!check_pairs([&](int p, int& a, int& b) { a = ps[p].a; b = ps[p].b; }, n_pairs, n, err)) return false;
    for (int p = 0; p < n_pairs; p++) {
        const mi355_sharp_pair_stats& s = ps[p];
        const int64_t v[5] = {s.n, s.e_a, s.e_b, s.s_a, s.s_b};
        const char* name[5] = {"n", "e_a", "e_b", "s_a", "s_b"};
        for (int i = 0; i < 5; i++)
            if (v[i] < 0) { err = "pair " + std::to_string(p) + " (" + std::to_string(s.a) + ", " + std::to_string(s.b) + "): " + name[i] + "=" + std::to_string(v[i]) + " < 0"; return false; }
    }
    return true;
}

bool usable_pair(const mi355_sharp_pair_stats& s) { return s.n > 0 && s.e_a > 0 && s.e_b > 0 && s.s_a > 0 && s.s_b > 0; }

// per frame the frames it shares a usable pair with, in pair-list order
std::vector<std::vector<int>> partners_of(const mi355_sharp_pair_stats* ps, int n_pairs, int n, const char* usable) {
    std::vector<std::vector<int>> part((size_t)n);
    for (int p = 0; p < n_pairs; p++)
        if (usable[p]) { part[ps[p].a].push_back(ps[p].b); part[ps[p].b].push_back(ps[p].a); }
    return part;
}

}  // namespace

int solve_sharpness(const mi355_sharp_pair_stats* ps, int n_pairs, int n, const mi355_sharp_params& prm, double* l_out, double* rel_out, char* usable_out,
                    std::string& err) {
    if (!check_frames_n(n, err) || !check_sharp_params(prm, false, err)) return MI355_ERR_ARG;
    if (n_pairs < 0 || (n_pairs > 0 && !ps)) { err = "NULL argument or n_pairs < 0"; return MI355_ERR_ARG; }
    if (!check_records(ps, n_pairs, n, err)) return MI355_ERR_ARG;
    const double prior = (double)prm.prior;
    std::vector<char> usable((size_t)std::max(n_pairs, 1), 0);
    std::vector<int> live;
    std::vector<int> idx((size_t)n, -1), node;
    for (int p = 0; p < n_pairs; p++)
        if (usable_pair(ps[p])) { usable[p] = 1; live.push_back(p); }
    {
        std::vector<char> active((size_t)n, 0);
        for (int p : live) { active[ps[p].a] = 1; active[ps[p].b] = 1; }
        for (int k = 0; k < n; k++) if (active[k]) { idx[k] = (int)node.size(); node.push_back(k); }
    }
    const int m = (int)node.size();
    std::vector<double> l((size_t)n, 0.0);
    if (m > 0) {
        // the normal equations in pair-list order: A[a][a] += n, A[b][b] += n, A[a][b] -= n, rhs[a] += n d, rhs[b] -= n d; then A[k][k] += prior W_k
        std::vector<std::pair<int, int>> edges;
        std::vector<double> W((size_t)m, 0.0), diag((size_t)m), rhs((size_t)m, 0.0), off, x;
        edges.reserve(live.size()); off.reserve(live.size());
        for (int p : live) {
            const mi355_sharp_pair_stats& s = ps[p];
            const double nn = (double)s.n;
            const double d = 0.5 * (std::log((double)s.e_a) - std::log((double)s.e_b)) - (std::log((double)s.s_a) - std::log((double)s.s_b));
            const int u = idx[s.a], v = idx[s.b];
            edges.emplace_back(u, v);
            off.push_back(-nn);
            W[u] += nn; W[v] += nn;
            rhs[u] += nn * d; rhs[v] -= nn * d;
        }
        for (int i = 0; i < m; i++) diag[i] = W[i] + prior * W[i];
        EnvelopeGraph eg;
        eg.build(m, edges);
        const int bad = eg.solve(diag, off, rhs, x);
        if (bad >= 0) { err = "the normal equations are not positive definite at frame " + std::to_string(node[bad]); return MI355_ERR_FAILED; }
        for (int i = 0; i < m; i++) l[node[i]] = x[i];
    }
    if (rel_out) {
        const auto part = partners_of(ps, n_pairs, n, usable.data());
        std::vector<double> lp;
        for (int k = 0; k < n; k++) {
            if (part[k].empty()) { rel_out[k] = 0.0; continue; }
            lp.clear();
            for (int q : part[k]) lp.push_back(l[q]);
            std::sort(lp.begin(), lp.end());
            rel_out[k] = l[k] - lp[(lp.size() - 1) / 2];                 // the lower median
        }
    }
    if (l_out) std::copy(l.begin(), l.end(), l_out);
    if (usable_out) std::copy(usable.begin(), usable.begin() + n_pairs, usable_out);
    return MI355_OK;
}

int select_sharp_frames(const mi355_sharp_pair_stats* ps, int n_pairs, int n, const mi355_sharp_params& prm, uint8_t* status, float* sharp, std::string& err) {
    if (!status) { err = "NULL argument or n_pairs < 0"; return MI355_ERR_ARG; }
    if (!check_frames_n(n, err)) return MI355_ERR_ARG;                // before anything is sized by n
    std::vector<double> l((size_t)std::max(n, 1)), rel((size_t)std::max(n, 1));
    std::vector<char> usable((size_t)std::max(n_pairs, 1), 0);
    const int rc = solve_sharpness(ps, n_pairs, n, prm, l.data(), rel.data(), usable.data(), err);
    if (rc != MI355_OK) return rc;
    const auto part = partners_of(ps, n_pairs, n, usable.data());
    const double limit = std::log((double)prm.blur_ratio);
    std::vector<int> blurred;
    for (int k = 0; k < n; k++) {
        status[k] = part[k].empty() ? MI355_SHARP_NO_PAIR : MI355_SHARP_KEPT;
        if (!part[k].empty() && rel[k] < limit) blurred.push_back(k);
    }
    std::stable_sort(blurred.begin(), blurred.end(), [&](int x, int y) { return rel[x] < rel[y]; });     // ascending rel, lower index first on ties
    // the components of the usable-pair graph and how many kept frames each still holds (kept_graph.h)
    mi_graph::KeptGraph g;
    g.build(part);
    for (size_t i = 0; i < blurred.size(); i++) {
        const int k = blurred[i];
        // the kept frames of k's component without k: connected when a walk from one of k's kept partners reaches them all.  The last kept
        // frame of a component (no kept partner) is never dropped.
        const int reached = g.reach_without(k);
        if (reached > 0 && reached == g.others_kept(k)) { status[k] = MI355_SHARP_DROPPED; g.drop(k); }
        else status[k] = MI355_SHARP_CUT_VERTEX;
    }
    if (sharp)
        for (int k = 0; k < n; k++) sharp[k] = part[k].empty() ? 1.0f : (float)std::exp(l[k]);
    return MI355_OK;
}

}  // namespace mi_sharp

using namespace mi_sharp;

extern "C" void mi355_default_sharp_params(mi355_sharp_params* p) {
    if (!p) return;
    p->prior = 0.01f; p->blur_ratio = 0.58f; p->step = 8; p->reserved = 0;
}

extern "C" int mi355_solve_sharpness(const mi355_sharp_pair_stats* pair_stats, int n_pairs, int n, const mi355_sharp_params* p, float* sharp, double* rel) {
    mi355_sharp_params dp;
    if (!p) { mi355_default_sharp_params(&dp); p = &dp; }
    std::string err;
    int rc = MI355_ERR_ARG;
    if (!sharp) err = "NULL argument or n_pairs < 0";
    else if (check_frames_n(n, err)) {                                 // before anything is sized by n
        std::vector<double> l((size_t)std::max(n, 1));
        std::vector<char> usable((size_t)std::max(n_pairs, 1), 0);
        rc = solve_sharpness(pair_stats, n_pairs, n, *p, l.data(), rel, usable.data(), err);
        if (rc == MI355_OK) {
            std::vector<char> in_pair((size_t)n, 0);
            for (int q = 0; q < n_pairs; q++) if (usable[q]) { in_pair[pair_stats[q].a] = 1; in_pair[pair_stats[q].b] = 1; }
            for (int k = 0; k < n; k++) sharp[k] = in_pair[k] ? (float)std::exp(l[k]) : 1.0f;
        }
    }
    if (rc != MI355_OK) mi_set_host_error("solve_sharpness: " + err);
    return rc;
}

extern "C" int mi355_select_sharp_frames(const mi355_sharp_pair_stats* pair_stats, int n_pairs, int n, const mi355_sharp_params* p, uint8_t* status, float* sharp) {
    mi355_sharp_params dp;
    if (!p) { mi355_default_sharp_params(&dp); p = &dp; }
    std::string err;
    const int rc = select_sharp_frames(pair_stats, n_pairs, n, *p, status, sharp, err);
    if (rc != MI355_OK) mi_set_host_error("select_sharp_frames: " + err);
    return rc;
}
