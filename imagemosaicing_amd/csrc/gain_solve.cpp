// csrc/gain_solve.cpp -- the host half of exposure gain compensation (include/mi355_mosaic.h, "exposure gain compensation" and "block gain
// compensation"): the checks of parameters and pair lists, and the two solves.  Host-only code, no device work; gain.hip holds the kernels
// and their launchers and takes what it needs from here through gain.h.
//
//   mi355_solve_gains        single-threaded double: the normal equations over the frames that have one, reverse Cuthill-McKee order, an
//                            envelope Cholesky factor and one step of iterative refinement (EnvelopeGraph, which sharp_solve.cpp uses as
//                            well).  Fixed order throughout: the same bits every call.
//   mi355_solve_block_gains  the same solve (solve_nodes) over the nodes (frame, cell), iterating where the envelope would be too costly
//                            (solve_pcg), then the smoothing of each frame's map.
#include "gain.h"
#include "host_error.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <vector>


namespace mi_gain {

// reverse Cuthill-McKee: per component, start at the unvisited node of least degree (lowest index on ties), neighbours by (degree, index);
// then the envelope: row i (permuted) holds columns fst[i] .. i
void EnvelopeGraph::build(int m_, const std::vector<std::pair<int, int>>& edges_) {
    m = m_; edges = edges_;
    std::vector<std::vector<int>> adj((size_t)m);
    for (const auto& e : edges) { adj[e.first].push_back(e.second); adj[e.second].push_back(e.first); }
    for (auto& l : adj) std::sort(l.begin(), l.end());
    order.clear(); order.reserve(m);
    std::vector<char> seen((size_t)m, 0);
    std::vector<int> by_deg(m);
    for (int i = 0; i < m; i++) by_deg[i] = i;
    std::stable_sort(by_deg.begin(), by_deg.end(), [&](int x, int y) { return adj[x].size() < adj[y].size(); });
    for (int s : by_deg) {
        if (seen[s]) continue;
        size_t head = order.size();
        order.push_back(s); seen[s] = 1;
        std::vector<int> nb;
        while (head < order.size()) {
            const int u = order[head++];
            nb.clear();
            for (int v : adj[u]) if (!seen[v]) { nb.push_back(v); seen[v] = 1; }
            std::stable_sort(nb.begin(), nb.end(), [&](int x, int y) { return adj[x].size() < adj[y].size(); });
            order.insert(order.end(), nb.begin(), nb.end());
        }
    }
    std::reverse(order.begin(), order.end());
    pos.assign((size_t)m, 0);
    for (int i = 0; i < m; i++) pos[order[i]] = i;
    fst.assign((size_t)m, 0);
    for (int i = 0; i < m; i++) { int f = i; for (int v : adj[order[i]]) f = std::min(f, pos[v]); fst[i] = f; }
    rp.assign((size_t)m + 1, 0);
    for (int i = 0; i < m; i++) rp[i + 1] = rp[i] + (size_t)(i - fst[i] + 1);
    work = 0.0;
    for (int i = 0; i < m; i++) work += (double)(i - fst[i]) * (double)(i - fst[i]);
    E.clear();
}

int EnvelopeGraph::solve(const std::vector<double>& diag, const std::vector<double>& off, const std::vector<double>& rhs, std::vector<double>& x) {
    E.assign(rp[m], 0.0);
    r.resize((size_t)m); d.resize((size_t)m);
    auto at = [&](int i, int j) -> double& { return E[rp[i] + (size_t)(j - fst[i])]; };   // j in [fst[i], i]
    for (int i = 0; i < m; i++) at(pos[i], pos[i]) = diag[i];
    for (size_t q = 0; q < edges.size(); q++) {
        const int u = pos[edges[q].first], v = pos[edges[q].second];
        if (u > v) at(u, v) += off[q]; else at(v, u) += off[q];
    }
    // envelope Cholesky, row by row
    for (int i = 0; i < m; i++) {
        for (int j = fst[i]; j < i; j++) {
            double s = at(i, j);
            for (int k = std::max(fst[i], fst[j]); k < j; k++) s -= at(i, k) * at(j, k);
            at(i, j) = s / at(j, j);
        }
        double s = at(i, i);
        for (int k = fst[i]; k < i; k++) s -= at(i, k) * at(i, k);
        if (!(s > 0.0)) return order[i];
        at(i, i) = std::sqrt(s);
    }
    auto lsolve = [&](std::vector<double>& b) {              // b := (L L^T)^-1 b, permuted positions
        for (int i = 0; i < m; i++) { double s = b[i]; for (int k = fst[i]; k < i; k++) s -= at(i, k) * b[k]; b[i] = s / at(i, i); }
        for (int i = m - 1; i >= 0; i--) { b[i] /= at(i, i); const double bi = b[i]; for (int k = fst[i]; k < i; k++) b[k] -= at(i, k) * bi; }
    };
    xp.resize((size_t)m);
    for (int i = 0; i < m; i++) xp[pos[i]] = rhs[i];
    lsolve(xp);
    // one step of iterative refinement on the unfactored system: r = rhs - A x
    for (int i = 0; i < m; i++) r[pos[i]] = rhs[i] - diag[i] * xp[pos[i]];
    for (size_t q = 0; q < edges.size(); q++) {
        const int u = pos[edges[q].first], v = pos[edges[q].second];
        r[u] -= off[q] * xp[v]; r[v] -= off[q] * xp[u];
    }
    d = r;
    lsolve(d);
    for (int i = 0; i < m; i++) xp[i] += d[i];
    x.resize((size_t)m);
    for (int i = 0; i < m; i++) x[i] = xp[pos[i]];
    return -1;
}

}  // namespace mi_gain

using mi_gain::EnvelopeGraph;

namespace {

constexpr int BG_MAX_SMOOTH = 8;

std::string pair_str(int p, int a, int b) { return "pair " + std::to_string(p) + " (" + std::to_string(a) + ", " + std::to_string(b) + ")"; }

constexpr double ENVELOPE_WORK_MAX = 2e9;     // multiply-adds of one envelope factorisation above which solve_nodes may iterate instead
constexpr int PCG_MAX_ITER = 2000;

// One channel of solve_nodes by conjugate gradients with the diagonal as preconditioner, from x = 1, every sum in index or pair-list order.
// Unknowns are the active ones (positions in node); diag / off / rhs are the channel's system in pair-list order.
// The stop is a bound, not a guess.  Every pair term 2 alpha n (I_ab e_a - I_ba e_b)(...)^T is positive semidefinite, so A >= beta diag(M) with
// M_i = N_i + the n of i's live pairs (integers >= 1).  With e = x - x*, r = rhs - A x:  e^T A e = r^T A^-1 r <= sum r_i^2 / (beta M_i)  and
// e^T A e >= beta min(M) |e|_inf^2, hence |e|_inf <= sqrt(sum r_i^2 / (beta M_i) / (beta min M)).  The iteration ends when that bound, taken on
// the residual computed afresh from x, is below 5e-10 max|x| (so below 1e-9 |x*|_inf); a system on which double arithmetic cannot bring the
// residual that low (a weak prior on a large graph) is refused.
int solve_pcg(const mi355_gain_pair_stats* ps, const std::vector<int>& live, const std::vector<int>& idx, const std::vector<int>& node, const int64_t* cover,
              const std::vector<double>& diag, const std::vector<double>& off, const std::vector<double>& rhs, double beta, std::vector<double>& x,
              std::string& err) {
    const int m = (int)node.size();
    std::vector<double> M((size_t)m), r((size_t)m), z((size_t)m), p((size_t)m), Ap((size_t)m);
    for (int i = 0; i < m; i++) M[i] = (double)cover[node[i]];
    for (int q : live) { M[idx[ps[q].a]] += (double)ps[q].n; M[idx[ps[q].b]] += (double)ps[q].n; }
    double mmin = M[0];
    for (int i = 1; i < m; i++) mmin = std::min(mmin, M[i]);
    auto matvec = [&](const std::vector<double>& v, std::vector<double>& y) {
        for (int i = 0; i < m; i++) y[i] = diag[i] * v[i];
        for (size_t q = 0; q < live.size(); q++) {
            const int a = idx[ps[live[q]].a], b = idx[ps[live[q]].b];
            y[a] += off[q] * v[b]; y[b] += off[q] * v[a];
        }
    };
    auto dot = [&](const std::vector<double>& a, const std::vector<double>& b) { double s = 0.0; for (int i = 0; i < m; i++) s += a[i] * b[i]; return s; };
    auto error_bound = [&]() { double s = 0.0; for (int i = 0; i < m; i++) s += r[i] * r[i] / (beta * M[i]); return std::sqrt(s / (beta * mmin)); };
    auto restart = [&]() {                                     // r, z, p from x
        matvec(x, Ap);
        for (int i = 0; i < m; i++) { r[i] = rhs[i] - Ap[i]; z[i] = r[i] / diag[i]; p[i] = z[i]; }
        return dot(r, z);
    };
    std::fill(x.begin(), x.end(), 1.0);
    double rho = restart();
    for (int it = 0; it < PCG_MAX_ITER; it++) {
        double xmax = 0.0;
        for (int i = 0; i < m; i++) xmax = std::max(xmax, std::fabs(x[i]));
        if (error_bound() <= 2.5e-10 * xmax) {
            rho = restart();                                   // the recurrence's residual drifts from the true one: decide on the true one
            if (error_bound() <= 5e-10 * xmax) return MI355_OK;
        }
        matvec(p, Ap);
        const double a = rho / dot(p, Ap);
        for (int i = 0; i < m; i++) { x[i] += a * p[i]; r[i] -= a * Ap[i]; z[i] = r[i] / diag[i]; }
        const double rho2 = dot(r, z);
        const double b = rho2 / rho;
        for (int i = 0; i < m; i++) p[i] = z[i] + b * p[i];
        rho = rho2;
    }
    err = "the iterative solve of " + std::to_string(m) + " unknowns did not reach 1e-9 in " + std::to_string(PCG_MAX_ITER) + " steps (prior too weak for a graph this large)";
    return MI355_ERR_FAILED;
}

// The normal equations of the header over n unknowns ("frames" for mi355_solve_gains, the nodes (frame, cell) for the block gains): ps[p].a / .b
// are unknowns, cover[k] is N_k.  x3: n x 3 doubles, 1 for an unknown without an equation (channels == 1: the one value in all three).
// The factorisation is EnvelopeGraph's envelope Cholesky.  may_iterate (block gains only): where its envelope would cost more than ENVELOPE_WORK_MAX
// multiply-adds per channel, a Jacobi-preconditioned conjugate gradient in the same fixed order takes its place; it stops on a bound of the
// error that it can prove (see there) and fails rather than return less.  unit names an unknown in the messages.
int solve_nodes(const mi355_gain_pair_stats* ps, int n_pairs, const int64_t* cover, int n, float sigma_n, float sigma_g, int channels, const char* unit,
                bool may_iterate, double* x3, std::string& err) {
    const double alpha = 1.0 / ((double)sigma_n * (double)sigma_n), beta = 1.0 / ((double)sigma_g * (double)sigma_g);
    // the frames with an equation and the graph of the pairs with n > 0 (the same for every channel)
    std::vector<char> active((size_t)n, 0);
    for (int k = 0; k < n; k++) if (cover[k] > 0) active[k] = 1;
    std::vector<int> live;                                    // pairs that add terms
    for (int p = 0; p < n_pairs; p++) if (ps[p].n > 0) { live.push_back(p); active[ps[p].a] = 1; active[ps[p].b] = 1; }
    std::vector<int> idx((size_t)n, -1), node;
    for (int k = 0; k < n; k++) if (active[k]) { idx[k] = (int)node.size(); node.push_back(k); }
    const int m = (int)node.size();
    std::fill(x3, x3 + 3 * (size_t)n, 1.0);
    if (m == 0) return MI355_OK;
    std::vector<std::pair<int, int>> edges;
    edges.reserve(live.size());
    for (int p : live) edges.emplace_back(idx[ps[p].a], idx[ps[p].b]);
    EnvelopeGraph eg;
    eg.build(m, edges);
    const bool iterate = may_iterate && eg.work > ENVELOPE_WORK_MAX;
    std::vector<double> diag((size_t)m), rhs((size_t)m), x((size_t)m);
    std::vector<double> off((size_t)live.size());
    const int nch = channels;
    for (int c = 0; c < nch; c++) {
        // the normal equations in pair-list order
        for (int i = 0; i < m; i++) { diag[i] = beta * (double)cover[node[i]]; rhs[i] = beta * (double)cover[node[i]]; }
        for (size_t q = 0; q < live.size(); q++) {
            const mi355_gain_pair_stats& s = ps[live[q]];
            const double nn = (double)s.n;
            double Iab, Iba;
            if (nch == 3) { Iab = (double)s.sum_a[c] / nn; Iba = (double)s.sum_b[c] / nn; }
            else { Iab = (double)(s.sum_a[0] + s.sum_a[1] + s.sum_a[2]) / (3.0 * nn); Iba = (double)(s.sum_b[0] + s.sum_b[1] + s.sum_b[2]) / (3.0 * nn); }
            const int u = idx[s.a], v = idx[s.b];
            diag[u] += 2.0 * alpha * Iab * Iab * nn + beta * nn;
            diag[v] += 2.0 * alpha * Iba * Iba * nn + beta * nn;
            off[q] = -2.0 * alpha * Iab * Iba * nn;
            rhs[u] += beta * nn; rhs[v] += beta * nn;
        }
        if (iterate) {
            const int rc = solve_pcg(ps, live, idx, node, cover, diag, off, rhs, beta, x, err);
            if (rc != MI355_OK) return rc;
        } else {
            const int bad = eg.solve(diag, off, rhs, x);
            if (bad >= 0) { err = std::string("the normal equations are not positive definite at ") + unit + " " + std::to_string(node[bad]); return MI355_ERR_FAILED; }
        }
        for (int i = 0; i < m; i++) {
            if (nch == 3) x3[3 * (size_t)node[i] + c] = x[i];
            else x3[3 * (size_t)node[i]] = x3[3 * (size_t)node[i] + 1] = x3[3 * (size_t)node[i] + 2] = x[i];
        }
    }
    return MI355_OK;
}

}  // namespace

namespace mi_gain {

// a == b, a position out of range, an unordered pair listed twice; pair_at(p, a, b) gives pair p
bool check_pairs(const std::function<void(int, int&, int&)>& pair_at, int n_pairs, int n, std::string& err) {
    std::unordered_map<uint64_t, int> seen;
    seen.reserve((size_t)n_pairs * 2 + 1);
    for (int p = 0; p < n_pairs; p++) {
        int a, b;
        pair_at(p, a, b);
        if (a < 0 || a >= n || b < 0 || b >= n) { err = pair_str(p, a, b) + ": position outside [0, " + std::to_string(n) + ")"; return false; }
        if (a == b) { err = pair_str(p, a, b) + ": a == b"; return false; }
        const uint64_t key = ((uint64_t)std::min(a, b) << 32) | (uint64_t)std::max(a, b);
        auto it = seen.find(key);
        if (it != seen.end()) { err = pair_str(p, a, b) + " repeats pair " + std::to_string(it->second); return false; }
        seen.emplace(key, p);
    }
    return true;
}

bool check_frames_n(int n, std::string& err) {
    if (n < 1 || n > MAX_FRAMES) { err = "n=" + std::to_string(n) + " outside [1, 65535]"; return false; }
    return true;
}

bool check_params(float sigma_n, float sigma_g, int channels, const int* step, std::string& err) {
    if (step && (*step < 1 || *step > 64)) { err = "step=" + std::to_string(*step) + " outside [1, 64]"; return false; }
    if (channels != 1 && channels != 3) { err = "channels=" + std::to_string(channels) + " (need 1 or 3)"; return false; }
    if (!(sigma_n > 0.0f) || !std::isfinite(sigma_n)) { err = "sigma_n=" + std::to_string(sigma_n) + " must be > 0"; return false; }
    if (!(sigma_g > 0.0f) || !std::isfinite(sigma_g)) { err = "sigma_g=" + std::to_string(sigma_g) + " must be > 0"; return false; }
    return true;
}

bool check_grid(int gx, int gy, std::string& err) {
    if (gx < 1 || gx > MAX_GRID || gy < 1 || gy > MAX_GRID) { err = "grid " + std::to_string(gx) + "x" + std::to_string(gy) + " outside [1, 16] x [1, 16]"; return false; }
    return true;
}

bool check_block_params(const mi355_block_gain_params& p, bool need_step, std::string& err) {
    if (!check_params(p.sigma_n, p.sigma_g, p.channels, need_step ? &p.step : nullptr, err) || !check_grid(p.grid_x, p.grid_y, err)) return false;
    if (p.smooth < 0 || p.smooth > BG_MAX_SMOOTH) { err = "smooth=" + std::to_string(p.smooth) + " outside [0, 8]"; return false; }
    return true;
}

int solve_gains(const mi355_gain_pair_stats* ps, int n_pairs, const int64_t* cover, int n, const mi355_gain_params& prm, float* gains, std::string& err) {
    if (!check_frames_n(n, err) || !check_params(prm.sigma_n, prm.sigma_g, prm.channels, nullptr, err)) return MI355_ERR_ARG;
    if (n_pairs < 0 || (n_pairs > 0 && !ps) || !cover || !gains) { err = "NULL argument or n_pairs < 0"; return MI355_ERR_ARG; }
    if (!check_pairs([&](int p, int& a, int& b) { a = ps[p].a; b = ps[p].b; }, n_pairs, n, err)) return MI355_ERR_ARG;
    for (int p = 0; p < n_pairs; p++)
        if (ps[p].n < 0) { err = pair_str(p, ps[p].a, ps[p].b) + ": n=" + std::to_string(ps[p].n) + " < 0"; return MI355_ERR_ARG; }
    for (int k = 0; k < n; k++)
        if (cover[k] < 0) { err = "frame " + std::to_string(k) + ": frame_cover=" + std::to_string(cover[k]) + " < 0"; return MI355_ERR_ARG; }
    std::vector<double> x3((size_t)n * 3);
    const int rc = solve_nodes(ps, n_pairs, cover, n, prm.sigma_n, prm.sigma_g, prm.channels, "frame", false, x3.data(), err);
    if (rc != MI355_OK) return rc;
    for (size_t i = 0; i < x3.size(); i++) gains[i] = (float)x3[i];
    return MI355_OK;
}

int solve_block_gains(const mi355_block_gain_stats* rs, int64_t n_recs, const int32_t* pairs_ab, int n_pairs, const int64_t* cell_cover, int n,
                      const mi355_block_gain_params& prm, float* gains, std::string& err) {
    if (!check_frames_n(n, err) || !check_block_params(prm, false, err)) return MI355_ERR_ARG;
    if (n_recs < 0 || n_pairs < 0 || (n_recs > 0 && !rs) || (n_pairs > 0 && !pairs_ab) || !cell_cover || !gains) { err = "NULL argument or a count < 0"; return MI355_ERR_ARG; }
    if (!check_pairs(flat_pairs(pairs_ab), n_pairs, n, err)) return MI355_ERR_ARG;
    const int gx = prm.grid_x, gy = prm.grid_y, cells = gx * gy;
    if (n_recs > (int64_t)0x7fffffff) { err = "n_records=" + std::to_string(n_recs) + " too large"; return MI355_ERR_ARG; }
    std::vector<mi355_gain_pair_stats> edges((size_t)n_recs);
    for (int64_t i = 0; i < n_recs; i++) {
        const mi355_block_gain_stats& r = rs[i];
        const std::string ri = "record " + std::to_string(i);
        if (r.pair < 0 || r.pair >= n_pairs) { err = ri + ": pair=" + std::to_string(r.pair) + " outside [0, " + std::to_string(n_pairs) + ")"; return MI355_ERR_ARG; }
        if (r.cell_a < 0 || r.cell_a >= cells || r.cell_b < 0 || r.cell_b >= cells) { err = ri + ": cell (" + std::to_string(r.cell_a) + ", " + std::to_string(r.cell_b) + ") outside [0, " + std::to_string(cells) + ")"; return MI355_ERR_ARG; }
        if (r.n < 0) { err = ri + ": n=" + std::to_string(r.n) + " < 0"; return MI355_ERR_ARG; }
        mi355_gain_pair_stats& e = edges[(size_t)i];
        e.a = pairs_ab[2 * r.pair] * cells + r.cell_a; e.b = pairs_ab[2 * r.pair + 1] * cells + r.cell_b; e.n = r.n;
        for (int c = 0; c < 3; c++) { e.sum_a[c] = r.sum_a[c]; e.sum_b[c] = r.sum_b[c]; }
    }
    const int nodes = n * cells;
    for (int i = 0; i < nodes; i++)
        if (cell_cover[i] < 0) { err = "frame " + std::to_string(i / cells) + " cell " + std::to_string(i % cells) + ": cell_cover=" + std::to_string(cell_cover[i]) + " < 0"; return MI355_ERR_ARG; }
    std::vector<double> x3((size_t)nodes * 3);
    const int rc = solve_nodes(edges.data(), (int)n_recs, cell_cover, nodes, prm.sigma_n, prm.sigma_g, prm.channels, "node", true, x3.data(), err);
    if (rc != MI355_OK) return rc;
    // smoothing: per frame and channel, x then y, edges replicated
    std::vector<double> a((size_t)cells), b((size_t)cells);
    for (int k = 0; k < n; k++)
        for (int c = 0; c < 3; c++) {
            double* m = x3.data() + (size_t)k * cells * 3 + c;           // m[3 * cell]
            for (int i = 0; i < cells; i++) a[i] = m[3 * i];
            for (int s = 0; s < prm.smooth; s++) {
                for (int y = 0; y < gy; y++)
                    for (int x = 0; x < gx; x++)
                        b[y * gx + x] = 0.25 * a[y * gx + std::max(x - 1, 0)] + 0.5 * a[y * gx + x] + 0.25 * a[y * gx + std::min(x + 1, gx - 1)];
                for (int y = 0; y < gy; y++)
                    for (int x = 0; x < gx; x++)
                        a[y * gx + x] = 0.25 * b[std::max(y - 1, 0) * gx + x] + 0.5 * b[y * gx + x] + 0.25 * b[std::min(y + 1, gy - 1) * gx + x];
            }
            for (int i = 0; i < cells; i++) gains[((size_t)k * cells + i) * 3 + c] = (float)a[i];
        }
    return MI355_OK;
}

}  // namespace mi_gain

using namespace mi_gain;

extern "C" void mi355_default_gain_params(mi355_gain_params* p) {
    if (!p) return;
    p->sigma_n = 10.0f; p->sigma_g = 0.1f; p->channels = 3; p->step = 8;
}

extern "C" int mi355_solve_gains(const mi355_gain_pair_stats* pair_stats, int n_pairs, const int64_t* frame_cover, int n, const mi355_gain_params* p,
                                 float* gains) {
    mi355_gain_params dp;
    if (!p) { mi355_default_gain_params(&dp); p = &dp; }
    std::string err;
    const int rc = solve_gains(pair_stats, n_pairs, frame_cover, n, *p, gains, err);
    if (rc != MI355_OK) mi_set_host_error("solve_gains: " + err);
    return rc;
}

extern "C" void mi355_default_block_gain_params(mi355_block_gain_params* p) {
    if (!p) return;
    p->sigma_n = 10.0f; p->sigma_g = 0.1f; p->channels = 3; p->step = 8; p->grid_x = 8; p->grid_y = 6; p->smooth = 2; p->reserved = 0;
}

extern "C" int mi355_solve_block_gains(const mi355_block_gain_stats* records, int64_t n_records, const int32_t* pairs_ab, int n_pairs, const int64_t* cell_cover,
                                       int n, const mi355_block_gain_params* p, float* gains) {
    mi355_block_gain_params dp;
    if (!p) { mi355_default_block_gain_params(&dp); p = &dp; }
    std::string err;
    const int rc = solve_block_gains(records, n_records, pairs_ab, n_pairs, cell_cover, n, *p, gains, err);
    if (rc != MI355_OK) mi_set_host_error("solve_block_gains: " + err);
    return rc;
}
