// csrc/calib_solve.cpp -- the host half of the lens self-calibration (include/mi355_mosaic.h, "lens self-calibration"): the argument checks,
// the blocks on the host (the twin of calib.hip's kernel, the same bits), the records of a flat list, and the Levenberg-Marquardt loop that
// eliminates every record's eight unknowns into the system of the free coefficients.  Host-only code, no device work; calib.hip hands the
// loop its blocks through calib.h.
#include "calib.h"
#include "host_error.h"
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace {

void block_host(const mi355_pair_result& e, const double* h, const mi355_camera& cam, int min_ties, mi355_pair_calib_block& o, int* first_bad = nullptr) {
    memset(&o, 0, sizeof(o));
    o.i = e.i; o.j = e.j;
    if (!mi_cal_used(e.accepted, e.n_in, e.i, e.j, min_ties, h)) return;
    o.n_in = e.n_in;
    double S[MI_CAL_ROW * (MI_CAL_ROW + 1) / 2] = {};
    for (int k = 0; k < e.n_in; k++) {
        CalSide a, b;
        CalChain ch;
        mi_cal_undistort(cam, (double)e.a[k].x, (double)e.a[k].y, a);
        mi_cal_undistort(cam, (double)e.b[k].x, (double)e.b[k].y, b);
        mi_cal_chain(cam, h, b, ch);
        if (!(a.good && ch.good)) { if (first_bad && o.n_bad == 0) *first_bad = k; o.n_bad++; continue; }
        double X[MI_CAL_ROW], Y[MI_CAL_ROW];
        for (int c = 0; c < 8; c++) { X[c] = ch.X[c]; Y[c] = ch.Y[c]; }
        mi_cal_close(cam, a, ch.px, ch.py, ch.cx, ch.cy, X + 8, Y + 8);
        mi_tri_add<MI_CAL_ROW>(S, X, Y);
    }
    mi_tri_split<MI_CAL_ROW>(S, o);
}

// the loop's records on the host (blocks: tie_blocks.h, threads from 4000 ties on)
struct HostSource : CalibSource {
    std::vector<const mi355_pair_result*> recs;
    std::vector<mi355_pair_calib_block> blk;
    int count() override { return (int)recs.size(); }
    int heads(CalibHead* out, std::string&) override {
        for (size_t p = 0; p < recs.size(); p++) { out[p].i = recs[p]->i; out[p].j = recs[p]->j; out[p].n_in = recs[p]->n_in; memcpy(out[p].H, recs[p]->H, sizeof(float) * 9); }
        return MI355_OK;
    }
    int blocks(const double* h8, const mi355_camera& cam, int min_ties, const mi355_pair_calib_block** out, std::string&) override {
        blk.resize(recs.size());
        mi_host_blocks(recs.size(), 4000, [&](size_t p) { return (size_t)(recs[p]->n_in > 0 && recs[p]->n_in <= MI355_MAX_SELECTED ? recs[p]->n_in : 0); },
                       [&](size_t p) { block_host(*recs[p], h8 + 8 * p, cam, min_ties, blk[p]); });
        *out = blk.data();
        return MI355_OK;
    }
    int record(int p, mi355_pair_result* out, std::string&) override { *out = *recs[(size_t)p]; return MI355_OK; }
};

// in-place Cholesky of the lower triangle of a dense n x n matrix (row-major, leading dimension ld); false on a pivot that is not positive
bool chol(double* A, int n, int ld) {
    for (int i = 0; i < n; i++) {
        for (int j = 0; j <= i; j++) {
            double s = A[i * ld + j];
            for (int k = 0; k < j; k++) s = s - A[i * ld + k] * A[j * ld + k];
            if (j < i) A[i * ld + j] = s / A[j * ld + j];
            else { if (!(s > 0.0) || !std::isfinite(s)) return false; A[i * ld + i] = std::sqrt(s); }
        }
    }
    return true;
}
void solve_lower(const double* L, int n, int ld, double* y) {            // L y' = y
    for (int i = 0; i < n; i++) { double s = y[i]; for (int k = 0; k < i; k++) s = s - L[i * ld + k] * y[k]; y[i] = s / L[i * ld + i]; }
}
void solve_upper(const double* L, int n, int ld, double* y) {            // L^T y' = y
    for (int i = n - 1; i >= 0; i--) { double s = y[i]; for (int k = i + 1; k < n; k++) s = s - L[k * ld + i] * y[k]; y[i] = s / L[i * ld + i]; }
}

// what the elimination of one record leaves: its factor, W, z, and its contribution to the system of the free coefficients
struct RecWork { double L[64], W[5][8], z[8], S[5][5], s[5], Cd[5]; bool ok; };

void eliminate(const mi355_pair_calib_block& b, double lambda, const int* fr, int np, RecWork& w) {
    for (int r = 0; r < 8; r++)
        for (int c = 0; c <= r; c++) w.L[r * 8 + c] = b.N[r * (r + 1) / 2 + c];
    for (int r = 0; r < 8; r++) w.L[r * 8 + r] = w.L[r * 8 + r] + lambda * w.L[r * 8 + r];
    w.ok = chol(w.L, 8, 8);
    if (!w.ok) return;
    for (int m = 0; m < np; m++) {
        const int row = 8 + fr[m];
        for (int r = 0; r < 8; r++) w.W[m][r] = b.N[row * (row + 1) / 2 + r];
        solve_lower(w.L, 8, 8, w.W[m]);
    }
    for (int r = 0; r < 8; r++) w.z[r] = b.g[r];
    solve_lower(w.L, 8, 8, w.z);
    for (int m = 0; m < np; m++) {
        const int row = 8 + fr[m];
        for (int n = 0; n <= m; n++) {
            double v = b.N[row * (row + 1) / 2 + 8 + fr[n]];
            for (int r = 0; r < 8; r++) v = v - w.W[m][r] * w.W[n][r];
            w.S[m][n] = v;
        }
        double v = b.g[row];
        for (int r = 0; r < 8; r++) v = v - w.W[m][r] * w.z[r];
        w.s[m] = v;
        w.Cd[m] = b.N[row * (row + 1) / 2 + row];
    }
}

void start_state(const float* H, const mi355_camera& c, double* h) {
    double M[9], T[9], G[9];
    for (int k = 0; k < 9; k++) M[k] = (double)H[k];
    M[8] = 1.0;
    for (int r = 0; r < 3; r++) {
        T[3 * r] = M[3 * r] * c.fx;
        T[3 * r + 1] = M[3 * r + 1] * c.fy;
        T[3 * r + 2] = (M[3 * r] * c.cx + M[3 * r + 1] * c.cy) + M[3 * r + 2];
    }
    for (int k = 0; k < 3; k++) {
        G[k] = (T[k] - c.cx * T[6 + k]) / c.fx;
        G[3 + k] = (T[3 + k] - c.cy * T[6 + k]) / c.fy;
        G[6 + k] = T[6 + k];
    }
    bool ok = true;
    for (int k = 0; k < 8; k++) { h[k] = G[k] / G[8]; ok = ok && mi_finite(h[k]); }
    if (!ok) for (int k = 0; k < 8; k++) h[k] = std::numeric_limits<double>::quiet_NaN();
}

// the least-squares homography of one run of the flat list (include/mi355_mosaic.h, mi355_match_pairs_to_results)
void fit_h(const mi355_match_point_pairs* v, int n, float* H) {
    for (int k = 0; k < 9; k++) H[k] = std::numeric_limits<float>::quiet_NaN();
    double m[4] = {0.0, 0.0, 0.0, 0.0};                 // means: a.x, a.y, b.x, b.y
    for (int k = 0; k < n; k++) { m[0] = m[0] + (double)v[k].ptA.x; m[1] = m[1] + (double)v[k].ptA.y; m[2] = m[2] + (double)v[k].ptB.x; m[3] = m[3] + (double)v[k].ptB.y; }
    for (int q = 0; q < 4; q++) m[q] = m[q] / (double)n;
    double va = 0.0, vb = 0.0;
    for (int k = 0; k < n; k++) {
        const double ax = (double)v[k].ptA.x - m[0], ay = (double)v[k].ptA.y - m[1], bx = (double)v[k].ptB.x - m[2], by = (double)v[k].ptB.y - m[3];
        va = va + (ax * ax + ay * ay); vb = vb + (bx * bx + by * by);
    }
    const double sa = 1.0 / std::sqrt(va / (double)n), sb = 1.0 / std::sqrt(vb / (double)n);
    if (!mi_finite(sa) || !mi_finite(sb)) return;
    double N[64], g[8];
    for (int k = 0; k < 64; k++) N[k] = 0.0;
    for (int k = 0; k < 8; k++) g[k] = 0.0;
    for (int k = 0; k < n; k++) {
        const double xa = ((double)v[k].ptA.x - m[0]) * sa, ya = ((double)v[k].ptA.y - m[1]) * sa, x = ((double)v[k].ptB.x - m[2]) * sb, y = ((double)v[k].ptB.y - m[3]) * sb;
        const double R[2][8] = {{x, y, 1.0, 0.0, 0.0, 0.0, -(xa * x), -(xa * y)}, {0.0, 0.0, 0.0, x, y, 1.0, -(ya * x), -(ya * y)}};
        const double rhs[2] = {xa, ya};
        for (int q = 0; q < 2; q++)
            for (int r = 0; r < 8; r++) {
                for (int c = 0; c <= r; c++) N[r * 8 + c] = N[r * 8 + c] + R[q][r] * R[q][c];
                g[r] = g[r] + R[q][r] * rhs[q];
            }
    }
    if (!chol(N, 8, 8)) return;
    solve_lower(N, 8, 8, g);
    solve_upper(N, 8, 8, g);
    // H = Ta^-1 Hn Tb with Tb = [sb, 0, -sb mbx; 0, sb, -sb mby; 0, 0, 1] and Ta^-1 = [1/sa, 0, max; 0, 1/sa, may; 0, 0, 1]
    const double Hn[9] = {g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], 1.0};
    double P[9], Q[9];
    for (int r = 0; r < 3; r++) {
        P[3 * r] = Hn[3 * r] * sb; P[3 * r + 1] = Hn[3 * r + 1] * sb;
        P[3 * r + 2] = Hn[3 * r + 2] - (Hn[3 * r] * (sb * m[2]) + Hn[3 * r + 1] * (sb * m[3]));
    }
    for (int c = 0; c < 3; c++) { Q[c] = P[c] / sa + m[0] * P[6 + c]; Q[3 + c] = P[3 + c] / sa + m[1] * P[6 + c]; Q[6 + c] = P[6 + c]; }
    float out[9];
    for (int k = 0; k < 9; k++) { const double q = Q[k] / Q[8]; if (!mi_finite(q)) return; out[k] = (float)q; }
    memcpy(H, out, sizeof(out));
}

int flat_runs(const mi355_match_point_pairs* v, int n, mi355_pair_result* out) {      // out NULL: count only
    int cnt = 0;
    mi_flat_runs(v, n, MI355_MAX_SELECTED, [&](int p, int q) {
        if (out) {
            mi355_pair_result& r = out[cnt];
            memset(&r, 0, sizeof(r));
            r.i = v[p].ptA_i; r.j = v[p].ptB_i; r.n_in = q - p; r.n_selected = q - p; r.ok = 1; r.accepted = 1;
            for (int k = p; k < q; k++) { r.a[k - p] = v[k].ptA; r.b[k - p] = v[k].ptB; }
            fit_h(v + p, q - p, r.H);
        }
        cnt++;
    });
    return cnt;
}

}  // namespace

extern "C" void mi355_default_calib_params(mi355_calib_params* p) {
    if (!p) return;
    p->max_iters = 20; p->mask = MI355_CALIB_K1 | MI355_CALIB_K2; p->min_ties = 16; p->reserved = 0;
    p->lambda0 = 1e-3; p->lambda_up = 10.0; p->lambda_down = 10.0; p->min_rel_decrease = 1e-6;
}

static int check_camera(const char* who, const mi355_camera* cam, std::string& err) {
    if (!cam) { err = std::string(who) + ": NULL camera"; return MI355_ERR_ARG; }
    const double v[9] = {cam->fx, cam->fy, cam->cx, cam->cy, cam->k1, cam->k2, cam->p1, cam->p2, cam->k3};
    static const char* const name[9] = {"fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3"};
    for (int k = 0; k < 9; k++)
        if (!mi_finite(v[k])) { err = std::string(who) + ": camera " + name[k] + " = " + std::to_string(v[k]) + " (finite)"; return MI355_ERR_ARG; }
    for (int k = 0; k < 2; k++)
        if (v[k] <= 0.0) { err = std::string(who) + ": camera " + name[k] + " = " + std::to_string(v[k]) + " (above 0)"; return MI355_ERR_ARG; }
    return MI355_OK;
}
static int check_min_ties(const char* who, int min_ties, std::string& err) {
    if (min_ties < 8 || min_ties > MI355_MAX_SELECTED) { err = std::string(who) + ": min_ties = " + std::to_string(min_ties) + " (8 .. 400)"; return MI355_ERR_ARG; }
    return MI355_OK;
}

int mi_calib_check(const char* who, const mi355_camera* cam, const mi355_calib_params* pp, std::string& err) {
    { const int rc = check_camera(who, cam, err); if (rc != MI355_OK) return rc; }
    if (!pp) return MI355_OK;
    const mi355_calib_params& p = *pp;
    if (p.mask <= 0 || p.mask > 31) { err = std::string(who) + ": mask = " + std::to_string(p.mask) + " (1 .. 31: bits 0..4 = k1, k2, p1, p2, k3)"; return MI355_ERR_ARG; }
    { const int rc = check_min_ties(who, p.min_ties, err); if (rc != MI355_OK) return rc; }
    return mi_lm_check(who, mi_lm_schedule(p), err);
}

int mi_calib_check_blocks(const char* who, int n, const void* records, const double* h8, const mi355_camera* cam, int min_ties, const void* out, std::string& err) {
    if (n < 0) { err = std::string(who) + ": n = " + std::to_string(n) + " (not negative)"; return MI355_ERR_ARG; }
    { const int rc = check_camera(who, cam, err); if (rc != MI355_OK) return rc; }
    { const int rc = check_min_ties(who, min_ties, err); if (rc != MI355_OK) return rc; }
    if (n > 0 && (!records || !h8 || !out)) { err = std::string(who) + ": NULL " + (!records ? "records" : !h8 ? "h8" : "out"); return MI355_ERR_ARG; }
    return MI355_OK;
}

int mi_calibrate_lens(CalibSource& src, const mi355_camera* start, const mi355_calib_params* params, mi355_camera* out, mi355_calib_report* report,
                      std::string& err) {
    { const int rc = mi_calib_check("calibrate_lens", start, params, err); if (rc != MI355_OK) return rc; }
    if (!out) { err = "calibrate_lens: NULL out"; return MI355_ERR_ARG; }
    mi355_calib_params P;
    mi355_default_calib_params(&P);
    if (params) P = *params;
    mi355_calib_report rep;
    memset(&rep, 0, sizeof(rep));
    if (report) *report = rep;
    const mi355_camera cam0 = *start;
    *out = cam0;
    const int n = src.count();
    if (n <= 0) return MI355_OK;

    int fr[5], np = 0;
    for (int m = 0; m < 5; m++) if (P.mask >> m & 1) fr[np++] = m;
    std::vector<CalibHead> head((size_t)n);
    { const int rc = src.heads(head.data(), err); if (rc != MI355_OK) return rc; }
    std::vector<double> hc((size_t)8 * n), ht((size_t)8 * n);
    bool any = false;                              // the records decide whether they are used: nothing is launched for a set without one
    for (int p = 0; p < n; p++) {
        start_state(head[p].H, cam0, hc.data() + (size_t)8 * p);
        any = any || mi_cal_used(1, head[p].n_in, head[p].i, head[p].j, P.min_ties, hc.data() + (size_t)8 * p);
    }
    if (!any) return MI355_OK;
    double th[5] = {cam0.k1, cam0.k2, cam0.p1, cam0.p2, cam0.k3};
    auto camera_of = [&](const double* t) { mi355_camera c = cam0; c.k1 = t[0]; c.k2 = t[1]; c.p1 = t[2]; c.p2 = t[3]; c.k3 = t[4]; return c; };

    const mi355_pair_calib_block* blk = nullptr;
    { const int rc = src.blocks(hc.data(), cam0, P.min_ties, &blk, err); if (rc != MI355_OK) return rc; }
    std::vector<int> used;
    int64_t n_points = 0;
    for (int p = 0; p < n; p++) if (blk[p].n_in > 0) { used.push_back(p); n_points += blk[p].n_in; }
    if (used.empty()) return MI355_OK;
    for (int p : used)
        if (blk[p].n_bad > 0) {
            std::vector<mi355_pair_result> rec(1);
            int tie = -1;
            { const int rc = src.record(p, rec.data(), err); if (rc != MI355_OK) return rc; }
            mi355_pair_calib_block tmp;
            block_host(rec[0], hc.data() + (size_t)8 * p, cam0, P.min_ties, tmp, &tie);
            err = "calibrate_lens: accepted record " + std::to_string(p) + " (" + std::to_string(blk[p].i) + ", " + std::to_string(blk[p].j) + ") has " +
                  std::to_string(blk[p].n_bad) + " bad ties at the start camera, the first is tie " + std::to_string(tie) +
                  " (its undistortion does not settle or its projection is not finite)";
            return MI355_ERR_FAILED;
        }
    const size_t nu = used.size();
    std::vector<mi355_pair_calib_block> cur(nu);
    double c = 0.0;
    for (size_t o = 0; o < nu; o++) { cur[o] = blk[used[o]]; c = c + cur[o].cost; }
    if (!mi_finite(c)) { err = "calibrate_lens: the cost at the start is not finite"; return MI355_ERR_FAILED; }
    rep.n_pairs_used = (int)nu; rep.n_unused_records = n - (int)nu; rep.n_points = n_points; rep.cost0 = c;

    std::vector<RecWork> work(nu);
    const int threads = nu >= 256 ? (host_threads() < 8 ? host_threads() : 8) : 1;
    LmState lm;
    double tt[5];
    const mi355_pair_calib_block* tb = nullptr;
    // a trial: every record's eight unknowns eliminated into the system of the free coefficients, the back-substitution, the blocks there
    auto try_step = [&](double lambda, double, double& c2, int& rc) {
        parallel_chunks(nu, threads, [&](size_t lo, size_t hi) { for (size_t o = lo; o < hi; o++) eliminate(cur[o], lambda, fr, np, work[o]); });
        double S[25], s[5], Cd[5];
        for (int k = 0; k < 25; k++) S[k] = 0.0;
        for (int k = 0; k < 5; k++) { s[k] = 0.0; Cd[k] = 0.0; tt[k] = th[k]; }
        for (size_t o = 0; o < nu; o++) {
            const RecWork& w = work[o];
            if (!w.ok) return false;
            for (int m = 0; m < np; m++) {
                for (int q = 0; q <= m; q++) S[m * 5 + q] = S[m * 5 + q] + w.S[m][q];
                s[m] = s[m] + w.s[m];
                Cd[m] = Cd[m] + w.Cd[m];
            }
        }
        for (int m = 0; m < np; m++) S[m * 5 + m] = S[m * 5 + m] + lambda * Cd[m];
        if (!chol(S, np, 5)) return false;
        solve_lower(S, np, 5, s);
        solve_upper(S, np, 5, s);
        for (int m = 0; m < np; m++) { tt[fr[m]] = th[fr[m]] + s[m]; if (!mi_finite(tt[fr[m]])) return false; }
        ht = hc;
        parallel_chunks(nu, threads, [&](size_t lo, size_t hi) {
            for (size_t o = lo; o < hi; o++) {
                const RecWork& w = work[o];
                double y[8];
                for (int r = 0; r < 8; r++) { double v = w.z[r]; for (int m = 0; m < np; m++) v = v - w.W[m][r] * s[m]; y[r] = v; }
                solve_upper(w.L, 8, 8, y);
                double* h = ht.data() + (size_t)8 * used[o];
                for (int r = 0; r < 8; r++) h[r] = h[r] + y[r];
            }
        });
        rc = src.blocks(ht.data(), camera_of(tt), P.min_ties, &tb, err);
        if (rc != MI355_OK) return false;
        for (size_t o = 0; o < nu; o++) {
            const mi355_pair_calib_block& b = tb[used[o]];
            if (b.n_in != cur[o].n_in || b.n_bad != 0) return false;
            c2 = c2 + b.cost;
        }
        return true;
    };
    auto accept = [&] {
        hc.swap(ht);
        for (int k = 0; k < 5; k++) th[k] = tt[k];
        for (size_t o = 0; o < nu; o++) cur[o] = tb[used[o]];
    };
    { const int rc = mi_lm_run(mi_lm_schedule(P), c, lm, try_step, accept); if (rc != MI355_OK) return rc; }
    rep.trials = lm.trials; rep.accepted = lm.accepted; rep.cost = lm.c; rep.lambda = lm.lambda;
    *out = camera_of(th);
    if (report) *report = rep;
    return MI355_OK;
}

extern "C" int mi355_pair_calib_blocks_host(const mi355_pair_result* r, int n, const double* h8, const mi355_camera* cam, int min_ties, mi355_pair_calib_block* out) {
    std::string err;
    { const int rc = mi_calib_check_blocks("pair_calib_blocks_host", n, r, h8, cam, min_ties, out, err); if (rc != MI355_OK) { mi_set_host_error(err); return rc; } }
    for (int p = 0; p < n; p++) block_host(r[p], h8 + (size_t)8 * p, *cam, min_ties, out[p]);
    return MI355_OK;
}

extern "C" int mi355_calibrate_lens_results(const mi355_pair_result* r, int n_pairs, const mi355_camera* start, const mi355_calib_params* params, mi355_camera* out,
                                            mi355_calib_report* report) {
    std::string err;
    if (n_pairs < 0 || (n_pairs > 0 && !r)) { mi_set_host_error("calibrate_lens_results: n_pairs = " + std::to_string(n_pairs) + (n_pairs < 0 ? " (not negative)" : " with NULL records")); return MI355_ERR_ARG; }
    HostSource src;
    for (int p = 0; p < n_pairs; p++) if (r[p].accepted) src.recs.push_back(r + p);
    const int rc = mi_calibrate_lens(src, start, params, out, report, err);
    if (rc != MI355_OK) mi_set_host_error(err);
    return rc;
}

extern "C" int mi355_match_pairs_to_results(const mi355_match_point_pairs* v, int n, mi355_pair_result* out, int cap, int* n_out) {
    if (n < 0 || (n > 0 && !v) || !n_out) { mi_set_host_error("match_pairs_to_results: n = " + std::to_string(n) + (n < 0 ? " (not negative)" : !n_out ? " with NULL n_out" : " with a NULL list")); return MI355_ERR_ARG; }
    const int cnt = flat_runs(v, n, nullptr);
    *n_out = cnt;
    if (!out) return MI355_OK;
    if (cap < cnt) { mi_set_host_error("match_pairs_to_results: cap = " + std::to_string(cap) + " (the list holds " + std::to_string(cnt) + " records)"); return MI355_ERR_ARG; }
    flat_runs(v, n, out);
    return MI355_OK;
}

extern "C" int mi355_calibrate_lens(const mi355_match_point_pairs* v, int n, const mi355_camera* start, const mi355_calib_params* params, mi355_camera* out,
                                    mi355_calib_report* report) {
    std::string err;
    if (n < 0 || (n > 0 && !v)) { mi_set_host_error("calibrate_lens: n = " + std::to_string(n) + (n < 0 ? " (not negative)" : " with a NULL list")); return MI355_ERR_ARG; }
    { const int rc = mi_calib_check("calibrate_lens", start, params, err); if (rc != MI355_OK) { mi_set_host_error(err); return rc; } }
    std::vector<mi355_pair_result> recs((size_t)flat_runs(v, n, nullptr));
    flat_runs(v, n, recs.data());
    HostSource src;
    for (const mi355_pair_result& r : recs) src.recs.push_back(&r);
    const int rc = mi_calibrate_lens(src, start, params, out, report, err);
    if (rc != MI355_OK) mi_set_host_error(err);
    return rc;
}
