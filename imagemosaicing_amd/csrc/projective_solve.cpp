// csrc/projective_solve.cpp -- the host half of the projective refinement (include/mi355_mosaic.h, "projective refinement of the global
// alignment"): the argument checks, the blocks on the host (the twin of projective.hip's kernel, the same bits), the assembly of the scaled
// damped system, the prior, and the Levenberg-Marquardt loop.  Host-only code, no device work; projective.hip hands the loop its blocks
// through projective.h.  The factorisation is the affine alignment's envelope Cholesky (envelope_chol.h), 8 rows per image, one right-hand side.
#include "projective.h"
#include "host_error.h"
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

// a pair's points, wherever they lie: the record's two lists (stride sizeof(mi355_sfpoint)) or the flat list's entries (stride of its record)
struct PairView { int32_t i, j, n_in, accepted; const char* a; const char* b; size_t stride; };

void block_host(const PairView& e, const double* h8, const uint8_t* part, int n_images, mi355_pair_normal_block& o) {
    memset(&o, 0, sizeof(o));
    o.i = e.i; o.j = e.j;
    int keep = 0;
    const bool used = mi_proj_used(e.accepted, e.n_in, e.i, e.j, part, n_images, &keep);
    o.n_in = keep;
    if (!used) return;
    const double* hi = h8 + (size_t)8 * e.i;
    const double* hj = h8 + (size_t)8 * e.j;
    double S[MI_PROJ_ROW * (MI_PROJ_ROW + 1) / 2] = {};
    for (int k = 0; k < e.n_in; k++) {
        const mi355_sfpoint& pa = *reinterpret_cast<const mi355_sfpoint*>(e.a + e.stride * (size_t)k);
        const mi355_sfpoint& pb = *reinterpret_cast<const mi355_sfpoint*>(e.b + e.stride * (size_t)k);
        double X[MI_PROJ_ROW], Y[MI_PROJ_ROW], Ua, Va, Ub, Vb;
        mi_proj_side(hi, (double)pa.x, (double)pa.y, 1.0, X, Y, Ua, Va);
        mi_proj_side(hj, (double)pb.x, (double)pb.y, -1.0, X + 8, Y + 8, Ub, Vb);
        X[16] = Ub - Ua; Y[16] = Vb - Va;
        mi_tri_add<MI_PROJ_ROW>(S, X, Y);
    }
    mi_tri_split<MI_PROJ_ROW>(S, o);
}

// blocks of a list of views (tie_blocks.h: threads from 20000 points on)
struct HostSource : ProjectiveSource {
    std::vector<PairView> views;
    std::vector<mi355_pair_normal_block> blk;
    int blocks(const double* h8, const uint8_t* part, int n_images, const mi355_pair_normal_block** out, int* n, std::string&) override {
        blk.resize(views.size());
        mi_host_blocks(views.size(), 20000, [&](size_t p) { return (size_t)(views[p].n_in > 0 ? views[p].n_in : 0); },
                       [&](size_t p) { block_host(views[p], h8, part, n_images, blk[p]); });
        *out = blk.data(); *n = (int)blk.size();
        return MI355_OK;
    }
};

// the system of one parameter set: the band of N (lower, envelope layout), g, the two costs
struct System {
    std::vector<double> N, g;
    double cost_data = 0.0, cost_prior = 0.0;
};

}  // namespace

extern "C" void mi355_default_projective_params(mi355_projective_params* p) {
    if (!p) return;
    p->max_iters = 20; p->reserved = 0; p->prior = 0.01; p->lambda0 = 1e-3; p->lambda_up = 10.0; p->lambda_down = 10.0; p->min_rel_decrease = 1e-6;
}

int mi_projective_check(int n_images, const int32_t* w, const int32_t* h, const mi355_image_transform* start, const mi355_projective_params* pp,
                        mi355_image_transform* out, std::string& err) {
    if (n_images < 1) { err = "projective_refine: n_images = " + std::to_string(n_images) + " (at least 1)"; return MI355_ERR_ARG; }
    if (!w || !h || !start || !out) { err = std::string("projective_refine: NULL ") + (!w ? "w" : !h ? "h" : !start ? "start" : "out"); return MI355_ERR_ARG; }
    if (!pp) return MI355_OK;
    if (pp->max_iters >= 0 && (!mi_finite(pp->prior) || pp->prior < 0.0)) {          // reported after max_iters, before the rest of the schedule
        err = "projective_refine: prior = " + std::to_string(pp->prior) + " (finite, not negative)";
        return MI355_ERR_ARG;
    }
    return mi_lm_check("projective_refine", mi_lm_schedule(*pp), err);
}

int mi_projective_refine(ProjectiveSource& src, int n_images, const int32_t* w, const int32_t* h, const int32_t* fixed, const int32_t* label,
                         const mi355_image_transform* start, const mi355_projective_params* params, mi355_image_transform* out,
                         mi355_projective_report* report, std::string& err) {
    { const int rc = mi_projective_check(n_images, w, h, start, params, out, err); if (rc != MI355_OK) return rc; }
    mi355_projective_params P;
    mi355_default_projective_params(&P);
    if (params) P = *params;
    mi355_projective_report rep;
    memset(&rep, 0, sizeof(rep));
    if (report) *report = rep;
    if (out != start) memcpy(out, start, sizeof(mi355_image_transform) * (size_t)n_images);

    // taking part, parameters
    std::vector<uint8_t> part((size_t)n_images, 0);
    std::vector<double> hc((size_t)8 * n_images, 0.0);
    for (int k = 0; k < n_images; k++) {
        const float m8 = start[k].m[8];
        if (!std::isfinite(m8) || m8 == 0.0f || (label && label[k] == 0)) continue;
        const bool fx = fixed ? fixed[k] != 0 : (k == 0);
        part[k] = fx ? 2 : 1;
        for (int j = 0; j < 8; j++) hc[(size_t)8 * k + j] = (double)start[k].m[j] / (double)m8;
    }
    const mi355_pair_normal_block* blk = nullptr;
    int nb = 0;
    { const int rc = src.blocks(hc.data(), part.data(), n_images, &blk, &nb, err); if (rc != MI355_OK) return rc; }
    // the used pairs and the free images (the same for every trial: they depend on the records and the start alone)
    std::vector<int> used;
    std::vector<int64_t> nk((size_t)n_images, 0);
    int64_t n_points = 0;
    for (int p = 0; p < nb; p++) {
        const mi355_pair_normal_block& b = blk[p];
        if (b.n_in <= 0) continue;
        if (b.n_in > MI355_MAX_SELECTED || b.i < 0 || b.i >= n_images || b.j < 0 || b.j >= n_images) {
            err = "projective_refine: accepted record " + std::to_string(p) + " (" + std::to_string(b.i) + ", " + std::to_string(b.j) + ") has n_in = " + std::to_string(b.n_in) +
                  " (at most " + std::to_string(MI355_MAX_SELECTED) + ") or an image index outside [0, " + std::to_string(n_images) + ")";
            return MI355_ERR_ARG;
        }
        used.push_back(p);
        nk[b.i] += b.n_in; nk[b.j] += b.n_in; n_points += b.n_in;
    }
    std::vector<int> col((size_t)n_images, -1), freeimg;
    for (int k = 0; k < n_images; k++) if (part[k] == 1 && nk[k] > 0) { col[k] = (int)freeimg.size(); freeimg.push_back(k); }
    const int nf = (int)freeimg.size();
    if (nf == 0 || used.empty()) return MI355_OK;
    for (int k : freeimg)
        if (w[k] < 2 || h[k] < 2) { err = "projective_refine: image " + std::to_string(k) + " is " + std::to_string(w[k]) + " x " + std::to_string(h[k]) + " (at least 2 x 2)"; return MI355_ERR_ARG; }

    // the envelope: fixed by the used pairs
    const int D = 8 * nf;
    int bw = 0;
    std::vector<int> fst;
    envelope_profile(8, nf, used.size(), [&](size_t q, int& oa, int& ob) { oa = col[blk[used[q]].i]; ob = col[blk[used[q]].j]; }, bw, fst);
    const size_t W = (size_t)bw + 1;
    auto at = [&](std::vector<double>& N, int i, int j) -> double& { return N[(size_t)i * W + (size_t)(j - i + bw)]; };     // i >= j >= i - bw

    // the prior's control points and targets (under the start parameters, once)
    std::vector<double> ctl((size_t)nf * 18), tgt((size_t)nf * 18), omega((size_t)nf);
    for (int o = 0; o < nf; o++) {
        const int k = freeimg[o];
        omega[o] = (P.prior * (double)nk[k]) / 9.0;
        for (int q = 0; q < 3; q++)
            for (int p = 0; p < 3; p++) {
                const double x = ((double)p * (double)(w[k] - 1)) / 2.0, y = ((double)q * (double)(h[k] - 1)) / 2.0;
                double jx[8], jy[8], U, V;
                mi_proj_side(hc.data() + (size_t)8 * k, x, y, 1.0, jx, jy, U, V);
                const size_t t = (size_t)o * 18 + (size_t)(q * 3 + p) * 2;
                ctl[t] = x; ctl[t + 1] = y; tgt[t] = U; tgt[t + 1] = V;
            }
    }
    auto assemble = [&](const double* h8, const mi355_pair_normal_block* B, System& s) {
        s.N.assign((size_t)D * W, 0.0);
        s.g.assign((size_t)D, 0.0);
        s.cost_data = 0.0; s.cost_prior = 0.0;
        for (int p : used) {
            const mi355_pair_normal_block& b = B[p];
            const int oi = col[b.i], oj = col[b.j];
            if (oi >= 0) for (int r = 0; r < 8; r++) { s.g[8 * oi + r] += b.g[r]; for (int c = 0; c <= r; c++) at(s.N, 8 * oi + r, 8 * oi + c) += b.N[r * (r + 1) / 2 + c]; }
            if (oj >= 0) for (int r = 0; r < 8; r++) { s.g[8 * oj + r] += b.g[8 + r]; for (int c = 0; c <= r; c++) at(s.N, 8 * oj + r, 8 * oj + c) += b.N[(8 + r) * (9 + r) / 2 + 8 + c]; }
            if (oi >= 0 && oj >= 0)
                for (int r = 0; r < 8; r++)
                    for (int c = 0; c < 8; c++) {           // the block's (8 + r, c) = N(j's row r, i's row c): into the lower triangle
                        const double v = b.N[(8 + r) * (9 + r) / 2 + c];
                        if (oj > oi) at(s.N, 8 * oj + r, 8 * oi + c) += v; else at(s.N, 8 * oi + c, 8 * oj + r) += v;
                    }
            s.cost_data += b.cost;
        }
        for (int o = 0; o < nf; o++) {
            const int k = freeimg[o];
            double Pm[36], pg[8], pc = 0.0;
            for (int t = 0; t < 36; t++) Pm[t] = 0.0;
            for (int t = 0; t < 8; t++) pg[t] = 0.0;
            for (int q = 0; q < 9; q++) {
                const size_t t = (size_t)o * 18 + (size_t)q * 2;
                double jx[8], jy[8], U, V;
                mi_proj_side(h8 + (size_t)8 * k, ctl[t], ctl[t + 1], 1.0, jx, jy, U, V);
                const double rx = tgt[t] - U, ry = tgt[t + 1] - V;
                for (int r = 0; r < 8; r++) {
                    for (int c = 0; c <= r; c++) { double v = Pm[r * (r + 1) / 2 + c]; v = v + jx[r] * jx[c]; v = v + jy[r] * jy[c]; Pm[r * (r + 1) / 2 + c] = v; }
                    double gv = pg[r]; gv = gv + jx[r] * rx; gv = gv + jy[r] * ry; pg[r] = gv;
                }
                pc = pc + rx * rx; pc = pc + ry * ry;
            }
            for (int r = 0; r < 8; r++) {
                for (int c = 0; c <= r; c++) at(s.N, 8 * o + r, 8 * o + c) += omega[o] * Pm[r * (r + 1) / 2 + c];
                s.g[8 * o + r] += omega[o] * pg[r];
            }
            s.cost_prior += omega[o] * pc;
        }
    };

    System cur, tri;
    assemble(hc.data(), blk, cur);
    double c = cur.cost_data + cur.cost_prior;
    if (!mi_finite(c)) { err = "projective_refine: the cost at the start is not finite"; return MI355_ERR_FAILED; }
    rep.n_free = nf; rep.n_pairs_used = (int)used.size(); rep.n_points = n_points; rep.cost0 = c;
    std::vector<double> M((size_t)D * W), sc((size_t)D), y((size_t)D), ht(hc.size());
    LmState lm;
    // a trial: the scaled damped system by the envelope Cholesky, the blocks at the stepped parameters, their cost
    auto try_step = [&](double lambda, double, double& c2, int& rc) {
        for (int i = 0; i < D; i++) { const double d = at(cur.N, i, i); sc[i] = d > 0.0 ? 1.0 / std::sqrt(d) : 1.0; }
        for (int i = 0; i < D; i++) {
            for (int j = fst[i]; j < i; j++) at(M, i, j) = (sc[i] * at(cur.N, i, j)) * sc[j];
            at(M, i, i) = (sc[i] * at(cur.N, i, i)) * sc[i] + lambda;
            y[i] = sc[i] * cur.g[i];
        }
        if (!envelope_cholesky(M.data(), D, bw, fst)) return false;
        envelope_solve(M.data(), D, bw, fst, y.data(), nullptr);
        ht = hc;
        for (int o = 0; o < nf; o++) for (int r = 0; r < 8; r++) ht[(size_t)8 * freeimg[o] + r] = hc[(size_t)8 * freeimg[o] + r] + sc[8 * o + r] * y[8 * o + r];
        const mi355_pair_normal_block* tb = nullptr;
        int tn = 0;
        rc = src.blocks(ht.data(), part.data(), n_images, &tb, &tn, err);
        if (rc == MI355_OK && tn != nb) { err = "projective_refine: the block count changed between trials"; rc = MI355_ERR_FAILED; }
        if (rc != MI355_OK) return false;
        assemble(ht.data(), tb, tri);
        c2 = tri.cost_data + tri.cost_prior;
        return true;
    };
    { const int rc = mi_lm_run(mi_lm_schedule(P), c, lm, try_step, [&] { hc.swap(ht); std::swap(cur, tri); }); if (rc != MI355_OK) return rc; }
    rep.trials = lm.trials; rep.accepted = lm.accepted;
    rep.cost_data = cur.cost_data; rep.cost_prior = cur.cost_prior; rep.lambda = lm.lambda;
    for (int k : freeimg) {
        for (int j = 0; j < 8; j++) out[k].m[j] = (float)hc[(size_t)8 * k + j];
        out[k].m[8] = 1.0f; out[k].fixed = 0;
    }
    if (report) *report = rep;
    return MI355_OK;
}

extern "C" int mi355_pair_normal_blocks_host(const mi355_pair_result* r, int n, const double* h8, const uint8_t* part, int n_images, mi355_pair_normal_block* out) {
    if (n < 0 || n_images < 1 || !h8 || !part || (n > 0 && (!r || !out))) { mi_set_host_error("pair_normal_blocks_host: bad arguments (n, n_images or a NULL pointer)"); return MI355_ERR_ARG; }
    for (int p = 0; p < n; p++) {
        const PairView v{r[p].i, r[p].j, r[p].n_in, r[p].accepted, reinterpret_cast<const char*>(r[p].a), reinterpret_cast<const char*>(r[p].b), sizeof(mi355_sfpoint)};
        block_host(v, h8, part, n_images, out[p]);
    }
    return MI355_OK;
}

extern "C" int mi355_global_projective_refine_results(const mi355_pair_result* r, int n_pairs, int n_images, const int32_t* w, const int32_t* h,
                                                      const int32_t* fixed, const int32_t* label, const mi355_image_transform* start, const mi355_projective_params* params,
                                                      mi355_image_transform* out, mi355_projective_report* report) {
    std::string err;
    if (n_pairs < 0 || (n_pairs > 0 && !r)) { mi_set_host_error("projective_refine_results: n_pairs = " + std::to_string(n_pairs) + " or NULL records"); return MI355_ERR_ARG; }
    HostSource src;
    for (int p = 0; p < n_pairs; p++)
        if (r[p].accepted) src.views.push_back(PairView{r[p].i, r[p].j, r[p].n_in, 1, reinterpret_cast<const char*>(r[p].a), reinterpret_cast<const char*>(r[p].b), sizeof(mi355_sfpoint)});
    const int rc = mi_projective_refine(src, n_images, w, h, fixed, label, start, params, out, report, err);
    if (rc != MI355_OK) mi_set_host_error(err);
    return rc;
}

extern "C" int mi355_global_projective_refine(const mi355_match_point_pairs* v, int n, int n_images, const int32_t* w, const int32_t* h,
                                              const int32_t* fixed, const int32_t* label, const mi355_image_transform* start, const mi355_projective_params* params,
                                              mi355_image_transform* out, mi355_projective_report* report) {
    std::string err;
    if (n < 0 || (n > 0 && !v)) { mi_set_host_error("projective_refine: n = " + std::to_string(n) + " or a NULL list"); return MI355_ERR_ARG; }
    HostSource src;
    mi_flat_runs(v, n, MI355_MAX_SELECTED, [&](int p, int q) {          // at most 400 per block
        src.views.push_back(PairView{v[p].ptA_i, v[p].ptB_i, q - p, 1, reinterpret_cast<const char*>(&v[p].ptA), reinterpret_cast<const char*>(&v[p].ptB), sizeof(mi355_match_point_pairs)});
    });
    const int rc = mi_projective_refine(src, n_images, w, h, fixed, label, start, params, out, report, err);
    if (rc != MI355_OK) mi_set_host_error(err);
    return rc;
}
