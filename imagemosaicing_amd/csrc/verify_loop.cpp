// csrc/verify_loop.cpp -- the host half of pair verification (include/mi355_mosaic.h, "pair verification"): the adjacency of the testable
// edges and stage 3, the loop.  No HIP: the loop sees its records through a VerifySource (verify.h) and aligns with the library's own
// mi355_select_connected_moments / mi355_global_affine_align_moments, so what it returns is what they return for the kept records.
#include "verify.h"
#include <algorithm>
#include <cmath>
#include <limits>

namespace {
enum State : uint8_t { NOT_USED = 0, KEPT = 1, PENDING = 2, REJECTED = 3 };
int sum_labelled(const std::vector<int32_t>& label) { int c = 0; for (int32_t v : label) c += v != 0; return c; }
}

int mi_verify_check(int n_pairs, int n_images, const mi355_verify_params* params, mi355_verify_params& p, std::string& err) {
    if (params) p = *params; else mi355_default_verify_params(&p);
    const char* names[3] = {"cycle_tol", "gate_abs", "gate_k"};
    const double vals[3] = {p.cycle_tol, p.gate_abs, p.gate_k};
    for (int q = 0; q < 3; q++)
        if (!(vf_finite(vals[q]) && vals[q] > 0.0)) { err = std::string(names[q]) + "=" + std::to_string(vals[q]) + " must be finite and > 0"; return MI355_ERR_ARG; }
    if (p.max_rounds < 1) { err = "max_rounds=" + std::to_string(p.max_rounds) + " < 1"; return MI355_ERR_ARG; }
    if (n_images < 1 || n_images > VF_MAX_IMAGES) { err = "n_images=" + std::to_string(n_images) + " outside [1, 65535]"; return MI355_ERR_ARG; }
    if (n_pairs < 0) { err = "n_pairs=" + std::to_string(n_pairs) + " < 0"; return MI355_ERR_ARG; }
    return MI355_OK;
}

int mi_verify_adjacency(const mi355_pair_edge* edges, int n, int n_images, std::vector<int32_t>& row, std::vector<VfAdj>& adj, std::string& err) {
    // what a kernel indexes with is checked here: a usable or testable edge names two different frames inside the table
    struct Key { uint64_t pair; int32_t rec; };
    std::vector<Key> keys;
    row.assign((size_t)n_images + 1, 0);
    for (int p = 0; p < n; p++) {
        const mi355_pair_edge& e = edges[p];
        if (!(e.flags & (MI355_EDGE_USABLE | MI355_EDGE_TESTABLE))) continue;
        if (e.i < 0 || e.j < 0 || e.i >= n_images || e.j >= n_images || e.i == e.j) {
            err = "edge " + std::to_string(p) + " is flagged usable with i=" + std::to_string(e.i) + ", j=" + std::to_string(e.j) + " (n_images=" + std::to_string(n_images) + ")";
            return MI355_ERR_ARG;
        }
        const uint32_t lo = (uint32_t)(e.i < e.j ? e.i : e.j), hi = (uint32_t)(e.i < e.j ? e.j : e.i);
        keys.push_back(Key{((uint64_t)lo << 32) | hi, p});
        if (e.flags & MI355_EDGE_TESTABLE) { row[(size_t)e.i + 1]++; row[(size_t)e.j + 1]++; }
    }
    std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.pair != b.pair ? a.pair < b.pair : a.rec < b.rec; });
    for (size_t q = 1; q < keys.size(); q++)
        if (keys[q].pair == keys[q - 1].pair) {
            err = "records " + std::to_string(keys[q - 1].rec) + " and " + std::to_string(keys[q].rec) + " are both usable records of the frame pair (" +
                  std::to_string((uint32_t)(keys[q].pair >> 32)) + ", " + std::to_string((uint32_t)keys[q].pair) + ")";
            return MI355_ERR_ARG;
        }
    for (int k = 0; k < n_images; k++) row[(size_t)k + 1] += row[k];
    adj.assign((size_t)row[n_images], VfAdj{0, 0u});
    std::vector<int32_t> fill(row.begin(), row.end() - 1);
    for (int p = 0; p < n; p++) {
        const mi355_pair_edge& e = edges[p];
        if (!(e.flags & MI355_EDGE_TESTABLE)) continue;
        adj[(size_t)fill[e.i]++] = VfAdj{e.j, ((uint32_t)p << 1) | 1u};
        adj[(size_t)fill[e.j]++] = VfAdj{e.i, ((uint32_t)p << 1)};
    }
    for (int k = 0; k < n_images; k++)          // no two entries of a list name the same neighbour (the duplicate check above)
        std::sort(adj.begin() + row[k], adj.begin() + row[(size_t)k + 1], [](const VfAdj& a, const VfAdj& b) { return a.nbr < b.nbr; });
    return MI355_OK;
}

int mi_verify_loop(VerifySource& src, int n_pairs, int n_images, const int32_t* fixed, const mi355_verify_params& p, uint8_t* demote,
                   int32_t* label_out, mi355_image_transform* transforms_out, mi355_verify_report* report, mi355_verify_summary* summary,
                   std::string& err) {
    const int n = n_pairs;
    const mi355_pair_moments* mom = nullptr;
    { const int rc = src.moments(&mom, err); if (rc != MI355_OK) return rc; }
    for (int q = 0; q < n; q++)
        if (mom[q].n_in > 0 && (mom[q].n_in > MI355_MAX_SELECTED || mom[q].i < 0 || mom[q].i >= n_images || mom[q].j < 0 || mom[q].j >= n_images)) {
            err = "record " + std::to_string(q) + " is accepted with n_in=" + std::to_string(mom[q].n_in) + ", i=" + std::to_string(mom[q].i) + ", j=" +
                  std::to_string(mom[q].j) + " (n_images=" + std::to_string(n_images) + ")";
            return MI355_ERR_ARG;
        }
    const mi355_pair_edge* edges = nullptr;
    { const int rc = src.edges(&edges, err); if (rc != MI355_OK) return rc; }
    std::vector<int32_t> row;
    std::vector<VfAdj> adj;
    if (mi_verify_adjacency(edges, n, n_images, row, adj, err) != MI355_OK) return MI355_ERR_ARG;
    const mi355_pair_cycle* cyc = nullptr;
    { const int rc = src.cycles(edges, row, adj, p.cycle_tol, &cyc, err); if (rc != MI355_OK) return rc; }

    std::vector<uint8_t> state((size_t)n, NOT_USED);
    std::vector<int32_t> verdict((size_t)n, MI355_VERDICT_NOT_USED), round((size_t)n, 0);
    auto usable = [&](int q) { return (edges[q].flags & MI355_EDGE_USABLE) != 0; };
    auto untested = [&](int q) { return state[q] == PENDING && cyc[q].n_ok == 0 && cyc[q].n_bad == 0; };
    int n_kept = 0;
    for (int q = 0; q < n; q++) {
        if (!usable(q)) continue;
        if (cyc[q].n_ok >= 1 && cyc[q].n_ok > cyc[q].n_bad) { state[q] = KEPT; verdict[q] = MI355_VERDICT_VERIFIED; n_kept++; }
        else state[q] = PENDING;
    }
    if (n_kept == 0) {
        int best = -1;
        for (int q = 0; q < n; q++)
            if (untested(q) && (best < 0 || edges[q].n_in > edges[best].n_in)) best = q;
        if (best < 0) { err = "no pair could be verified"; return MI355_ERR_FAILED; }
        state[best] = KEPT; verdict[best] = MI355_VERDICT_BRIDGE;
    }

    std::vector<mi355_pair_moments> mk((size_t)(n > 0 ? n : 1));
    std::vector<int32_t> label((size_t)n_images, 0);
    std::vector<mi355_image_transform> tr((size_t)n_images);
    std::vector<float> h9s((size_t)n_images * 9);
    std::vector<double> rms((size_t)n), sorted;
    const mi355_pair_residual* res = nullptr;
    double s = 0.0, gate = p.gate_abs;
    // steps 1 to 3 for the pairs KEPT now.  The solver needs a fixed frame among the labelled ones: a round whose component holds none (the
    // seed pair far from frame 0) anchors the lowest labelled frame for that round's alignment only; the output pass does not, and refuses.
    std::vector<int32_t> fixed_round((size_t)n_images);
    bool anchored = false;
    auto align_and_measure = [&](bool final_pass) -> int {
        for (int q = 0; q < n; q++) { mk[q] = mom[q]; if (state[q] != KEPT) mk[q].n_in = 0; }
        if (mi355_select_connected_moments(mk.data(), n, n_images, label.data()) != MI355_OK) { err = "select_connected_moments refused the kept pairs"; return MI355_ERR_FAILED; }
        int lowest = -1;
        bool has_fixed = false;
        for (int k = 0; k < n_images; k++) {
            fixed_round[k] = fixed ? (fixed[k] != 0) : (k == 0);
            if (label[k] && lowest < 0) lowest = k;
            if (label[k] && fixed_round[k]) has_fixed = true;
        }
        anchored = !has_fixed && lowest >= 0;
        if (anchored && final_pass) { err = "no fixed frame among the " + std::to_string(sum_labelled(label)) + " frames the kept pairs connect"; return MI355_ERR_FAILED; }
        if (anchored) fixed_round[lowest] = 1;
        const int rc = mi355_global_affine_align_moments(mk.data(), n, n_images, anchored ? fixed_round.data() : fixed, label.data(), tr.data());
        if (rc != MI355_OK) { err = "global_affine_align_moments failed on the kept pairs (" + std::to_string(rc) + ")"; return rc; }
        for (int k = 0; k < n_images; k++) memcpy(&h9s[(size_t)9 * k], tr[k].m, sizeof(float) * 9);
        { const int rc2 = src.residuals(h9s.data(), label.data(), &res, err); if (rc2 != MI355_OK) return rc2; }
        sorted.clear();
        for (int q = 0; q < n; q++) {
            rms[q] = res[q].n_used > 0 ? std::sqrt(res[q].sum_r2 / (double)res[q].n_used) : std::numeric_limits<double>::infinity();
            if (state[q] == KEPT && vf_measured(1, edges[q].n_in, edges[q].i, edges[q].j, n_images, h9s.data(), label.data())) sorted.push_back(rms[q]);
        }
        std::sort(sorted.begin(), sorted.end());
        s = sorted.empty() ? 0.0 : sorted[(sorted.size() - 1) / 2];
        const double g = p.gate_k * s;
        gate = g > p.gate_abs ? g : p.gate_abs;
        return MI355_OK;
    };

    int rounds = 0;
    bool fresh = false;                    // label, transforms and residuals belong to the pairs KEPT now and to the caller's fixed
    for (int r = 1; r <= p.max_rounds; r++) {
        rounds = r;
        { const int rc = align_and_measure(false); if (rc != MI355_OK) return rc; }
        fresh = !anchored;
        bool changed = false;
        for (int q = 0; q < n; q++) {
            if (state[q] != PENDING || !vf_measured(1, edges[q].n_in, edges[q].i, edges[q].j, n_images, h9s.data(), label.data())) continue;
            if (rms[q] <= gate) { state[q] = KEPT; verdict[q] = MI355_VERDICT_ADMITTED; }
            else { state[q] = REJECTED; verdict[q] = MI355_VERDICT_REJECTED; }
            round[q] = r;
            changed = true;
        }
        if (!changed && p.bridges != 0) {
            std::vector<int32_t> best((size_t)n_images);
            for (;;) {
                std::fill(best.begin(), best.end(), -1);
                for (int q = 0; q < n; q++) {
                    if (!untested(q)) continue;
                    const int a = edges[q].i, b = edges[q].j;
                    const int f = (label[a] != 0 && label[b] == 0) ? b : (label[b] != 0 && label[a] == 0) ? a : -1;
                    if (f >= 0 && (best[f] < 0 || edges[q].n_in > edges[best[f]].n_in)) best[f] = q;
                }
                bool any = false;
                for (int k = 0; k < n_images; k++) {
                    if (best[k] < 0) continue;
                    state[best[k]] = KEPT; verdict[best[k]] = MI355_VERDICT_BRIDGE; round[best[k]] = r;
                    label[k] = 1;
                    any = true;
                }
                if (!any) break;
                changed = true;
            }
        }
        if (!changed) break;
        fresh = false;
    }
    if (!fresh) { const int rc = align_and_measure(true); if (rc != MI355_OK) return rc; }

    mi355_verify_summary sum;
    memset(&sum, 0, sizeof(sum));
    sum.rounds = rounds; sum.s = s; sum.gate = gate;
    for (int k = 0; k < n_images; k++) { label_out[k] = label[k]; transforms_out[k] = tr[k]; if (label[k]) sum.n_labelled++; }
    for (int q = 0; q < n; q++) {
        if (state[q] == PENDING) verdict[q] = MI355_VERDICT_UNDECIDED;
        demote[q] = (usable(q) && state[q] != KEPT) ? 1 : 0;
        sum.count[verdict[q]]++;
        if (!report) continue;
        mi355_verify_report& o = report[q];
        memset(&o, 0, sizeof(o));
        o.i = edges[q].i; o.j = edges[q].j; o.n_in = edges[q].n_in; o.verdict = verdict[q];
        o.n_ok = cyc[q].n_ok; o.n_bad = cyc[q].n_bad; o.round = round[q];
        o.min_e2 = cyc[q].min_e2; o.rms = rms[q]; o.max_r2 = res[q].max_r2;
        o.flags = (state[q] == KEPT && res[q].n_used > 0 && rms[q] > gate) ? MI355_VERIFY_SUSPECT : 0;
    }
    if (summary) *summary = sum;
    return MI355_OK;
}
