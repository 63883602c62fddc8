// tests/cxx/projective_sanitize.cpp -- the projective refinement's host code (csrc/projective_solve.cpp with csrc/host_io.cpp's affine
// alignment for the start) under sanitizers, as a stand-alone program: a strip of 150 frames, every frame tied to its neighbour and to the
// frame 30 further on -- 1192 unknowns, an envelope of 240 columns, 7e7 multiply-subtracts per factorisation: a team of two threads (the
// test sets MI355_HOST_THREADS=4; the blocks use four).  Checks: the refinement runs, lowers the cost, and gives the same bits twice and
// from the flat list.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "mi355_mosaic.h"

static std::string g_err;
void mi_set_host_error(const std::string& s) { g_err = s; }            // api.hip's, for a program without the HIP units

static unsigned long long g_state = 88172645463325252ull;
static double uniform() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (double)(g_state >> 11) / 9007199254740992.0; }

int main() {
    const int n = 150, W = 640, H = 480, PER = 24;
    const double step = 10.0;
    std::vector<mi355_pair_result> recs;
    for (int k = 0; k < n; k++)
        for (int d : {1, 30}) {
            if (k + d >= n) continue;
            mi355_pair_result r;
            memset(&r, 0, sizeof(r));
            r.i = k; r.j = k + d; r.n_in = PER; r.n_selected = PER; r.ok = 1; r.accepted = 1;
            for (int q = 0; q < PER; q++) {
                const double cx = step * (k + d) + uniform() * (W - 1 - step * d), cy = uniform() * (H - 1);
                r.a[q].x = (float)(cx - step * k + 0.3 * (uniform() - 0.5)); r.a[q].y = (float)(cy + 0.3 * (uniform() - 0.5));
                r.b[q].x = (float)(cx - step * (k + d) + 0.3 * (uniform() - 0.5)); r.b[q].y = (float)(cy + 0.3 * (uniform() - 0.5));
            }
            recs.push_back(r);
        }
    recs[3].accepted = 0;
    std::vector<mi355_image_transform> start(n), out(n), again(n), flat_out(n);
    if (mi355_global_affine_align_results(recs.data(), (int)recs.size(), n, nullptr, nullptr, start.data()) != MI355_OK) { printf("affine start failed\n"); return 1; }
    std::vector<int32_t> w(n, W), h(n, H);
    mi355_projective_params p;
    mi355_default_projective_params(&p);
    p.max_iters = 2;
    mi355_projective_report rep, rep2, rep3;
    if (mi355_global_projective_refine_results(recs.data(), (int)recs.size(), n, w.data(), h.data(), nullptr, nullptr, start.data(), &p, out.data(), &rep) != MI355_OK) { printf("refine failed: %s\n", g_err.c_str()); return 1; }
    if (mi355_global_projective_refine_results(recs.data(), (int)recs.size(), n, w.data(), h.data(), nullptr, nullptr, start.data(), &p, again.data(), &rep2) != MI355_OK) return 1;
    if (rep.n_free != n - 1 || rep.accepted < 1 || !(rep.cost_data < rep.cost0)) { printf("report: free %d accepted %d cost %g -> %g\n", rep.n_free, rep.accepted, rep.cost0, rep.cost_data); return 2; }
    if (memcmp(out.data(), again.data(), sizeof(out[0]) * n) != 0 || memcmp(&rep, &rep2, sizeof(rep)) != 0) { printf("two calls differ\n"); return 3; }
    std::vector<mi355_match_point_pairs> flat;
    for (const mi355_pair_result& r : recs) {
        if (!r.accepted) continue;
        for (int q = 0; q < r.n_in; q++) {
            mi355_match_point_pairs m;
            memset(&m, 0, sizeof(m));
            m.ptA = r.a[q]; m.ptA_i = r.i; m.ptB = r.b[q]; m.ptB_i = r.j;
            flat.push_back(m);
        }
    }
    if (mi355_global_projective_refine(flat.data(), (int)flat.size(), n, w.data(), h.data(), nullptr, nullptr, start.data(), &p, flat_out.data(), &rep3) != MI355_OK) return 1;
    if (memcmp(out.data(), flat_out.data(), sizeof(out[0]) * n) != 0 || memcmp(&rep, &rep3, sizeof(rep)) != 0) { printf("the flat list differs\n"); return 4; }
    // the error paths release what they hold
    p.lambda_up = 1.0;
    if (mi355_global_projective_refine_results(recs.data(), (int)recs.size(), n, w.data(), h.data(), nullptr, nullptr, start.data(), &p, out.data(), &rep) != MI355_ERR_ARG || g_err.find("lambda_up") == std::string::npos) return 5;
    mi355_default_projective_params(&p);
    recs[5].n_in = 401;
    if (mi355_global_projective_refine_results(recs.data(), (int)recs.size(), n, w.data(), h.data(), nullptr, nullptr, start.data(), &p, out.data(), &rep) != MI355_ERR_ARG) return 5;
    std::vector<double> h8((size_t)8 * n, 0.0);
    std::vector<uint8_t> part(n, 1);
    for (int k = 0; k < n; k++) for (int j = 0; j < 8; j++) h8[8 * k + j] = start[k].m[j];
    std::vector<mi355_pair_normal_block> blk(recs.size());
    if (mi355_pair_normal_blocks_host(recs.data(), (int)recs.size(), h8.data(), part.data(), n, blk.data()) != MI355_OK || blk[5].n_in != 401 || blk[5].cost != 0.0 || blk[3].n_in != 0) return 6;
    printf("SANITIZE_OK trials %d accepted %d cost %.6g -> %.6g\n", rep2.trials, rep2.accepted, rep2.cost0, rep2.cost_data);
    return 0;
}
