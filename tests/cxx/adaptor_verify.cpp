// tests/cxx/adaptor_verify.cpp -- mi355::GetMatchedPairsOneToAllSIFT with pair verification through include/mi355_adaptor.h alone (built and
// run by tests/test_gpu_adaptor_verify.py).
//   adaptor_verify <dir>
// reads <dir>/images.bin (n, then per image int32 w, h, ws, the rows, 9 floats), extracts every frame, and checks: the verifying overload's
// list equals mi355_match_pairs + mi355_verify_pairs_results + mi355_results_to_match_pairs applied by hand and is a part of the window
// form's list (every kept record's correspondences, nothing else); with one verified record's ties moved by a period the by-hand path no
// longer keeps that pair; bad parameters are refused and leave the list alone.  The middle frame is the fixed one: a short strip's end
// frames have thin overlaps and may drop out (the header's limit on surveys with little redundancy).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mi355_adaptor.h"

using namespace mi355ref;

static bool same(const std::vector<MatchPointPairs>& a, const std::vector<MatchPointPairs>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(&a[0], &b[0], sizeof(MatchPointPairs) * a.size()) == 0);
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: adaptor_verify <dir>\n"); return 2; }
    const std::string dir = argv[1];
    mi355_ctx* c = mi355::context();
    if (!c) { std::fprintf(stderr, "no context: %s\n", mi355_last_error(NULL)); return 5; }
    FILE* f = std::fopen((dir + "/images.bin").c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open images.bin\n"); return 3; }
    int n = 0;
    if (std::fread(&n, sizeof(int), 1, f) != 1 || n < 3 || n > 4096) { std::fclose(f); return 3; }
    std::vector<int32_t> fixed(n, 0);
    const int anchor = n / 2;
    fixed[anchor] = 1;
    for (int k = 0; k < n; k++) {
        int g[3];
        float h9[9];
        if (std::fread(g, sizeof(int), 3, f) != 3 || g[0] < 16 || g[1] < 16 || g[2] < 3 * g[0]) { std::fclose(f); return 3; }
        std::vector<uint8_t> img((size_t)g[2] * g[1]);
        if (std::fread(&img[0], 1, img.size(), f) != img.size() || std::fread(h9, sizeof(float), 9, f) != 9) { std::fclose(f); return 3; }
        if (mi355_sift_extract(c, k, &img[0], g[0], g[1], g[2], NULL, NULL, 0, NULL) != MI355_OK) { std::fprintf(stderr, "extract: %s\n", mi355_last_error(c)); return 4; }
    }
    std::fclose(f);
    std::vector<MatchPointPairs> plain, verified, by_hand;
    if (mi355::GetMatchedPairsOneToAllSIFT(n, 2.5f, 3u, &fixed[0], plain, 182) != 0) { std::fprintf(stderr, "window form: %s\n", mi355_last_error(c)); return 6; }
    mi355_verify_params vp;
    mi355_default_verify_params(&vp);
    mi355_verify_summary sum;
    if (mi355::GetMatchedPairsOneToAllSIFT(n, 2.5f, 3u, &fixed[0], verified, 182, &vp, &sum) != 0) { std::fprintf(stderr, "verifying form: %s\n", mi355_last_error(NULL)); return 8; }
    // by hand
    int n_pairs = 0;
    mi355_pair_schedule(n, 182, 0, 1, NULL, 0, &n_pairs);
    std::vector<int32_t> pairs((size_t)n_pairs * 2), label(n);
    mi355_pair_schedule(n, 182, 0, 1, &pairs[0], n_pairs, &n_pairs);
    std::vector<mi355_pair_result> res(n_pairs), out(n_pairs);
    std::vector<mi355_verify_report> rep(n_pairs);
    std::vector<mi355_image_transform> tr(n);
    mi355_verify_summary sum2;
    if (mi355_match_pairs(c, &pairs[0], n_pairs, 2.5f, 3u, &res[0]) != MI355_OK) return 9;
    if (mi355_verify_pairs_results(&res[0], n_pairs, n, &fixed[0], &vp, &out[0], &label[0], &tr[0], &rep[0], &sum2) != MI355_OK) { std::fprintf(stderr, "verify: %s\n", mi355_last_error(NULL)); return 9; }
    mi355_match_point_pairs* v = NULL; int nv = 0;
    if (mi355_results_to_match_pairs(&out[0], n_pairs, &fixed[0], &v, &nv) != MI355_OK) return 9;
    by_hand.resize(nv);
    if (nv) std::memcpy(&by_hand[0], v, sizeof(mi355_match_point_pairs) * nv);
    mi355_free(v);
    if (verified.empty() || !same(verified, by_hand)) { std::fprintf(stderr, "the overload differs from mi355_verify_pairs_results by hand\n"); return 10; }
    if (std::memcmp(&sum, &sum2, sizeof(sum)) != 0) { std::fprintf(stderr, "the overload's summary differs\n"); return 10; }
    int n_acc = 0, n_kept = 0;
    long ties_kept = 0;
    for (int p = 0; p < n_pairs; p++) {
        n_acc += res[p].accepted ? 1 : 0;
        if (!out[p].accepted) continue;
        n_kept++;
        ties_kept += out[p].n_in;
        if (std::memcmp(&out[p], &res[p], sizeof(mi355_pair_result)) != 0) { std::fprintf(stderr, "kept record %d was changed\n", p); return 11; }
    }
    if (n_kept < 3 || n_kept > n_acc || (long)verified.size() != ties_kept || verified.size() > plain.size() || sum.count[MI355_VERDICT_VERIFIED] < 3) {
        std::fprintf(stderr, "%d accepted, %d kept, %d verified, list %d of %d, ties kept %ld\n", n_acc, n_kept, sum.count[MI355_VERDICT_VERIFIED], (int)verified.size(),
                     (int)plain.size(), ties_kept);
        return 11;
    }
    // one verified pair matched a period off: its b list moves by (40, 5) and its H with it (H maps b to a: H' = H T(-40, -5)).  The pair
    // is one between two frames that are not neighbours and not the fixed one, so that the strip stays connected without it.
    int victim = -1;
    for (int p = 0; p < n_pairs && victim < 0; p++)
        if (rep[p].verdict == MI355_VERDICT_VERIFIED && res[p].i != anchor && res[p].j != anchor && (res[p].j - res[p].i > 1 || res[p].i - res[p].j > 1)) victim = p;
    for (int p = 0; p < n_pairs && victim < 0; p++) if (rep[p].verdict == MI355_VERDICT_VERIFIED && res[p].i != anchor && res[p].j != anchor) victim = p;
    if (victim < 0) { std::fprintf(stderr, "no verified pair beside the fixed frame\n"); return 12; }
    mi355_pair_result& e = res[victim];
    for (int k = 0; k < e.n_in; k++) { e.b[k].x += 40.0f; e.b[k].y += 5.0f; }
    e.H[2] = e.H[2] - (e.H[0] * 40.0f + e.H[1] * 5.0f);
    e.H[5] = e.H[5] - (e.H[3] * 40.0f + e.H[4] * 5.0f);
    if (mi355_verify_pairs_results(&res[0], n_pairs, n, &fixed[0], &vp, &out[0], &label[0], &tr[0], &rep[0], &sum2) != MI355_OK) { std::fprintf(stderr, "verify: %s\n", mi355_last_error(NULL)); return 13; }
    if (out[victim].accepted || (rep[victim].verdict != MI355_VERDICT_REJECTED && rep[victim].verdict != MI355_VERDICT_UNDECIDED)) {
        std::fprintf(stderr, "the shifted pair (record %d) has the verdict %d\n", victim, rep[victim].verdict);
        return 14;
    }
    if (out[victim].n_in != res[victim].n_in || out[victim].H[0] != 0.0f || out[victim].ok) { std::fprintf(stderr, "the shifted pair is not demoted by the convention\n"); return 14; }
    if (sum2.count[MI355_VERDICT_VERIFIED] + sum2.count[MI355_VERDICT_ADMITTED] + sum2.count[MI355_VERDICT_BRIDGE] < 2) { std::fprintf(stderr, "nothing else was kept\n"); return 14; }
    // a refusal leaves the list alone
    vp.cycle_tol = 0.0;
    const size_t before = verified.size();
    if (mi355::GetMatchedPairsOneToAllSIFT(n, 2.5f, 3u, &fixed[0], verified, 182, &vp, (mi355_verify_summary*)NULL) != MI355_ERR_ARG || verified.size() != before) {
        std::fprintf(stderr, "cycle_tol = 0 was not refused\n");
        return 15;
    }
    std::printf("ADAPTOR VERIFY OK pairs %d accepted %d kept %d verified %d admitted %d bridges %d list %d\n", n_pairs, n_acc, n_kept, sum.count[MI355_VERDICT_VERIFIED],
                sum.count[MI355_VERDICT_ADMITTED], sum.count[MI355_VERDICT_BRIDGE], (int)verified.size());
    return 0;
}
