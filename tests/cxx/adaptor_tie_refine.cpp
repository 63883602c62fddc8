// tests/cxx/adaptor_tie_refine.cpp -- mi355::GetMatchedPairsOneToAllSIFT with tie refinement through include/mi355_adaptor.h alone (built and
// run by tests/test_gpu_adaptor_tie_refine.py).
//   adaptor_tie_refine <dir>
// reads <dir>/images.bin (n, then per image int32 w, h, ws, the rows, 9 floats), extracts every frame with "keep_frames" on, and checks:
// ties == NULL gives the bytes of the window overload; with ties the list equals mi355_match_pairs + mi355_refine_ties +
// mi355_results_to_match_pairs applied by hand, and differs from the unrefined list.
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
    if (argc < 2) { std::fprintf(stderr, "usage: adaptor_tie_refine <dir>\n"); return 2; }
    const std::string dir = argv[1];
    mi355_ctx* c = mi355::context();
    if (!c) { std::fprintf(stderr, "no context: %s\n", mi355_last_error(NULL)); return 5; }
    FILE* f = std::fopen((dir + "/images.bin").c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open images.bin\n"); return 3; }
    int n = 0;
    if (std::fread(&n, sizeof(int), 1, f) != 1 || n < 2 || n > 4096) { std::fclose(f); return 3; }
    std::vector<int32_t> fixed(n, 0), ids(n);
    std::vector<int> w(n), h(n), ws(n);
    fixed[0] = 1;
    // without kept frames the refining overload has nothing to read
    std::vector<MatchPointPairs> none;
    mi355_tie_params tp;
    mi355_default_tie_params(&tp);
    if (mi355::GetMatchedPairsOneToAllSIFT(n, 2.5f, 3u, &fixed[0], none, 182, &tp) != MI355_ERR_ARG) { std::fprintf(stderr, "no kept frame was not refused\n"); return 11; }
    mi355_set_option(c, "keep_frames", 1);
    for (int k = 0; k < n; k++) {
        int g[3];
        float h9[9];
        if (std::fread(g, sizeof(int), 3, f) != 3 || g[0] < 16 || g[1] < 16 || g[2] < 3 * g[0]) { std::fclose(f); return 3; }
        std::vector<uint8_t> img((size_t)g[2] * g[1]);
        if (std::fread(&img[0], 1, img.size(), f) != img.size() || std::fread(h9, sizeof(float), 9, f) != 9) { std::fclose(f); return 3; }
        if (mi355_sift_extract(c, k, &img[0], g[0], g[1], g[2], NULL, NULL, 0, NULL) != MI355_OK) { std::fprintf(stderr, "extract: %s\n", mi355_last_error(c)); return 4; }
        ids[k] = k; w[k] = g[0]; h[k] = g[1]; ws[k] = g[2];
    }
    std::fclose(f);
    std::vector<MatchPointPairs> plain, null_ties, refined, by_hand;
    if (mi355::GetMatchedPairsOneToAllSIFT(n, 2.5f, 3u, &fixed[0], plain, 182) != 0) { std::fprintf(stderr, "window form: %s\n", mi355_last_error(c)); return 6; }
    if (mi355::GetMatchedPairsOneToAllSIFT(n, 2.5f, 3u, &fixed[0], null_ties, 182, (const mi355_tie_params*)NULL) != 0) return 6;
    if (plain.empty() || !same(plain, null_ties)) { std::fprintf(stderr, "ties == NULL changed the list\n"); return 7; }
    tp.drop_mask = 0x3c;
    if (mi355::GetMatchedPairsOneToAllSIFT(n, 2.5f, 3u, &fixed[0], refined, 182, &tp) != 0) { std::fprintf(stderr, "refining form: %s\n", mi355_last_error(c)); return 8; }
    // by hand
    int n_pairs = 0;
    mi355_pair_schedule(n, 182, 0, 1, NULL, 0, &n_pairs);
    std::vector<int32_t> pairs((size_t)n_pairs * 2);
    mi355_pair_schedule(n, 182, 0, 1, &pairs[0], n_pairs, &n_pairs);
    std::vector<mi355_pair_result> res(n_pairs), out(n_pairs);
    std::vector<mi355_tie_report> rep(n_pairs);
    if (mi355_match_pairs(c, &pairs[0], n_pairs, 2.5f, 3u, &res[0]) != MI355_OK) return 9;
    if (mi355_refine_ties(c, &res[0], n_pairs, NULL, &ids[0], &w[0], &h[0], &ws[0], n, &tp, &out[0], NULL, NULL, &rep[0]) != MI355_OK) { std::fprintf(stderr, "refine_ties: %s\n", mi355_last_error(c)); return 9; }
    mi355_match_point_pairs* v = NULL; int nv = 0;
    if (mi355_results_to_match_pairs(&out[0], n_pairs, &fixed[0], &v, &nv) != MI355_OK) return 9;
    by_hand.resize(nv);
    if (nv) std::memcpy(&by_hand[0], v, sizeof(mi355_match_point_pairs) * nv);
    mi355_free(v);
    if (!same(refined, by_hand)) { std::fprintf(stderr, "the overload differs from mi355_refine_ties by hand\n"); return 10; }
    long n_ref = 0, n_all = 0;
    for (int p = 0; p < n_pairs; p++) if (rep[p].flags == 0 || rep[p].flags == MI355_TIE_FLAG_DEMOTED) { n_ref += rep[p].count[MI355_TIE_REFINED]; n_all += rep[p].n_in; }
    if (n_ref == 0 || same(refined, plain)) { std::fprintf(stderr, "nothing was refined\n"); return 12; }
    std::printf("ADAPTOR TIE REFINE OK pairs %d ties %ld refined %ld list %d -> %d\n", n_pairs, n_all, n_ref, (int)plain.size(), (int)refined.size());
    return 0;
}
