// tests/cxx/adaptor_local_warp.cpp -- mi355::LocalRegistration through include/mi355_adaptor.h alone (built with MI355_ADAPTOR_KEEP_FRAMES and
// run by tests/test_gpu_adaptor_local_warp.py).
//   adaptor_local_warp <dir>
// reads <dir>/images.bin (n, then per image int32 w, h, ws, the rows, 9 floats), runs the driver's sequence -- SIFT front-end over
// ImagePoseInfo frames (kept in HBM), global alignment, MosaicImagesRefined -- then mi355::LocalRegistration and the render again, and checks:
// without kept frames the call is refused; its grids equal mi355_tie_residual_stats_host + mi355_solve_local_warps on records cut by hand;
// the second render equals mi355_local_register_results + mi355_mosaic_refined_into applied by hand to second copies of the frames, and
// differs from the first; the host images are unchanged.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mi355_adaptor.h"

using namespace mi355ref;

static std::vector<mi355_pair_result> cut_records(const std::vector<MatchPointPairs>& v) {
    std::vector<mi355_pair_result> rec;
    for (size_t p = 0; p < v.size(); p++) {
        if (rec.empty() || rec.back().i != v[p].ptA_i || rec.back().j != v[p].ptB_i || rec.back().n_in == 400) {
            mi355_pair_result r;
            std::memset(&r, 0, sizeof(r));
            r.i = v[p].ptA_i; r.j = v[p].ptB_i; r.ok = 1; r.accepted = 1;
            rec.push_back(r);
        }
        mi355_pair_result& r = rec.back();
        r.a[r.n_in].x = v[p].ptA.x; r.a[r.n_in].y = v[p].ptA.y; r.a[r.n_in].id = v[p].ptA.id;
        r.b[r.n_in].x = v[p].ptB.x; r.b[r.n_in].y = v[p].ptB.y; r.b[r.n_in].id = v[p].ptB.id;
        r.n_in++; r.n_selected = r.n_in;
    }
    return rec;
}

static bool same_image(const IplImage* a, const IplImage* b) {
    if (!a || !b || a->width != b->width || a->height != b->height) return false;
    for (int y = 0; y < a->height; y++)
        if (std::memcmp(a->imageData + (size_t)y * a->widthStep, b->imageData + (size_t)y * b->widthStep, (size_t)3 * a->width) != 0) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: adaptor_local_warp <dir>\n"); return 2; }
    const std::string dir = argv[1];
    mi355_ctx* c = mi355::context();
    if (!c) { std::fprintf(stderr, "no context: %s\n", mi355_last_error(NULL)); return 5; }
    FILE* f = std::fopen((dir + "/images.bin").c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open images.bin\n"); return 3; }
    int n = 0;
    if (std::fread(&n, sizeof(int), 1, f) != 1 || n < 2 || n > 4096) { std::fclose(f); return 3; }
    std::vector<ImagePoseInfo> poses(n);
    std::vector<std::vector<char> > copies(n);
    for (int k = 0; k < n; k++) {
        int g[3];
        float h9[9];
        if (std::fread(g, sizeof(int), 3, f) != 3 || g[0] < 16 || g[1] < 16 || g[2] < 3 * g[0]) { std::fclose(f); return 3; }
        IplImage* im = cvCreateImage8U(g[0], g[1], 3);
        if (!im) { std::fclose(f); return 4; }
        std::vector<char> row((size_t)g[2]);
        for (int y = 0; y < g[1]; y++) {
            if (std::fread(&row[0], 1, (size_t)g[2], f) != (size_t)g[2]) { std::fclose(f); return 3; }
            std::memcpy(im->imageData + (size_t)y * im->widthStep, &row[0], (size_t)3 * g[0]);
        }
        if (std::fread(h9, sizeof(float), 9, f) != 9) { std::fclose(f); return 3; }
        poses[k].pImg = im;
        poses[k].fixed = k == 0 ? 1 : 0;
        copies[k].assign(im->imageData, im->imageData + im->imageSize);
    }
    std::fclose(f);
    std::vector<ImageTransform> T(n);
    for (int k = 0; k < n; k++) { std::memset(&T[k], 0, sizeof(T[k])); T[k].h.m[0] = T[k].h.m[4] = T[k].h.m[8] = 1.0f; }
    // nothing is kept yet: refused
    if (mi355::LocalRegistration(NULL, 0, &T[0], n) != MI355_ERR_ARG) { std::fprintf(stderr, "no kept frame was not refused\n"); return 11; }
    if (mi355::LocalRegistration(NULL, 0, NULL, n) != -1 || mi355::LocalRegistration(NULL, 3, &T[0], n) != -1) { std::fprintf(stderr, "bad arguments were not refused\n"); return 11; }
    std::vector<MatchPointPairs> pairs;
    int nSuccess = 0;
    if (mi355::GetMatchedPairsOneToAllSIFT_MultiThread(&poses[0], n, pairs, nSuccess, 2.5f, 3u) != 0) { std::fprintf(stderr, "match: %s\n", mi355_last_error(c)); return 6; }
    std::vector<int32_t> fixed(n, 0);
    fixed[0] = 1;
    if (pairs.empty() || mi355_global_affine_align(reinterpret_cast<const mi355_match_point_pairs*>(&pairs[0]), (int)pairs.size(), n, &fixed[0],
                                                   reinterpret_cast<mi355_image_transform*>(&T[0])) != MI355_OK) { std::fprintf(stderr, "align failed\n"); return 7; }
    IplImage *before = NULL, *after = NULL;
    if (mi355::MosaicImagesRefined(&poses[0], n, &T[0], before) != 0) { std::fprintf(stderr, "render failed\n"); return 8; }
    // second copies of the frames under ids n .. 2n - 1, for the sequence by hand
    std::vector<uint8_t*> second(n);
    std::vector<int32_t> ids2(n);
    std::vector<int> w(n), h(n), ws(n);
    std::vector<float> h9s((size_t)9 * n);
    for (int k = 0; k < n; k++) {
        const IplImage* im = poses[k].pImg;
        if (mi355_sift_extract(c, n + k, (const uint8_t*)im->imageData, im->width, im->height, im->widthStep, NULL, NULL, 0, NULL) != MI355_OK) { std::fprintf(stderr, "extract: %s\n", mi355_last_error(c)); return 4; }
        const uint8_t* d = NULL;
        if (mi355_get_frame_dev(c, n + k, &d, &w[k], &h[k], &ws[k]) != MI355_OK) { std::fprintf(stderr, "get_frame_dev: %s\n", mi355_last_error(c)); return 4; }
        second[k] = const_cast<uint8_t*>(d);
        ids2[k] = n + k;
        std::memcpy(&h9s[(size_t)9 * k], T[k].h.m, 9 * sizeof(float));
    }
    mi355_local_warp_params lp;
    mi355_default_local_warp_params(&lp);
    const size_t gsz = (size_t)n * (lp.grid_y + 1) * (lp.grid_x + 1) * 2;
    std::vector<float> grids(gsz, 7.0f), grids_host(gsz, 9.0f), grids_hand(gsz, 11.0f);
    std::vector<mi355_local_warp_report> rep(n), rep_host(n);
    if (mi355::LocalRegistration(&pairs[0], (int)pairs.size(), &T[0], n, NULL, &grids[0], &rep[0]) != 0) { std::fprintf(stderr, "LocalRegistration: %s\n", mi355_last_error(c)); return 9; }
    if (mi355::MosaicImagesRefined(&poses[0], n, &T[0], after) != 0) { std::fprintf(stderr, "render failed\n"); return 8; }
    // the grids by hand, on the host
    std::vector<mi355_pair_result> rec = cut_records(pairs);
    std::vector<int64_t> stats((size_t)n * MI355_LOCAL_WARP_STATS_STRIDE(lp.grid_x, lp.grid_y) + 8);
    if (mi355_tie_residual_stats_host(&rec[0], (int)rec.size(), &w[0], &h[0], &h9s[0], n, NULL, &stats[0]) != MI355_OK ||
        mi355_solve_local_warps(&stats[0], n, NULL, &grids_host[0], &rep_host[0]) != MI355_OK) { std::fprintf(stderr, "host statistics / solve: %s\n", mi355_last_error(NULL)); return 10; }
    if (std::memcmp(&grids[0], &grids_host[0], sizeof(float) * gsz) != 0 || std::memcmp(&rep[0], &rep_host[0], sizeof(rep[0]) * n) != 0) {
        std::fprintf(stderr, "the adaptor's grids differ from the host statistics and solve\n");
        return 12;
    }
    long ties = 0; int solved = 0; float big = 0.0f;
    for (int k = 0; k < n; k++) { ties += (long)rep[k].n_ties; solved += rep[k].solved; }
    for (size_t q = 0; q < gsz; q++) { const float a = grids[q] < 0 ? -grids[q] : grids[q]; if (a > big) big = a; }
    if (solved == 0 || ties == 0 || big < 1.0f / 256.0f) { std::fprintf(stderr, "nothing was registered (solved %d ties %ld largest %g)\n", solved, ties, big); return 13; }
    // the frames by hand: the C call on the second copies, the render from them
    if (mi355_local_register_results(c, &rec[0], (int)rec.size(), &second[0], &w[0], &h[0], &ws[0], n, &h9s[0], &lp, &grids_hand[0], NULL) != MI355_OK) { std::fprintf(stderr, "local_register_results: %s\n", mi355_last_error(c)); return 14; }
    if (std::memcmp(&grids[0], &grids_hand[0], sizeof(float) * gsz) != 0) { std::fprintf(stderr, "the adaptor's grids differ from the C call's\n"); return 14; }
    IplImage* hand = cvCreateImage8U(after->width, after->height, 3);
    if (!hand || mi355_mosaic_refined_into(c, NULL, &ids2[0], &w[0], &h[0], &ws[0], n, &h9s[0], (uint8_t*)hand->imageData, hand->widthStep, hand->width, hand->height) != MI355_OK) {
        std::fprintf(stderr, "render by hand: %s\n", mi355_last_error(c));
        return 15;
    }
    if (!same_image(after, hand)) { std::fprintf(stderr, "the render after LocalRegistration differs from the sequence by hand\n"); return 16; }
    if (same_image(after, before)) { std::fprintf(stderr, "LocalRegistration changed no rendered pixel\n"); return 17; }
    for (int k = 0; k < n; k++)
        if (std::memcmp(poses[k].pImg->imageData, &copies[k][0], copies[k].size()) != 0) { std::fprintf(stderr, "a host image changed\n"); return 18; }
    std::printf("ADAPTOR LOCAL WARP OK pairs %d records %d ties %ld solved %d largest shift %.3f\n", (int)pairs.size(), (int)rec.size(), ties, solved, big);
    cvReleaseImage(&before); cvReleaseImage(&after); cvReleaseImage(&hand);
    for (int k = 0; k < n; k++) cvReleaseImage(&poses[k].pImg);
    return 0;
}
