// tests/cxx/adaptor_projective.cpp -- mi355::BundleAdjustmentNonlinear through include/mi355_adaptor.h alone, on a flat list read from
// DIR/projective.bin: int32 nPairs, nImages, sizes (0 or 1), pad; nPairs MatchPointPairs; nImages ImageTransform; nImages int32 w; nImages
// int32 h.  Writes DIR/with_sizes.out and DIR/without_sizes.out (nImages ImageTransform + the report).  Host only: no device is touched.
#include <cstdio>
#include <string>
#include <vector>
#include "mi355_adaptor.h"

static bool dump(const std::string& path, const std::vector<mi355ref::ImageTransform>& t, const mi355_projective_report& rep) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fwrite(t.data(), sizeof(mi355ref::ImageTransform), t.size(), f);
    fwrite(&rep, sizeof(rep), 1, f);
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    FILE* f = fopen((dir + "/projective.bin").c_str(), "rb");
    if (!f) return 3;
    int32_t hdr[4];
    if (fread(hdr, sizeof(hdr), 1, f) != 1) return 3;
    const int nPairs = hdr[0], nImages = hdr[1];
    std::vector<mi355ref::MatchPointPairs> pairs((size_t)nPairs);
    std::vector<mi355ref::ImageTransform> init((size_t)nImages), out;
    std::vector<int> w((size_t)nImages), h((size_t)nImages);
    if (fread(pairs.data(), sizeof(pairs[0]), pairs.size(), f) != pairs.size() || fread(init.data(), sizeof(init[0]), init.size(), f) != init.size() ||
        fread(w.data(), sizeof(int), w.size(), f) != w.size() || fread(h.data(), sizeof(int), h.size(), f) != h.size()) return 3;
    fclose(f);
    const std::vector<mi355ref::ImageTransform> before = init;
    mi355_projective_report rep;
    int rc = mi355::BundleAdjustmentNonlinear(&pairs[0], nPairs, &init[0], nImages, 1, out, w.data(), h.data(), 0, &rep);
    if (rc != 0 || (int)out.size() != nImages || !dump(dir + "/with_sizes.out", out, rep)) { printf("with sizes: rc %d %s\n", rc, mi355_last_error(0)); return 4; }
    rc = mi355::BundleAdjustmentNonlinear(&pairs[0], nPairs, &init[0], nImages, 1, out);
    if (rc != 0) { printf("without sizes: rc %d %s\n", rc, mi355_last_error(0)); return 5; }
    memset(&rep, 0, sizeof(rep));
    if (!dump(dir + "/without_sizes.out", out, rep)) return 5;
    if (memcmp(before.data(), init.data(), sizeof(init[0]) * init.size()) != 0) { printf("the input changed\n"); return 6; }
    if (mi355::BundleAdjustmentNonlinear(&pairs[0], nPairs, &init[0], 1, 1, out) != -2 || mi355::BundleAdjustmentNonlinear(&pairs[0], 4, &init[0], nImages, 1, out) != -3) return 7;
    printf("ADAPTOR PROJECTIVE OK trials %d accepted %d\n", rep.trials, rep.accepted);
    return 0;
}
