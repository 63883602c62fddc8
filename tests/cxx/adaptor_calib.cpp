// tests/cxx/adaptor_calib.cpp -- mi355::CalibrateLens through include/mi355_adaptor.h alone, on a flat list read from DIR/calib.bin: int32
// nPairs, mask, pad, pad; the start camera (9 doubles); nPairs MatchPointPairs.  Writes DIR/calib.out (the camera and the report) and
// DIR/calib_default.out (the same with params = 0).  Host only: no device is touched.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mi355_adaptor.h"

static bool dump(const std::string& path, const mi355_camera& cam, const mi355_calib_report& rep) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fwrite(&cam, sizeof(cam), 1, f);
    fwrite(&rep, sizeof(rep), 1, f);
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    FILE* f = fopen((dir + "/calib.bin").c_str(), "rb");
    if (!f) return 3;
    int32_t hdr[4];
    mi355_camera start, out;
    if (fread(hdr, sizeof(hdr), 1, f) != 1 || fread(&start, sizeof(start), 1, f) != 1) return 3;
    std::vector<mi355ref::MatchPointPairs> pairs((size_t)hdr[0]);
    if (fread(pairs.data(), sizeof(pairs[0]), pairs.size(), f) != pairs.size()) return 3;
    fclose(f);
    mi355_calib_params p;
    mi355_default_calib_params(&p);
    p.mask = hdr[1];
    mi355_calib_report rep;
    int rc = mi355::CalibrateLens(&pairs[0], hdr[0], start, out, &p, &rep);
    if (rc != 0 || !dump(dir + "/calib.out", out, rep)) { printf("with params: rc %d %s\n", rc, mi355_last_error(0)); return 4; }
    rc = mi355::CalibrateLens(&pairs[0], hdr[0], start, out);
    memset(&rep, 0, sizeof(rep));
    if (rc != 0 || !dump(dir + "/calib_default.out", out, rep)) { printf("defaults: rc %d %s\n", rc, mi355_last_error(0)); return 5; }
    if (mi355::CalibrateLens(0, 3, start, out) != -1 || mi355::CalibrateLens(&pairs[0], -1, start, out) != -1) return 6;
    p.mask = 0;
    if (mi355::CalibrateLens(&pairs[0], hdr[0], start, out, &p) != MI355_ERR_ARG || std::string(mi355_last_error(0)).find("mask = 0") == std::string::npos) return 7;
    if (mi355::CalibrateLens(0, 0, start, out) != 0 || memcmp(&out, &start, sizeof(out)) != 0) return 8;
    printf("ADAPTOR CALIB OK k1 %.9g k2 %.9g\n", out.k1, out.k2);
    return 0;
}
