// tests/cxx/cover_select_sanitize.cpp -- the cover-depth selection's host code (csrc/cover_select.cpp with csrc/gain_solve.cpp's list checks and
// csrc/kept_graph.h) under sanitizers, as a stand-alone program: two layouts of tests/cover_patterns.py (strip5_waits, leaf_frees_cut_vertex)
// given as rectangles, the statistics counted here on the step-1 lattice, the statuses those of the numpy reference; then the refusals, which
// return before anything is sized.  No GPU, no Python.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "cover.h"

static std::string g_err;
void mi_set_host_error(const std::string& s) { g_err = s; }            // api.hip's, for a program without the HIP units
// cover.hip's, for mi355_cover_select (not called here: the layouts come as boxes)
int mi_cover::frame_boxes(const int*, const int*, int, const float*, Box*, char*, std::string& err) { err = "no geometry in this program"; return MI355_ERR_FAILED; }

struct Rect { int x, y, w, h; };                                       // a w x h frame at canvas offset (x, y): covers x .. x + w - 2, y .. y + h - 2

static int run(const std::vector<Rect>& fr, const std::vector<int32_t>& order, const std::vector<int32_t>& pairs, int min_depth, long long max_loss,
               const std::vector<int>& want_status, int want_rounds, long long want_lost) {
    const int n = (int)fr.size();
    int cw = 0, ch = 0;
    for (const Rect& r : fr) { cw = std::max(cw, r.x + r.w); ch = std::max(ch, r.y + r.h); }
    std::vector<mi_cover::Box> box((size_t)n);
    std::vector<char> part((size_t)n, 1);
    for (int k = 0; k < n; k++)
        box[k] = mi_cover::Box{std::max(fr[k].x - 1, 0), std::min(fr[k].x + fr[k].w - 1, cw - 1), std::max(fr[k].y - 1, 0), std::min(fr[k].y + fr[k].h - 1, ch - 1)};
    auto stats = [&](const uint8_t* keep, mi355_cover_frame_stats* fs, std::string&) {
        std::vector<int> d((size_t)cw * ch, 0);
        auto each = [&](int k, auto f) { for (int y = fr[k].y; y <= fr[k].y + fr[k].h - 2; y++) for (int x = fr[k].x; x <= fr[k].x + fr[k].w - 2; x++) f(d[(size_t)y * cw + x]); };
        for (int k = 0; k < n; k++) if (keep[k]) each(k, [](int& v) { v++; });
        memset(fs, 0, sizeof(*fs) * (size_t)n);
        for (int k = 0; k < n; k++) if (keep[k]) each(k, [&](int& v) { fs[k].at_depth[std::min(v, 8) - 1]++; });
        return MI355_OK;
    };
    mi355_cover_params p;
    mi355_default_cover_params(&p);
    p.step = 1; p.min_depth = min_depth; p.max_loss = max_loss;
    std::vector<uint8_t> status((size_t)n), keep_out((size_t)n);
    int32_t rounds = -1;
    int64_t lost = -1;
    std::string err;
    const int rc = mi_cover::select(n, box.data(), part.data(), nullptr, order.data(), (int)order.size(), pairs.empty() ? nullptr : pairs.data(), (int)pairs.size() / 2, p,
                                    stats, status.data(), keep_out.data(), &rounds, &lost, err);
    if (rc != MI355_OK) { printf("select failed: %s\n", err.c_str()); return 1; }
    for (int k = 0; k < n; k++)
        if (status[k] != want_status[k] || keep_out[k] != (status[k] == MI355_COVER_DROPPED ? 0 : 1)) { printf("frame %d: status %d keep %d\n", k, status[k], keep_out[k]); return 1; }
    if (rounds != want_rounds || lost != want_lost) { printf("rounds %d lost %lld\n", rounds, (long long)lost); return 1; }
    return 0;
}

static int refused(int n, int step, int min_depth, long long max_loss, const std::vector<int32_t>& order, const char* needle) {
    std::vector<mi_cover::Box> box(4, mi_cover::Box{0, 9, 0, 9});
    std::vector<char> part(4, 1);
    std::vector<uint8_t> status(4), keep_out(4);
    mi355_cover_params p;
    p.step = step; p.min_depth = min_depth; p.max_loss = max_loss;
    std::string err;
    const int rc = mi_cover::select(n, box.data(), part.data(), nullptr, order.data(), (int)order.size(), nullptr, 0, p,
                                    [](const uint8_t*, mi355_cover_frame_stats*, std::string&) { return MI355_ERR_FAILED; }, status.data(), keep_out.data(), nullptr, nullptr, err);
    if (rc != MI355_ERR_ARG || err.find(needle) == std::string::npos) { printf("expected a refusal with '%s', got %d '%s'\n", needle, rc, err.c_str()); return 1; }
    return 0;
}

int main() {
    int bad = 0;
    {   // strip5_waits
        std::vector<Rect> fr;
        for (int k = 0; k < 5; k++) fr.push_back(Rect{8 * k, 0, 21, 11});
        bad += run(fr, {1, 2, 3}, {}, 1, 40, {0, 1, 1, 2, 0}, 3, 40);
    }
    {   // leaf_frees_cut_vertex
        const std::vector<Rect> fr = {{2, 1, 20, 10}, {4, 1, 20, 10}, {6, 1, 20, 10}, {0, 0, 40, 14}};
        bad += run(fr, {1, 2}, {0, 1, 1, 2}, 1, 0, {0, 3, 1, 0}, 1, 0);
    }
    bad += refused(4, 0, 1, 0, {0}, "step=0");
    bad += refused(4, 8, 9, 0, {0}, "min_depth=9");
    bad += refused(4, 8, 1, -1, {0}, "max_loss=-1");
    bad += refused(65536, 8, 1, 0, {0}, "n=65536");
    bad += refused(4, 8, 1, 0, {0, 4}, "order[1]=4");
    bad += refused(4, 8, 1, 0, {2, 0, 2}, "order[2]=2 repeats order[0]");
    if (bad) return 1;
    printf("SANITIZE_OK\n");
    return 0;
}
