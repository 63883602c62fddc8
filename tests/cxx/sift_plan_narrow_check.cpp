// tests/cxx/sift_plan_narrow_check.cpp -- stand-alone driver of csrc/sift_plan.cpp for Routes::narrow (tests/test_sift_plan_narrow.py
// builds both with g++ -fsanitize=address,undefined and runs the program; nothing here needs HIP or a GPU).
//
//   sift_plan_narrow_check off      narrow = 0 written out gives the launch list of a Routes whose narrow member was left at its default
//   sift_plan_narrow_check on       the invariants of the launch lists with narrow = 1 (listed at check_on)
//   sift_plan_narrow_check show W H N   the blur and extrema launches of one case, narrow = 0 and 1 (for reading)
//
// Both sweeps: w in MINW - 8 .. MINW + 8, 508 .. 520, 996 .. 1004 and h in 62 .. 70, 372 .. 378 crossed, plus 4000 x 3000 and its
// three halvings' parents (2000 x 1500, 1000 x 750); n = 1, 4, 21, 32; both `aligned` values; xstream_min_w 1000 and 1500.
#include "../../imagemosaicing_amd/csrc/sift_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace sift_plan;

static long long g_checks = 0;
static int g_fail = 0;
static std::string g_what;

#define NEED(cond, text)                                                                  \
    do {                                                                                  \
        g_checks++;                                                                       \
        if (!(cond)) {                                                                    \
            if (g_fail++ < 20) fprintf(stderr, "FAIL %s: %s\n", g_what.c_str(), text);    \
        }                                                                                 \
    } while (0)

static bool same(const Launch& a, const Launch& b) {
    return a.kind == b.kind && a.octave == b.octave && a.level == b.level && a.radius == b.radius && a.waves == b.waves && a.ds == b.ds && a.gx == b.gx &&
           a.gy == b.gy && a.gz == b.gz && a.L == b.L && a.nstrip == b.nstrip && a.nseg == b.nseg && a.xsw == b.xsw && a.bytes == b.bytes;
}

static std::vector<std::pair<int, int>> sizes() {
    std::vector<int> ws, hs;
    for (int w = STREAM_NARROW_MIN_W - 8; w <= STREAM_NARROW_MIN_W + 8; w++) ws.push_back(w);
    for (int w = 508; w <= 520; w++) ws.push_back(w);
    for (int w = 996; w <= 1004; w++) ws.push_back(w);
    for (int h = 62; h <= 70; h++) hs.push_back(h);
    for (int h = 372; h <= 378; h++) hs.push_back(h);
    std::vector<std::pair<int, int>> out;
    for (int w : ws) for (int h : hs) out.push_back({w, h});
    out.push_back({4000, 3000}); out.push_back({2000, 1500}); out.push_back({1000, 750});
    return out;
}

static long long g_kinds[5];

// narrow = 1.  Of every streamed blur: L even, at least STREAM_NARROW_MIN_L and at most what narrow = 0 gives; the segments cover every row
// exactly once ((nseg - 1) L < h <= nseg L: segment s holds the rows s L .. min((s + 1) L, h) - 1, blur16_stream_body); a width the
// kernel takes (a multiple of 4, at least STREAM_NARROW_MIN_W, the last strip full or wider than MAX_R) and 64 rows; the grid holds
// nstrip x nseg x n waves in blocks of four; the fused decimation only at R = 8, level N_LAYERS, on an even height.  Of every streamed
// extrema launch the same cover and grid.  A level that narrow = 0 streams still streams, with the same waves and strips; levels at
// least 512 wide route as with narrow = 0; downsample and extrema launches are those of narrow = 0 (but see the loop's first comment).
static void check_on(const Layout& l, int n, const Routes& r0) {
    Routes r1 = r0; r1.narrow = 1;
    const std::vector<Launch> a = pyramid_launches(l, n, r0), b = pyramid_launches(l, n, r1);
    // launch for launch the same work in the same order, except that a level 3 which now streams on an odd height leaves its decimation
    // to a downsample16 launch in front of the next octave (the tiled kernel writes the copy at any height, the streamed one does not)
    size_t ia = 0;
    for (size_t i = 0; i < b.size(); i++) {
        const Launch& L = b[i];
        if (ia < a.size() && !(a[ia].octave == L.octave && a[ia].level == L.level && (a[ia].kind == DOWNSAMPLE) == (L.kind == DOWNSAMPLE))) {
            bool extra = L.kind == DOWNSAMPLE && i >= 2 && b[i - 2].kind == BLUR_STREAM;      // b[i - 1]: the extrema launch of the octave before
            for (size_t j = 0; extra && j < i; j++) if (b[j].octave == L.octave - 1 && b[j].level == N_LAYERS) extra = b[j].kind == BLUR_STREAM && !b[j].ds && (l.oc[b[j].octave].h & 1);
            NEED(extra, "narrow adds or reorders a launch that is no downsample16 behind an odd-height streamed level 3");
            if (!extra) return;
            g_kinds[L.kind]++;
            continue;
        }
        NEED(ia < a.size(), "narrow adds launches at the end");
        if (ia >= a.size()) return;
        const Launch& P = a[ia++];
        const Octave& oc = l.oc[L.octave];
        g_kinds[L.kind]++;
        NEED(L.octave == P.octave && L.level == P.level && L.radius == P.radius && L.bytes == P.bytes, "narrow changes what a launch computes");
        if (L.kind == BLUR_STREAM || L.kind == EXTREMA_STREAM) {
            NEED(L.L >= 1 && L.nseg >= 1 && (long long)(L.nseg - 1) * L.L < oc.h && (long long)L.nseg * L.L >= oc.h, "segments do not cover every row exactly once");
            NEED(L.gx == (unsigned)(L.nstrip * L.nseg * n + 3) / 4 && L.gy == 1 && L.gz == 1, "grid does not hold nstrip x nseg x n waves");
            NEED(r1.blur_stream, "a streamed launch with blur_stream 0");
        }
        if (L.kind == BLUR_STREAM) {
            NEED((L.L & 1) == 0 && L.L >= STREAM_NARROW_MIN_L, "L odd or under the floor");
            NEED((oc.w & 3) == 0 && oc.w >= STREAM_NARROW_MIN_W && oc.h >= 64, "streamed blur on a level the kernel does not take");
            NEED(L.nstrip == (oc.w + 255) / 256 && oc.w - 256 * (L.nstrip - 1) > MAX_R, "last strip not wider than MAX_R");
            NEED(L.waves == (L.radius <= STREAM_W4_MAX_R ? 4 : 3), "waves");
            NEED(!L.ds || (L.radius == 8 && L.level == N_LAYERS && (oc.h & 1) == 0 && L.octave + 1 < l.n_oct), "ds launch is not the R = 8 level of an even-height octave");
            NEED(L.level != 0 || r1.base_frames_aligned, "base level streamed from unaligned frames");
            if (P.kind == BLUR_STREAM) {
                NEED(L.L <= P.L && L.waves == P.waves && L.nstrip == P.nstrip && L.ds == P.ds, "a level streamed either way differs in more than L");
                NEED(L.L == P.L || (long long)L.nstrip * L.nseg * n <= (long long)WAVE_SLOTS * STREAM_NARROW_WAVES + L.nstrip * n || L.L == STREAM_NARROW_MIN_L,
                     "shorter segments than two waves per SIMD ask for");
                NEED(L.L == P.L || (long long)P.nstrip * P.nseg * n < (long long)WAVE_SLOTS * P.waves, "segments shortened in a launch that filled its round");
            } else NEED(P.kind == BLUR_TILE && oc.w < 512, "narrow streams a level of 512 columns or more that narrow = 0 tiles");
        } else if (L.kind == BLUR_TILE) {
            NEED(P.kind == BLUR_TILE && same(L, P), "narrow tiles a level that narrow = 0 streams");
        } else NEED(same(L, P), "narrow changes a downsample or extrema launch");
    }
    NEED(ia == a.size(), "narrow drops a launch");
}

static int sweep(bool on) {
    for (const auto& s : sizes()) for (int n : {1, 4, 21, 32}) for (int aligned = 0; aligned < 2; aligned++) for (int xw : {1000, 1500}) {
        std::string err;
        const Layout l = make_layout(s.first, s.second, false, 0, err);
        if (!err.empty()) { fprintf(stderr, "refused %d x %d\n", s.first, s.second); return 1; }
        g_what = std::to_string(s.first) + " x " + std::to_string(s.second) + ", " + std::to_string(n) + " frames, aligned " + std::to_string(aligned) + ", xstream_min_w " + std::to_string(xw);
        const Routes r = {1, xw, 4, aligned != 0};
        if (on) { check_on(l, n, r); continue; }
        Routes z = {1, xw, 4, aligned != 0, 0};
        const std::vector<Launch> a = pyramid_launches(l, n, r), b = pyramid_launches(l, n, z);
        NEED(a.size() == b.size(), "narrow = 0 changes the number of launches");
        for (size_t i = 0; i < a.size() && i < b.size(); i++) { NEED(same(a[i], b[i]), "narrow = 0 differs from the default member"); g_kinds[a[i].kind]++; }
    }
    for (int k = 0; k < 5; k++) { g_what = "kind " + std::to_string(k); NEED(g_kinds[k] > 0, "a launch kind never occurs in the sweep"); }
    printf("%s: %lld checks, %d failed; launches by kind %lld %lld %lld %lld %lld\n", on ? "on" : "off", g_checks, g_fail, g_kinds[0], g_kinds[1], g_kinds[2], g_kinds[3], g_kinds[4]);
    return g_fail ? 1 : 0;
}

static int show(int w, int h, int n) {
    std::string err;
    const Layout l = make_layout(w, h, false, 0, err);
    if (!err.empty()) return 1;
    for (int narrow = 0; narrow < 2; narrow++) {
        const Routes r = {1, 1000, 4, true, narrow};
        for (const Launch& L : pyramid_launches(l, n, r))
            if (L.kind != DOWNSAMPLE) printf("narrow %d octave %d level %d kind %d R %d L %d nstrip %d nseg %d grid %u x %u\n", narrow, L.octave, L.level, (int)L.kind, L.radius, L.L, L.nstrip, L.nseg, L.gx, L.gy);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "off")) return sweep(false);
    if (argc == 2 && !strcmp(argv[1], "on")) return sweep(true);
    if (argc == 5 && !strcmp(argv[1], "show")) return show(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
    fprintf(stderr, "usage: sift_plan_narrow_check off | on | show W H N\n");
    return 2;
}
