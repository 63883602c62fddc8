// tests/cxx/sift_plan_check.cpp -- stand-alone driver of csrc/sift_plan.cpp (tests/test_sift_plan.py builds both with
// g++ -fsanitize=address,undefined and runs the program; nothing here needs HIP or a GPU).
//
//   sift_plan_check print FILE   the taps, and the layout and launch list of every case of FILE
//   sift_plan_check sweep        the invariants of layouts and launch lists (listed at do_sweep) over a sweep of sizes, batches and routes
//
// FILE: "<cases>", then per case "<tag> <w> <h> <keepall> <kmax> <n> <blur_stream> <xstream_min_w> <xstream_min_frames> <aligned>".
// Output of print: "taps <r> <2r + 1 taps>" for the base level and levels 1 .. 5; then per case "<tag> REFUSED <text>" or
//   "<tag> <n_oct> <cand_cap> <ref_cap> <kp_cap> <cube_cap> <ksort_stride> <strides: pyr claimed cand refined kps cube sel mins> <batch a> <batch b> <launches>"
//   (batch a: batch_frames of n requested, 3 slots, 288 GiB; batch b: of 40 requested, memory unknown),
//   per octave "<w> <h> <lv 0..5> <claimed> <mins>", per launch "<kind> <octave> <level> <radius> <waves> <ds> <gx> <gy> <gz> <L> <nstrip> <nseg> <xsw> <bytes>".
#include "../../imagemosaicing_amd/csrc/sift_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

using namespace sift_plan;

static int do_print(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    const PyramidTaps& taps = pyramid_taps();
    for (int i = 0; i < N_LEVELS; i++) {
        const Taps& t = i ? taps.lv[i] : taps.base;
        printf("taps %d", t.r);
        for (int k = 0; k <= 2 * t.r; k++) printf(" %.9g", (double)t.k[k]);
        printf("\n");
    }
    int cases = 0;
    if (fscanf(f, "%d", &cases) != 1) return 2;
    for (int c = 0; c < cases; c++) {
        char tag[128]; int w, h, keepall, kmax, n; Routes r; int aligned;
        if (fscanf(f, "%127s %d %d %d %d %d %d %d %d %d", tag, &w, &h, &keepall, &kmax, &n, &r.blur_stream, &r.xstream_min_w, &r.xstream_min_frames, &aligned) != 10) return 2;
        r.base_frames_aligned = aligned != 0;
        std::string err;
        const Layout l = make_layout(w, h, keepall != 0, kmax, err);
        if (!err.empty()) { printf("%s REFUSED %s\n", tag, err.c_str()); continue; }
        const std::vector<Launch> ls = pyramid_launches(l, n, r);
        printf("%s %d %u %u %u %u %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %zu\n", tag, l.n_oct, l.cand_cap, l.ref_cap, l.kp_cap, l.cube_cap, l.ksort_stride,
               l.bs.pyr, l.bs.claimed, l.bs.cand, l.bs.refined, l.bs.kps, l.bs.cube, l.bs.sel, l.bs.mins,
               batch_frames(w, h, keepall != 0, n, 3, (size_t)288 << 30), batch_frames(w, h, keepall != 0, 40, 3, 0), ls.size());
        for (int o = 0; o < l.n_oct; o++) {
            const Octave& oc = l.oc[o];
            printf("%d %d %zu %zu %zu %zu %zu %zu %zu %zu\n", oc.w, oc.h, oc.lv[0], oc.lv[1], oc.lv[2], oc.lv[3], oc.lv[4], oc.lv[5], oc.claimed, oc.mins);
        }
        for (const Launch& L : ls)
            printf("%d %d %d %d %d %d %u %u %u %d %d %d %d %.0f\n", (int)L.kind, L.octave, L.level, L.radius, L.waves, (int)L.ds, L.gx, L.gy, L.gz, L.L, L.nstrip, L.nseg, L.xsw, L.bytes);
    }
    fclose(f);
    return 0;
}

// ---- sweep ----------------------------------------------------------------------------------------------------------------------------------
static long long g_checks = 0, g_cases = 0;
static int g_fail = 0;
static std::string g_what;                                   // the configuration being checked

#define NEED(cond, ...)                                                                   \
    do {                                                                                  \
        g_checks++;                                                                       \
        if (!(cond)) {                                                                    \
            if (g_fail++ < 20) { printf("FAIL %s: ", g_what.c_str()); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                 \
    } while (0)

// the ranges of one buffer, in layout order: each starts at or after the end of the one before, the last ends inside the frame's stride
struct Ranges {
    const char* name; size_t end = 0;
    void add(size_t off, size_t len, int o) { NEED(off >= end, "%s of octave %d starts at %zu, inside the range before it (ends %zu)", name, o, off, end); end = off + len; }
};

static void check_layout(const Layout& l) {
    Ranges pyr{"level"}, claimed{"bitmap"}, mins{"start keys"};
    NEED(l.n_oct >= 1 && l.n_oct <= MAX_OCT, "%d octaves", l.n_oct);
    for (int o = 0; o < l.n_oct; o++) {
        const Octave& oc = l.oc[o];
        const size_t px = (size_t)oc.w * oc.h;
        NEED(oc.w == l.w >> o && oc.h == l.h >> o, "octave %d is %d x %d", o, oc.w, oc.h);
        for (int i = 0; i < N_LEVELS; i++) {
            NEED(oc.lv[i] % 64 == 0, "octave %d level %d at %zu: no multiple of 64", o, i, oc.lv[i]);
            pyr.add(oc.lv[i], px, o);
        }
        claimed.add(oc.claimed, (px * 4 + 31) / 32, o);
        if (l.keepall) mins.add(oc.mins, px * 4, o);
    }
    NEED(l.bs.pyr % 64 == 0, "bs.pyr %zu: no multiple of 64", l.bs.pyr);
    NEED(pyr.end <= l.bs.pyr && claimed.end <= l.bs.claimed && mins.end <= l.bs.mins, "ranges end at %zu / %zu / %zu, strides %zu / %zu / %zu", pyr.end, claimed.end, mins.end,
         l.bs.pyr, l.bs.claimed, l.bs.mins);
}

// The launch list of one batch:
//   per octave, in order: the base blur (octave 0) or at most one DOWNSAMPLE, the blurs of levels 1 .. 5, one extrema launch;
//   a blur with the decimated copy is level 3 and is followed by no DOWNSAMPLE for the next octave, one without it by exactly one;
//   streamed blur: L even and >= 64, nseg L >= h, (nseg - 1) L < h, nstrip 256 >= w, a radius the kernel exists for (6 for the base level;
//     5, 6, 8, 10 or 13 otherwise; 8 with the copy), the grid holds every unit;
//   streamed extrema: xsw % 4 == 0, xsw <= XSW, nstrip xsw >= w, nseg L >= h, the grid holds every unit;
//   the byte figures the profile brackets are given: level_bytes + 3 w h n for the base, 2 level_bytes per blur and per
//     downsample, 6 level_bytes per extrema launch, with level_bytes = 2 w h n of the octave.
static void check_launches(const Layout& l, int n, const std::vector<Launch>& ls) {
    size_t at = 0;
    double sum = 0.0, want = 0.0;
    bool copied = false;                                     // the octave before wrote this one's base
    for (int o = 0; o < l.n_oct; o++) {
        const Octave& oc = l.oc[o];
        const double level_bytes = (double)oc.w * oc.h * 2.0 * n;
        for (int step = 0; step <= N_LEVELS; step++) {       // 0: base or downsample, 1 .. 5: blurs, 6: extrema
            if (step == 0 && o > 0 && copied) continue;
            NEED(at < ls.size(), "octave %d step %d: the list ends after %zu launches", o, step, at);
            if (at >= ls.size()) return;
            const Launch& L = ls[at++];
            sum += L.bytes;
            NEED(L.octave == o, "launch %zu is of octave %d, expected %d", at - 1, L.octave, o);
            if (step == 0 && o > 0) {
                NEED(L.kind == DOWNSAMPLE, "octave %d opens with kind %d", o, (int)L.kind);
                NEED(L.gx == (unsigned)(oc.w + 63) / 64 && L.gy == (unsigned)(oc.h + 3) / 4 && L.gz == (unsigned)n, "downsample grid %u %u %u", L.gx, L.gy, L.gz);
                want += 2.0 * level_bytes;
            } else if (step < N_LEVELS) {
                NEED((L.kind == BLUR_STREAM || L.kind == BLUR_TILE) && L.level == step, "octave %d step %d: kind %d level %d", o, step, (int)L.kind, L.level);
                want += step == 0 ? level_bytes + 3.0 * oc.w * oc.h * n : 2.0 * level_bytes;
                NEED(!L.ds || (step == N_LAYERS && o + 1 < l.n_oct), "octave %d level %d writes a decimated copy", o, step);
                if (step == N_LAYERS) copied = L.ds;
                if (L.kind == BLUR_STREAM) {
                    NEED(L.L % 2 == 0 && L.L >= 64, "octave %d level %d: L %d", o, step, L.L);
                    NEED(L.nseg * L.L >= oc.h && (L.nseg - 1) * L.L < oc.h, "octave %d level %d: %d segments of %d rows, h %d", o, step, L.nseg, L.L, oc.h);
                    NEED(L.nstrip * 256 >= oc.w && (L.nstrip - 1) * 256 < oc.w, "octave %d level %d: %d strips, w %d", o, step, L.nstrip, oc.w);
                    NEED(step == 0 ? L.radius == 6 : L.ds ? L.radius == 8 : (L.radius == 5 || L.radius == 6 || L.radius == 8 || L.radius == 10 || L.radius == 13),
                         "octave %d level %d: streamed radius %d (ds %d)", o, step, L.radius, (int)L.ds);
                    NEED(L.waves == (L.radius <= 8 ? 4 : 3), "octave %d level %d: %d waves at radius %d", o, step, L.waves, L.radius);
                    NEED((long long)L.gx * 4 >= (long long)L.nstrip * L.nseg * n && L.gy == 1 && L.gz == 1, "octave %d level %d: grid %u for %d x %d x %d units", o, step, L.gx, L.nstrip, L.nseg, n);
                } else {
                    NEED(L.radius >= 2 && L.radius <= MAX_R, "octave %d level %d: tile radius %d", o, step, L.radius);
                    NEED(L.gx == (unsigned)(((oc.w + T16W - 1) / T16W) * ((oc.h + T16H - 1) / T16H)) && L.gy == (unsigned)n && L.gz == 1, "octave %d level %d: tile grid %u %u", o, step, L.gx, L.gy);
                }
            } else {
                NEED(L.kind == EXTREMA_STREAM || L.kind == EXTREMA_TILE, "octave %d ends with kind %d", o, (int)L.kind);
                want += 6.0 * level_bytes;
                if (L.kind == EXTREMA_STREAM) {
                    NEED(L.xsw % 4 == 0 && L.xsw <= XSW && L.nstrip * L.xsw >= oc.w, "octave %d extrema: %d strips of %d columns, w %d", o, L.nstrip, L.xsw, oc.w);
                    NEED(L.L >= 1 && L.nseg * L.L >= oc.h, "octave %d extrema: %d segments of %d rows, h %d", o, L.nseg, L.L, oc.h);
                    NEED((long long)L.gx * 4 >= (long long)L.nstrip * L.nseg * n && L.gy == 1 && L.gz == 1, "octave %d extrema: grid %u for %d x %d x %d units", o, L.gx, L.nstrip, L.nseg, n);
                } else {
                    NEED(L.gx == (unsigned)(((oc.w + EW - 1) / EW) * ((oc.h + EH - 1) / EH)) && L.gy == (unsigned)n && L.gz == 1, "octave %d extrema: tile grid %u %u", o, L.gx, L.gy);
                }
            }
        }
    }
    NEED(at == ls.size(), "%zu launches, %zu expected", ls.size(), at);
    NEED(sum == want, "byte figures sum to %.0f, the brackets were given %.0f", sum, want);
}

static int do_sweep() {
    std::vector<int> sizes;
    const int spans[5][2] = {{16, 70}, {250, 262}, {508, 520}, {1020, 1030}, {2040, 2056}};
    for (const auto& s : spans) for (int v = s[0]; v <= s[1]; v++) sizes.push_back(v);
    const Routes routes[] = {{1, 1500, 4, true}, {1, 256, 1, true}, {1, 256, 1, false}, {1, 1000, 4, true}, {0, 256, 1, true}};
    long long streamed_blurs = 0, streamed_extrema = 0, copies = 0, downsamples = 0;
    for (int w : sizes) for (int h : sizes) {
        for (int keepall = 0; keepall < 2; keepall++) {
            g_what = std::to_string(w) + " x " + std::to_string(h) + (keepall ? " keep-all" : "");
            std::string err;
            const Layout l = make_layout(w, h, keepall != 0, keepall ? 32768 : 0, err);
            g_cases++;
            NEED(err.empty(), "refused: %s", err.c_str());
            if (!err.empty()) continue;
            check_layout(l);
            if (keepall) continue;                            // the launches do not depend on it
            for (int n : {1, 2, 5, 32}) for (const Routes& r : routes) {
                g_what = std::to_string(w) + " x " + std::to_string(h) + ", " + std::to_string(n) + " frames, routes " + std::to_string(r.blur_stream) + " " +
                         std::to_string(r.xstream_min_w) + " " + std::to_string(r.xstream_min_frames) + " " + std::to_string((int)r.base_frames_aligned);
                const std::vector<Launch> ls = pyramid_launches(l, n, r);
                g_cases++;
                check_launches(l, n, ls);
                for (const Launch& L : ls) {
                    NEED(r.blur_stream || (L.kind != BLUR_STREAM && L.kind != EXTREMA_STREAM), "a streamed launch with blur_stream 0");
                    NEED(r.base_frames_aligned || !(L.kind == BLUR_STREAM && L.level == 0), "the base level streams from frames that are not aligned");
                    streamed_blurs += L.kind == BLUR_STREAM; streamed_extrema += L.kind == EXTREMA_STREAM; copies += L.ds; downsamples += L.kind == DOWNSAMPLE;
                }
            }
        }
    }
    g_what = "the sweep";
    NEED(streamed_blurs > 0 && streamed_extrema > 0 && copies > 0 && downsamples > 0, "routes not reached: %lld streamed blurs, %lld streamed extrema, %lld copies, %lld downsamples",
         streamed_blurs, streamed_extrema, copies, downsamples);
    printf("sweep: %lld configurations, %lld checks, %d failed\n", g_cases, g_checks, g_fail);
    if (g_fail == 0) printf("SIFT_PLAN_OK\n");
    return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "print")) return do_print(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "sweep")) return do_sweep();
    fprintf(stderr, "usage: sift_plan_check print FILE | sweep\n");
    return 2;
}
