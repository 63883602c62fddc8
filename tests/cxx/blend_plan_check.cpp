// tests/cxx/blend_plan_check.cpp -- stand-alone driver of csrc/blend_plan.cpp (tests/test_blend_plan.py builds both with
// g++ -fsanitize=address,undefined and runs the program; nothing here needs HIP or a GPU).
//
//   blend_plan_check print FILE   the plan of every case of FILE: level count, padded size, regions, batch offsets
//   blend_plan_check sweep        the invariants stated above chip_windows, over a sweep of regions, chips, owned boxes and stripes
//
// FILE: "<cases>", then per case "<tag> <W> <H> <band> <n>" and n lines "<x0> <y0> <w> <h>".
// Output of print, per case: "<tag> <nb> <Wp> <Hp> <regions>", then per region "<tlx> <tly> <rw> <rh> <left> <top> <cw> <ch> <tmp>".
#include "../../imagemosaicing_amd/csrc/blend_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace blend_plan;

static int do_print(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    int cases = 0;
    if (fscanf(f, "%d", &cases) != 1) return 2;
    for (int i = 0; i < cases; i++) {
        char tag[128]; int W, H, band, n;
        if (fscanf(f, "%127s %d %d %d %d", tag, &W, &H, &band, &n) != 5) return 2;
        std::vector<mi355_chip_info> info(n > 0 ? n : 1);
        memset(info.data(), 0, sizeof(mi355_chip_info) * info.size());
        for (int k = 0; k < n; k++)
            if (fscanf(f, "%d %d %d %d", &info[k].x0, &info[k].y0, &info[k].w, &info[k].h) != 4) return 2;
        const std::vector<const uint8_t*> none(n > 0 ? n : 1, nullptr);
        const Plan p = make_plan(W, H, band);
        Feed feed;
        if (!feed_regions(p, none.data(), none.data(), info.data(), n, nullptr, feed)) { printf("%s OUTSIDE\n", tag); continue; }
        make_batches(feed.par, p.nb, true);
        printf("%s %d %d %d %d\n", tag, p.nb, p.Wp, p.Hp, (int)feed.par.size());
        for (const ChipP& c : feed.par) printf("%d %d %d %d %d %d %d %d %zu\n", c.tlx, c.tly, c.rw, c.rh, c.left, c.top, c.cw, c.ch, c.tmp);
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

static int reflect101(int p, int n) { if (n == 1) return 0; while (p < 0 || p >= n) { if (p < 0) p = -p; else p = 2 * n - 2 - p; } return p; }
static int reflect(int p, int n) { while (p < 0 || p >= n) { if (p < 0) p = -p - 1; else p = 2 * n - 1 - p; } return p; }

struct Iv { int a, b; bool empty() const { return a > b; } };
static Iv win_axis(const Win& w, int axis) { return axis ? Iv{w.y0, w.y1} : Iv{w.x0, w.x1}; }
static bool inside(Iv in, Iv out) { return in.empty() || (!out.empty() && in.a >= out.a && in.b <= out.b); }
static Iv clipped(Iv v, int n) { if (v.a < 0) v.a = 0; if (v.b > n - 1) v.b = n - 1; return v; }

// the invariants of one chip's windows (comment above chip_windows); axes: bit 0 = columns, bit 1 = rows
static void check_windows(const ChipP& c, int nb, int axes) {
    for (int axis = 0; axis < 2; axis++) {
        if (!((axes >> axis) & 1)) continue;
        const int dim = axis ? c.rh : c.rw;
        for (int l = 0; l <= nb; l++) {
            const Iv T = win_axis(c.twin[l], axis), C = win_axis(c.cwin[l], axis);
            const int nl = dim >> l;
            // every window lies inside its level
            if (!T.empty()) NEED(T.a >= 0 && T.b <= (l < nb ? (nl >> 1) : nl) - 1, "axis %d level %d: twin %d..%d outside the level (%d)", axis, l, T.a, T.b, nl);
            if (l >= 1 && !C.empty()) NEED(C.a >= 0 && C.b <= nl - 1, "axis %d level %d: cwin %d..%d outside the level (%d)", axis, l, C.a, C.b, nl);
            if (T.empty()) continue;
            // 2 T_l .. 2 T_l + 1 inside C_l for l >= 1 (the top level's threads are its pixels)
            if (l >= 1) {
                const Iv F = l < nb ? Iv{2 * T.a, 2 * T.b + 1} : T;
                NEED(inside(F, C), "axis %d level %d: blocks %d..%d not in cwin %d..%d", axis, l, F.a, F.b, C.a, C.b);
            }
            // T_l widened by one and clipped inside C_l+1
            if (l < nb) {
                const Iv E = clipped(Iv{T.a - 1, T.b + 1}, nl >> 1), C1 = win_axis(c.cwin[l + 1], axis);
                NEED(inside(E, C1), "axis %d level %d: EXPAND reads %d..%d of level %d, cwin %d..%d", axis, l, E.a, E.b, l + 1, C1.a, C1.b);
            }
        }
        // the REDUCE inputs of C_l+1, clipped, inside C_l
        for (int l = 1; l < nb; l++) {
            const Iv C1 = win_axis(c.cwin[l + 1], axis), C = win_axis(c.cwin[l], axis);
            if (C1.empty()) continue;
            const Iv R = clipped(Iv{2 * C1.a - 2, 2 * C1.b + 2}, dim >> l);
            NEED(inside(R, C), "axis %d level %d: REDUCE inputs %d..%d of cwin[%d] %d..%d not in cwin %d..%d", axis, l, R.a, R.b, l + 1, C1.a, C1.b, C.a, C.b);
        }
    }
}

// chip_pixel_window against the reads of the level-0 accumulation over twin[0] (blend_lap0_body) and of the first REDUCE over cwin[1]
// (pyr_down0_batch_kernel), both reflections applied as the kernels apply them
static void check_pixel_window(const ChipP& c, int axes) {
    int w4[4];
    chip_pixel_window(c, w4[0], w4[1], w4[2], w4[3]);
    const bool t_on = c.twin[0].x0 <= c.twin[0].x1 && c.twin[0].y0 <= c.twin[0].y1;
    const bool c_on = c.cwin[1].x0 <= c.cwin[1].x1 && c.cwin[1].y0 <= c.cwin[1].y1;
    for (int axis = 0; axis < 2; axis++) {
        if (!((axes >> axis) & 1)) continue;
        const int rdim = axis ? c.rh : c.rw, cdim = axis ? c.ch : c.cw, off = axis ? c.top : c.left;
        const Iv P{w4[axis], w4[2 + axis]};
        NEED(P.empty() || (P.a >= 0 && P.b <= cdim - 1), "axis %d: pixel window %d..%d outside the chip (%d)", axis, P.a, P.b, cdim);
        auto need_pixel = [&](int chip_px, const char* who, int from) {
            NEED(!P.empty() && chip_px >= P.a && chip_px <= P.b, "axis %d: %s reads chip pixel %d (region %d), pixel window %d..%d", axis, who, chip_px, from, P.a, P.b);
        };
        if (t_on) {
            const Iv T = win_axis(c.twin[0], axis);
            for (int t = T.a; t <= T.b && t < (rdim >> 1); t++)
                for (int d = 0; d < 2; d++) need_pixel(reflect(2 * t + d - off, cdim), "level 0", 2 * t + d);
        }
        if (c_on) {
            const Iv C = win_axis(c.cwin[1], axis);
            const int dn = rdim >> 1;
            if (axis == 0) {                                  // a thread forms the outputs x, x + 1 from the seven columns 2x - 2 .. 2x + 4
                for (int x = C.a & ~1; x <= C.b && x < dn; x += 2)
                    for (int j = 0; j < 7; j++) need_pixel(reflect(reflect101(2 * x - 2 + j, rdim) - off, cdim), "REDUCE", 2 * x - 2 + j);
            } else {
                for (int y = C.a; y <= C.b && y < dn; y++)
                    for (int k = 0; k < 5; k++) need_pixel(reflect(reflect101(2 * y - 2 + k, rdim) - off, cdim), "REDUCE", 2 * y - 2 + k);
            }
        }
    }
}

static std::vector<int> uniq(std::vector<int> v, int lo, int hi) {
    std::vector<int> out;
    for (int x : v) if (x >= lo && x <= hi && std::find(out.begin(), out.end(), x) == out.end()) out.push_back(x);
    std::sort(out.begin(), out.end());
    return out;
}

static ChipP make_chip(int rw, int rh, int left, int top, int cw, int ch, int tly) {
    ChipP c; memset(&c, 0, sizeof(c));
    c.cw = cw; c.ch = ch; c.cws = (cw * 3 + 3) & ~3; c.mws = (cw + 3) & ~3;
    c.left = left; c.top = top; c.rw = rw; c.rh = rh; c.tlx = 0; c.tly = tly;
    return c;
}

static int do_sweep() {
    for (int nb = 1; nb <= 5; nb++) {
        const int al = 1 << nb;
        for (int m = 1; m <= 5; m++) {
            const int rw = al * m, rh = al * ((m + 1) % 5 + 1);          // region sides 2^nb (1 .. 5) on either axis
            const int tly = (m & 1) ? al : 0;                           // the region's origin on the canvas (a multiple of 2^nb)
            const int H = tly + rh, Hp = H;                             // canvas rows: the region ends the canvas
            const std::vector<int> lefts = uniq({0, 1, al - 1, 3 * al}, 0, rw - 1), tops = uniq({0, 1, al - 1, 3 * al}, 0, rh - 1);
            for (size_t oi = 0; oi < std::max(lefts.size(), tops.size()); oi++) {
                const int left = lefts[oi % lefts.size()], top = tops[oi % tops.size()];
                const std::vector<int> cws = uniq({1, 2, (rw - left) / 2, rw - left}, 1, rw - left), chs = uniq({1, 2, (rh - top) / 2, rh - top}, 1, rh - top);
                for (size_t si = 0; si < std::max(cws.size(), chs.size()); si++) {
                    const int cw = cws[si % cws.size()], ch = chs[si % chs.size()];
                    const std::vector<int> gx = uniq({0, 1, cw / 2, cw - 2, cw - 1}, 0, cw - 1), gy = uniq({0, 1, ch / 2, ch - 2, ch - 1}, 0, ch - 1);
                    char head[160];
                    snprintf(head, sizeof(head), "nb %d region %d x %d at row %d, chip %d x %d at (%d, %d)", nb, rw, rh, tly, cw, ch, left, top);
                    // the whole canvas: every owned box with corners on the grid (one-pixel boxes and the chip's corners are among them)
                    for (int xa : gx) for (int xb : gx) for (int ya : gy) for (int yb : gy) {
                        if (xb < xa || yb < ya) continue;
                        const int bb[4] = {xa, ya, xb, yb};
                        g_what = std::string(head) + ", owned (" + std::to_string(xa) + ", " + std::to_string(ya) + ") .. (" + std::to_string(xb) + ", " + std::to_string(yb) + ")";
                        ChipP whole = make_chip(rw, rh, left, top, cw, ch, tly);
                        g_cases++;
                        NEED(chip_windows(whole, nb, bb), "the whole canvas: no level left");
                        check_windows(whole, nb, 3);
                        check_pixel_window(whole, 3);
                        // stripes: the rows' windows do not depend on the columns', so every row range goes with two column ranges only (the
                        // chip's width, one pixel in its middle)
                        if (!((xa == gx.front() && xb == gx.back()) || (xa == xb && xa == gx[gx.size() / 2]))) continue;
                        // every single-row stripe, and the two halves of a cut inside one 2^nb block
                        std::vector<std::pair<int, int>> stripes;
                        for (int r = 0; r < H; r++) stripes.push_back({r, 1});
                        const int cut = tly + al / 2 + (rh > al ? al : 0);
                        stripes.push_back({0, cut}); stripes.push_back({cut, H - cut});
                        std::vector<std::vector<char>> rows_single(nb + 1, std::vector<char>(rh + 1, 0)), rows_halves = rows_single;      // per level: thread rows seen
                        for (size_t s = 0; s < stripes.size(); s++) {
                            std::vector<int> nlo, nhi;
                            stripe_levels(stripes[s].first, stripes[s].second, nb, Hp, nlo, nhi);
                            ChipP c = make_chip(rw, rh, left, top, cw, ch, tly);
                            const std::string keep = g_what;
                            g_what += ", stripe rows " + std::to_string(stripes[s].first) + " + " + std::to_string(stripes[s].second);
                            g_cases++;
                            // (stripe_levels' own statement: the collapse forms fine row Y from the coarse rows (Y >> 1) - 1 .. (Y >> 1) + 1)
                            for (int l = 0; l < nb; l++) {
                                const Iv R = clipped(Iv{(nlo[l] >> 1) - 1, (nhi[l] >> 1) + 1}, Hp >> (l + 1));
                                NEED(inside(R, Iv{nlo[l + 1], nhi[l + 1]}), "level %d: the collapse reads rows %d..%d of level %d, held %d..%d", l, R.a, R.b, l + 1, nlo[l + 1], nhi[l + 1]);
                            }
                            const bool left = chip_windows(c, nb, bb, nlo.data(), nhi.data());
                            // ... and a thread of the whole canvas whose canvas rows meet the level's held rows is a thread of the stripe
                            for (int l = 0; l <= nb; l++)
                                for (int t = whole.twin[l].y0; t <= whole.twin[l].y1; t++) {
                                    const int oy = tly >> l, ra = l < nb ? oy + 2 * t : oy + t, rb = l < nb ? ra + 1 : ra;
                                    if (rb < nlo[l] || ra > nhi[l]) continue;
                                    NEED(left && t >= c.twin[l].y0 && t <= c.twin[l].y1, "level %d: thread row %d (canvas rows %d..%d, held %d..%d) is not in the stripe's %d..%d", l, t, ra, rb, nlo[l], nhi[l], c.twin[l].y0, c.twin[l].y1);
                                }
                            if (left) {
                                check_windows(c, nb, 2);
                                check_pixel_window(c, 2);
                                for (int l = 0; l <= nb; l++) {
                                    NEED(inside(win_axis(c.twin[l], 1), win_axis(whole.twin[l], 1)), "level %d: the stripe's threads %d..%d are not the whole canvas's %d..%d", l, c.twin[l].y0, c.twin[l].y1, whole.twin[l].y0, whole.twin[l].y1);
                                    for (int t = c.twin[l].y0; t <= c.twin[l].y1; t++) (s < (size_t)H ? rows_single : rows_halves)[l][t] = 1;
                                }
                            }
                            g_what = keep;
                        }
                        // together the stripes' thread rows are the whole canvas's, at every level
                        for (int l = 0; l <= nb; l++)
                            for (int t = whole.twin[l].y0; t <= whole.twin[l].y1; t++) {
                                NEED(rows_single[l][t] == 1, "level %d: thread row %d of the whole canvas is in no single-row stripe", l, t);
                                NEED(rows_halves[l][t] == 1, "level %d: thread row %d of the whole canvas is in neither half of the cut at row %d", l, t, cut);
                            }
                    }
                }
            }
        }
    }
    printf("sweep: %lld configurations, %lld checks, %d failed\n", g_cases, g_checks, g_fail);
    if (g_fail == 0) printf("BLEND_PLAN_OK\n");
    return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "print")) return do_print(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "sweep")) return do_sweep();
    fprintf(stderr, "usage: blend_plan_check print FILE | sweep\n");
    return 2;
}
