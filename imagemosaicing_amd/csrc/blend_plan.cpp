// csrc/blend_plan.cpp -- see blend_plan.h.  Host only: integers (and one double logarithm), no HIP.
#include "blend_plan.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace blend_plan {

// Active windows of one chip (ChipP::cwin / twin), one axis at a time.  n_l = extent of level l, S_0 = the owned pixels' range in region
// coordinates (bb == NULL: everything).  Every set is a superset of what is needed, so a window can only cost time, never change a value:
//   S_l    where the weight of level l can be non-zero: REDUCE output q sees the inputs 2q - 2 .. 2q + 2 (reflected indices fall on inputs
//          the unreflected ones already reach), so S_l+1 = [floor((a - 2) / 2) - 1, floor((b + 2) / 2) + 1], one more on each side for slack;
//   T_l    the accumulation's threads: 2 x 2 blocks of level l below the top level ([a >> 1, b >> 1]), pixels at the top level;
//   F_l    the pixels of level l those threads read (Gaussian + weight): the blocks themselves;
//   E_l+1  the pixels of level l + 1 the EXPAND of those blocks reads: T_l widened by one;
//   C_l    what is computed of level l >= 1: F_l, E_l and the inputs of the REDUCE that forms C_l+1 ([2a - 2, 2b + 2]).
// Everything outside C_l stays unwritten in the batch's pyramid buffers and is never read (the pair kernels' second output may be formed
// from such pixels when C_l+1 starts at an odd column; it lies outside C_l+1 and is never read either).
// nlo / nhi (not NULL: a stripe of the canvas is blended): per level the canvas rows whose pyramid values the stripe's output depends on; the
// accumulation windows are cut to them, a level whose window is empty then has y1 < y0 (and adds nothing to F / E / C).  Returns false when
// no level of the chip is left: the chip adds nothing to the stripe.
bool chip_windows(ChipP& c, int nb, const int* bb, const int* nlo, const int* nhi) {
    const int L = nb < MAX_BANDS ? nb : MAX_BANDS;
    if (!bb || nb > MAX_BANDS) {
        for (int l = 0; l <= L; l++) {
            c.cwin[l] = Win{0, 0, (c.rw >> l) - 1, (c.rh >> l) - 1};
            c.twin[l] = l < nb ? Win{0, 0, (c.rw >> (l + 1)) - 1, (c.rh >> (l + 1)) - 1} : c.cwin[l];
        }
        return true;
    }
    bool any = false;
    for (int axis = 0; axis < 2; axis++) {
        const int dim = axis ? c.rh : c.rw, off = axis ? c.top : c.left;
        int Sa[MAX_BANDS + 1], Sb[MAX_BANDS + 1], Ta[MAX_BANDS + 1], Tb[MAX_BANDS + 1], Fa[MAX_BANDS + 1], Fb[MAX_BANDS + 1], Ea[MAX_BANDS + 2], Eb[MAX_BANDS + 2];
        int Ca[MAX_BANDS + 2], Cb[MAX_BANDS + 2];
        auto clip = [](int& a, int& b, int n) { if (a < 0) a = 0; if (b > n - 1) b = n - 1; if (a > b) { a = a < n ? a : n - 1; b = a; } };
        auto uni = [](int& a, int& b, int a2, int b2) { if (a2 > b2) return; if (a > b) { a = a2; b = b2; return; } a = a2 < a ? a2 : a; b = b2 > b ? b2 : b; };
        Sa[0] = bb[axis] + off; Sb[0] = bb[2 + axis] + off;
        clip(Sa[0], Sb[0], dim);
        for (int l = 0; l < nb; l++) {
            Sa[l + 1] = ((Sa[l] - 2) >> 1) - 1; Sb[l + 1] = ((Sb[l] + 2) >> 1) + 1;
            clip(Sa[l + 1], Sb[l + 1], dim >> (l + 1));
        }
        for (int l = 0; l <= nb + 1; l++) { Ea[l] = 0; Eb[l] = -1; }
        for (int l = 0; l <= nb; l++) {
            if (l < nb) { Ta[l] = Sa[l] >> 1; Tb[l] = Sb[l] >> 1; } else { Ta[l] = Sa[l]; Tb[l] = Sb[l]; }
            if (axis == 1 && nlo) {
                // the threads whose canvas rows meet nlo[l] .. nhi[l]: thread t covers the level's rows 2t, 2t + 1 below the top level
                const int oy = c.tly >> l, lo = nlo[l] - oy, hi = nhi[l] - oy;
                const int ta = l < nb ? (lo >= 1 ? lo >> 1 : 0) : (lo > 0 ? lo : 0), tb = l < nb ? (hi >= 0 ? hi >> 1 : -1) : hi;
                if (ta > Ta[l]) Ta[l] = ta;
                if (tb < Tb[l]) Tb[l] = tb;
            }
            if (Ta[l] > Tb[l]) { Ta[l] = 0; Tb[l] = -1; Fa[l] = 0; Fb[l] = -1; continue; }
            if (axis == 1) any = true;
            if (l < nb) {
                Fa[l] = 2 * Ta[l]; Fb[l] = 2 * Tb[l] + 1;
                Ea[l + 1] = Ta[l] - 1; Eb[l + 1] = Tb[l] + 1;
                clip(Ea[l + 1], Eb[l + 1], dim >> (l + 1));
            } else { Fa[l] = Ta[l]; Fb[l] = Tb[l]; }
        }
        Ca[nb + 1] = 0; Cb[nb + 1] = -1;
        for (int l = nb; l >= 1; l--) {
            int a = 0, b = -1;
            uni(a, b, Fa[l], Fb[l]); uni(a, b, Ea[l], Eb[l]);
            if (l < nb && Ca[l + 1] <= Cb[l + 1]) uni(a, b, 2 * Ca[l + 1] - 2, 2 * Cb[l + 1] + 2);
            if (a <= b) clip(a, b, dim >> l);
            Ca[l] = a; Cb[l] = b;
        }
        Ca[0] = 0; Cb[0] = dim - 1;
        for (int l = 0; l <= nb; l++) {
            if (axis == 0) { c.cwin[l].x0 = Ca[l]; c.cwin[l].x1 = Cb[l]; c.twin[l].x0 = Ta[l]; c.twin[l].x1 = Tb[l]; }
            else           { c.cwin[l].y0 = Ca[l]; c.cwin[l].y1 = Cb[l]; c.twin[l].y0 = Ta[l]; c.twin[l].y1 = Tb[l]; }
        }
    }
    return any;
}

// The chip pixels a chip's windows read: the 2 x 2 blocks of the level-0 accumulation (twin[0]) and the inputs of the first REDUCE over
// cwin[1] (both outputs of a thread, rows and columns 2q - 2 .. 2q + 2), taken through the two reflections the kernels apply (BORDER_REFLECT_101
// at the region's border, then BORDER_REFLECT into the chip).  Chip coordinates, inclusive.
void chip_pixel_window(const ChipP& c, int& x0, int& y0, int& x1, int& y1) {
    for (int axis = 0; axis < 2; axis++) {
        const int rdim = axis ? c.rh : c.rw, cdim = axis ? c.ch : c.cw, off = axis ? c.top : c.left;
        const int ta = axis ? c.twin[0].y0 : c.twin[0].x0, tb = axis ? c.twin[0].y1 : c.twin[0].x1;
        int ca = axis ? c.cwin[1].y0 : (c.cwin[1].x0 & ~1), cb = axis ? c.cwin[1].y1 : (c.cwin[1].x1 | 1);
        int a = 0, b = -1;                                    // (a stripe may leave either window empty: y1 < y0)
        if (ta <= tb) { a = 2 * ta; b = 2 * tb + 1; }
        if (ca <= cb) { if (a > b) { a = 2 * ca - 2; b = 2 * cb + 2; } else { a = a < 2 * ca - 2 ? a : 2 * ca - 2; b = b > 2 * cb + 2 ? b : 2 * cb + 2; } }
        if (a > b) { if (axis == 0) { x0 = 0; x1 = -1; } else { y0 = 0; y1 = -1; } continue; }
        if (a < 0) { b = b > -a ? b : -a; a = 0; }
        if (b > rdim - 1) { const int m = 2 * (rdim - 1) - b; a = a < m ? a : m; b = rdim - 1; }
        if (a < 0) a = 0;
        a -= off; b -= off;
        if (a < 0) { b = b > -a - 1 ? b : -a - 1; a = 0; }
        if (b > cdim - 1) { const int m = 2 * cdim - 1 - b; a = a < m ? a : m; b = cdim - 1; }
        if (a < 0) a = 0;
        if (b < a) b = a;
        if (axis == 0) { x0 = a; x1 = b; } else { y0 = a; y1 = b; }
    }
}

// The canvas rows of every pyramid level that the output rows row0 .. row0 + rows - 1 depend on (a stripe of the canvas: one rank's part of
// LaplacianPyramidBlending).  The collapse forms level l from its Laplacian and EXPAND of level l + 1: fine row Y reads the coarse rows
// (Y >> 1) - 1 .. (Y >> 1) + 1, so N_0 = the stripe, N_l+1 = [(a >> 1) - 1, (b >> 1) + 1]; below the top level the ranges are widened to whole
// 2 x 2 blocks (the accumulation's threads).  Everything a rank forms is what the whole canvas holds there: the canvas geometry (padded
// size, level count, the chips' regions) is the full canvas's, only rows are left out.
void stripe_levels(int row0, int rows, int nb, int Hp, std::vector<int>& nlo, std::vector<int>& nhi) {
    nlo.assign(nb + 1, 0); nhi.assign(nb + 1, 0);
    nlo[0] = row0; nhi[0] = row0 + rows - 1;
    for (int l = 0; l <= nb; l++) {
        const int hl = Hp >> l;
        if (l > 0) { nlo[l] = (nlo[l - 1] >> 1) - 1; nhi[l] = (nhi[l - 1] >> 1) + 1; }
        if (l < nb) { nlo[l] &= ~1; nhi[l] |= 1; }
        if (nlo[l] < 0) nlo[l] = 0;
        if (nhi[l] > hl - 1) nhi[l] = hl - 1;
    }
}
// ... and the canvas rows whose ownership (FindMasksByDistMap) those values can depend on: a level-l value sees 2^l q -+ (2^(l+1) - 2) rows of
// level 0 through its l REDUCE steps, its Laplacian one more level; 8 * 2^l on either side covers both with room to spare
void stripe_mask_rows(const std::vector<int>& nlo, const std::vector<int>& nhi, int H, int& r0, int& r1) {
    r0 = nlo[0]; r1 = nhi[0];
    for (size_t l = 0; l < nlo.size(); l++) {
        const long long a = ((long long)nlo[l] << l) - (8ll << l), b = (((long long)nhi[l] + 1) << l) - 1 + (8ll << l);
        if (a < r0) r0 = a < 0 ? 0 : (int)a;
        if (b > r1) r1 = b > H - 1 ? H - 1 : (int)b;
    }
    if (r1 > H - 1) r1 = H - 1;
}

Plan make_plan(int W, int H, int band, int row0, int rows) {
    Plan p;
    int nb = W > 0 || H > 0 ? (int)std::ceil(std::log((double)(W > H ? W : H)) / std::log(2.0)) : 0;      // (an empty canvas is refused by the caller)
    if (nb > band) nb = band;
    if (nb < 0) nb = 0;
    const int al = 1 << nb;
    const int Wp = (W + al - 1) / al * al, Hp = (H + al - 1) / al * al;
    const bool part = rows >= 0 && !(row0 == 0 && rows == H);
    p.W = W; p.H = H; p.band = band; p.nb = nb; p.Wp = Wp; p.Hp = Hp;
    p.striped = part && nb >= 1 && nb <= MAX_BANDS;      // (no pyramid, or more levels than the windows hold:) the whole canvas is formed and the stripe copied out
    p.copy_out = part && !p.striped;
    p.row0 = part ? row0 : 0; p.rows = part ? rows : H;
    p.nlo.assign(nb + 1, 0); p.nhi.assign(nb + 1, 0);
    for (int l = 0; l <= nb; l++) p.nhi[l] = (Hp >> l) - 1;
    if (p.striped) stripe_levels(row0, rows, nb, Hp, p.nlo, p.nhi);
    p.loff.assign(nb + 2, 0); p.voff.assign(nb + 1, 0);
    for (int l = 0; l <= nb; l++) {
        p.loff[l + 1] = p.loff[l] + (size_t)(Wp >> l) * (size_t)(p.nhi[l] - p.nlo[l] + 1);
        p.voff[l] = (long long)p.loff[l] - (long long)p.nlo[l] * (Wp >> l);
    }
    return p;
}

// geometry of every chip (MultiBandBlender::feed: gap 3 * 2^bands, corners snapped to the level grid, region pulled back inside the canvas)
// owned_bbox != NULL (the masks are FindMasksByDistMap's, made on this device): per chip the box of its non-zero mask bytes -- a chip
// that owns nothing is left out, the others work inside their active windows (chip_windows)
bool feed_regions(const Plan& p, const uint8_t* const* chips, const uint8_t* const* masks, const mi355_chip_info* info, int n, const int* owned_bbox, Feed& out) {
    const int nb = p.nb, al = 1 << nb, Wp = p.Wp, Hp = p.Hp;
    out.par.clear(); out.chip.clear();
    out.par.reserve(n); out.chip.reserve(n);
    for (int k = 0; k < n; k++) {
        const int cw = info[k].w, chh = info[k].h, x0 = info[k].x0, y0 = info[k].y0;
        if (cw <= 0 || chh <= 0) continue;
        if (owned_bbox && (owned_bbox[4 * k + 2] < owned_bbox[4 * k] || owned_bbox[4 * k + 3] < owned_bbox[4 * k + 1])) continue;      // all weights +0: adds nothing
        const int gap = 3 * al;
        int tlx = x0 - gap > 0 ? x0 - gap : 0, tly = y0 - gap > 0 ? y0 - gap : 0;
        int brx = x0 + cw + gap < Wp ? x0 + cw + gap : Wp, bry = y0 + chh + gap < Hp ? y0 + chh + gap : Hp;
        tlx = (tlx >> nb) << nb; tly = (tly >> nb) << nb;
        int rw = brx - tlx, rh = bry - tly;
        rw += (al - rw % al) % al;
        rh += (al - rh % al) % al;
        brx = tlx + rw; bry = tly + rh;
        const int dx = brx - Wp > 0 ? brx - Wp : 0, dy = bry - Hp > 0 ? bry - Hp : 0;
        tlx -= dx; tly -= dy;
        if (tlx < 0 || tly < 0 || rw <= 0 || rh <= 0) return false;
        ChipP c; memset(&c, 0, sizeof(c));
        c.chip = chips[k]; c.mask = masks[k];
        c.cw = cw; c.ch = chh; c.cws = (cw * 3 + 3) & ~3; c.mws = (cw + 3) & ~3;
        c.left = x0 - tlx; c.top = y0 - tly; c.rw = rw; c.rh = rh; c.tlx = tlx; c.tly = tly;
        if (!chip_windows(c, nb, owned_bbox ? owned_bbox + 4 * k : nullptr, p.striped ? p.nlo.data() : nullptr, p.striped ? p.nhi.data() : nullptr)) continue;      // nothing of it reaches the stripe
        out.par.push_back(c); out.chip.push_back(k);
    }
    return true;
}

Batches make_batches(std::vector<ChipP>& par, int nb, bool staged) {
    const int nc = (int)par.size();
    constexpr int MAXB = 32;
    const size_t tmp_budget_px = ((size_t)2 << 30) / 10;
    auto levels_px = [&](const ChipP& c) { size_t px = 0; for (int l = 1; l <= nb; l++) px += (size_t)(c.rw >> l) * (c.rh >> l); return px; };
    Batches out;
    for (int b0 = 0; b0 < nc;) {
        Batch bt = {b0, b0, 0, 0, 0};
        while (bt.b1 < nc && bt.b1 - b0 < MAXB) {
            ChipP& c = par[bt.b1];
            const size_t p = nb > 0 ? levels_px(c) : (size_t)c.rw * c.rh;
            if (bt.b1 > b0 && bt.px + p > tmp_budget_px) break;
            c.tmp = bt.px; bt.px += p;
            if (staged) { bt.cbytes += ((size_t)c.cws * c.ch + 15) & ~(size_t)15; bt.mbytes += ((size_t)c.mws * c.ch + 15) & ~(size_t)15; }
            bt.b1++;
        }
        out.max_px = std::max(out.max_px, bt.px); out.max_cb = std::max(out.max_cb, bt.cbytes); out.max_mb = std::max(out.max_mb, bt.mbytes);
        out.v.push_back(bt);
        b0 = bt.b1;
    }
    return out;
}

}  // namespace blend_plan
