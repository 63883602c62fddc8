// csrc/blend_plan.h -- the integer geometry of the multiband blend (blend.hip): level count and padded canvas, stripe level ranges, the
// chips' regions, active windows and batches.  Host only, no HIP header (blend_plan.cpp is built by g++ as well: tests/test_blend_plan.py
// runs it under sanitizers); everything the kernels read of it is plain data.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/mi355_mosaic.h"

namespace blend_plan {

// one chip of a batch: where its pixels are, how its region lies on the chip, where its pyramid levels >= 1 live
constexpr int MAX_BANDS = 16;
struct Win { int x0, y0, x1, y1; };   // inclusive
struct ChipP {
    const uint8_t* chip; const uint8_t* mask;
    int cw, ch, cws, mws;             // chip size, row pitches of chip (3 B / pixel) and mask
    int left, top, rw, rh;            // chip origin inside its region, region size (multiples of 2^bands)
    size_t tmp;                       // pixel offset of this chip's level 1 inside the batch's pyramid buffers
    int tlx, tly;                     // the region's origin on the canvas
    // Active windows (round 4).  With FindMasksByDistMap's masks a chip's weights are non-zero only over the cell of the mosaic it owns (+ the
    // reach of the REDUCE filter per level), and a pixel of weight +0 adds nothing to the canvas: only the part of the pyramids that the
    // non-zero weights can see is ever formed.  cwin[l], l = 1 .. bands: the pixels of level l (Gaussian and weight) that are computed --
    // everything outside is never written and never read; twin[l], l = 0 .. bands: the threads of the accumulation of level l (one per
    // 2 x 2 block of level l below the top level, one per pixel at the top level).  See chip_windows() for the derivation.
    Win cwin[MAX_BANDS + 1];
    Win twin[MAX_BANDS + 1];
};

bool chip_windows(ChipP& c, int nb, const int* bb, const int* nlo = nullptr, const int* nhi = nullptr);
void chip_pixel_window(const ChipP& c, int& x0, int& y0, int& x1, int& y1);
void stripe_levels(int row0, int rows, int nb, int Hp, std::vector<int>& nlo, std::vector<int>& nhi);
void stripe_mask_rows(const std::vector<int>& nlo, const std::vector<int>& nhi, int H, int& r0, int& r1);

// What one blend call forms, from (W, H, band, row0, rows) alone.  rows < 0 or the whole canvas: no stripe.  A stripe needs a pyramid the
// windows can hold (1 <= nb <= MAX_BANDS); otherwise `copy_out` is set: the whole canvas is formed and the caller copies the rows out.
// nb: level count (levels 0 .. nb); Wp, Hp: padded canvas (multiples of 2^nb); row0, rows: the output rows asked for.
// nlo / nhi: rows of level l held by the canvas pyramids: all of them, or the stripe's (stripe_levels).  loff: level offsets in pixels inside
// one pyramid buffer; voff: the same minus the rows left out above the stripe, so that canvas coordinates index the buffers unchanged
struct Plan {
    int W, H, band, nb, Wp, Hp, row0, rows; bool striped, copy_out;
    std::vector<int> nlo, nhi; std::vector<size_t> loff; std::vector<long long> voff;
    size_t level_px(int l) const { return (size_t)(Wp >> l) * (size_t)(nhi[l] - nlo[l] + 1); }      // the level's stored rows are contiguous from loff[l]
};
Plan make_plan(int W, int H, int band, int row0 = 0, int rows = -1);

// The chips that take part, in chip order: par[i] is chip chip[i] of the caller's arrays.  false: a chip lies outside the canvas.
struct Feed { std::vector<ChipP> par; std::vector<int> chip; };
bool feed_regions(const Plan& p, const uint8_t* const* chips, const uint8_t* const* masks, const mi355_chip_info* info, int n, const int* owned_bbox, Feed& out);

// batches of up to 32 chips whose levels >= 1 (10 bytes per pixel, a third of the region) fit 2 GB; host chips are staged per batch
struct Batch { int b0, b1; size_t px, cbytes, mbytes; };
struct Batches { std::vector<Batch> v; size_t max_px = 0, max_cb = 0, max_mb = 0; };
Batches make_batches(std::vector<ChipP>& par, int nb, bool staged);      // sets ChipP::tmp

}  // namespace blend_plan
