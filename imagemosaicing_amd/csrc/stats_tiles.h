// csrc/stats_tiles.h -- the host side that the lattice statistics share (gain.hip: gain_stats_kernel, block_gain_stats_kernel; sharp.hip:
// sharp_stats_kernel): the tile record, the work list over pair intersections and frame boxes, and the launchers' checks, canvas layout and
// frame table (stats_setup).  Moved here from gain.hip line for line when sharp.hip became their third user.  Everything sits in an unnamed
// namespace, as in mosaic_frame.h: each unit that includes it gets its own copy.
#pragma once
#include "common.h"
#include "gain.h"
#include "mosaic_frame.h"
#include <algorithm>
#include <string>
#include <vector>

namespace {

using namespace mi_gain;

constexpr int GT_X = 64, GT_Y = 16;           // lattice columns x rows of a stats tile (256 lanes: 64 x 4, 4 rows each)

struct GainTile { int a, b, rec; int lx0, ly0, lx1, ly1; int _pad; };   // b < 0: cover tile of frame a (rec = a); else pair record rec

int lattice_lo(int x0, int step) { return (x0 + step - 1) / step; }       // x0 >= 0

void push_tiles(std::vector<GainTile>& tiles, int a, int b, int rec, int x0, int x1, int y0, int y1, int step) {
    const int lx0 = lattice_lo(x0, step), lx1 = x1 / step, ly0 = lattice_lo(y0, step), ly1 = y1 / step;
    if (lx0 > lx1 || ly0 > ly1) return;
    for (int ty = ly0; ty <= ly1; ty += GT_Y)
        for (int tx = lx0; tx <= lx1; tx += GT_X) {
            GainTile t;
            t.a = a; t.b = b; t.rec = rec; t.lx0 = tx; t.ly0 = ty;
            t.lx1 = std::min(tx + GT_X - 1, lx1); t.ly1 = std::min(ty + GT_Y - 1, ly1); t._pad = 0;
            tiles.push_back(t);
        }
}

// What a stats launcher knows after stats_setup: the frame table (also on the device, ctx buffer "gain_frames"), which frames take part,
// the canvas offset, and from them the work list.
struct StatsFrames {
    std::vector<FrameDev> fr;
    std::vector<char> part;
    float dG[2];
    const FrameDev* d_fr;
    void push_cover_tiles(std::vector<GainTile>& tiles, int step) const {
        for (size_t k = 0; k < fr.size(); k++)
            if (part[k]) push_tiles(tiles, (int)k, -1, (int)k, fr[k].begX, fr[k].endX, fr[k].begY, fr[k].endY, step);
    }
    // tiles over the intersection of the two canvas boxes; none where either frame takes no part
    void push_pair_tiles(std::vector<GainTile>& tiles, int a, int b, int rec, int step) const {
        if (!part[a] || !part[b]) return;
        const FrameDev &A = fr[a], &B = fr[b];
        push_tiles(tiles, a, b, rec, std::max(A.begX, B.begX), std::min(A.endX, B.endX), std::max(A.begY, B.begY), std::min(A.endY, B.endY), step);
    }
};

constexpr int BG_MAX_DIM = 1 << 20;           // block gains: the widest and tallest frame (bg_cell, bg_axis)

// The argument checks, the canvas layout and the frame table of the stats launchers; who ("gain_stats: ") prefixes the refusals.  grid
// (grid_x, grid_y; NULL for the per-frame stages) adds the block stage's limits: the grid's range, no side above BG_MAX_DIM, no frame that
// takes part smaller than the grid.  s.fr must stay until the stream has been synchronised.
int stats_setup(mi355_ctx* ctx, const std::string& who, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                const int32_t* pairs_ab, int n_pairs, int step, const int* grid, StatsFrames& s) {
    std::string err;
    if (!d_imgs || !w || !h || !ws || !h9s || (n_pairs > 0 && !pairs_ab) || n_pairs < 0) { ctx->set_error(who + "NULL argument or n_pairs < 0"); return MI355_ERR_ARG; }
    if (!check_frames_n(n, err) || !check_pairs(flat_pairs(pairs_ab), n_pairs, n, err) || (grid && !check_grid(grid[0], grid[1], err))) { ctx->set_error(who + err); return MI355_ERR_ARG; }
    if (step < 1 || step > 64) { ctx->set_error(who + "step=" + std::to_string(step) + " outside [1, 64]"); return MI355_ERR_ARG; }
    int cw, ch, cws;
    if (mi355_mosaic_layout(w, h, n, h9s, &cw, &ch, &cws, s.dG) != MI355_OK) { ctx->set_error(who + "no image with h[8] != 0 / empty canvas"); return MI355_ERR_FAILED; }
    s.fr.assign((size_t)n, FrameDev());
    s.part.assign((size_t)n, 0);
    for (int k = 0; k < n; k++) {
        if (!mi_frame_dev_setup(h9s + 9 * k, w[k], h[k], s.dG, cw, ch, 0, ch, s.fr[k])) continue;
        const std::string fk = who + "frame " + std::to_string(k);
        if (w[k] < 2 || h[k] < 2 || ws[k] < 3 * w[k] || (grid && (w[k] > BG_MAX_DIM || h[k] > BG_MAX_DIM))) { ctx->set_error(fk + ": bad geometry w=" + std::to_string(w[k]) + " h=" + std::to_string(h[k]) + " ws=" + std::to_string(ws[k])); return MI355_ERR_ARG; }
        if (grid && (w[k] < grid[0] || h[k] < grid[1])) { ctx->set_error(fk + " (" + std::to_string(w[k]) + "x" + std::to_string(h[k]) + ") is smaller than the " + std::to_string(grid[0]) + "x" + std::to_string(grid[1]) + " grid"); return MI355_ERR_ARG; }
        if (!d_imgs[k]) { ctx->set_error(fk + " takes part but its pointer is NULL"); return MI355_ERR_ARG; }
        s.fr[k].src = d_imgs[k]; s.fr[k].w = w[k]; s.fr[k].h = h[k]; s.fr[k].ws = ws[k];
        s.part[k] = 1;
    }
    DevBuf& dfr = ctx->buf("gain_frames");
    MI_HIP(dfr.reserve(sizeof(FrameDev) * (size_t)n));
    MI_HIP(hipMemcpyAsync(dfr.p, s.fr.data(), sizeof(FrameDev) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    s.d_fr = dfr.as<FrameDev>();
    return MI355_OK;
}

}  // namespace
