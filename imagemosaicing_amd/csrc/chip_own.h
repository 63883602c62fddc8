// csrc/chip_own.h -- what the kernels that decide the chips' ownership share: warp.hip (distmax_kernel, owner_kernel, mask_bbox_kernel) and
// blend_seam.hip (blend_seam_candidates_kernel, owner_cells_kernel).  The types stay in an anonymous namespace, one copy per translation unit:
// they are part of the kernels' names, "(anonymous namespace)::owner_kernel((anonymous namespace)::ChipDev const*, ...", which profiles/ quote.
// The device tables of one ownership call cross between the two files as chips::OwnTables, untyped.
#pragma once
#include "common.h"

namespace {

struct ChipDev { int x0, y0, w, h, mws; size_t map_off; };

struct LineSet { float A[4], B[4], C[4], inv[4]; };

// distance of chip pixel (c, r) to the nearest of the 4 quad edges (MosaicImage.cpp:1790-1826); ONE expression for the kernels that use it:
// the ownership kernel recomputes what the maximum kernel saw, so the values must be the same bits
__device__ __forceinline__ float quad_min_dist(const LineSet& L, int c, int r) {
    float minDist = (float)(1 << 29);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float d = fabsf(L.A[i] * (float)c + L.B[i] * (float)r + L.C[i]) * L.inv[i];
        if (d < minDist) minDist = d;
    }
    return minDist;
}

constexpr int OWN_BLK = 256;
constexpr int OWN_ROWS = 4;
// The chips of the block (uniform over the workgroup: 64 x 4 threads inside one block) are staged in LDS, 32 at a time: with the
// descriptors read per thread and per chip from global memory every candidate was a chain of four dependent loads (list -> chip ->
// mask pointer -> mask byte) and the kernel ran at 0.2 TB/s of its own byte traffic.
struct OwnEntry { int x0, y0, w, h, mws, k; float maxv; int pad; uint8_t* mask; LineSet L; };

}  // namespace

namespace chips {

// the device tables of one ownership call (ChipStage::ownership, warp.hip), entries by chip position: ChipDev, mask pointers, chip pixel pointers,
// image indices, maxima (float bits), LineSet, and the per-256 x 256-block chip lists (list_off[blocks + 1], list)
struct OwnTables {
    const void* chips; uint8_t* const* masks; const uint8_t* const* pixels; const int* img; const unsigned* maxbits; const void* lines;
    const int* list_off; const int* list; int bx_n, W, H;
};

}  // namespace chips

// blend_seam.hip: stage 1 of the multiband blend along optimised seams into d_cand (gh x gw records), and the ownership that follows d_cells
int mi_blend_seam_candidates_launch(mi355_ctx* ctx, const chips::OwnTables& t, const mi355_seamcut_params* params, mi355_seam_cell* d_cand, int gw, int gh);
int mi_owner_cells_launch(mi355_ctx* ctx, const chips::OwnTables& t, const uint16_t* d_cells, int gw, int level);
