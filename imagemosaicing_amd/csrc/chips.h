// csrc/chips.h -- what the chip stage of LaplacianPyramidBlending (warp.hip: warps, validity, FindMasksByDistMap ownership) hands to its
// callers (warp.hip's C ABI boundary, blend.hip's one-call blend): one object per call, nothing left behind in the context.
#pragma once
#include "common.h"

namespace chips {

struct WarpArgs {
    const uint8_t* src; int w, h, ws;          // source image
    uint8_t* dst; int dws;                      // destination (canvas / chip / tight image), row stride
    uint8_t* mask; int mws;                     // chip validity mask (CHIP mode) or nullptr
    int x_beg, x_end, y_beg, y_end;             // inclusive destination range to visit
    float inv[9];                               // inverse homography (destination -> source)
    float dx, dy;                               // mode 0: xs = (float)xD - dx
    float sx, sy; int x0, y0;                   // mode 1 (chips): ((float)xD - dx) - sx + (float)x0
};

// The forms of the stage that exist:
//   PUBLIC        mi355_chips_and_masks: host frames, find_masks either way, the pixels made at once, the whole canvas
//   BLEND_HOST    the one-call blend: ownership with the owned boxes; the validity masks at once, the PIXELS only where asked for afterwards,
//                 chip by chip (mi_chip_pixels_prepare / _launch: the blender needs them inside a chip's active window only)
//   BLEND_DEVICE  ... from frames in HBM, for the canvas rows row_lo .. row_hi (inclusive); cover_only != NULL: cover_only[k] = 1 for the frames
//                 whose chips the call would form, nothing else is done
//   SEAM_HOST /  the blend along optimised seams (blend_seam.hip), from host frames (the two-stage public form) or from frames in HBM: the
//   SEAM_DEVICE   validity masks, then the pixels of WHOLE chips (stage 1 reads every candidate's bytes around the seams), the maxima, stage 1
//                 and the labels unless a cell map came with the request, and the ownership that follows the map, with the owned boxes.  The
//                 whole canvas only.  seam.stop_after_cells: nothing after the cell map is done (mi355_blend_seam_cells_dev).
// Deferred pixels, owned boxes and a row window are one form, not three flags; a row window in another form is refused.
struct SeamRequest {
    const mi355_seamcut_params* params = nullptr;       // range-checked by the caller
    uint16_t* d_cells = nullptr; int gw = 0, gh = 0;     // DEVICE gh x gw: read when make_cells is false, written first when it is true
    bool make_cells = false, stop_after_cells = false;
    mi355_seam_cell* d_cand = nullptr;                   // DEVICE, may be NULL: where stage 1's records go (the ctx's own buffer otherwise)
    mi355_seam_report* report = nullptr;                 // HOST, may be NULL
};
struct Request {
    enum Form { PUBLIC, BLEND_HOST, BLEND_DEVICE, SEAM_HOST, SEAM_DEVICE } form;
    int find_masks = 1, row_lo = 0, row_hi = 0x7fffffff; uint8_t* cover_only = nullptr;
    SeamRequest seam = {};
    bool one_call() const { return form != PUBLIC; }
    bool on_device() const { return form == BLEND_DEVICE || form == SEAM_DEVICE; }
    bool seams() const { return form == SEAM_HOST || form == SEAM_DEVICE; }
};

// The chips and masks themselves stay in the ctx buffers "chip_imgs" / "chip_masks" at chip_off[v] / mask_off[v].
struct ChipSet {
    int W = 0, H = 0;                           // canvas
    std::vector<mi355_chip_info> info;          // per chip, in the reference's order (ascending frame)
    std::vector<size_t> chip_off, mask_off;
    std::vector<int> owned;                     // one-call form: per chip {min col, min row, max col, max row} of its non-zero mask bytes (max < min: none)
    std::vector<WarpArgs> warps;                // one-call form: the chips' warp arguments, their pixels still to be made ...
    bool pixels_made = false;                   // ... unless the stage made whole chips already (the seam forms)
    std::vector<int> dims;                      // ... and per prepared entry the launch extent (groups of 4 columns, rows)
    int n() const { return (int)info.size(); }
};

}  // namespace chips

int mi_chips_and_masks_dev(mi355_ctx*, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                           const uint8_t* keep, const chips::Request& req, chips::ChipSet& set);
int mi_chip_pixels_prepare(mi355_ctx*, chips::ChipSet& set, int n, const int* chips, const int* win4);      // entry e = chip chips[e] inside win4[4e..] (columns / rows inclusive, clipped to the chip): arguments to the device
int mi_chip_pixels_launch(mi355_ctx*, const chips::ChipSet& set, int first, int count);                   // one launch for entries first .. first + count - 1
// the C ABI's form of the chip set, for the forms whose chips hold their pixels on return (PUBLIC, SEAM_HOST): malloc'd arrays, chips and masks on the host
int mi_chips_and_masks_host(mi355_ctx*, const uint8_t* const* imgs, const int* w, const int* h, const int* ws, int n, const float* h9s, const uint8_t* keep,
                            const chips::Request& req, int* n_chips, mi355_chip_info** chips, uint8_t*** chip_imgs, uint8_t*** masks, int* cw, int* ch);
