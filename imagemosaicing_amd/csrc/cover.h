// csrc/cover.h -- what cover.hip (kernel, launcher, geometry) and cover_select.cpp (host only: parameter checks and the selection loop) take
// from each other.  err receives the refusal without a prefix; the caller names itself in front of it.
#pragma once
#include "../../include/mi355_mosaic.h"
#include <functional>
#include <string>

namespace mi_cover {

struct Box { int x0, x1, y0, y1; };              // a frame's clipped canvas box, ends included (FrameDev begX, endX, begY, endY)

bool check_cover_params(const mi355_cover_params& p, std::string& err);

// one round's statistics under keep (n bytes) into fs (n records); other than MI355_OK: the selection ends with that code and err
using StatsFn = std::function<int(const uint8_t* keep, mi355_cover_frame_stats* fs, std::string& err)>;

// The selection of "cover depth" on boxes: part[k] != 0 where frame k takes part, box[k] its clipped box (read only where it takes part).
// Checks n, the parameters, order and the pair list.  status / keep_out: n bytes; rounds / lost may be NULL.
int select(int n, const Box* box, const char* part, const uint8_t* keep, const int32_t* order, int n_order, const int32_t* pairs_ab, int n_pairs,
           const mi355_cover_params& p, const StatsFn& stats, uint8_t* status, uint8_t* keep_out, int32_t* rounds, int64_t* lost, std::string& err);

// cover.hip: the layout for h9s as passed and, per frame, whether it takes part and its box (n entries each; n already checked).  Refuses a
// taking-part frame with w < 2 or h < 2 (MI355_ERR_ARG) and a survey without a canvas (MI355_ERR_FAILED).
int frame_boxes(const int* w, const int* h, int n, const float* h9s, Box* box, char* part, std::string& err);

}  // namespace mi_cover
