// csrc/feature_rows.h -- what the feature kernels of match.hip (rows already resident) and comm.hip (rows arriving in a record) share: the
// layout of a feature record and the one body that turns a descriptor row into the matcher's operands.  Included by those two units only.
#pragma once
#include "common.h"

// record layout: [0, 57344) keypoints (2048 x 28 B), [57344, 319488) descriptors u8 (2048 x 128); rows beyond the record's count are zero
constexpr size_t REC_KP_BYTES = (size_t)2048 * sizeof(mi355_keypoint), REC_D8_OFF = REC_KP_BYTES, REC_D8_BYTES = (size_t)2048 * 128;
static_assert(MI355_FEATURE_RECORD_BYTES >= REC_D8_OFF + REC_D8_BYTES && MI355_FEATURE_RECORD_BYTES % 256 == 0, "feature record");
static_assert(MI355_FEATURE_CHUNK_ROWS * sizeof(mi355_keypoint) == REC_KP_BYTES && MI355_FEATURE_CHUNK_ROWS * 128 == REC_D8_BYTES, "chunk rows");
static_assert((MI355_FEATURE_CHUNK_ROWS * sizeof(mi355_keypoint)) % 16 == 0, "a chunk's keypoints start 16-byte aligned");

constexpr unsigned FEATURE_BIAS4 = 0x80808080u;         // u - 128 = u ^ 0x80 as a byte: four descriptor bytes to the matcher's int8
// a padding row's piece: zeros after the shift
__device__ __forceinline__ uint4 feature_pad_piece() { return make_uint4(FEATURE_BIAS4, FEATURE_BIAS4, FEATURE_BIAS4, FEATURE_BIAS4); }

// The matcher's operands of one descriptor row: 8 lanes per row, lane `part` holds the row's bytes [16 part, 16 part + 16) in v (a padding
// row: feature_pad_piece()).  Writes the int8 piece s8[row][16 part ..] and, lane 0, the row's squared norm n8[row].  The 8 lanes of a row
// call it together: the sum crosses them by __shfl_xor.
//
// The norm is the int8 piece's dot product with itself, four bytes per v_dot4_i32_i8: the same integers as sixteen (u - 128)^2 summed one
// by one.  (That loop, written here, is unrolled before it is inlined; the kernels' reassociation pass then parts the sixteen products from
// their additions and the kernels take 27-28 VGPRs for the 19-20 the loop took when it stood in each of them.  The dot products take 16-17.)
__device__ __forceinline__ void feature_row_piece(uint4 v, int8_t* s8, int* n8, size_t row, int part) {
    const uint4 t = make_uint4(v.x ^ FEATURE_BIAS4, v.y ^ FEATURE_BIAS4, v.z ^ FEATURE_BIAS4, v.w ^ FEATURE_BIAS4);
    *reinterpret_cast<uint4*>(s8 + row * 128 + part * 16) = t;
    int s = __builtin_amdgcn_sdot4((int)t.x, (int)t.x, 0, false);
    s = __builtin_amdgcn_sdot4((int)t.y, (int)t.y, s, false);
    s = __builtin_amdgcn_sdot4((int)t.z, (int)t.z, s, false);
    s = __builtin_amdgcn_sdot4((int)t.w, (int)t.w, s, false);
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
    if (part == 0) n8[row] = s;
}
