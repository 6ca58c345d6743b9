// What the two table-walking resamplers share (frame_resize.hip, frame_imresize.hip): the limits of a tile and the wave-uniform
// table row -- the weights of one output in lanes 0 .. taps-1 of a register, its window start in lane RS_FIRST_LANE.
#pragma once
#include <cstddef>

namespace dvsr {

constexpr int RS_THREADS = 256;
constexpr int RS_ROWS = 64;        // staged rows at most: the lanes of a wave in the horizontal pass
constexpr int RS_MAXV = 12;        // 16-byte staging loads of a thread at most
constexpr int RS_MAX_TW = 64, RS_MAX_TH = 32;
constexpr int RS_COLS = RS_MAX_TW / 4, RS_OUTS = RS_MAX_TH / 4;   // output columns / rows of one wave at most
constexpr int RS_MAX_TAPS = 18;
constexpr int RS_FIRST_LANE = 32;  // the lane that holds a window's start beside the weights in lanes 0 .. taps-1
constexpr size_t RS_LDS_BYTES = 65536;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// lanes 0 .. taps-1: the weights of output `i`, lane RS_FIRST_LANE: its window start (as bits), every other lane 0
__device__ __forceinline__ float table_row(const int* first, const float* weights, int taps, int i, int lane) {
  const unsigned* p = lane == RS_FIRST_LANE ? reinterpret_cast<const unsigned*>(first + i)
                                            : reinterpret_cast<const unsigned*>(weights + (size_t)i * taps + min(lane, taps - 1));
  const unsigned v = *p;
  return (lane < taps || lane == RS_FIRST_LANE) ? __builtin_bit_cast(float, v) : 0.f;
}

__device__ __forceinline__ float lane_value(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

}  // namespace dvsr
