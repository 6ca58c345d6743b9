// What the frame kernels share (frame_io.hip, frame_yuv.hip): the padded axis, and the host checks of the planar fp32 side and of
// the pad mode.
#pragma once
#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace dvsr {

// index i of a padded axis -> index of the frame's own axis of length n (i < 2n - 1 under REFLECT: frame_pad_check)
__device__ __forceinline__ int pad_index(int i, int n, int mode) {
  return i < n ? i : (mode == DVSR_FRAME_PAD_REFLECT ? 2 * (n - 1) - i : n - 1);
}

// the planar fp32 side: [3][H][W], 16-byte accesses; a workgroup covers wg_rows rows (grid.y <= 65535)
inline int frame_planar_check(const char* what, const float* ptr, int H, int W, int wg_rows) {
  DVSR_REQUIRE(ptr, DVSR_ERR_INVALID, "%s: null planar tensor", what);
  DVSR_REQUIRE(H >= 1 && W >= 4 && W % 4 == 0 && H <= wg_rows * 65535, DVSR_ERR_INVALID,
               "%s: planar tensor H=%d W=%d (W must be a positive multiple of 4)", what, H, W);
  DVSR_REQUIRE(reinterpret_cast<uintptr_t>(ptr) % 16 == 0, DVSR_ERR_INVALID, "%s: misaligned planar fp32 tensor (16 bytes)", what);
  return DVSR_OK;
}

// an h x w frame padded to Hp x Wp at the bottom and right
inline int frame_pad_check(const char* what, int pad_mode, int h, int w, int Hp, int Wp) {
  DVSR_REQUIRE(pad_mode == DVSR_FRAME_PAD_REFLECT || pad_mode == DVSR_FRAME_PAD_REPLICATE, DVSR_ERR_INVALID,
               "%s: unknown pad mode %d", what, pad_mode);
  DVSR_REQUIRE(pad_mode != DVSR_FRAME_PAD_REFLECT || (Hp - h < h && Wp - w < w), DVSR_ERR_INVALID,
               "%s: reflect pad %d x %d not smaller than the frame %d x %d", what, Hp - h, Wp - w, h, w);
  return DVSR_OK;
}

}  // namespace dvsr
