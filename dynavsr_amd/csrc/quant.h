// The one quantiser of the library (metrics.hip: dvsr_frame_metrics, frame_io.hip / frame_rgb.hip: dvsr_frame_emit), so that the
// image they write is the same image.
#pragma once
#include <hip/hip_runtime.h>

namespace dvsr {

// clamp, rescale to [0,1], x top = 2^d - 1 (exact in fp32 up to d = 16), round half to even -- all in fp32 like torch / numpy
__device__ __forceinline__ int quant_levels(float v, float lo, float hi, float top) {
  const float t = (fminf(fmaxf(v, lo), hi) - lo) / (hi - lo);
  return (int)rintf(t * top);
}

// tensor2img: the 8-bit image
__device__ __forceinline__ int quant_u8(float v, float lo, float hi) { return quant_levels(v, lo, hi, 255.0f); }

}  // namespace dvsr
