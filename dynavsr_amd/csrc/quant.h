// The one 8-bit quantiser of the library (metrics.hip: dvsr_frame_metrics, frame_io.hip: dvsr_frame_emit), so that the
// image both write is the same image.
#pragma once
#include <hip/hip_runtime.h>

namespace dvsr {

// tensor2img: clamp, rescale to [0,1], x 255, round half to even -- all in fp32 like torch / numpy do it
__device__ __forceinline__ int quant_u8(float v, float lo, float hi) {
  const float t = (fminf(fmaxf(v, lo), hi) - lo) / (hi - lo);
  return (int)rintf(t * 255.0f);
}

}  // namespace dvsr
