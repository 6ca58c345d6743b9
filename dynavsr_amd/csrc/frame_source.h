// Where the staging loops of the kernels that read a frame as it arrives (degrade.hip, frame_imresize.hip) read from.  A policy
// gives row(plane, y, lut), the row y of plane `plane`, col(x), the offset of column x inside a row, and
// Row::operator[](offset), the sample as fp32; LUT is the number of floats of LDS it wants behind the kernel's own, filled by
// fill(lut, tid, threads) ahead of a barrier.  Everything behind the staging sees fp32 in LDS and is the same code for every
// source.
#pragma once

namespace dvsr {

struct SrcPlanarF32 {  // fp32 planes by stride: the [N,C,H,W] clip of dvsr_degrade_apply, a DVSR_FRAME_F32_CHW frame
  static constexpr int LUT = 0;
  const float* base;
  long long row_stride, plane_stride;  // floats
  struct Row {
    const float* p;
    __device__ __forceinline__ float operator[](int off) const { return p[off]; }
  };
  __device__ __forceinline__ void fill(float*, int, int) const {}
  __device__ __forceinline__ Row row(int plane, int y, const float*) const {
    return Row{base + plane * plane_stride + y * row_stride};
  }
  __device__ __forceinline__ int col(int x) const { return x; }
};

// 8-bit interleaved RGB / BGR by stride and channel: v / 255.0f, dvsr_frame_ingest's true division -- made once per value and
// workgroup into a 256-entry table in LDS.  With a division per staged sample a uint8 720 x 1280 frame at scale 4, K = 27 took
// 34.8 us against 30.9 us with the table, a 2160 x 3840 frame 194.4 against 175.7 (profiles/r19_frame_degrade.txt).  The three
// workgroups of a tile (one per channel) each fetch its bytes: the second and third find them in the caches.
struct SrcBytesHWC {
  static constexpr int LUT = 256;
  const unsigned char* base;
  long long row_stride;  // bytes
  int pixel_stride, swap;
  struct Row {
    const unsigned char* p;
    const float* lut;
    __device__ __forceinline__ float operator[](int off) const { return lut[p[off]]; }
  };
  __device__ __forceinline__ void fill(float* lut, int tid, int threads) const {
    for (int i = tid; i < LUT; i += threads) lut[i] = (float)i / 255.0f;
  }
  __device__ __forceinline__ Row row(int plane, int y, const float* lut) const {
    return Row{base + y * row_stride + (swap ? 2 - plane : plane), lut};
  }
  __device__ __forceinline__ int col(int x) const { return x * pixel_stride; }
};

}  // namespace dvsr
