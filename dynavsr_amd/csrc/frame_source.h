// Where the staging loops of the kernels that read a frame as it arrives (degrade.hip, frame_imresize.hip) read from.  A policy
// gives row(plane, y, lut), the row y of plane `plane`, col(x), the offset of column x inside a row, and
// Row::operator[](offset), the sample as fp32; LUT is the number of floats of LDS it wants behind the kernel's own, filled by
// fill(lut, tid, threads) ahead of a barrier.  Everything behind the staging sees fp32 in LDS and is the same code for every
// source.
//
// A TABLE policy (degrade.hip, task.hip) reads a batch: plane p of the launch is channel p % 3 of item p / 3 of a table of
// dvsr_task_frame in device memory, which gives the item's base, strides and kernel index (kernel(item)).  The entry has
// validated every row of the host copy of that table before the launch.  The reads of the table are uniform over a workgroup.
//
// Where the same kernels store to: a destination policy gives plane(p, Ho, Wo), the [Ho][Wo] plane p of the output, and
// Plane::store(oy, ox, v).  DstStrided is a plane by stride; DstTask stores through the item's flags -- the reference's augment
// (hflip, vflip, then the permute) on the result, not on the input.
#pragma once

#include "../../include/dynavsr_hip.h"

namespace dvsr {

struct SrcPlanarF32 {  // fp32 planes by stride: the [N,C,H,W] clip of dvsr_degrade_apply, a DVSR_FRAME_F32_CHW frame
  static constexpr int LUT = 0;
  static constexpr bool TABLE = false;
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
  static constexpr bool TABLE = false;
  const unsigned char* base;
  long long row_stride;  // bytes
  int pixel_stride, swap;
  struct Row {
    const unsigned char* p;
    const float* lut;
    __device__ __forceinline__ float operator[](int off) const { return lut[p[off]]; }
  };
  __device__ __forceinline__ static void fill(float* lut, int tid, int threads) {
    for (int i = tid; i < LUT; i += threads) lut[i] = (float)i / 255.0f;
  }
  __device__ __forceinline__ Row row(int plane, int y, const float* lut) const {
    return Row{base + y * row_stride + (swap ? 2 - plane : plane), lut};
  }
  __device__ __forceinline__ int col(int x) const { return x * pixel_stride; }
};

// the items of a table as fp32 planes: item.src is channel 0 of the crop, row_stride and plane_stride in floats
struct SrcTaskF32 {
  static constexpr int LUT = 0;
  static constexpr bool TABLE = true;
  const dvsr_task_frame* __restrict__ items;
  using Row = SrcPlanarF32::Row;
  __device__ __forceinline__ void fill(float*, int, int) const {}
  __device__ __forceinline__ Row row(int plane, int y, const float*) const {
    const int i = plane / 3;
    const dvsr_task_frame t = items[i];
    return Row{static_cast<const float*>(t.src) + (plane - 3 * i) * t.plane_stride + y * t.row_stride};
  }
  __device__ __forceinline__ int col(int x) const { return x; }
  __device__ __forceinline__ int kernel(int item) const { return items[item].kernel; }
};

// the items of a table as interleaved bytes: item.src is the crop's first pixel, row_stride in bytes; one pixel stride and one
// channel order for the launch
struct SrcTaskBytes {
  static constexpr int LUT = 256;
  static constexpr bool TABLE = true;
  const dvsr_task_frame* __restrict__ items;
  int pixel_stride, swap;
  using Row = SrcBytesHWC::Row;
  __device__ __forceinline__ void fill(float* lut, int tid, int threads) const { SrcBytesHWC::fill(lut, tid, threads); }
  __device__ __forceinline__ Row row(int plane, int y, const float* lut) const {
    const int i = plane / 3, c = plane - 3 * i;
    const dvsr_task_frame t = items[i];
    return Row{static_cast<const unsigned char*>(t.src) + y * t.row_stride + (swap ? 2 - c : c), lut};
  }
  __device__ __forceinline__ int col(int x) const { return x * pixel_stride; }
  __device__ __forceinline__ int kernel(int item) const { return items[item].kernel; }
};

struct DstStrided {  // [Ho][Wo] planes by stride, in floats
  float* y;
  long long row_stride, plane_stride;
  struct Plane {
    float* p;
    long long row_stride;
    __device__ __forceinline__ void store(int oy, int ox, float v) const { p[oy * row_stride + ox] = v; }
  };
  __device__ __forceinline__ Plane plane(int plane, int, int) const { return Plane{y + plane * plane_stride, row_stride}; }
};

// contiguous [n][3][Ho][Wo] through the flags of the plane's item: result r, f[y][x] = r[fy(y)][fx(x)] (dvsr_frame_flip's fx and
// fy, each its own inverse), dst[y][x] = f[y][x], or f[x][y] under DVSR_TASK_TRANSPOSE (Ho == Wo).  So r[oy][ox] lands at
// f[fy(oy)][fx(ox)].  A transposed store puts consecutive lanes a row apart: it does not coalesce, and at the 64 x 64 and
// 16 x 16 planes of a task that is accepted.
struct DstTask {
  float* y;
  const dvsr_task_frame* __restrict__ items;
  struct Plane {
    float* p;
    int Ho, Wo, flags;
    __device__ __forceinline__ void store(int oy, int ox, float v) const {
      const int a = (flags & DVSR_FLIP_H) ? Ho - 1 - oy : oy, b = (flags & DVSR_FLIP_W) ? Wo - 1 - ox : ox;
      p[(flags & DVSR_TASK_TRANSPOSE) ? b * Wo + a : a * Wo + b] = v;
    }
  };
  __device__ __forceinline__ Plane plane(int plane, int Ho, int Wo) const {
    return Plane{y + (long long)plane * Ho * Wo, Ho, Wo, items[plane / 3].flags};
  }
};

}  // namespace dvsr
