// A batch of meta-training tasks cut from HR frames that live on the device (dvsr_task_degrade / dvsr_task_gather).
//
// The reference makes one task per __getitem__ (codes/data/meta_learner/vsrbase.py:135-198): N frames are cropped at one
// position, blurred and sub-sampled with one kernel (HR -> LR), quantised to 8 bits, blurred again (LR -> SLR), and the three
// clips are flipped / transposed alike (preprocessing.py:209-237).  A batch of B tasks is B N items of a table of
// dvsr_task_frame: each names its crop (a pointer and strides into a frame as it was decoded), its kernel and its flags.
//
//   task_table_check      what both entries verify on the HOST copy of the table before anything is launched
//   task_gather_kernel    item i, channel c -> dst[i][c] = the crop as fp32 (bytes: v / 255.0f, dvsr_frame_ingest's division;
//                         fp32: copied), stored through the item's flags.  dvsr_task_degrade (degrade.hip) is the same table
//                         in front of the two degrade kernels.
//
// One workgroup = TG_THREADS * TG_UNROLL consecutive elements of one [H][W] plane of dst (grid.y = the 3 n planes); the item's
// row of the table is read once per workgroup (uniform).  A thread owns TG_UNROLL elements of dst, TG_THREADS apart, finds each
// one's source sample through the inverse of the store map -- dst[y][x] = r[fy(y)][fx(x)], or r[fy(x)][fx(y)] under
// DVSR_TASK_TRANSPOSE -- and issues all of its loads ahead of its first store, unconditionally (the spare threads of a plane's
// last workgroup are clamped to the last element), as frame_flip_kernel does and for its reasons.  Stores are consecutive
// 4-byte words of a wave; loads are consecutive (ascending or descending) samples except under the transpose, where consecutive
// lanes read a row apart: at the 64 x 64 planes of a task the whole crop sits in L2 and that is accepted.  No LDS, no atomics;
// every element of dst is written once.
#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace dvsr {

constexpr int TG_THREADS = 256, TG_UNROLL = 4;

template <bool BYTES>
__global__ __launch_bounds__(TG_THREADS) void task_gather_kernel(const dvsr_task_frame* __restrict__ items, float* __restrict__ dst,
                                                                 int H, int W, int pixel_stride, int swap) {
  const int plane = blockIdx.y, item = plane / 3, c = plane - 3 * item;
  const dvsr_task_frame t = items[item];
  const int hw = H * W;
  const int e0 = blockIdx.x * (TG_THREADS * TG_UNROLL) + threadIdx.x;
  const bool FULL = (int)(blockIdx.x + 1) * (TG_THREADS * TG_UNROLL) <= hw;   // (uniform: every workgroup of a plane but the last)
  long long off[TG_UNROLL];
#pragma unroll
  for (int k = 0; k < TG_UNROLL; ++k) {
    const int e = min(e0 + k * TG_THREADS, hw - 1);
    const int y = e / W, x = e - y * W;
    const int a = (t.flags & DVSR_TASK_TRANSPOSE) ? x : y, b = (t.flags & DVSR_TASK_TRANSPOSE) ? y : x;   // (H == W there)
    const int sy = (t.flags & DVSR_FLIP_H) ? H - 1 - a : a, sx = (t.flags & DVSR_FLIP_W) ? W - 1 - b : b;
    off[k] = BYTES ? sy * t.row_stride + sx * pixel_stride + (swap ? 2 - c : c) : c * t.plane_stride + sy * t.row_stride + sx;
  }
  float v[TG_UNROLL];
  if (BYTES) {
    unsigned char u[TG_UNROLL];
#pragma unroll
    for (int k = 0; k < TG_UNROLL; ++k) u[k] = static_cast<const unsigned char*>(t.src)[off[k]];
#pragma unroll
    for (int k = 0; k < TG_UNROLL; ++k) v[k] = (float)u[k] / 255.0f;   // IEEE division, as numpy's
  } else {
#pragma unroll
    for (int k = 0; k < TG_UNROLL; ++k) v[k] = static_cast<const float*>(t.src)[off[k]];
  }
  float* out = dst + (long long)plane * hw + e0;
  if (FULL) {
#pragma unroll
    for (int k = 0; k < TG_UNROLL; ++k) out[k * TG_THREADS] = v[k];
    return;
  }
#pragma unroll
  for (int k = 0; k < TG_UNROLL; ++k)
    if (e0 + k * TG_THREADS < hw) out[k * TG_THREADS] = v[k];
}

int task_table_check(const char* what, const dvsr_task_frame* items, const dvsr_task_frame* items_dev, int n, int format,
                     int pixel_stride, int H, int W, int n_kernels, bool square) {
  DVSR_REQUIRE(items && items_dev, DVSR_ERR_INVALID, "%s: null table (host / device copy)", what);
  DVSR_REQUIRE(n >= 1, DVSR_ERR_INVALID, "%s: n=%d items", what, n);
  DVSR_REQUIRE(3LL * n <= 65535, DVSR_ERR_UNSUPPORTED, "%s: n=%d items are more than 65535 planes", what, n);
  const bool u8 = format == DVSR_FRAME_U8_HWC_RGB || format == DVSR_FRAME_U8_HWC_BGR;
  DVSR_REQUIRE(u8 || format == DVSR_FRAME_F32_CHW, DVSR_ERR_INVALID, "%s: unknown frame format %d", what, format);
  DVSR_REQUIRE(!u8 || pixel_stride == 3 || pixel_stride == 4, DVSR_ERR_INVALID, "%s: pixel stride %d (3 or 4)", what, pixel_stride);
  DVSR_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= 0x7FFFFFFFLL - TG_THREADS * TG_UNROLL, DVSR_ERR_INVALID,
               "%s: crop size H=%d W=%d", what, H, W);
  DVSR_REQUIRE(reinterpret_cast<uintptr_t>(items_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(items) % 8 == 0, DVSR_ERR_INVALID,
               "%s: misaligned table (8 bytes)", what);
  const long long row = u8 ? (long long)W * pixel_stride : W;
  for (int i = 0; i < n; ++i) {
    const dvsr_task_frame& t = items[i];
    DVSR_REQUIRE(t.src, DVSR_ERR_INVALID, "%s: item %d: null source", what, i);
    DVSR_REQUIRE(t.row_stride >= row, DVSR_ERR_INVALID, "%s: item %d: row stride %lld shorter than a crop row of %lld %s", what, i,
                 t.row_stride, row, u8 ? "bytes" : "floats");
    if (!u8) {
      DVSR_REQUIRE(t.plane_stride >= (long long)(H - 1) * t.row_stride + W, DVSR_ERR_INVALID,
                   "%s: item %d: plane stride %lld shorter than a plane of %d rows", what, i, t.plane_stride, H);
      DVSR_REQUIRE(reinterpret_cast<uintptr_t>(t.src) % 4 == 0, DVSR_ERR_INVALID, "%s: item %d: misaligned fp32 source (4 bytes)",
                   what, i);
    }
    DVSR_REQUIRE(t.flags >= 0 && t.flags <= 7, DVSR_ERR_INVALID,
                 "%s: item %d: flags=%d outside 0 .. 7 (DVSR_FLIP_W | DVSR_FLIP_H | DVSR_TASK_TRANSPOSE)", what, i, t.flags);
    DVSR_REQUIRE(square || !(t.flags & DVSR_TASK_TRANSPOSE), DVSR_ERR_INVALID,
                 "%s: item %d: DVSR_TASK_TRANSPOSE of an output that is not square", what, i);
    DVSR_REQUIRE(n_kernels == 0 || (t.kernel >= 0 && t.kernel < n_kernels), DVSR_ERR_INVALID,
                 "%s: item %d: kernel index %d outside the %d kernels", what, i, t.kernel, n_kernels);
  }
  return DVSR_OK;
}

}  // namespace dvsr

using namespace dvsr;

extern "C" int dvsr_task_gather(const dvsr_task_frame* items, const dvsr_task_frame* items_dev, int n, int format,
                                int pixel_stride, int H, int W, float* dst, dvsr_stream_t stream) {
  DVSR_REQUIRE(dst, DVSR_ERR_INVALID, "task_gather: null dst");
  int rc = task_table_check("task_gather", items, items_dev, n, format, pixel_stride, H, W, 0, H == W);
  if (rc != DVSR_OK) return rc;
  DVSR_REQUIRE(reinterpret_cast<uintptr_t>(dst) % 4 == 0, DVSR_ERR_INVALID, "task_gather: misaligned fp32 destination (4 bytes)");
  const dim3 grid(ceil_div(H * W, TG_THREADS * TG_UNROLL), 3 * n);
  hipStream_t st = (hipStream_t)stream;
  if (format == DVSR_FRAME_F32_CHW)
    hipLaunchKernelGGL(task_gather_kernel<false>, grid, dim3(TG_THREADS), 0, st, items_dev, dst, H, W, 1, 0);
  else
    hipLaunchKernelGGL(task_gather_kernel<true>, grid, dim3(TG_THREADS), 0, st, items_dev, dst, H, W, pixel_stride,
                       format == DVSR_FRAME_U8_HWC_BGR ? 1 : 0);
  return check_launch("task_gather_kernel");
}
