// Flip-test x4 self-ensemble of the video path (dvsr_frame_flip / dvsr_frame_flip_mean).
//
// The reference's flipx4_forward (utils/util.py:232-254) runs the network on a clip as it is, flipped in W, in H and in both,
// un-flips the three outputs and returns (((y0 + flipW(y1)) + flipH(y2)) + flipHW(y3)) / 4.  The two data movements of it:
//
//   frame_flip_kernel        fp32 planar [planes][H][W] -> the same, mirrored in W (DVSR_FLIP_W), in H (DVSR_FLIP_H), in both,
//                            or copied (flags 0): what is fed to the network
//   frame_flip_mean_kernel   four such tensors -> dst = (((y0 + flipW(yw)) + flipH(yh)) + flipHW(yhw)) * 0.25f: the un-flips
//                            and the mean in one pass, four reads and one write per element
//
// W % 4 == 0 and every pointer is 16-byte aligned, so a row is W / 4 chunks of one float4.  A thread owns a chunk of dst: the
// mirrored source chunk is the float4 at column W - 4 - x with its four components reversed in registers, the H flip is row
// arithmetic -- every load and store is a 16-byte access, consecutive lanes at consecutive (or, mirrored, descending) addresses,
// 1 KiB per wave instruction either way.  A thread takes UNROLL chunks, 256 chunks apart, and issues all of their loads ahead
// of its first store (a load behind a store that the compiler cannot prove disjoint waits for it).  No LDS, no atomics, one
// launch; every element of dst is written once and nothing else is.  The loads are unconditional -- those of the last
// workgroup's spare threads are clamped to the last chunk -- and every workgroup but the last stores without a test: a load or a
// store under a branch gets a wait of its own.  The chunk index is 32-bit where the tensor allows it (its two divisions are the
// kernel's only arithmetic of note).
// The additions of the mean are in the reference's statement order, in fp32, never contracted: the result equals the torch
// composition bit for bit; * 0.25f is exact.
#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace dvsr {

constexpr int FL_THREADS = 256;
constexpr int FL_UNROLL_FLIP = 4, FL_UNROLL_MEAN = 2;   // chunks of a thread: 4 resp. 8 16-byte loads in flight

__device__ __forceinline__ f32x4 reversed(f32x4 v) { return f32x4{v[3], v[2], v[1], v[0]}; }

// chunk q of dst = (row q / w4 of planes * H rows, chunk q % w4 of the row) -> the source chunk under `flags`
template <typename Idx>
__device__ __forceinline__ Idx flipped_chunk(Idx q, int H, int w4, int flags) {
  const Idx row = q / (Idx)w4;
  const int c = (int)(q - row * (Idx)w4);
  const Idx plane = row / (Idx)H;
  const int y = (int)(row - plane * (Idx)H);
  const int sy = (flags & 2) ? H - 1 - y : y;
  const int sc = (flags & 1) ? w4 - 1 - c : c;
  return (plane * (Idx)H + (Idx)sy) * (Idx)w4 + (Idx)sc;
}

template <typename Idx>
__global__ __launch_bounds__(FL_THREADS) void frame_flip_kernel(const f32x4* __restrict__ src, f32x4* __restrict__ dst, Idx n4,
                                                                int H, int w4, int flags) {
  const Idx q0 = (Idx)blockIdx.x * (Idx)(FL_THREADS * FL_UNROLL_FLIP) + (Idx)threadIdx.x;
  const bool FULL = (Idx)(blockIdx.x + 1) * (Idx)(FL_THREADS * FL_UNROLL_FLIP) <= n4;   // (uniform: every workgroup but the last)
  f32x4 v[FL_UNROLL_FLIP];
#pragma unroll
  for (int k = 0; k < FL_UNROLL_FLIP; ++k) {
    const Idx q = min(q0 + (Idx)(k * FL_THREADS), n4 - 1);
    v[k] = src[flipped_chunk<Idx>(q, H, w4, flags)];
  }
  if (FULL) {
#pragma unroll
    for (int k = 0; k < FL_UNROLL_FLIP; ++k) dst[q0 + (Idx)(k * FL_THREADS)] = (flags & 1) ? reversed(v[k]) : v[k];
    return;
  }
#pragma unroll
  for (int k = 0; k < FL_UNROLL_FLIP; ++k) {
    const Idx q = q0 + (Idx)(k * FL_THREADS);
    if (q < n4) dst[q] = (flags & 1) ? reversed(v[k]) : v[k];
  }
}

template <typename Idx>
__global__ __launch_bounds__(FL_THREADS) void frame_flip_mean_kernel(const f32x4* __restrict__ y0, const f32x4* __restrict__ yw,
                                                                     const f32x4* __restrict__ yh, const f32x4* __restrict__ yhw,
                                                                     f32x4* __restrict__ dst, Idx n4, int H, int w4) {
#pragma clang fp contract(off)
  const Idx q0 = (Idx)blockIdx.x * (Idx)(FL_THREADS * FL_UNROLL_MEAN) + (Idx)threadIdx.x;
  const bool FULL = (Idx)(blockIdx.x + 1) * (Idx)(FL_THREADS * FL_UNROLL_MEAN) <= n4;   // (uniform: every workgroup but the last)
  f32x4 a[FL_UNROLL_MEAN], b[FL_UNROLL_MEAN], c[FL_UNROLL_MEAN], d[FL_UNROLL_MEAN];
#pragma unroll
  for (int k = 0; k < FL_UNROLL_MEAN; ++k) {
    const Idx q = min(q0 + (Idx)(k * FL_THREADS), n4 - 1);
    a[k] = y0[q];
    b[k] = yw[flipped_chunk<Idx>(q, H, w4, 1)];
    c[k] = yh[flipped_chunk<Idx>(q, H, w4, 2)];
    d[k] = yhw[flipped_chunk<Idx>(q, H, w4, 3)];
  }
  f32x4 r[FL_UNROLL_MEAN];
#pragma unroll
  for (int k = 0; k < FL_UNROLL_MEAN; ++k) {
    const f32x4 bw = reversed(b[k]), dw = reversed(d[k]);
#pragma unroll
    for (int e = 0; e < 4; ++e) r[k][e] = (((a[k][e] + bw[e]) + c[k][e]) + dw[e]) * 0.25f;
  }
  if (FULL) {
#pragma unroll
    for (int k = 0; k < FL_UNROLL_MEAN; ++k) dst[q0 + (Idx)(k * FL_THREADS)] = r[k];
    return;
  }
#pragma unroll
  for (int k = 0; k < FL_UNROLL_MEAN; ++k) {
    const Idx q = q0 + (Idx)(k * FL_THREADS);
    if (q < n4) dst[q] = r[k];
  }
}

static bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// the chunks of [planes][H][W] and the grid of `per_block` chunks per workgroup; DVSR_ERR_INVALID for a bad shape
static int flip_geometry(const char* what, long long planes, int H, int W, int per_block, long long* n4, unsigned* blocks) {
  DVSR_REQUIRE(planes >= 1 && H >= 1 && W >= 1, DVSR_ERR_INVALID, "%s: planes=%lld, H=%d, W=%d must be positive", what, planes, H, W);
  DVSR_REQUIRE(W % 4 == 0, DVSR_ERR_INVALID, "%s: W=%d must be a multiple of 4", what, W);
  const long long rows_max = (0x7FFFFFFFLL * per_block) / (W / 4);      // n4 / per_block must fit a grid's x dimension
  DVSR_REQUIRE(planes <= rows_max / H, DVSR_ERR_INVALID, "%s: %lld planes of %d x %d are too many for one launch", what, planes, H, W);
  *n4 = planes * H * (W / 4);
  *blocks = (unsigned)((*n4 + per_block - 1) / per_block);
  return DVSR_OK;
}

}  // namespace dvsr

using namespace dvsr;

extern "C" int dvsr_frame_flip(const float* src, float* dst, long long planes, int H, int W, int flags, dvsr_stream_t stream) {
  DVSR_REQUIRE(src && dst, DVSR_ERR_INVALID, "frame_flip: null tensor");
  long long n4 = 0;
  unsigned blocks = 0;
  int rc = flip_geometry("frame_flip", planes, H, W, FL_THREADS * FL_UNROLL_FLIP, &n4, &blocks);
  if (rc != DVSR_OK) return rc;
  DVSR_REQUIRE(flags >= 0 && flags <= 3, DVSR_ERR_INVALID, "frame_flip: flags=%d outside 0 .. 3 (DVSR_FLIP_W | DVSR_FLIP_H)", flags);
  DVSR_REQUIRE(aligned16(src) && aligned16(dst), DVSR_ERR_INVALID, "frame_flip: misaligned planar fp32 tensor (16 bytes)");
  DVSR_REQUIRE(src != dst, DVSR_ERR_INVALID, "frame_flip: dst is src (flipping in place is not provided)");
  const f32x4* s = reinterpret_cast<const f32x4*>(src);
  f32x4* d = reinterpret_cast<f32x4*>(dst);
  hipStream_t st = (hipStream_t)stream;
  if (n4 <= 0x7FFFFFFFLL)
    hipLaunchKernelGGL(frame_flip_kernel<unsigned>, dim3(blocks), dim3(FL_THREADS), 0, st, s, d, (unsigned)n4, H, W / 4, flags);
  else
    hipLaunchKernelGGL(frame_flip_kernel<unsigned long long>, dim3(blocks), dim3(FL_THREADS), 0, st, s, d, (unsigned long long)n4, H,
                       W / 4, flags);
  return check_launch("frame_flip_kernel");
}

extern "C" int dvsr_frame_flip_mean(const float* y0, const float* yw, const float* yh, const float* yhw, float* dst,
                                    long long planes, int H, int W, dvsr_stream_t stream) {
  DVSR_REQUIRE(y0 && yw && yh && yhw && dst, DVSR_ERR_INVALID, "frame_flip_mean: null tensor");
  long long n4 = 0;
  unsigned blocks = 0;
  int rc = flip_geometry("frame_flip_mean", planes, H, W, FL_THREADS * FL_UNROLL_MEAN, &n4, &blocks);
  if (rc != DVSR_OK) return rc;
  DVSR_REQUIRE(aligned16(y0) && aligned16(yw) && aligned16(yh) && aligned16(yhw) && aligned16(dst), DVSR_ERR_INVALID,
               "frame_flip_mean: misaligned planar fp32 tensor (16 bytes)");
  DVSR_REQUIRE(dst != y0 && dst != yw && dst != yh && dst != yhw, DVSR_ERR_INVALID,
               "frame_flip_mean: dst is one of the sources (averaging in place is not provided)");
  const f32x4 *a = reinterpret_cast<const f32x4*>(y0), *b = reinterpret_cast<const f32x4*>(yw);
  const f32x4 *c = reinterpret_cast<const f32x4*>(yh), *e = reinterpret_cast<const f32x4*>(yhw);
  f32x4* d = reinterpret_cast<f32x4*>(dst);
  hipStream_t st = (hipStream_t)stream;
  if (n4 <= 0x7FFFFFFFLL)
    hipLaunchKernelGGL(frame_flip_mean_kernel<unsigned>, dim3(blocks), dim3(FL_THREADS), 0, st, a, b, c, e, d, (unsigned)n4, H, W / 4);
  else
    hipLaunchKernelGGL(frame_flip_mean_kernel<unsigned long long>, dim3(blocks), dim3(FL_THREADS), 0, st, a, b, c, e, d,
                       (unsigned long long)n4, H, W / 4);
  return check_launch("frame_flip_mean_kernel");
}
