// Frames in and out of the video path (dvsr_frame_ingest / dvsr_frame_emit, engine.hip: dvsr_edvr_stream_extract_frame).
//
// A decoder delivers 8-bit interleaved RGB / BGR rows (sometimes with a fourth byte per pixel) at any size, address and row
// pitch; the network wants fp32 planar [3][Hp][Wp] in [0,1] with Hp, Wp multiples of 4, and the encoder wants 8-bit
// interleaved back.  The reference does both on the host: `img.astype(np.float32) / 255.` (data/util.py:82), BGR -> RGB
// (:109), and util.tensor2img (clamp, x 255, round half to even) on a frame copied back as fp32.
//   frame_ingest_*_kernel   source frame h x w -> fp32 planar [3][Hp][Wp]: v / 255.0f (a true division: v * (1/255.f) differs
//                           from numpy on 126 of the 256 values), BGR swapped to RGB, rows / columns beyond h x w filled from
//                           the frame itself at the bottom and right (reflect without edge repeat, or replicate)
//   (16-bit interleaved and planar integer RGB / GBR: the same two entry points dispatch to frame_rgb.hip)
//   frame_emit_*_kernel     fp32 planar [3][Hs][Ws] -> the top-left h x w crop as 8-bit HWC (quant_u8 of quant.h, the
//                           quantiser of dvsr_frame_metrics) or as fp32 planar; bytes outside the crop are not touched
// One thread = 4 consecutive pixels of a row in all three planes: three 16-byte accesses on the aligned fp32 side and 12
// (pixel stride 4: 16) contiguous bytes on the other.  A workgroup is 64 x 4 threads, so a wave works on ONE row and whatever
// depends on the row's address is wave-uniform: a row of the byte side that starts on a dword boundary moves as dwords, any
// other row of a source is assembled from the aligned dwords around it (v_alignbyte_b32), and a lane's 12 bytes of any other
// row of a destination go out as the bytes up to the next dword boundary, two dwords and the rest.  No access is wider than
// its address is aligned; only the lanes that hold padded columns or the ragged end of a row work pixel by pixel.
// Pure streaming, every lane touches its pixels once: all its loads come ahead of its first store and there is no grid-stride
// loop (stream_gather.hip: gfx9 counts stores in vmcnt too, in order).
#include <cstdint>

#include "frame_common.h"
#include "quant.h"

namespace dvsr {

constexpr int FIO_X = 64, FIO_Y = 4;   // threads of a workgroup along a row (one wave) / rows of a workgroup

struct IngestArgs {
  const void* src;
  float* dst;
  int h, w, Hp, Wp;
  long long row_stride, plane_stride;   // bytes (8-bit formats) / floats (F32_CHW)
  int swap;                             // source is BGR
  int pad;                              // DVSR_FRAME_PAD_*
};

struct EmitArgs {
  const float* src;
  void* dst;
  int Hs, Ws, h, w;
  long long row_stride, plane_stride;
  int swap;
  float lo, hi;
};

__device__ __forceinline__ void store_planes(float* dst, long long plane, const f32x4 o[3], int swap) {
  *reinterpret_cast<f32x4*>(dst) = swap ? o[2] : o[0];
  *reinterpret_cast<f32x4*>(dst + plane) = o[1];
  *reinterpret_cast<f32x4*>(dst + 2 * plane) = swap ? o[0] : o[2];
}

template <int PS>
__global__ __launch_bounds__(FIO_X * FIO_Y) void frame_ingest_u8_kernel(IngestArgs a) {
  const int x0 = (blockIdx.x * FIO_X + threadIdx.x) * 4;
  const int y = blockIdx.y * FIO_Y + threadIdx.y;
  if (x0 >= a.Wp || y >= a.Hp) return;
  const unsigned char* row = static_cast<const unsigned char*>(a.src) + (long long)pad_index(y, a.h, a.pad) * a.row_stride;
  unsigned px[4][3];
  if (x0 + 3 < a.w) {
    // the lane's 4 pixels are bytes [p, p + NEED) (a fourth byte of the last pixel is not needed).  x0 * PS is a multiple of
    // 4, so the misalignment m is the row's: wave-uniform.  Only aligned dwords that hold at least one of those bytes are
    // read -- such a dword cannot reach into another page, whatever else it holds.
    constexpr int NEED = PS == 3 ? 12 : 15, NE = PS == 3 ? 3 : 4;
    const unsigned char* p = row + (long long)x0 * PS;
    const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
    const unsigned* q = reinterpret_cast<const unsigned*>(p - m);
    const int nd = (int)(m + NEED + 3) >> 2;
    unsigned d[NE + 1];
#pragma unroll
    for (int k = 0; k < NE + 1; ++k) d[k] = k < nd ? q[k] : 0u;
    unsigned e[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) e[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], m);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int j = i * PS + c;
        px[i][c] = (e[j >> 2] >> (8 * (j & 3))) & 0xffu;
      }
  } else {
    // padded columns / the ragged end of a row: each pixel's 3 bytes out of the one or two aligned dwords that hold them
    unsigned d0[4], d1[4], m[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned char* p = row + (long long)pad_index(x0 + i, a.w, a.pad) * PS;
      m[i] = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
      const unsigned* q = reinterpret_cast<const unsigned*>(p - m[i]);
      d0[i] = q[0];
      d1[i] = m[i] >= 2 ? q[1] : 0u;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned v = __builtin_amdgcn_alignbyte(d1[i], d0[i], m[i]);
#pragma unroll
      for (int c = 0; c < 3; ++c) px[i][c] = (v >> (8 * c)) & 0xffu;
    }
  }
  f32x4 o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) o[c][i] = (float)px[i][c] / 255.0f;   // IEEE division, as numpy's
  store_planes(a.dst + (long long)y * a.Wp + x0, (long long)a.Hp * a.Wp, o, a.swap);
}

__global__ __launch_bounds__(FIO_X * FIO_Y) void frame_ingest_f32_kernel(IngestArgs a) {
  const int x0 = (blockIdx.x * FIO_X + threadIdx.x) * 4;
  const int y = blockIdx.y * FIO_Y + threadIdx.y;
  if (x0 >= a.Wp || y >= a.Hp) return;
  const float* row = static_cast<const float*>(a.src) + (long long)pad_index(y, a.h, a.pad) * a.row_stride;
  f32x4 o[3];
  if (x0 + 3 < a.w) {
    const float* p = row + x0;
    // 16-byte loads where this row is 16-byte aligned in all three planes (x0 * 4 bytes is a multiple of 16: wave-uniform)
    const bool al = ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)(a.plane_stride * 4)) & 15) == 0;
    if (al) {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = *reinterpret_cast<const f32x4*>(p + c * a.plane_stride);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) o[c][i] = p[c * a.plane_stride + i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* p = row + pad_index(x0 + i, a.w, a.pad);
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c][i] = p[c * a.plane_stride];
    }
  }
  store_planes(a.dst + (long long)y * a.Wp + x0, (long long)a.Hp * a.Wp, o, 0);
}

template <bool U8>
__global__ __launch_bounds__(FIO_X * FIO_Y) void frame_emit_kernel(EmitArgs a) {
  const int x0 = (blockIdx.x * FIO_X + threadIdx.x) * 4;
  const int y = blockIdx.y * FIO_Y + threadIdx.y;
  if (x0 >= a.w || y >= a.h) return;
  const float* s = a.src + (long long)y * a.Ws + x0;   // x0 + 3 < Ws: Ws is a multiple of 4 and x0 < w <= Ws
  const long long plane = (long long)a.Hs * a.Ws;
  const f32x4 v0 = *reinterpret_cast<const f32x4*>(s), v1 = *reinterpret_cast<const f32x4*>(s + plane),
              v2 = *reinterpret_cast<const f32x4*>(s + 2 * plane);
  const bool whole = x0 + 3 < a.w;
  if (U8) {
    const f32x4 c0 = a.swap ? v2 : v0, c2 = a.swap ? v0 : v2;
    unsigned b[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      b[3 * i] = (unsigned)quant_u8(c0[i], a.lo, a.hi);
      b[3 * i + 1] = (unsigned)quant_u8(v1[i], a.lo, a.hi);
      b[3 * i + 2] = (unsigned)quant_u8(c2[i], a.lo, a.hi);
    }
    unsigned char* p = static_cast<unsigned char*>(a.dst) + (long long)y * a.row_stride + (long long)x0 * 3;
    if (whole) {
      // 12 bytes at p.  x0 * 3 is a multiple of 4, so m = p & 3 is the row's (wave-uniform).  m = 0: three dword stores; else
      // 4 - m bytes up to the next dword boundary, two dwords, the last m bytes -- every store naturally aligned.
      unsigned d[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) d[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
      const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
      if (m == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) reinterpret_cast<unsigned*>(p)[k] = d[k];
      } else {
        if (m & 1) *p = (unsigned char)d[0];
        if (m != 3) *reinterpret_cast<unsigned short*>(p + (m & 1)) = (unsigned short)(d[0] >> (8 * (m & 1)));
        unsigned char* q = p + (4 - m);
        reinterpret_cast<unsigned*>(q)[0] = __builtin_amdgcn_alignbyte(d[1], d[0], 4 - m);
        reinterpret_cast<unsigned*>(q)[1] = __builtin_amdgcn_alignbyte(d[2], d[1], 4 - m);
        const unsigned t = d[2] >> (8 * (4 - m));
        if (m >= 2) *reinterpret_cast<unsigned short*>(q + 8) = (unsigned short)t;
        if (m & 1) q[8 + (m & 2)] = (unsigned char)(t >> (8 * (m & 2)));
      }
    } else {
      // the ragged end of a row: single bytes (relaxed atomic stores are plain byte stores that are never merged into wider,
      // possibly misaligned ones)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (x0 + i < a.w) {
#pragma unroll
          for (int c = 0; c < 3; ++c)
            __hip_atomic_store(p + 3 * i + c, (unsigned char)b[3 * i + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
    }
  } else {
    float* p = static_cast<float*>(a.dst) + (long long)y * a.row_stride + x0;
    const bool al = ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)(a.plane_stride * 4)) & 15) == 0;
    if (whole && al) {
      *reinterpret_cast<f32x4*>(p) = v0;
      *reinterpret_cast<f32x4*>(p + a.plane_stride) = v1;
      *reinterpret_cast<f32x4*>(p + 2 * a.plane_stride) = v2;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (x0 + i < a.w) {
          p[i] = v0[i];
          p[a.plane_stride + i] = v1[i];
          p[2 * a.plane_stride + i] = v2[i];
        }
    }
  }
}

static bool is_u8(int format) { return format == DVSR_FRAME_U8_HWC_RGB || format == DVSR_FRAME_U8_HWC_BGR; }

// the frame on the "any address, any pitch" side, against the h x w it may have at most
int frame_desc_check(const char* what, const void* ptr, const dvsr_frame_desc* d, int Ht, int Wt, bool emit) {
  DVSR_REQUIRE(ptr && d, DVSR_ERR_INVALID, "%s: null frame / descriptor", what);
  DVSR_REQUIRE(d->format == DVSR_FRAME_F32_CHW || is_u8(d->format), DVSR_ERR_INVALID, "%s: unknown frame format %d", what,
               d->format);
  DVSR_REQUIRE(d->h >= 1 && d->w >= 1 && d->h <= Ht && d->w <= Wt, DVSR_ERR_INVALID,
               "%s: frame size h=%d w=%d outside [1, %d] x [1, %d]", what, d->h, d->w, Ht, Wt);
  if (is_u8(d->format)) {
    DVSR_REQUIRE(emit ? d->pixel_stride == 3 : (d->pixel_stride == 3 || d->pixel_stride == 4), DVSR_ERR_INVALID,
                 "%s: pixel stride %d (%s)", what, d->pixel_stride, emit ? "3" : "3 or 4");
    DVSR_REQUIRE(d->row_stride >= (long long)d->w * d->pixel_stride, DVSR_ERR_INVALID,
                 "%s: row stride %lld shorter than a row of %lld bytes", what, d->row_stride, (long long)d->w * d->pixel_stride);
  } else {
    DVSR_REQUIRE(d->row_stride >= d->w, DVSR_ERR_INVALID, "%s: row stride %lld shorter than a row of %d floats", what,
                 d->row_stride, d->w);
    DVSR_REQUIRE(d->plane_stride >= (long long)(d->h - 1) * d->row_stride + d->w, DVSR_ERR_INVALID,
                 "%s: plane stride %lld shorter than a plane of %d rows", what, d->plane_stride, d->h);
    DVSR_REQUIRE(reinterpret_cast<uintptr_t>(ptr) % 4 == 0, DVSR_ERR_INVALID, "%s: misaligned fp32 frame (4 bytes)", what);
  }
  return DVSR_OK;
}

int frame_ingest_check(const char* what, const void* src, const dvsr_frame_desc* sd, const float* dst, int Hp, int Wp,
                       int pad_mode) {
  int rc = frame_planar_check(what, dst, Hp, Wp, FIO_Y);
  if (rc != DVSR_OK) return rc;
  RgbFormat rgb;   // (frame_rgb.hip's formats have their own descriptor check; dvsr_frame_degrade / _imresize keep frame_desc_check alone)
  rc = sd && frame_rgb_format(sd->format, &rgb) ? frame_rgb_check(what, src, sd, Hp, Wp, false) : frame_desc_check(what, src, sd, Hp, Wp, false);
  if (rc != DVSR_OK) return rc;
  return frame_pad_check(what, pad_mode, sd->h, sd->w, Hp, Wp);
}

// (arguments checked by frame_ingest_check)
int frame_ingest_launch(const void* src, const dvsr_frame_desc& sd, float* dst, int Hp, int Wp, int pad_mode, hipStream_t st) {
  RgbFormat rgb;
  if (frame_rgb_format(sd.format, &rgb)) return frame_rgb_ingest_launch(src, sd, dst, Hp, Wp, pad_mode, st);
  IngestArgs a{src, dst, sd.h, sd.w, Hp, Wp, sd.row_stride, sd.plane_stride, sd.format == DVSR_FRAME_U8_HWC_BGR, pad_mode};
  const dim3 grid(ceil_div(Wp / 4, FIO_X), ceil_div(Hp, FIO_Y)), block(FIO_X, FIO_Y);
  if (!is_u8(sd.format)) hipLaunchKernelGGL(frame_ingest_f32_kernel, grid, block, 0, st, a);
  else if (sd.pixel_stride == 3) hipLaunchKernelGGL(frame_ingest_u8_kernel<3>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(frame_ingest_u8_kernel<4>, grid, block, 0, st, a);
  return check_launch("frame_ingest_kernel");
}

}  // namespace dvsr

using namespace dvsr;

extern "C" int dvsr_frame_ingest(const void* src, const dvsr_frame_desc* sd, float* dst, int Hp, int Wp, int pad_mode,
                                 dvsr_stream_t stream) {
  int rc = frame_ingest_check("frame_ingest", src, sd, dst, Hp, Wp, pad_mode);
  if (rc != DVSR_OK) return rc;
  return frame_ingest_launch(src, *sd, dst, Hp, Wp, pad_mode, (hipStream_t)stream);
}

extern "C" int dvsr_frame_emit(const float* src, int Hs, int Ws, void* dst, const dvsr_frame_desc* dd, float lo, float hi,
                               dvsr_stream_t stream) {
  int rc = frame_planar_check("frame_emit", src, Hs, Ws, FIO_Y);
  if (rc != DVSR_OK) return rc;
  RgbFormat rgb;
  if (dd && frame_rgb_format(dd->format, &rgb)) {
    rc = frame_rgb_check("frame_emit", dst, dd, Hs, Ws, true);
    if (rc != DVSR_OK) return rc;
    DVSR_REQUIRE(hi > lo, DVSR_ERR_INVALID, "frame_emit: range [%g, %g]", (double)lo, (double)hi);
    return frame_rgb_emit_launch(src, Hs, Ws, dst, *dd, lo, hi, (hipStream_t)stream);
  }
  rc = frame_desc_check("frame_emit", dst, dd, Hs, Ws, true);
  if (rc != DVSR_OK) return rc;
  DVSR_REQUIRE(!is_u8(dd->format) || hi > lo, DVSR_ERR_INVALID, "frame_emit: range [%g, %g]", (double)lo, (double)hi);
  EmitArgs a{src, dst, Hs, Ws, dd->h, dd->w, dd->row_stride, dd->plane_stride, dd->format == DVSR_FRAME_U8_HWC_BGR, lo, hi};
  const dim3 grid(ceil_div(ceil_div(dd->w, 4), FIO_X), ceil_div(dd->h, FIO_Y)), block(FIO_X, FIO_Y);
  if (is_u8(dd->format)) hipLaunchKernelGGL(frame_emit_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(frame_emit_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
  return check_launch("frame_emit_kernel");
}
