// 16-bit interleaved RGB / BGR and planar integer RGB / GBR frames in and out of the video path: the formats
// DVSR_FRAME_U16_HWC_RGB / _BGR, _U8_CHW_RGB / _GBR and _U16_CHW_RGB / _GBR of dvsr_frame_ingest / dvsr_frame_emit (frame_io.hip
// dispatches here; engine.hip's dvsr_edvr_stream_extract_frame follows through frame_ingest_launch), beside the 8-bit interleaved
// and fp32 planar frames of frame_io.hip.  DESIGN 3.2w.
//
// What 16-bit PNG / TIFF / DPX, torchvision's decoders and an FFV1 archive (gbrp, gbrp10le / 12le / 16le) hold: levels of d bits,
// d = 8 in a byte, d = 10, 12 or 16 in the LOW bits of a 16-bit little-endian word; top = 2^d - 1 is exact in fp32.
//   ingest   level = word & top; value = (float)level / (float)top, an IEEE division -- numpy's np.float32(level) /
//            np.float32(top), and at d = 8 the v / 255.0f of frame_io.hip.  GBR planes and BGR words go to R, G, B.  Rows and
//            columns beyond h x w are filled from the frame itself, on the source index (pad_index).
//   emit     level = quant_levels(v, lo, hi, top) of quant.h: clamp, rescale, x top, round half to even; the bits of a word above
//            the level are 0.  Nothing outside the rows of the crop is written.
// The kernels keep the shape of frame_io.hip and frame_yuv.hip: one thread = 4 consecutive pixels of a row in all three planes, a
// workgroup is 64 x 4 threads, so a wave works on ONE row and whatever depends on a row's address is wave-uniform.  The fp32 side
// moves as three 16-byte accesses.  On the sample side a lane's group -- 24 or 32 bytes of interleaved words, 4 or 8 bytes per
// plane -- moves in the widest naturally aligned pieces its address allows (frame_sample.h: ld_words / st_words12, S::ld4 /
// S::st4); the offset of a lane's group inside its row is a multiple of 8 bytes (of the group, for a plane), so the choice of
// pieces is the row's -- and, for planar frames, the plane's, as plane strides are arbitrary.  No access is wider than its
// address is aligned or narrower than a sample.  Lanes that hold padded columns or the ragged end of a row work sample by
// sample.  Pure streaming: all of a lane's loads come ahead of its first store, no grid-stride loop.
#include <cstdint>

#include "frame_common.h"
#include "frame_sample.h"
#include "quant.h"

namespace dvsr {

constexpr int RGB_X = 64, RGB_Y = 4;   // threads of a workgroup along a row (one wave) / rows of a workgroup

struct RgbIngestArgs {
  const unsigned char* src;
  float* dst;
  int h, w, Hp, Wp;
  long long row_stride;               // bytes
  long long po[3];                    // planar: the byte offsets of the R, G and B plane
  int swap;                           // interleaved: the words of a pixel are B, G, R
  int pad;                            // DVSR_FRAME_PAD_*
  unsigned mask;                      // planar words: level = word & mask
  float top;
};

struct RgbEmitArgs {
  const float* src;
  unsigned char* dst;
  int Hs, Ws, h, w;
  long long row_stride;
  long long po[3];
  int swap;
  float lo, hi, top;
};

__device__ __forceinline__ void store_rgb(float* dst, long long plane, const f32x4& r, const f32x4& g, const f32x4& b) {
  *reinterpret_cast<f32x4*>(dst) = r;
  *reinterpret_cast<f32x4*>(dst + plane) = g;
  *reinterpret_cast<f32x4*>(dst + 2 * plane) = b;
}

// interleaved words, PSW = 3 or 4 words per pixel
template <int PSW>
__global__ __launch_bounds__(RGB_X * RGB_Y) void frame_ingest_hwc16_kernel(RgbIngestArgs a) {
  const int x0 = (blockIdx.x * RGB_X + threadIdx.x) * 4;
  const int y = blockIdx.y * RGB_Y + threadIdx.y;
  if (x0 >= a.Wp || y >= a.Hp) return;
  const unsigned char* row = a.src + (long long)pad_index(y, a.h, a.pad) * a.row_stride;
  unsigned px[4][3];
  if (x0 + 3 < a.w) {
    // the lane's group starts 8 x0 PSW / 4 bytes into the row, a multiple of 8: its pieces are the row's (wave-uniform)
    unsigned d[2 * PSW];
    ld_words<4 * PSW>(row + (long long)x0 * (2 * PSW), d);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) px[i][c] = word_of(d, i * PSW + c);
  } else {
    // padded columns / the ragged end of a row: word by word
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned char* p = row + (long long)pad_index(x0 + i, a.w, a.pad) * (2 * PSW);
#pragma unroll
      for (int c = 0; c < 3; ++c) px[i][c] = Words16::ld1(p + 2 * c);
    }
  }
  f32x4 o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) o[c][i] = (float)px[i][c] / 65535.0f;   // IEEE division, as numpy's
  store_rgb(a.dst + (long long)y * a.Wp + x0, (long long)a.Hp * a.Wp, a.swap ? o[2] : o[0], o[1], a.swap ? o[0] : o[2]);
}

// three planes of samples S (Bytes8 / Words16)
template <class S>
__global__ __launch_bounds__(RGB_X * RGB_Y) void frame_ingest_chw_kernel(RgbIngestArgs a) {
  const int x0 = (blockIdx.x * RGB_X + threadIdx.x) * 4;
  const int y = blockIdx.y * RGB_Y + threadIdx.y;
  if (x0 >= a.Wp || y >= a.Hp) return;
  const long long row = (long long)pad_index(y, a.h, a.pad) * a.row_stride;
  unsigned v[3][4];
  if (x0 + 3 < a.w) {
    // a lane's group of a plane starts 4 x0 samples into its row, a multiple of the group: the pieces are the plane's row's
    typename S::G4 g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = S::ld4(a.src + a.po[c] + row + (long long)x0 * S::B);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) v[c][i] = S::raw(g[c], i);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long off = row + (long long)pad_index(x0 + i, a.w, a.pad) * S::B;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c][i] = S::ld1(a.src + a.po[c] + off);
    }
  }
  // (bytes: a literal divisor and no mask, the v / 255.0f of frame_io.hip)
  const float top = S::B == 1 ? 255.0f : a.top;
  const unsigned mask = S::B == 1 ? 0xffu : a.mask;
  f32x4 o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) o[c][i] = (float)(v[c][i] & mask) / top;   // IEEE division
  store_rgb(a.dst + (long long)y * a.Wp + x0, (long long)a.Hp * a.Wp, o[0], o[1], o[2]);
}

__global__ __launch_bounds__(RGB_X * RGB_Y) void frame_emit_hwc16_kernel(RgbEmitArgs a) {
  const int x0 = (blockIdx.x * RGB_X + threadIdx.x) * 4;
  const int y = blockIdx.y * RGB_Y + threadIdx.y;
  if (x0 >= a.w || y >= a.h) return;
  const float* s = a.src + (long long)y * a.Ws + x0;   // x0 + 3 < Ws: Ws is a multiple of 4 and x0 < w <= Ws
  const long long plane = (long long)a.Hs * a.Ws;
  const f32x4 v0 = *reinterpret_cast<const f32x4*>(s), v1 = *reinterpret_cast<const f32x4*>(s + plane),
              v2 = *reinterpret_cast<const f32x4*>(s + 2 * plane);
  const f32x4 c0 = a.swap ? v2 : v0, c2 = a.swap ? v0 : v2;
  unsigned b[12];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    b[3 * i] = (unsigned)quant_levels(c0[i], a.lo, a.hi, 65535.0f);
    b[3 * i + 1] = (unsigned)quant_levels(v1[i], a.lo, a.hi, 65535.0f);
    b[3 * i + 2] = (unsigned)quant_levels(c2[i], a.lo, a.hi, 65535.0f);
  }
  unsigned char* p = a.dst + (long long)y * a.row_stride + (long long)x0 * 6;   // 24 bytes a lane: p & 7 is the row's
  if (x0 + 3 < a.w) {
    unsigned d[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = b[2 * k] | (b[2 * k + 1] << 16);
    st_words12(p, d);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x0 + i < a.w) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Words16::st1(p + 6 * i + 2 * c, b[3 * i + c]);
      }
  }
}

template <class S>
__global__ __launch_bounds__(RGB_X * RGB_Y) void frame_emit_chw_kernel(RgbEmitArgs a) {
  const int x0 = (blockIdx.x * RGB_X + threadIdx.x) * 4;
  const int y = blockIdx.y * RGB_Y + threadIdx.y;
  if (x0 >= a.w || y >= a.h) return;
  const float* s = a.src + (long long)y * a.Ws + x0;
  const long long plane = (long long)a.Hs * a.Ws;
  const f32x4 v[3] = {*reinterpret_cast<const f32x4*>(s), *reinterpret_cast<const f32x4*>(s + plane),
                      *reinterpret_cast<const f32x4*>(s + 2 * plane)};
  const float top = S::B == 1 ? 255.0f : a.top;
  unsigned l[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) l[c][i] = (unsigned)quant_levels(v[c][i], a.lo, a.hi, top);
  const long long off = (long long)y * a.row_stride + (long long)x0 * S::B;
  if (x0 + 3 < a.w) {
#pragma unroll
    for (int c = 0; c < 3; ++c) S::st4(a.dst + a.po[c] + off, l[c]);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (x0 + i < a.w) S::st1(a.dst + a.po[c] + off + i * S::B, l[c][i]);
  }
}

bool frame_rgb_format(int format, RgbFormat* f) {
  const int base = format & 0xff, field = (format >> 8) & 15;
  if (format < 0 || (format >> 12) != 0 || base < DVSR_FRAME_U16_HWC_RGB || base > DVSR_FRAME_U16_CHW_GBR) return false;
  f->planar = base >= DVSR_FRAME_U8_CHW_RGB;
  f->reorder = base == DVSR_FRAME_U16_HWC_BGR || base == DVSR_FRAME_U8_CHW_GBR || base == DVSR_FRAME_U16_CHW_GBR;
  f->bytes = (base == DVSR_FRAME_U8_CHW_RGB || base == DVSR_FRAME_U8_CHW_GBR) ? 1 : 2;
  if (f->bytes == 1) f->depth = field == 0 ? 8 : 0;
  else if (!f->planar) f->depth = field == 0 ? 16 : 0;
  else f->depth = field == 0 ? 16 : ((field == 10 || field == 12) ? field : 0);
  return true;
}

int frame_rgb_check(const char* what, const void* ptr, const dvsr_frame_desc* d, int Ht, int Wt, bool emit) {
  DVSR_REQUIRE(ptr && d, DVSR_ERR_INVALID, "%s: null frame / descriptor", what);
  RgbFormat f;
  DVSR_REQUIRE(frame_rgb_format(d->format, &f), DVSR_ERR_INVALID, "%s: unknown frame format %d", what, d->format);
  DVSR_REQUIRE(f.depth != 0, DVSR_ERR_INVALID, "%s: unknown depth %d of frame format %d (%s)", what, (d->format >> 8) & 15,
               d->format & 0xff, f.bytes == 1 ? "bytes: 8 alone" : (f.planar ? "10, 12 or 16" : "interleaved words: 16 alone"));
  DVSR_REQUIRE(d->h >= 1 && d->w >= 1 && d->h <= Ht && d->w <= Wt, DVSR_ERR_INVALID,
               "%s: frame size h=%d w=%d outside [1, %d] x [1, %d]", what, d->h, d->w, Ht, Wt);
  if (f.bytes == 2)
    DVSR_REQUIRE(reinterpret_cast<uintptr_t>(ptr) % 2 == 0 && d->row_stride % 2 == 0 && (!f.planar || d->plane_stride % 2 == 0),
                 DVSR_ERR_INVALID, "%s: odd address or stride (row %lld, plane %lld) of a frame of 16-bit words", what, d->row_stride,
                 f.planar ? d->plane_stride : 0ll);
  if (f.planar) {
    DVSR_REQUIRE(d->pixel_stride == f.bytes, DVSR_ERR_INVALID, "%s: pixel stride %d of a plane of %d-byte samples (%d)", what,
                 d->pixel_stride, f.bytes, f.bytes);
    DVSR_REQUIRE(d->row_stride >= (long long)d->w * f.bytes, DVSR_ERR_INVALID, "%s: row stride %lld shorter than a row of %lld bytes",
                 what, d->row_stride, (long long)d->w * f.bytes);
    DVSR_REQUIRE(d->plane_stride >= (long long)(d->h - 1) * d->row_stride + (long long)d->w * f.bytes, DVSR_ERR_INVALID,
                 "%s: plane stride %lld shorter than a plane of %d rows", what, d->plane_stride, d->h);
  } else {
    DVSR_REQUIRE(emit ? d->pixel_stride == 6 : (d->pixel_stride == 6 || d->pixel_stride == 8), DVSR_ERR_INVALID,
                 "%s: pixel stride %d of interleaved 16-bit words (%s bytes)", what, d->pixel_stride, emit ? "6" : "6 or 8");
    DVSR_REQUIRE(d->row_stride >= (long long)d->w * d->pixel_stride, DVSR_ERR_INVALID,
                 "%s: row stride %lld shorter than a row of %lld bytes", what, d->row_stride, (long long)d->w * d->pixel_stride);
  }
  return DVSR_OK;
}

// the byte offsets of the R, G and B plane: planes in the order R, G, B, or G, B, R
static void plane_offsets(const RgbFormat& f, long long plane_stride, long long po[3]) {
  po[0] = f.reorder ? 2 * plane_stride : 0;
  po[1] = f.reorder ? 0 : plane_stride;
  po[2] = f.reorder ? plane_stride : 2 * plane_stride;
}

// (arguments checked by frame_ingest_check)
int frame_rgb_ingest_launch(const void* src, const dvsr_frame_desc& sd, float* dst, int Hp, int Wp, int pad_mode, hipStream_t st) {
  RgbFormat f;
  frame_rgb_format(sd.format, &f);
  RgbIngestArgs a{static_cast<const unsigned char*>(src), dst, sd.h, sd.w, Hp, Wp, sd.row_stride, {0, 0, 0}, f.reorder, pad_mode,
                  (1u << f.depth) - 1u, (float)((1u << f.depth) - 1u)};
  if (f.planar) plane_offsets(f, sd.plane_stride, a.po);
  const dim3 grid(ceil_div(Wp / 4, RGB_X), ceil_div(Hp, RGB_Y)), block(RGB_X, RGB_Y);
  if (!f.planar) {
    if (sd.pixel_stride == 6) hipLaunchKernelGGL(frame_ingest_hwc16_kernel<3>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(frame_ingest_hwc16_kernel<4>, grid, block, 0, st, a);
  } else if (f.bytes == 1) {
    hipLaunchKernelGGL(frame_ingest_chw_kernel<Bytes8>, grid, block, 0, st, a);
  } else {
    hipLaunchKernelGGL(frame_ingest_chw_kernel<Words16>, grid, block, 0, st, a);
  }
  return check_launch("frame_ingest_rgb_kernel");
}

// (arguments checked by dvsr_frame_emit)
int frame_rgb_emit_launch(const float* src, int Hs, int Ws, void* dst, const dvsr_frame_desc& dd, float lo, float hi, hipStream_t st) {
  RgbFormat f;
  frame_rgb_format(dd.format, &f);
  RgbEmitArgs a{src, static_cast<unsigned char*>(dst), Hs, Ws, dd.h, dd.w, dd.row_stride, {0, 0, 0}, f.reorder, lo, hi,
                (float)((1u << f.depth) - 1u)};
  if (f.planar) plane_offsets(f, dd.plane_stride, a.po);
  const dim3 grid(ceil_div(ceil_div(dd.w, 4), RGB_X), ceil_div(dd.h, RGB_Y)), block(RGB_X, RGB_Y);
  if (!f.planar) hipLaunchKernelGGL(frame_emit_hwc16_kernel, grid, block, 0, st, a);
  else if (f.bytes == 1) hipLaunchKernelGGL(frame_emit_chw_kernel<Bytes8>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(frame_emit_chw_kernel<Words16>, grid, block, 0, st, a);
  return check_launch("frame_emit_rgb_kernel");
}

}  // namespace dvsr
