// Scene cuts found on the device (dvsr_frame_luma_sad; frames.py: luma_sad / scene_scores / detect_cuts).
//
// A hard cut shows as a jump of the mean absolute luma difference between consecutive frames.  As torch ops on decoder bytes
// that is a widening copy, a permute, the luma, a subtraction, an absolute value and a sum per pair, with several times the
// frame in temporaries; here one pass reads every byte of both frames once:
//   luma of a pixel, an 8-bit integer
//     Y plane (NV12 / I420)     the byte itself
//     16-bit Y plane            the top 8 bits of the level: word >> 8 (P010 / P012), (word & 1023) >> 2 (yuv420p10le),
//                               (word & 4095) >> 4 (yuv420p12le) -- scores mean what they mean for 8-bit video
//     8-bit RGB / BGR (3 | 4 B) Y8 = (77 R + 150 G + 29 B + 128) >> 8
//     fp32 planar               the same formula on quant_u8(v, 0, 1) of each channel (quant.h: the library's one quantiser)
//     16-bit RGB / BGR words,   the same formula on the top 8 bits of each level: word >> 8 (interleaved, 3 | 4 words a pixel),
//     integer RGB / GBR planes  (word & (2^d - 1)) >> (d - 8) or the byte itself (planes; frame_rgb.hip's formats)
//   sad[pair] = sum over the h x w frame of |Y8_b(p) - Y8_a(p)|, an exact unsigned 64-bit integer: integer sums are
//   associative, so the result does not depend on the order in which lanes, waves and workgroups add.
// One thread = 4 consecutive pixels (Y plane: 16; 16-bit Y plane: 8) of a row of BOTH frames, in SAD_ROWS rows; a workgroup is 64 x 4 threads, so a
// wave works on one row at a time and a row's misalignment is wave-uniform.  The byte side follows frame_io.hip: a row that
// starts on a dword boundary moves as dwords, any other is assembled from the aligned dwords around it (v_alignbyte_b32) -- no load is wider than its
// address is aligned and only aligned dwords that hold a needed byte are read; the ragged end of a row goes pixel by pixel.
// Four lumas are packed into a dword and differenced by v_sad_u8.  The per-lane sum (<= 8 x 16 x 255) is reduced over the wave
// by shuffles and over the 4 waves through the LDS as 32-bit (<= 32768 x 255 per workgroup); the workgroup ends with ONE 64-bit
// vector atomic add into sad[pair].  grid.z is the pair; no grid-stride loop -- a workgroup's rows are a fixed, unrolled count.
// Why 8 rows per wave: the adds of a launch land on one cache line (8 sums of 8 bytes) and go through one after the other, at
// about 12 ns each as measured; with one row per wave a 1080 x 1920 RGB pair ended in 2160 of them, 26 us against 3 us of
// reading.  Eight rows make it 272.
#include <cstdint>
#include <type_traits>

#include "common.h"
#include "frame_sample.h"
#include "kernels.h"
#include "quant.h"

namespace dvsr {

constexpr int SAD_X = 64, SAD_Y = 4;   // threads of a workgroup along a row (one wave) / rows of a workgroup at a time
constexpr int SAD_ROWS = 8;            // rows of a wave: a workgroup covers SAD_Y * SAD_ROWS rows
enum : int { SAD_F32 = 0, SAD_YPLANE = 1, SAD_HWC3 = 3, SAD_HWC4 = 4, SAD_Y16_MSB = 5, SAD_Y16_10 = 6, SAD_Y16_12 = 7,
             SAD_HWC16_3 = 8, SAD_HWC16_4 = 9, SAD_CHW8 = 10, SAD_CHW16 = 11 };   // frame_rgb.hip's formats: 4 pixels a thread

struct SadArgs {
  const void* a;
  const void* b;
  unsigned long long* sad;
  int h, w;
  long long row_stride, plane_stride, frame_stride;   // bytes (8-bit formats) / floats (F32_CHW)
  int swap;                                           // BGR
  long long po[3];                                    // planar integer RGB / GBR: the byte offsets of the R, G and B plane
  unsigned mask;                                      // ... and of its words: level = word & mask, luma from level >> shift
  int shift;
};

__device__ __forceinline__ unsigned luma8(unsigned r, unsigned g, unsigned b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// the lumas of pixels x0 .. x0 + 3 of an interleaved row, one per byte of the result (0 for a pixel beyond w)
template <int PS>
__device__ __forceinline__ unsigned luma4_hwc(const unsigned char* row, int x0, int w, int swap) {
  unsigned px[4][3];
  if (x0 + 3 < w) {
    // bytes [p, p + NEED); x0 * PS is a multiple of 4, so the misalignment m is the row's (frame_io.hip: frame_ingest_u8_kernel)
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
    // the ragged end of a row: each pixel's 3 bytes out of the one or two aligned dwords that hold them
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned v = 0;
      if (x0 + i < w) {
        const unsigned char* p = row + (long long)(x0 + i) * PS;
        const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
        const unsigned* q = reinterpret_cast<const unsigned*>(p - m);
        const unsigned d0 = q[0], d1 = m >= 2 ? q[1] : 0u;
        v = __builtin_amdgcn_alignbyte(d1, d0, m);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) px[i][c] = (v >> (8 * c)) & 0xffu;
    }
  }
  unsigned y4 = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) y4 |= luma8(swap ? px[i][2] : px[i][0], px[i][1], swap ? px[i][0] : px[i][2]) << (8 * i);
  return y4;
}

// bytes x0 .. x0 + 15 of a Y row as four dwords (0 for a byte beyond w)
__device__ __forceinline__ void luma16_plane(const unsigned char* row, int x0, int w, unsigned e[4]) {
  if (x0 + 15 < w) {
    const unsigned char* p = row + x0;                 // x0 is a multiple of 16: m is the row's
    const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
    const unsigned* q = reinterpret_cast<const unsigned*>(p - m);
    unsigned d[5];
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = q[k];
    d[4] = m ? q[4] : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], m);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (x0 + i < w) e[i >> 2] |= (unsigned)row[x0 + i] << (8 * (i & 3));   // (a byte load is always aligned)
  }
}

// the top 8 bits of the levels of the two 16-bit words of a dword, in bytes 0 and 1 of the result
template <int KIND>
__device__ __forceinline__ unsigned luma2_w16(unsigned v) {
  constexpr unsigned MASK = KIND == SAD_Y16_MSB ? 0xffffu : (KIND == SAD_Y16_10 ? 1023u : 4095u);
  constexpr int SH = KIND == SAD_Y16_MSB ? 8 : (KIND == SAD_Y16_10 ? 2 : 4);
  return (((v & 0xffffu) & MASK) >> SH) | ((((v >> 16) & MASK) >> SH) << 8);
}

// words x0 .. x0 + 7 of a 16-bit Y row (2-byte aligned) as the two dwords of their lumas (0 for a word beyond w)
template <int KIND>
__device__ __forceinline__ void luma8_plane16(const unsigned char* row, int x0, int w, unsigned e[2]) {
  unsigned d4[4];
  if (x0 + 7 < w) {
    const unsigned char* p = row + 2 * (long long)x0;  // x0 * 2 is a multiple of 16: m (0 or 2) is the row's
    const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
    const unsigned* q = reinterpret_cast<const unsigned*>(p - m);
    unsigned d[5];
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = q[k];
    d[4] = m ? q[4] : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) d4[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], m);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) d4[k] = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (x0 + i < w) d4[i >> 1] |= (unsigned)reinterpret_cast<const unsigned short*>(row)[x0 + i] << (16 * (i & 1));
  }
  e[0] = luma2_w16<KIND>(d4[0]) | (luma2_w16<KIND>(d4[1]) << 16);
  e[1] = luma2_w16<KIND>(d4[2]) | (luma2_w16<KIND>(d4[3]) << 16);
}

// the lumas of pixels x0 .. x0 + 3 of a row of interleaved 16-bit words (PSW = 3 | 4 words a pixel), from the top 8 bits of
// each level, one per byte (0 for a pixel beyond w); the group moves as in frame_rgb.hip (frame_sample.h: ld_words)
template <int PSW>
__device__ __forceinline__ unsigned luma4_hwc16(const unsigned char* row, int x0, int w, int swap) {
  unsigned px[4][3];
  if (x0 + 3 < w) {
    unsigned d[2 * PSW];
    ld_words<4 * PSW>(row + (long long)x0 * (2 * PSW), d);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) px[i][c] = word_of(d, i * PSW + c) >> 8;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        px[i][c] = x0 + i < w ? Words16::ld1(row + (long long)(x0 + i) * (2 * PSW) + 2 * c) >> 8 : 0u;
  }
  unsigned y4 = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) y4 |= luma8(swap ? px[i][2] : px[i][0], px[i][1], swap ? px[i][0] : px[i][2]) << (8 * i);
  return y4;
}

// the same of three planes of samples S (Bytes8 / Words16) whose rows start at row + po[c]: (level & mask) >> shift
template <class S>
__device__ __forceinline__ unsigned luma4_chw(const unsigned char* row, const long long po[3], int x0, int w, unsigned mask, int shift) {
  unsigned v[3][4];
  if (x0 + 3 < w) {
    typename S::G4 g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = S::ld4(row + po[c] + (long long)x0 * S::B);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) v[c][i] = S::raw(g[c], i);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) v[c][i] = x0 + i < w ? S::ld1(row + po[c] + (long long)(x0 + i) * S::B) : 0u;
  }
  unsigned y4 = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) y4 |= luma8((v[0][i] & mask) >> shift, (v[1][i] & mask) >> shift, (v[2][i] & mask) >> shift) << (8 * i);
  return y4;
}

// the lumas of pixels x0 .. x0 + 3 of an fp32 planar row, one per byte (0 for a pixel beyond w)
__device__ __forceinline__ unsigned luma4_f32(const float* row, long long plane, int x0, int w) {
  float v[3][4];
  if (x0 + 3 < w) {
    const float* p = row + x0;
    // 16-byte loads where this row is 16-byte aligned in all three planes (x0 * 4 bytes is a multiple of 16: wave-uniform)
    const bool al = ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)(plane * 4)) & 15) == 0;
    if (al) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p + c * plane);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[c][i] = t[i];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) v[c][i] = p[c * plane + i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c][i] = x0 + i < w ? row[c * plane + x0 + i] : 0.f;
  }
  unsigned y4 = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    y4 |= luma8((unsigned)quant_u8(v[0][i], 0.f, 1.f), (unsigned)quant_u8(v[1][i], 0.f, 1.f), (unsigned)quant_u8(v[2][i], 0.f, 1.f))
          << (8 * i);
  return y4;
}

template <int KIND>
__global__ __launch_bounds__(SAD_X * SAD_Y) void frame_luma_sad_kernel(SadArgs a) {
  constexpr bool Y16 = KIND == SAD_Y16_MSB || KIND == SAD_Y16_10 || KIND == SAD_Y16_12;
  constexpr int PX = KIND == SAD_YPLANE ? 16 : (Y16 ? 8 : 4);
  const int x0 = (blockIdx.x * SAD_X + threadIdx.x) * PX;
  unsigned s = 0;
#pragma unroll
  for (int r = 0; r < SAD_ROWS; ++r) {
    const int y = (blockIdx.y * SAD_ROWS + r) * SAD_Y + threadIdx.y;   // (the workgroup reads SAD_Y neighbouring rows at a time)
    if (x0 >= a.w || y >= a.h) continue;
    const long long off = (long long)blockIdx.z * a.frame_stride + (long long)y * a.row_stride;
    if constexpr (KIND == SAD_F32) {
      const unsigned ya = luma4_f32(static_cast<const float*>(a.a) + off, a.plane_stride, x0, a.w);
      const unsigned yb = luma4_f32(static_cast<const float*>(a.b) + off, a.plane_stride, x0, a.w);
      s = __builtin_amdgcn_sad_u8(ya, yb, s);
    } else if constexpr (KIND == SAD_YPLANE) {
      unsigned ea[4], eb[4];
      luma16_plane(static_cast<const unsigned char*>(a.a) + off, x0, a.w, ea);
      luma16_plane(static_cast<const unsigned char*>(a.b) + off, x0, a.w, eb);
#pragma unroll
      for (int k = 0; k < 4; ++k) s = __builtin_amdgcn_sad_u8(ea[k], eb[k], s);
    } else if constexpr (Y16) {
      unsigned ea[2], eb[2];
      luma8_plane16<KIND>(static_cast<const unsigned char*>(a.a) + off, x0, a.w, ea);
      luma8_plane16<KIND>(static_cast<const unsigned char*>(a.b) + off, x0, a.w, eb);
#pragma unroll
      for (int k = 0; k < 2; ++k) s = __builtin_amdgcn_sad_u8(ea[k], eb[k], s);
    } else if constexpr (KIND == SAD_HWC16_3 || KIND == SAD_HWC16_4) {
      constexpr int PSW = KIND == SAD_HWC16_3 ? 3 : 4;
      const unsigned ya = luma4_hwc16<PSW>(static_cast<const unsigned char*>(a.a) + off, x0, a.w, a.swap);
      const unsigned yb = luma4_hwc16<PSW>(static_cast<const unsigned char*>(a.b) + off, x0, a.w, a.swap);
      s = __builtin_amdgcn_sad_u8(ya, yb, s);
    } else if constexpr (KIND == SAD_CHW8 || KIND == SAD_CHW16) {
      using S = typename std::conditional<KIND == SAD_CHW8, Bytes8, Words16>::type;
      const unsigned ya = luma4_chw<S>(static_cast<const unsigned char*>(a.a) + off, a.po, x0, a.w, a.mask, a.shift);
      const unsigned yb = luma4_chw<S>(static_cast<const unsigned char*>(a.b) + off, a.po, x0, a.w, a.mask, a.shift);
      s = __builtin_amdgcn_sad_u8(ya, yb, s);
    } else {
      const unsigned ya = luma4_hwc<KIND>(static_cast<const unsigned char*>(a.a) + off, x0, a.w, a.swap);
      const unsigned yb = luma4_hwc<KIND>(static_cast<const unsigned char*>(a.b) + off, x0, a.w, a.swap);
      s = __builtin_amdgcn_sad_u8(ya, yb, s);
    }
  }
  // every thread arrives here: the wave, then the workgroup's four waves through the LDS, then one 64-bit add
#pragma unroll
  for (int o = 32; o; o >>= 1) s += __shfl_down(s, o);
  __shared__ unsigned part[SAD_Y];
  if (threadIdx.x == 0) part[threadIdx.y] = s;
  __syncthreads();
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    unsigned long long t = 0;
#pragma unroll
    for (int k = 0; k < SAD_Y; ++k) t += part[k];
    if (t) atomicAdd(a.sad + blockIdx.z, t);
  }
}

}  // namespace dvsr

using namespace dvsr;

extern "C" int dvsr_frame_luma_sad(const void* a, const void* b, const dvsr_frame_desc* d, long long frame_stride, int pairs,
                                   unsigned long long* sad, dvsr_stream_t stream) {
  DVSR_REQUIRE(a && b && d && sad, DVSR_ERR_INVALID, "frame_luma_sad: null frame / descriptor / result");
  const bool y16 = d->format == DVSR_FRAME_U16_Y_MSB || d->format == DVSR_FRAME_U16_Y_10 || d->format == DVSR_FRAME_U16_Y_12;
  RgbFormat rgb;
  const bool is_rgb = frame_rgb_format(d->format, &rgb);   // frame_rgb.hip's formats
  DVSR_REQUIRE(d->format == DVSR_FRAME_F32_CHW || d->format == DVSR_FRAME_U8_HWC_RGB || d->format == DVSR_FRAME_U8_HWC_BGR ||
                   d->format == DVSR_FRAME_U8_Y || y16 || is_rgb,
               DVSR_ERR_INVALID, "frame_luma_sad: unknown frame format %d", d->format);
  DVSR_REQUIRE(d->h >= 1 && d->w >= 1 && d->h <= (1 << 20) && d->w <= (1 << 24), DVSR_ERR_INVALID,
               "frame_luma_sad: frame size h=%d w=%d outside [1, %d] x [1, %d]", d->h, d->w, 1 << 20, 1 << 24);
  DVSR_REQUIRE(pairs >= 1, DVSR_ERR_INVALID, "frame_luma_sad: pairs=%d must be positive", pairs);
  DVSR_REQUIRE(reinterpret_cast<uintptr_t>(sad) % 8 == 0, DVSR_ERR_INVALID, "frame_luma_sad: misaligned result (8 bytes)");
  int kind;
  long long po[3] = {0, 0, 0};
  if (is_rgb) {
    int rc = frame_rgb_check("frame_luma_sad", a, d, d->h, d->w, false);
    if (rc == DVSR_OK) rc = frame_rgb_check("frame_luma_sad", b, d, d->h, d->w, false);
    if (rc != DVSR_OK) return rc;
    DVSR_REQUIRE(rgb.bytes == 1 || frame_stride % 2 == 0, DVSR_ERR_INVALID, "frame_luma_sad: odd frame stride %lld of 16-bit words",
                 frame_stride);
    kind = rgb.planar ? (rgb.bytes == 1 ? SAD_CHW8 : SAD_CHW16) : (d->pixel_stride == 6 ? SAD_HWC16_3 : SAD_HWC16_4);
    if (rgb.planar) {
      po[0] = rgb.reorder ? 2 * d->plane_stride : 0;
      po[1] = rgb.reorder ? 0 : d->plane_stride;
      po[2] = rgb.reorder ? d->plane_stride : 2 * d->plane_stride;
    }
  } else if (d->format == DVSR_FRAME_F32_CHW) {
    kind = SAD_F32;
    DVSR_REQUIRE(d->row_stride >= d->w, DVSR_ERR_INVALID, "frame_luma_sad: row stride %lld shorter than a row of %d floats",
                 d->row_stride, d->w);
    DVSR_REQUIRE(d->plane_stride >= (long long)(d->h - 1) * d->row_stride + d->w, DVSR_ERR_INVALID,
                 "frame_luma_sad: plane stride %lld shorter than a plane of %d rows", d->plane_stride, d->h);
    DVSR_REQUIRE(reinterpret_cast<uintptr_t>(a) % 4 == 0 && reinterpret_cast<uintptr_t>(b) % 4 == 0, DVSR_ERR_INVALID,
                 "frame_luma_sad: misaligned fp32 frame (4 bytes)");
  } else {
    if (d->format == DVSR_FRAME_U8_Y) {
      DVSR_REQUIRE(d->pixel_stride == 1, DVSR_ERR_INVALID, "frame_luma_sad: pixel stride %d of a Y plane (1)", d->pixel_stride);
      kind = SAD_YPLANE;
    } else if (y16) {
      DVSR_REQUIRE(d->pixel_stride == 2, DVSR_ERR_INVALID, "frame_luma_sad: pixel stride %d of a 16-bit Y plane (2)",
                   d->pixel_stride);
      DVSR_REQUIRE(reinterpret_cast<uintptr_t>(a) % 2 == 0 && reinterpret_cast<uintptr_t>(b) % 2 == 0, DVSR_ERR_INVALID,
                   "frame_luma_sad: odd address of a 16-bit Y plane");
      DVSR_REQUIRE(d->row_stride % 2 == 0 && frame_stride % 2 == 0, DVSR_ERR_INVALID,
                   "frame_luma_sad: odd row stride %lld / frame stride %lld of a 16-bit Y plane", d->row_stride, frame_stride);
      kind = d->format == DVSR_FRAME_U16_Y_MSB ? SAD_Y16_MSB : (d->format == DVSR_FRAME_U16_Y_10 ? SAD_Y16_10 : SAD_Y16_12);
    } else {
      DVSR_REQUIRE(d->pixel_stride == 3 || d->pixel_stride == 4, DVSR_ERR_INVALID, "frame_luma_sad: pixel stride %d (3 or 4)",
                   d->pixel_stride);
      kind = d->pixel_stride;
    }
    DVSR_REQUIRE(d->row_stride >= (long long)d->w * d->pixel_stride, DVSR_ERR_INVALID,
                 "frame_luma_sad: row stride %lld shorter than a row of %lld bytes", d->row_stride,
                 (long long)d->w * d->pixel_stride);
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(sad, 0, (size_t)pairs * sizeof(unsigned long long), st) != hipSuccess) {
    (void)hipGetLastError();
    set_error("frame_luma_sad: hipMemsetAsync of %d sums failed", pairs);
    return DVSR_ERR_HIP;
  }
  const long long unit = kind == SAD_F32 ? 4 : 1;
  const int per_thread = kind == SAD_YPLANE ? 16 : (y16 ? 8 : 4);
  const dim3 block(SAD_X, SAD_Y);
  for (int first = 0; first < pairs; first += 65535) {               // grid.z is the pair: at most 65535 per launch
    const int n = pairs - first < 65535 ? pairs - first : 65535;
    const long long skip = (long long)first * frame_stride * unit;
    SadArgs args{static_cast<const char*>(a) + skip, static_cast<const char*>(b) + skip, sad + first, d->h, d->w,
                 d->row_stride, d->plane_stride, frame_stride,
                 d->format == DVSR_FRAME_U8_HWC_BGR || (is_rgb && !rgb.planar && rgb.reorder), {po[0], po[1], po[2]},
                 is_rgb ? (1u << rgb.depth) - 1u : 0u, is_rgb ? rgb.depth - 8 : 0};
    const dim3 grid(ceil_div(ceil_div(d->w, per_thread), SAD_X), ceil_div(d->h, SAD_Y * SAD_ROWS), n);
    switch (kind) {
      case SAD_F32: hipLaunchKernelGGL(frame_luma_sad_kernel<SAD_F32>, grid, block, 0, st, args); break;
      case SAD_YPLANE: hipLaunchKernelGGL(frame_luma_sad_kernel<SAD_YPLANE>, grid, block, 0, st, args); break;
      case SAD_HWC3: hipLaunchKernelGGL(frame_luma_sad_kernel<SAD_HWC3>, grid, block, 0, st, args); break;
      case SAD_Y16_MSB: hipLaunchKernelGGL(frame_luma_sad_kernel<SAD_Y16_MSB>, grid, block, 0, st, args); break;
      case SAD_Y16_10: hipLaunchKernelGGL(frame_luma_sad_kernel<SAD_Y16_10>, grid, block, 0, st, args); break;
      case SAD_Y16_12: hipLaunchKernelGGL(frame_luma_sad_kernel<SAD_Y16_12>, grid, block, 0, st, args); break;
      case SAD_HWC16_3: hipLaunchKernelGGL(frame_luma_sad_kernel<SAD_HWC16_3>, grid, block, 0, st, args); break;
      case SAD_HWC16_4: hipLaunchKernelGGL(frame_luma_sad_kernel<SAD_HWC16_4>, grid, block, 0, st, args); break;
      case SAD_CHW8: hipLaunchKernelGGL(frame_luma_sad_kernel<SAD_CHW8>, grid, block, 0, st, args); break;
      case SAD_CHW16: hipLaunchKernelGGL(frame_luma_sad_kernel<SAD_CHW16>, grid, block, 0, st, args); break;
      default: hipLaunchKernelGGL(frame_luma_sad_kernel<SAD_HWC4>, grid, block, 0, st, args); break;
    }
    const int rc = check_launch("frame_luma_sad_kernel");
    if (rc != DVSR_OK) return rc;
  }
  return DVSR_OK;
}
