// YCbCr 4:2:0 frames in and out of the video path (dvsr_frame_ingest_yuv / dvsr_frame_emit_yuv, engine.hip:
// dvsr_edvr_stream_extract_frame_yuv), beside the 8-bit RGB / BGR frames of frame_io.hip.
//
// What a video decoder delivers and an encoder takes is 8-bit YCbCr 4:2:0, as NV12 (a Y plane [h][w] and one plane of
// interleaved Cb, Cr pairs [Hc][Wc][2]) or planar I420 (Y, Cb [Hc][Wc], Cr [Hc][Wc]), Hc x Wc = ceil(h/2) x ceil(w/2), every
// plane at any address and row pitch.  The network computes on fp32 planar RGB [3][Hp][Wp] in [0,1].
//
// The arithmetic (DESIGN 3.2k says the same):
//   matrix  BT601: Kr = 0.299, Kb = 0.114;  BT709: Kr = 0.2126, Kb = 0.0722;  Kg = 1 - Kr - Kb
//   range   LIMITED: y0 = 16, ys = 219, cs = 224;  FULL: y0 = 0, ys = 255, cs = 255
//   BT601 + LIMITED are the reference's ycbcr2rgb / rgb2ycbcr ("same as matlab", data/util.py:234-299).
//   siting  MPEG-2 / H.264 "left": chroma sample (j, k) sits on luma column 2k, midway between luma rows 2j and 2j+1.
//   ingest, per luma pixel (y, x) of the frame, C one of the two chroma planes, j = y / 2:
//     Ch(j, x) = C[j][x/2] (x even) | (C[j][k] + C[j][min(k+1, Wc-1)]) / 2, k = (x-1)/2 (x odd)
//     C'       = 0.75 Ch(j, x) + 0.25 Ch(max(j-1, 0), x) (y even) | 0.75 Ch(j, x) + 0.25 Ch(min(j+1, Hc-1), x) (y odd)
//                (multiples of 1/8 of a level: exact in fp32)
//     yn = (Y - y0) / ys, cb = (Cb' - 128) / cs, cr = (Cr' - 128) / cs
//     R = yn + 2(1-Kr) cr,  G = yn - (2 Kb (1-Kb) / Kg) cb - (2 Kr (1-Kr) / Kg) cr,  B = yn + 2(1-Kb) cb, each clamped to
//     [0,1]; nothing is rounded to 8 bits.  Output pixel (y, x) of the padded [3][Hp][Wp] tensor is the converted pixel at
//     (pad_index(y, h), pad_index(x, w)): ingest(yuv, pad) = F.pad(convert(yuv), .., mode).
//   emit, of the top-left h x w crop of fp32 planar [3][Hs][Ws]:
//     t = (clamp(v, lo, hi) - lo) / (hi - lo) per channel (quant.h's first line)
//     y = Kr R + Kg G + Kb B, cb = (B - y) / (2(1-Kb)), cr = (R - y) / (2(1-Kr))
//     luma byte = clamp(rint(y0 + ys y), 0, 255), round half to even
//     chroma sample (j, k): taps [1,2,1]/4 on columns 2k-1, 2k, 2k+1, the mean of rows 2j and min(2j+1, h-1), indices clamped to
//     the crop -- nothing outside it influences a byte; chroma byte = clamp(rint(128 + cs c), 0, 255)
//
// One thread = a 4 x 2 luma block (two rows, four columns): one chroma row, two chroma columns, and the neighbours the filters
// need.  A workgroup is 64 x 4 threads, so a wave owns whole rows and whatever depends on a row's address is wave-uniform.
// The fp32 side moves as 16-byte accesses.  On the byte side no access is wider than its address is aligned and no byte
// outside the rows of a plane is read or written: a group of 4 (2) bytes moves as a dword (a short) where its address allows
// it and in naturally aligned pieces otherwise -- relaxed atomics, which are plain sub-dword accesses that are never merged
// into wider, possibly misaligned ones.  Blocks that hold padded rows / columns or the ragged end of the frame work pixel by
// pixel.  Pure streaming: all of a lane's loads come ahead of its first store, no grid-stride loop (frame_io.hip).
#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace dvsr {

constexpr int YUV_X = 64, YUV_Y = 4;   // threads of a workgroup along a row (one wave) / block rows of a workgroup

struct YuvCoef {
  float y0, ys, cs;
  float kr, kg, kb;
  float r_cr, g_cb, g_cr, b_cb;   // 2(1-Kr), 2 Kb (1-Kb) / Kg, 2 Kr (1-Kr) / Kg, 2(1-Kb)
};

struct YuvIngestArgs {
  const unsigned char* p[3];
  long long rs[3];
  float* dst;
  int h, w, Hp, Wp, pad;
  YuvCoef k;
};

struct YuvEmitArgs {
  const float* src;
  unsigned char* p[3];
  long long rs[3];
  int Hs, Ws, h, w;
  float lo, hi;
  YuvCoef k;
};

// (frame_io.hip's) index i of a padded axis -> index of the frame's own axis of length n
__device__ __forceinline__ int yuv_pad_index(int i, int n, int mode) {
  return i < n ? i : (mode == DVSR_FRAME_PAD_REFLECT ? 2 * (n - 1) - i : n - 1);
}

// ---- the byte side: little-endian groups of 1, 2, 4 bytes at any address, in naturally aligned pieces
__device__ __forceinline__ unsigned ld1(const unsigned char* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ unsigned ld2a(const unsigned char* p) {   // p even
  return __hip_atomic_load(reinterpret_cast<const unsigned short*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ unsigned ld2(const unsigned char* p) {
  return (reinterpret_cast<uintptr_t>(p) & 1) ? (ld1(p) | (ld1(p + 1) << 8)) : ld2a(p);
}
__device__ __forceinline__ unsigned ld4(const unsigned char* p) {
  const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
  if (m == 0) return *reinterpret_cast<const unsigned*>(p);
  if (m == 2) return ld2a(p) | (ld2a(p + 2) << 16);
  return ld1(p) | (ld2a(p + 1) << 8) | (ld1(p + 3) << 24);
}
__device__ __forceinline__ void st1(unsigned char* p, unsigned v) {
  __hip_atomic_store(p, (unsigned char)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void st2a(unsigned char* p, unsigned v) {   // p even
  __hip_atomic_store(reinterpret_cast<unsigned short*>(p), (unsigned short)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void st2(unsigned char* p, unsigned v) {
  if (reinterpret_cast<uintptr_t>(p) & 1) {
    st1(p, v);
    st1(p + 1, v >> 8);
  } else {
    st2a(p, v);
  }
}
__device__ __forceinline__ void st4(unsigned char* p, unsigned v) {
  const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
  if (m == 0) {
    *reinterpret_cast<unsigned*>(p) = v;
  } else if (m == 2) {
    st2a(p, v);
    st2a(p + 2, v >> 16);
  } else {
    st1(p, v);
    st2a(p + 1, v >> 8);
    st1(p + 3, v >> 24);
  }
}

// chroma sample (j, k) of both planes
template <int FMT>
__device__ __forceinline__ void chroma1(const YuvIngestArgs& a, int j, int k, float& cb, float& cr) {
  if (FMT == DVSR_YUV_NV12) {
    const unsigned v = ld2(a.p[1] + (long long)j * a.rs[1] + 2 * k);
    cb = (float)(v & 0xffu);
    cr = (float)(v >> 8);
  } else {
    cb = (float)ld1(a.p[1] + (long long)j * a.rs[1] + k);
    cr = (float)ld1(a.p[2] + (long long)j * a.rs[2] + k);
  }
}

// chroma samples (j, k0), (j, k0 + 1), (j, k2) of both planes; k0 is even and k0 + 1 < Wc
template <int FMT>
__device__ __forceinline__ void chroma3(const YuvIngestArgs& a, int j, int k0, int k2, float cb[3], float cr[3]) {
  if (FMT == DVSR_YUV_NV12) {
    const unsigned v = ld4(a.p[1] + (long long)j * a.rs[1] + 2 * k0);
    cb[0] = (float)(v & 0xffu);
    cr[0] = (float)((v >> 8) & 0xffu);
    cb[1] = (float)((v >> 16) & 0xffu);
    cr[1] = (float)(v >> 24);
  } else {
    const unsigned u = ld2(a.p[1] + (long long)j * a.rs[1] + k0), v = ld2(a.p[2] + (long long)j * a.rs[2] + k0);
    cb[0] = (float)(u & 0xffu);
    cb[1] = (float)(u >> 8);
    cr[0] = (float)(v & 0xffu);
    cr[1] = (float)(v >> 8);
  }
  chroma1<FMT>(a, j, k2, cb[2], cr[2]);
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

template <int FMT>
__global__ __launch_bounds__(YUV_X * YUV_Y) void frame_ingest_yuv_kernel(YuvIngestArgs a) {
  const int x0 = (blockIdx.x * YUV_X + threadIdx.x) * 4;
  const int y0 = (blockIdx.y * YUV_Y + threadIdx.y) * 2;
  if (x0 >= a.Wp || y0 >= a.Hp) return;
  const int Hc = (a.h + 1) >> 1, Wc = (a.w + 1) >> 1;
  float Y[2][4], Cb[2][4], Cr[2][4];   // levels: luma as stored, chroma upsampled to the luma grid
  if (x0 + 3 < a.w && y0 + 1 < a.h) {
    // a block inside the frame: luma rows y0, y0 + 1 share chroma row j; its columns x0 .. x0 + 3 lie on chroma columns
    // k0, k0 + 1 and reach to k0 + 2 for the last (odd) one
    const int j = y0 >> 1, k0 = x0 >> 1, k2 = min(k0 + 2, Wc - 1);
    const int jr[3] = {max(j - 1, 0), j, min(j + 1, Hc - 1)};
    unsigned yl[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) yl[r] = ld4(a.p[0] + (long long)(y0 + r) * a.rs[0] + x0);
    float cb[3][3], cr[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) chroma3<FMT>(a, jr[r], k0, k2, cb[r], cr[r]);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) Y[r][i] = (float)((yl[r] >> (8 * i)) & 0xffu);
    float hb[3][4], hr[3][4];           // the horizontal step, per chroma row
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      hb[r][0] = cb[r][0];
      hb[r][1] = (cb[r][0] + cb[r][1]) * 0.5f;
      hb[r][2] = cb[r][1];
      hb[r][3] = (cb[r][1] + cb[r][2]) * 0.5f;
      hr[r][0] = cr[r][0];
      hr[r][1] = (cr[r][0] + cr[r][1]) * 0.5f;
      hr[r][2] = cr[r][1];
      hr[r][3] = (cr[r][1] + cr[r][2]) * 0.5f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      Cb[0][i] = 0.75f * hb[1][i] + 0.25f * hb[0][i];
      Cb[1][i] = 0.75f * hb[1][i] + 0.25f * hb[2][i];
      Cr[0][i] = 0.75f * hr[1][i] + 0.25f * hr[0][i];
      Cr[1][i] = 0.75f * hr[1][i] + 0.25f * hr[2][i];
    }
  } else {
    // padded rows / columns, the ragged end of a row, the last row of an odd height: pixel by pixel, every index clamped
    float cbv[2][4][4], crv[2][4][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int sy = yuv_pad_index(min(y0 + r, a.Hp - 1), a.h, a.pad);
      const int j = sy >> 1, jn = (sy & 1) ? min(j + 1, Hc - 1) : max(j - 1, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int sx = yuv_pad_index(x0 + i, a.w, a.pad);
        const int ka = sx >> 1, kb = (sx & 1) ? min(ka + 1, Wc - 1) : ka;
        Y[r][i] = (float)ld1(a.p[0] + (long long)sy * a.rs[0] + sx);
        chroma1<FMT>(a, j, ka, cbv[r][i][0], crv[r][i][0]);
        chroma1<FMT>(a, j, kb, cbv[r][i][1], crv[r][i][1]);
        chroma1<FMT>(a, jn, ka, cbv[r][i][2], crv[r][i][2]);
        chroma1<FMT>(a, jn, kb, cbv[r][i][3], crv[r][i][3]);
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Cb[r][i] = 0.75f * ((cbv[r][i][0] + cbv[r][i][1]) * 0.5f) + 0.25f * ((cbv[r][i][2] + cbv[r][i][3]) * 0.5f);
        Cr[r][i] = 0.75f * ((crv[r][i][0] + crv[r][i][1]) * 0.5f) + 0.25f * ((crv[r][i][2] + crv[r][i][3]) * 0.5f);
      }
  }
  f32x4 o[2][3];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float yn = (Y[r][i] - a.k.y0) / a.k.ys, cb = (Cb[r][i] - 128.0f) / a.k.cs, cr = (Cr[r][i] - 128.0f) / a.k.cs;
      o[r][0][i] = clamp01(yn + a.k.r_cr * cr);
      o[r][1][i] = clamp01(yn - a.k.g_cb * cb - a.k.g_cr * cr);
      o[r][2][i] = clamp01(yn + a.k.b_cb * cb);
    }
  const long long plane = (long long)a.Hp * a.Wp;
  float* d = a.dst + (long long)y0 * a.Wp + x0;
#pragma unroll
  for (int r = 0; r < 2; ++r)
    if (y0 + r < a.Hp) {
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(d + c * plane + (long long)r * a.Wp) = o[r][c];
    }
}

__device__ __forceinline__ unsigned quant_level(float v) { return (unsigned)(int)fminf(fmaxf(rintf(v), 0.0f), 255.0f); }

template <int FMT>
__global__ __launch_bounds__(YUV_X * YUV_Y) void frame_emit_yuv_kernel(YuvEmitArgs a) {
  const int x0 = (blockIdx.x * YUV_X + threadIdx.x) * 4;
  const int y0 = (blockIdx.y * YUV_Y + threadIdx.y) * 2;
  if (x0 >= a.w || y0 >= a.h) return;
  // rows y0 and min(y0 + 1, h - 1); columns max(x0 - 1, 0) and x0 .. x0 + 3 (x0 + 3 < Ws: Ws is a multiple of 4, x0 < w <= Ws)
  const long long plane = (long long)a.Hs * a.Ws;
  const int yr[2] = {y0, min(y0 + 1, a.h - 1)}, xl = max(x0 - 1, 0);
  f32x4 v[2][3];
  float l[2][3];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const float* row = a.src + (long long)yr[r] * a.Ws;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[r][c] = *reinterpret_cast<const f32x4*>(row + c * plane + x0);
      l[r][c] = row[c * plane + xl];
    }
  }
  const float scale = a.hi - a.lo;
  float yv[2][4], cbv[2][5], crv[2][5];   // column index 0 of cbv / crv is the left neighbour
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      float t[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float s = l[r][c];
        if (i > 0) {
          // a column beyond the crop takes the crop's last one (x0 < w, so that one is in this lane's four)
          if (i > 1 && x0 + i - 1 >= a.w) v[r][c][i - 1] = v[r][c][i - 2];
          s = v[r][c][i - 1];
        }
        t[c] = (fminf(fmaxf(s, a.lo), a.hi) - a.lo) / scale;
      }
      const float y = a.k.kr * t[0] + a.k.kg * t[1] + a.k.kb * t[2];
      cbv[r][i] = (t[2] - y) / a.k.b_cb;
      crv[r][i] = (t[0] - y) / a.k.r_cr;
      if (i > 0) yv[r][i - 1] = y;
    }
  unsigned yb[2] = {0u, 0u}, cbb[2], crb[2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) yb[r] |= quant_level(a.k.y0 + a.k.ys * yv[r][i]) << (8 * i);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = 2 * k;               // columns 2k - 1, 2k, 2k + 1 of this lane's chroma column k
    const float fb = 0.5f * (0.25f * (cbv[0][i] + 2.0f * cbv[0][i + 1] + cbv[0][i + 2]) +
                             0.25f * (cbv[1][i] + 2.0f * cbv[1][i + 1] + cbv[1][i + 2]));
    const float fr = 0.5f * (0.25f * (crv[0][i] + 2.0f * crv[0][i + 1] + crv[0][i + 2]) +
                             0.25f * (crv[1][i] + 2.0f * crv[1][i + 1] + crv[1][i + 2]));
    cbb[k] = quant_level(128.0f + a.k.cs * fb);
    crb[k] = quant_level(128.0f + a.k.cs * fr);
  }
  // ---- stores
#pragma unroll
  for (int r = 0; r < 2; ++r)
    if (y0 + r < a.h) {
      unsigned char* q = a.p[0] + (long long)(y0 + r) * a.rs[0] + x0;
      if (x0 + 3 < a.w) {
        st4(q, yb[r]);
      } else {
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (x0 + i < a.w) st1(q + i, yb[r] >> (8 * i));
      }
    }
  const int j = y0 >> 1;
  const bool two = x0 + 2 < a.w;        // this lane's second chroma column exists
  if (FMT == DVSR_YUV_NV12) {
    unsigned char* q = a.p[1] + (long long)j * a.rs[1] + x0;
    if (two) st4(q, cbb[0] | (crb[0] << 8) | (cbb[1] << 16) | (crb[1] << 24));
    else st2(q, cbb[0] | (crb[0] << 8));
  } else {
    unsigned char* qb = a.p[1] + (long long)j * a.rs[1] + (x0 >> 1);
    unsigned char* qr = a.p[2] + (long long)j * a.rs[2] + (x0 >> 1);
    if (two) {
      st2(qb, cbb[0] | (cbb[1] << 8));
      st2(qr, crb[0] | (crb[1] << 8));
    } else {
      st1(qb, cbb[0]);
      st1(qr, crb[0]);
    }
  }
}

static YuvCoef yuv_coef(int matrix, int range) {
  const double kr = matrix == DVSR_YUV_BT709 ? 0.2126 : 0.299, kb = matrix == DVSR_YUV_BT709 ? 0.0722 : 0.114, kg = 1.0 - kr - kb;
  const bool full = range == DVSR_YUV_FULL;
  return YuvCoef{full ? 0.0f : 16.0f, full ? 255.0f : 219.0f, full ? 255.0f : 224.0f, (float)kr, (float)kg, (float)kb,
                 (float)(2.0 * (1.0 - kr)), (float)(2.0 * kb * (1.0 - kb) / kg), (float)(2.0 * kr * (1.0 - kr) / kg),
                 (float)(2.0 * (1.0 - kb))};
}

// the 4:2:0 frame on the "any address, any pitch" side, against the h x w it may have at most
static int yuv_desc_check(const char* what, const dvsr_yuv_desc* d, int Ht, int Wt) {
  DVSR_REQUIRE(d, DVSR_ERR_INVALID, "%s: null descriptor", what);
  DVSR_REQUIRE(d->format == DVSR_YUV_NV12 || d->format == DVSR_YUV_I420, DVSR_ERR_INVALID, "%s: unknown YUV format %d", what,
               d->format);
  DVSR_REQUIRE(d->matrix == DVSR_YUV_BT601 || d->matrix == DVSR_YUV_BT709, DVSR_ERR_INVALID, "%s: unknown YUV matrix %d", what,
               d->matrix);
  DVSR_REQUIRE(d->range == DVSR_YUV_LIMITED || d->range == DVSR_YUV_FULL, DVSR_ERR_INVALID, "%s: unknown YUV range %d", what,
               d->range);
  DVSR_REQUIRE(d->h >= 1 && d->w >= 1 && d->h <= Ht && d->w <= Wt, DVSR_ERR_INVALID,
               "%s: frame size h=%d w=%d outside [1, %d] x [1, %d]", what, d->h, d->w, Ht, Wt);
  const int np = d->format == DVSR_YUV_NV12 ? 2 : 3;
  const long long Wc = (d->w + 1) / 2;
  for (int i = 0; i < np; ++i) {
    DVSR_REQUIRE(d->plane[i], DVSR_ERR_INVALID, "%s: null plane %d", what, i);
    const long long need = i == 0 ? d->w : (d->format == DVSR_YUV_NV12 ? 2 * Wc : Wc);
    DVSR_REQUIRE(d->row_stride[i] >= need, DVSR_ERR_INVALID, "%s: row stride %lld of plane %d shorter than a row of %lld bytes",
                 what, d->row_stride[i], i, need);
  }
  return DVSR_OK;
}

// the planar fp32 side: [3][H][W], 16-byte accesses; a workgroup covers 2 * YUV_Y rows
static int yuv_planar_check(const char* what, const float* ptr, int H, int W) {
  DVSR_REQUIRE(ptr, DVSR_ERR_INVALID, "%s: null planar tensor", what);
  DVSR_REQUIRE(H >= 1 && W >= 4 && W % 4 == 0 && H <= 2 * YUV_Y * 65535, DVSR_ERR_INVALID,
               "%s: planar tensor H=%d W=%d (W must be a positive multiple of 4)", what, H, W);
  DVSR_REQUIRE(reinterpret_cast<uintptr_t>(ptr) % 16 == 0, DVSR_ERR_INVALID, "%s: misaligned planar fp32 tensor (16 bytes)", what);
  return DVSR_OK;
}

int frame_ingest_yuv_check(const char* what, const dvsr_yuv_desc* sd, const float* dst, int Hp, int Wp, int pad_mode) {
  int rc = yuv_planar_check(what, dst, Hp, Wp);
  if (rc != DVSR_OK) return rc;
  rc = yuv_desc_check(what, sd, Hp, Wp);
  if (rc != DVSR_OK) return rc;
  DVSR_REQUIRE(pad_mode == DVSR_FRAME_PAD_REFLECT || pad_mode == DVSR_FRAME_PAD_REPLICATE, DVSR_ERR_INVALID,
               "%s: unknown pad mode %d", what, pad_mode);
  DVSR_REQUIRE(pad_mode != DVSR_FRAME_PAD_REFLECT || (Hp - sd->h < sd->h && Wp - sd->w < sd->w), DVSR_ERR_INVALID,
               "%s: reflect pad %d x %d not smaller than the frame %d x %d", what, Hp - sd->h, Wp - sd->w, sd->h, sd->w);
  return DVSR_OK;
}

// (arguments checked by frame_ingest_yuv_check)
int frame_ingest_yuv_launch(const dvsr_yuv_desc& sd, float* dst, int Hp, int Wp, int pad_mode, hipStream_t st) {
  YuvIngestArgs a{};
  for (int i = 0; i < 3; ++i) {
    a.p[i] = static_cast<const unsigned char*>(sd.plane[i]);
    a.rs[i] = sd.row_stride[i];
  }
  a.dst = dst;
  a.h = sd.h, a.w = sd.w, a.Hp = Hp, a.Wp = Wp, a.pad = pad_mode;
  a.k = yuv_coef(sd.matrix, sd.range);
  const dim3 grid(ceil_div(Wp / 4, YUV_X), ceil_div(ceil_div(Hp, 2), YUV_Y)), block(YUV_X, YUV_Y);
  if (sd.format == DVSR_YUV_NV12) hipLaunchKernelGGL(frame_ingest_yuv_kernel<DVSR_YUV_NV12>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(frame_ingest_yuv_kernel<DVSR_YUV_I420>, grid, block, 0, st, a);
  return check_launch("frame_ingest_yuv_kernel");
}

}  // namespace dvsr

using namespace dvsr;

extern "C" int dvsr_frame_ingest_yuv(const dvsr_yuv_desc* sd, float* dst, int Hp, int Wp, int pad_mode, dvsr_stream_t stream) {
  int rc = frame_ingest_yuv_check("frame_ingest_yuv", sd, dst, Hp, Wp, pad_mode);
  if (rc != DVSR_OK) return rc;
  return frame_ingest_yuv_launch(*sd, dst, Hp, Wp, pad_mode, (hipStream_t)stream);
}

extern "C" int dvsr_frame_emit_yuv(const float* src, int Hs, int Ws, const dvsr_yuv_desc* dd, float lo, float hi,
                                   dvsr_stream_t stream) {
  int rc = yuv_planar_check("frame_emit_yuv", src, Hs, Ws);
  if (rc != DVSR_OK) return rc;
  rc = yuv_desc_check("frame_emit_yuv", dd, Hs, Ws);
  if (rc != DVSR_OK) return rc;
  DVSR_REQUIRE(hi > lo, DVSR_ERR_INVALID, "frame_emit_yuv: range [%g, %g]", (double)lo, (double)hi);
  YuvEmitArgs a{};
  a.src = src;
  for (int i = 0; i < 3; ++i) {
    a.p[i] = static_cast<unsigned char*>(dd->plane[i]);
    a.rs[i] = dd->row_stride[i];
  }
  a.Hs = Hs, a.Ws = Ws, a.h = dd->h, a.w = dd->w, a.lo = lo, a.hi = hi;
  a.k = yuv_coef(dd->matrix, dd->range);
  const dim3 grid(ceil_div(ceil_div(dd->w, 4), YUV_X), ceil_div(ceil_div(dd->h, 2), YUV_Y)), block(YUV_X, YUV_Y);
  if (dd->format == DVSR_YUV_NV12) hipLaunchKernelGGL(frame_emit_yuv_kernel<DVSR_YUV_NV12>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(frame_emit_yuv_kernel<DVSR_YUV_I420>, grid, block, 0, (hipStream_t)stream, a);
  return check_launch("frame_emit_yuv_kernel");
}
