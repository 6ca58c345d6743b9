// 10- and 12-bit YCbCr 4:2:0 frames in and out of the video path (dvsr_frame_ingest_yuv16 / dvsr_frame_emit_yuv16, engine.hip:
// dvsr_edvr_stream_extract_frame_yuv16), beside the 8-bit 4:2:0 frames of frame_yuv.hip.
//
// What an HEVC Main10 / AV1 / VP9 profile 2 decoder delivers and a 10-bit encoder takes: 16-bit little-endian words that hold
// d = 10 or 12 bits, as
//   SEMI_MSB   (P010 / P012)                a Y plane [h][w] and one plane of interleaved Cb, Cr pairs [Hc][Wc][2];
//                                           word = level << (16 - d); ingest uses word >> (16 - d) (the low bits are ignored),
//                                           emit writes the low bits as 0
//   PLANAR_LSB (yuv420p10le / yuv420p12le)  planes Y, Cb [Hc][Wc], Cr [Hc][Wc]; word = level; ingest uses word & (2^d - 1)
//                                           (the high bits are ignored), emit writes the high bits as 0
// Hc x Wc = ceil(h/2) x ceil(w/2); every plane at any 2-byte aligned address and any even row pitch (in bytes).
//
// The arithmetic (DESIGN 3.2m says the same) is frame_yuv.hip's / DESIGN 3.2k's at a parametric depth -- matrix, chroma siting,
// the [1,1]/2 and 0.75 / 0.25 up-sampling, the [1,2,1]/4 x two-row down-sampling, padding on the source index, the clamp of RGB
// to [0,1] and round half to even are those; only the level scale changes, H.273 at depth d, s = 2^(d-8):
//   LIMITED: y0 = 16 s, ys = 219 s, cs = 224 s, chroma mid cm = 128 s;  FULL: y0 = 0, ys = cs = 2^d - 1, cm = 2^(d-1)
//   (d = 8 gives frame_yuv.hip's constants)
//   ingest, per luma pixel (y, x), C one of the two chroma planes (levels), j = y / 2:
//     Ch(j, x) = C[j][x/2] (x even) | (C[j][k] + C[j][min(k+1, Wc-1)]) / 2, k = (x-1)/2 (x odd)
//     C'       = 0.75 Ch(j, x) + 0.25 Ch(max(j-1, 0), x) (y even) | 0.75 Ch(j, x) + 0.25 Ch(min(j+1, Hc-1), x) (y odd)
//                (multiples of 1/8 of a level below 2^12: exact in fp32)
//     yn = (Y - y0) / ys, cb = (Cb' - cm) / cs, cr = (Cr' - cm) / cs
//     R = yn + 2(1-Kr) cr,  G = yn - (2 Kb (1-Kb) / Kg) cb - (2 Kr (1-Kr) / Kg) cr,  B = yn + 2(1-Kb) cb, each clamped to
//     [0,1]; output pixel (y, x) of the padded [3][Hp][Wp] tensor is the converted pixel at (pad_index(y, h), pad_index(x, w))
//   emit, of the top-left h x w crop of fp32 planar [3][Hs][Ws]:
//     t = (clamp(v, lo, hi) - lo) / (hi - lo) per channel
//     y = Kr R + Kg G + Kb B, cb = (B - y) / (2(1-Kb)), cr = (R - y) / (2(1-Kr))
//     luma level = clamp(rint(y0 + ys y), 0, 2^d - 1), round half to even
//     chroma sample (j, k): taps [1,2,1]/4 on columns 2k-1, 2k, 2k+1, the mean of rows 2j and min(2j+1, h-1), indices clamped to
//     the crop; chroma level = clamp(rint(cm + cs c), 0, 2^d - 1)
// The five divisions by constants -- ys, cs, 2(1-Kb), 2(1-Kr), hi - lo -- are multiplications by reciprocals formed on the host
// in double and rounded once to fp32: one more rounding of 2^-24 relative per quotient, inside the tests' bars.
//
// One thread = a 4 x 2 luma block, a workgroup is 64 x 4 threads (frame_yuv.hip's shape): a wave owns whole rows, so whatever
// depends on a row's address is wave-uniform.  The fp32 side moves as 16-byte accesses.  On the 16-bit side four luma samples
// or two CbCr pairs are 8 bytes: one 8-byte access where the address is 8-aligned, two 4-byte ones where it is 4-aligned, 2 + 4 +
// 2 bytes otherwise; two samples are 4 bytes or 2 + 2.  The offset of a lane's group inside its row is a multiple of the group's
// size, so that choice is the row's: per wave.  No access is wider than its address is aligned (relaxed atomics of wavefront
// scope: plain accesses that are never merged into wider ones), no sub-sample access exists (planes are 2-byte aligned, pitches
// even), and nothing outside the rows of a plane is read or written.  Blocks that hold padded rows / columns or the ragged end
// of the frame work sample by sample.  Depth is an argument (a shift, a mask and the coefficients), not a template parameter.
// Pure streaming: all of a lane's loads come ahead of its first store, no grid-stride loop.
#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace dvsr {

constexpr int Y16_X = 64, Y16_Y = 4;   // threads of a workgroup along a row (one wave) / block rows of a workgroup

struct Yuv16Coef {
  float y0, cm, ys, cs, top;        // luma offset, chroma mid, luma / chroma scale, 2^d - 1 (levels)
  float inv_ys, inv_cs;             // (double) 1 / ys, 1 / cs
  float kr, kg, kb;
  float r_cr, g_cb, g_cr, b_cb;     // 2(1-Kr), 2 Kb (1-Kb) / Kg, 2 Kr (1-Kr) / Kg, 2(1-Kb)
  float inv_r_cr, inv_b_cb;         // (double) 1 / (2(1-Kr)), 1 / (2(1-Kb))
};

struct Yuv16IngestArgs {
  const unsigned char* p[3];
  long long rs[3];                  // bytes
  float* dst;
  int h, w, Hp, Wp, pad;
  unsigned shift, mask;             // level = (word >> shift) & mask
  Yuv16Coef k;
};

struct Yuv16EmitArgs {
  const float* src;
  unsigned char* p[3];
  long long rs[3];
  int Hs, Ws, h, w;
  float lo, inv_scale, hi;          // inv_scale = (double) 1 / (hi - lo)
  unsigned shift;                   // word = level << shift
  Yuv16Coef k;
};

__device__ __forceinline__ int y16_pad_index(int i, int n, int mode) {
  return i < n ? i : (mode == DVSR_FRAME_PAD_REFLECT ? 2 * (n - 1) - i : n - 1);
}

// ---- the 16-bit side: groups of 1, 2, 4 words at a 2-byte aligned address, in naturally aligned pieces
__device__ __forceinline__ unsigned w16_ld1(const unsigned char* p) {
  return __hip_atomic_load(reinterpret_cast<const unsigned short*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ unsigned w16_ld2a(const unsigned char* p) {   // p 4-aligned
  return __hip_atomic_load(reinterpret_cast<const unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ unsigned w16_ld2(const unsigned char* p) {
  return (reinterpret_cast<uintptr_t>(p) & 2) ? (w16_ld1(p) | (w16_ld1(p + 2) << 16)) : w16_ld2a(p);
}
__device__ __forceinline__ void w16_ld4(const unsigned char* p, unsigned& lo, unsigned& hi) {
  const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 7);
  if (m == 0) {
    const unsigned long long v =
        __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    lo = (unsigned)v;
    hi = (unsigned)(v >> 32);
  } else if (m == 4) {
    lo = w16_ld2a(p);
    hi = w16_ld2a(p + 4);
  } else {
    const unsigned a = w16_ld1(p), b = w16_ld2a(p + 2), c = w16_ld1(p + 6);
    lo = a | (b << 16);
    hi = (b >> 16) | (c << 16);
  }
}
__device__ __forceinline__ void w16_st1(unsigned char* p, unsigned v) {
  __hip_atomic_store(reinterpret_cast<unsigned short*>(p), (unsigned short)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void w16_st2a(unsigned char* p, unsigned v) {   // p 4-aligned
  __hip_atomic_store(reinterpret_cast<unsigned*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void w16_st2(unsigned char* p, unsigned v) {
  if (reinterpret_cast<uintptr_t>(p) & 2) {
    w16_st1(p, v);
    w16_st1(p + 2, v >> 16);
  } else {
    w16_st2a(p, v);
  }
}
__device__ __forceinline__ void w16_st4(unsigned char* p, unsigned lo, unsigned hi) {
  const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 7);
  if (m == 0) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)lo | ((unsigned long long)hi << 32),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  } else if (m == 4) {
    w16_st2a(p, lo);
    w16_st2a(p + 4, hi);
  } else {
    w16_st1(p, lo);
    w16_st2a(p + 2, (lo >> 16) | (hi << 16));
    w16_st1(p + 6, hi >> 16);
  }
}

// the levels of the two words of a dword
__device__ __forceinline__ float y16_lev0(const Yuv16IngestArgs& a, unsigned v) { return (float)(((v & 0xffffu) >> a.shift) & a.mask); }
__device__ __forceinline__ float y16_lev1(const Yuv16IngestArgs& a, unsigned v) { return (float)((v >> (16 + a.shift)) & a.mask); }

// chroma sample (j, k) of both planes
template <int FMT>
__device__ __forceinline__ void y16_chroma1(const Yuv16IngestArgs& a, int j, int k, float& cb, float& cr) {
  if (FMT == DVSR_YUV16_SEMI_MSB) {
    const unsigned v = w16_ld2(a.p[1] + (long long)j * a.rs[1] + 4 * k);
    cb = y16_lev0(a, v);
    cr = y16_lev1(a, v);
  } else {
    cb = y16_lev0(a, w16_ld1(a.p[1] + (long long)j * a.rs[1] + 2 * k));
    cr = y16_lev0(a, w16_ld1(a.p[2] + (long long)j * a.rs[2] + 2 * k));
  }
}

// chroma samples (j, k0), (j, k0 + 1), (j, k2) of both planes; k0 is even and k0 + 1 < Wc
template <int FMT>
__device__ __forceinline__ void y16_chroma3(const Yuv16IngestArgs& a, int j, int k0, int k2, float cb[3], float cr[3]) {
  if (FMT == DVSR_YUV16_SEMI_MSB) {
    unsigned lo, hi;
    w16_ld4(a.p[1] + (long long)j * a.rs[1] + 4 * k0, lo, hi);
    cb[0] = y16_lev0(a, lo);
    cr[0] = y16_lev1(a, lo);
    cb[1] = y16_lev0(a, hi);
    cr[1] = y16_lev1(a, hi);
  } else {
    const unsigned u = w16_ld2(a.p[1] + (long long)j * a.rs[1] + 2 * k0), v = w16_ld2(a.p[2] + (long long)j * a.rs[2] + 2 * k0);
    cb[0] = y16_lev0(a, u);
    cb[1] = y16_lev1(a, u);
    cr[0] = y16_lev0(a, v);
    cr[1] = y16_lev1(a, v);
  }
  y16_chroma1<FMT>(a, j, k2, cb[2], cr[2]);
}

__device__ __forceinline__ float y16_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

template <int FMT>
__global__ __launch_bounds__(Y16_X * Y16_Y) void frame_ingest_yuv16_kernel(Yuv16IngestArgs a) {
  const int x0 = (blockIdx.x * Y16_X + threadIdx.x) * 4;
  const int y0 = (blockIdx.y * Y16_Y + threadIdx.y) * 2;
  if (x0 >= a.Wp || y0 >= a.Hp) return;
  const int Hc = (a.h + 1) >> 1, Wc = (a.w + 1) >> 1;
  float Y[2][4], Cb[2][4], Cr[2][4];   // levels: luma as stored, chroma upsampled to the luma grid
  if (x0 + 3 < a.w && y0 + 1 < a.h) {
    // a block inside the frame: luma rows y0, y0 + 1 share chroma row j; its columns x0 .. x0 + 3 lie on chroma columns
    // k0, k0 + 1 and reach to k0 + 2 for the last (odd) one
    const int j = y0 >> 1, k0 = x0 >> 1, k2 = min(k0 + 2, Wc - 1);
    const int jr[3] = {max(j - 1, 0), j, min(j + 1, Hc - 1)};
    unsigned yl[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r) w16_ld4(a.p[0] + (long long)(y0 + r) * a.rs[0] + 2 * x0, yl[r][0], yl[r][1]);
    float cb[3][3], cr[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) y16_chroma3<FMT>(a, jr[r], k0, k2, cb[r], cr[r]);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        Y[r][2 * i] = y16_lev0(a, yl[r][i]);
        Y[r][2 * i + 1] = y16_lev1(a, yl[r][i]);
      }
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
    // padded rows / columns, the ragged end of a row, the last row of an odd height: sample by sample, every index clamped
    float cbv[2][4][4], crv[2][4][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int sy = y16_pad_index(min(y0 + r, a.Hp - 1), a.h, a.pad);
      const int j = sy >> 1, jn = (sy & 1) ? min(j + 1, Hc - 1) : max(j - 1, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int sx = y16_pad_index(x0 + i, a.w, a.pad);
        const int ka = sx >> 1, kb = (sx & 1) ? min(ka + 1, Wc - 1) : ka;
        Y[r][i] = y16_lev0(a, w16_ld1(a.p[0] + (long long)sy * a.rs[0] + 2 * sx));
        y16_chroma1<FMT>(a, j, ka, cbv[r][i][0], crv[r][i][0]);
        y16_chroma1<FMT>(a, j, kb, cbv[r][i][1], crv[r][i][1]);
        y16_chroma1<FMT>(a, jn, ka, cbv[r][i][2], crv[r][i][2]);
        y16_chroma1<FMT>(a, jn, kb, cbv[r][i][3], crv[r][i][3]);
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
      const float yn = (Y[r][i] - a.k.y0) * a.k.inv_ys, cb = (Cb[r][i] - a.k.cm) * a.k.inv_cs, cr = (Cr[r][i] - a.k.cm) * a.k.inv_cs;
      o[r][0][i] = y16_clamp01(yn + a.k.r_cr * cr);
      o[r][1][i] = y16_clamp01(yn - a.k.g_cb * cb - a.k.g_cr * cr);
      o[r][2][i] = y16_clamp01(yn + a.k.b_cb * cb);
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

__device__ __forceinline__ unsigned y16_quant(float v, float top) { return (unsigned)(int)fminf(fmaxf(rintf(v), 0.0f), top); }

template <int FMT>
__global__ __launch_bounds__(Y16_X * Y16_Y) void frame_emit_yuv16_kernel(Yuv16EmitArgs a) {
  const int x0 = (blockIdx.x * Y16_X + threadIdx.x) * 4;
  const int y0 = (blockIdx.y * Y16_Y + threadIdx.y) * 2;
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
        t[c] = (fminf(fmaxf(s, a.lo), a.hi) - a.lo) * a.inv_scale;
      }
      const float y = a.k.kr * t[0] + a.k.kg * t[1] + a.k.kb * t[2];
      cbv[r][i] = (t[2] - y) * a.k.inv_b_cb;
      crv[r][i] = (t[0] - y) * a.k.inv_r_cr;
      if (i > 0) yv[r][i - 1] = y;
    }
  unsigned yw[2][4], cbw[2], crw[2];      // words
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) yw[r][i] = y16_quant(a.k.y0 + a.k.ys * yv[r][i], a.k.top) << a.shift;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = 2 * k;               // columns 2k - 1, 2k, 2k + 1 of this lane's chroma column k
    const float fb = 0.5f * (0.25f * (cbv[0][i] + 2.0f * cbv[0][i + 1] + cbv[0][i + 2]) +
                             0.25f * (cbv[1][i] + 2.0f * cbv[1][i + 1] + cbv[1][i + 2]));
    const float fr = 0.5f * (0.25f * (crv[0][i] + 2.0f * crv[0][i + 1] + crv[0][i + 2]) +
                             0.25f * (crv[1][i] + 2.0f * crv[1][i + 1] + crv[1][i + 2]));
    cbw[k] = y16_quant(a.k.cm + a.k.cs * fb, a.k.top) << a.shift;
    crw[k] = y16_quant(a.k.cm + a.k.cs * fr, a.k.top) << a.shift;
  }
  // ---- stores
#pragma unroll
  for (int r = 0; r < 2; ++r)
    if (y0 + r < a.h) {
      unsigned char* q = a.p[0] + (long long)(y0 + r) * a.rs[0] + 2 * x0;
      if (x0 + 3 < a.w) {
        w16_st4(q, yw[r][0] | (yw[r][1] << 16), yw[r][2] | (yw[r][3] << 16));
      } else {
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (x0 + i < a.w) w16_st1(q + 2 * i, yw[r][i]);
      }
    }
  const int j = y0 >> 1;
  const bool two = x0 + 2 < a.w;        // this lane's second chroma column exists
  if (FMT == DVSR_YUV16_SEMI_MSB) {
    unsigned char* q = a.p[1] + (long long)j * a.rs[1] + 2 * x0;      // pair k0 = x0 / 2 is 4 k0 bytes into the row
    if (two) w16_st4(q, cbw[0] | (crw[0] << 16), cbw[1] | (crw[1] << 16));
    else w16_st2(q, cbw[0] | (crw[0] << 16));
  } else {
    unsigned char* qb = a.p[1] + (long long)j * a.rs[1] + x0;          // sample k0 is 2 k0 bytes into the row
    unsigned char* qr = a.p[2] + (long long)j * a.rs[2] + x0;
    if (two) {
      w16_st2(qb, cbw[0] | (cbw[1] << 16));
      w16_st2(qr, crw[0] | (crw[1] << 16));
    } else {
      w16_st1(qb, cbw[0]);
      w16_st1(qr, crw[0]);
    }
  }
}

// (arguments checked by yuv16_desc_check)
static Yuv16Coef yuv16_coef(int matrix, int range, int depth) {
  const double kr = matrix == DVSR_YUV_BT709 ? 0.2126 : 0.299, kb = matrix == DVSR_YUV_BT709 ? 0.0722 : 0.114, kg = 1.0 - kr - kb;
  const bool full = range == DVSR_YUV_FULL;
  const double s = (double)(1 << (depth - 8)), top = (double)((1 << depth) - 1);
  const double y0 = full ? 0.0 : 16.0 * s, ys = full ? top : 219.0 * s, cs = full ? top : 224.0 * s, cm = 128.0 * s;
  const double r_cr = 2.0 * (1.0 - kr), b_cb = 2.0 * (1.0 - kb);
  return Yuv16Coef{(float)y0, (float)cm, (float)ys, (float)cs, (float)top, (float)(1.0 / ys), (float)(1.0 / cs),
                   (float)kr, (float)kg, (float)kb, (float)r_cr, (float)(2.0 * kb * (1.0 - kb) / kg),
                   (float)(2.0 * kr * (1.0 - kr) / kg), (float)b_cb, (float)(1.0 / r_cr), (float)(1.0 / b_cb)};
}

// the frame on the "any address, any pitch" side, against the h x w it may have at most
static int yuv16_desc_check(const char* what, const dvsr_yuv16_desc* d, int Ht, int Wt) {
  DVSR_REQUIRE(d, DVSR_ERR_INVALID, "%s: null descriptor", what);
  DVSR_REQUIRE(d->format == DVSR_YUV16_SEMI_MSB || d->format == DVSR_YUV16_PLANAR_LSB, DVSR_ERR_INVALID,
               "%s: unknown 16-bit YUV format %d", what, d->format);
  DVSR_REQUIRE(d->depth == 10 || d->depth == 12, DVSR_ERR_INVALID, "%s: unknown depth %d (10 or 12)", what, d->depth);
  DVSR_REQUIRE(d->matrix == DVSR_YUV_BT601 || d->matrix == DVSR_YUV_BT709, DVSR_ERR_INVALID, "%s: unknown YUV matrix %d", what,
               d->matrix);
  DVSR_REQUIRE(d->range == DVSR_YUV_LIMITED || d->range == DVSR_YUV_FULL, DVSR_ERR_INVALID, "%s: unknown YUV range %d", what,
               d->range);
  DVSR_REQUIRE(d->h >= 1 && d->w >= 1 && d->h <= Ht && d->w <= Wt, DVSR_ERR_INVALID,
               "%s: frame size h=%d w=%d outside [1, %d] x [1, %d]", what, d->h, d->w, Ht, Wt);
  const int np = d->format == DVSR_YUV16_SEMI_MSB ? 2 : 3;
  const long long Wc = (d->w + 1) / 2;
  for (int i = 0; i < np; ++i) {
    DVSR_REQUIRE(d->plane[i], DVSR_ERR_INVALID, "%s: null plane %d", what, i);
    DVSR_REQUIRE(reinterpret_cast<uintptr_t>(d->plane[i]) % 2 == 0, DVSR_ERR_INVALID, "%s: odd address of plane %d (16-bit samples)",
                 what, i);
    const long long need = 2 * (i == 0 ? d->w : (d->format == DVSR_YUV16_SEMI_MSB ? 2 * Wc : Wc));
    DVSR_REQUIRE(d->row_stride[i] >= need, DVSR_ERR_INVALID, "%s: row stride %lld of plane %d shorter than a row of %lld bytes",
                 what, d->row_stride[i], i, need);
    DVSR_REQUIRE(d->row_stride[i] % 2 == 0, DVSR_ERR_INVALID, "%s: odd row stride %lld of plane %d (16-bit samples)", what,
                 d->row_stride[i], i);
  }
  return DVSR_OK;
}

// the planar fp32 side: [3][H][W], 16-byte accesses; a workgroup covers 2 * Y16_Y rows
static int yuv16_planar_check(const char* what, const float* ptr, int H, int W) {
  DVSR_REQUIRE(ptr, DVSR_ERR_INVALID, "%s: null planar tensor", what);
  DVSR_REQUIRE(H >= 1 && W >= 4 && W % 4 == 0 && H <= 2 * Y16_Y * 65535, DVSR_ERR_INVALID,
               "%s: planar tensor H=%d W=%d (W must be a positive multiple of 4)", what, H, W);
  DVSR_REQUIRE(reinterpret_cast<uintptr_t>(ptr) % 16 == 0, DVSR_ERR_INVALID, "%s: misaligned planar fp32 tensor (16 bytes)", what);
  return DVSR_OK;
}

int frame_ingest_yuv16_check(const char* what, const dvsr_yuv16_desc* sd, const float* dst, int Hp, int Wp, int pad_mode) {
  int rc = yuv16_planar_check(what, dst, Hp, Wp);
  if (rc != DVSR_OK) return rc;
  rc = yuv16_desc_check(what, sd, Hp, Wp);
  if (rc != DVSR_OK) return rc;
  DVSR_REQUIRE(pad_mode == DVSR_FRAME_PAD_REFLECT || pad_mode == DVSR_FRAME_PAD_REPLICATE, DVSR_ERR_INVALID,
               "%s: unknown pad mode %d", what, pad_mode);
  DVSR_REQUIRE(pad_mode != DVSR_FRAME_PAD_REFLECT || (Hp - sd->h < sd->h && Wp - sd->w < sd->w), DVSR_ERR_INVALID,
               "%s: reflect pad %d x %d not smaller than the frame %d x %d", what, Hp - sd->h, Wp - sd->w, sd->h, sd->w);
  return DVSR_OK;
}

// (arguments checked by frame_ingest_yuv16_check)
int frame_ingest_yuv16_launch(const dvsr_yuv16_desc& sd, float* dst, int Hp, int Wp, int pad_mode, hipStream_t st) {
  Yuv16IngestArgs a{};
  for (int i = 0; i < 3; ++i) {
    a.p[i] = static_cast<const unsigned char*>(sd.plane[i]);
    a.rs[i] = sd.row_stride[i];
  }
  a.dst = dst;
  a.h = sd.h, a.w = sd.w, a.Hp = Hp, a.Wp = Wp, a.pad = pad_mode;
  const bool msb = sd.format == DVSR_YUV16_SEMI_MSB;
  a.shift = msb ? 16u - (unsigned)sd.depth : 0u;
  a.mask = (1u << sd.depth) - 1u;
  a.k = yuv16_coef(sd.matrix, sd.range, sd.depth);
  const dim3 grid(ceil_div(Wp / 4, Y16_X), ceil_div(ceil_div(Hp, 2), Y16_Y)), block(Y16_X, Y16_Y);
  if (msb) hipLaunchKernelGGL(frame_ingest_yuv16_kernel<DVSR_YUV16_SEMI_MSB>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(frame_ingest_yuv16_kernel<DVSR_YUV16_PLANAR_LSB>, grid, block, 0, st, a);
  return check_launch("frame_ingest_yuv16_kernel");
}

}  // namespace dvsr

using namespace dvsr;

extern "C" int dvsr_frame_ingest_yuv16(const dvsr_yuv16_desc* sd, float* dst, int Hp, int Wp, int pad_mode, dvsr_stream_t stream) {
  int rc = frame_ingest_yuv16_check("frame_ingest_yuv16", sd, dst, Hp, Wp, pad_mode);
  if (rc != DVSR_OK) return rc;
  return frame_ingest_yuv16_launch(*sd, dst, Hp, Wp, pad_mode, (hipStream_t)stream);
}

extern "C" int dvsr_frame_emit_yuv16(const float* src, int Hs, int Ws, const dvsr_yuv16_desc* dd, float lo, float hi,
                                     dvsr_stream_t stream) {
  int rc = yuv16_planar_check("frame_emit_yuv16", src, Hs, Ws);
  if (rc != DVSR_OK) return rc;
  rc = yuv16_desc_check("frame_emit_yuv16", dd, Hs, Ws);
  if (rc != DVSR_OK) return rc;
  DVSR_REQUIRE(hi > lo, DVSR_ERR_INVALID, "frame_emit_yuv16: range [%g, %g]", (double)lo, (double)hi);
  Yuv16EmitArgs a{};
  a.src = src;
  for (int i = 0; i < 3; ++i) {
    a.p[i] = static_cast<unsigned char*>(dd->plane[i]);
    a.rs[i] = dd->row_stride[i];
  }
  a.Hs = Hs, a.Ws = Ws, a.h = dd->h, a.w = dd->w, a.lo = lo, a.hi = hi;
  a.inv_scale = (float)(1.0 / ((double)hi - (double)lo));
  const bool msb = dd->format == DVSR_YUV16_SEMI_MSB;
  a.shift = msb ? 16u - (unsigned)dd->depth : 0u;
  a.k = yuv16_coef(dd->matrix, dd->range, dd->depth);
  const dim3 grid(ceil_div(ceil_div(dd->w, 4), Y16_X), ceil_div(ceil_div(dd->h, 2), Y16_Y)), block(Y16_X, Y16_Y);
  if (msb) hipLaunchKernelGGL(frame_emit_yuv16_kernel<DVSR_YUV16_SEMI_MSB>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(frame_emit_yuv16_kernel<DVSR_YUV16_PLANAR_LSB>, grid, block, 0, (hipStream_t)stream, a);
  return check_launch("frame_emit_yuv16_kernel");
}
