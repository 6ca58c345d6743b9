// YCbCr 4:2:0, 4:2:2 and 4:4:4 frames of 8, 10 and 12 bits in and out of the video path (dvsr_frame_ingest_yuv /
// dvsr_frame_emit_yuv and their _yuv16 counterparts, engine.hip: dvsr_edvr_stream_extract_frame_yuv / _yuv16), beside the RGB /
// BGR frames of frame_io.hip.
//
// What a video decoder delivers and an encoder takes: a Y plane [h][w] and either one plane of interleaved Cb, Cr pairs
// [Hc][Wc][2] (semi-planar) or a Cb and a Cr plane [Hc][Wc] (planar), Hc x Wc = ceil(h/2) x ceil(w/2), every plane at any
// sample-aligned address and row pitch.  The chroma field of the descriptor's format (format = base | chroma << 4) names the
// other two sub-samplings: 4:2:2, Hc x Wc = h x ceil(w/2), and 4:4:4, h x w (planar alone); what they change is listed under
// "4:2:2 and 4:4:4" below, everything else is 4:2:0's.  A sample holds a level of d bits:
//   descriptor        format                         sample          level <-> sample
//   dvsr_yuv_desc     NV12 (semi) | I420 (planar)    a byte, d = 8   level = byte
//   dvsr_yuv16_desc   SEMI_MSB (P010 / P012)         a 16-bit word   word = level << (16 - d); the low bits: ignored in, 0 out
//   dvsr_yuv16_desc   PLANAR_LSB (yuv420p10le/12le)  a 16-bit word   word = level, & (2^d - 1);   the high bits: ignored in, 0 out
// 16-bit words are little-endian, d = 10 or 12 is an argument (a shift, a mask and the coefficients), not a template parameter.
// The network computes on fp32 planar RGB [3][Hp][Wp] in [0,1].
//
// The arithmetic (DESIGN 3.2k and 3.2m say the same), s = 2^(d-8):
//   matrix  BT601: Kr = 0.299, Kb = 0.114;  BT709: Kr = 0.2126, Kb = 0.0722;  BT2020NC: Kr = 0.2627, Kb = 0.0593;  Kg = 1 - Kr - Kb
//   range   H.273 at depth d.  LIMITED: y0 = 16 s, ys = 219 s, cs = 224 s;  FULL: y0 = 0, ys = cs = 2^d - 1;  chroma mid cm = 128 s
//   BT601 + LIMITED at d = 8 are the reference's ycbcr2rgb / rgb2ycbcr ("same as matlab", data/util.py:234-299).
//   siting  MPEG-2 / H.264 "left": chroma sample (j, k) sits on luma column 2k, midway between luma rows 2j and 2j+1.
//   ingest, per luma pixel (y, x) of the frame, C one of the two chroma planes (levels), j = y / 2:
//     Ch(j, x) = C[j][x/2] (x even) | (C[j][k] + C[j][min(k+1, Wc-1)]) / 2, k = (x-1)/2 (x odd)
//     C'       = 0.75 Ch(j, x) + 0.25 Ch(max(j-1, 0), x) (y even) | 0.75 Ch(j, x) + 0.25 Ch(min(j+1, Hc-1), x) (y odd)
//                (multiples of 1/8 of a level below 2^12: exact in fp32)
//     yn = (Y - y0) / ys, cb = (Cb' - cm) / cs, cr = (Cr' - cm) / cs
//     R = yn + 2(1-Kr) cr,  G = yn - (2 Kb (1-Kb) / Kg) cb - (2 Kr (1-Kr) / Kg) cr,  B = yn + 2(1-Kb) cb, each clamped to
//     [0,1]; nothing is rounded to d bits.  Output pixel (y, x) of the padded [3][Hp][Wp] tensor is the converted pixel at
//     (pad_index(y, h), pad_index(x, w)): ingest(yuv, pad) = F.pad(convert(yuv), .., mode).
//   emit, of the top-left h x w crop of fp32 planar [3][Hs][Ws]:
//     t = (clamp(v, lo, hi) - lo) / (hi - lo) per channel (quant.h's first line)
//     y = Kr R + Kg G + Kb B, cb = (B - y) / (2(1-Kb)), cr = (R - y) / (2(1-Kr))
//     luma level = clamp(rint(y0 + ys y), 0, 2^d - 1), round half to even
//     chroma sample (j, k): taps [1,2,1]/4 on columns 2k-1, 2k, 2k+1, the mean of rows 2j and min(2j+1, h-1), indices clamped to
//     the crop -- nothing outside it influences a sample; chroma level = clamp(rint(cm + cs c), 0, 2^d - 1)
//   The five quotients -- by ys, cs, 2(1-Kb), 2(1-Kr), hi - lo -- are IEEE divisions for bytes (hi - lo formed in fp32 on the
//   device) and multiplications by reciprocals formed on the host in double and rounded once to fp32 for 16-bit words: one more
//   rounding of 2^-24 relative per quotient, inside the tests' bars.  They differ in the last bit and in emitted
//   samples near ties, so they stay apart (Sample8::quot / Sample16::quot).
//   4:2:2 and 4:4:4: no vertical step either way.
//     siting  4:2:2: chroma sample (y, k) sits on luma row y, column 2k.  4:4:4: on its pixel.
//     ingest  4:2:2: C' = Ch(y, x), the horizontal line above on chroma row y.  4:4:4: C' = C[y][x].
//     emit    4:2:2: chroma sample (y, k) = taps [1,2,1]/4 on columns 2k-1, 2k, 2k+1 of row y, indices clamped to the crop.
//             4:4:4: the pixel's own cb, cr.
//
// One thread = a 4 x 2 luma block (two rows, four columns): one chroma row, two chroma columns, and the neighbours the filters
// need.  A workgroup is 64 x 4 threads, so a wave owns whole rows and whatever depends on a row's address is wave-uniform.
// The fp32 side moves as 16-byte accesses.  On the sample side a group of 4 (2) samples -- four luma samples, two CbCr pairs --
// moves as one access where its address is aligned to the group's size and in naturally aligned pieces otherwise: 1 + 2 + 1
// or 2 + 2 samples; the offset of a lane's group inside its row is a multiple of the group's size, so that choice is the row's:
// per wave.  No access is wider than its address is aligned (relaxed atomics of wavefront scope: plain accesses that are never
// merged into wider, possibly misaligned ones), no access is narrower than a sample, and nothing outside the rows of a plane is
// read or written.  Blocks that hold padded rows / columns or the ragged end of the frame work sample by sample.  Pure
// streaming: all of a lane's loads come ahead of its first store, no grid-stride loop (frame_io.hip).
// The sub-sampling is a compile-time axis CS of the one kernel pair, beside S and SEMI; the lane's 4 x 2 luma block stays.  Its
// chroma group is two rows of 2 samples (4:2:2 planar), two rows of two CbCr pairs (4:2:2 semi-planar) or two rows of 4 samples
// (4:4:4), each at the same multiple of its size inside its row as the 4:2:0 group, so the choice of pieces is still the row's.
// Every CS_420 line is the line it was: those instantiations compile to what they compiled to before the axis.
//
// Chroma siting is a fourth compile-time axis SITE, beside S, SEMI and CS, left by default; the chroma field of a
// descriptor's format names a pair of sub-sampling and siting, which yuv_frame_from splits.  Chroma sample (j, k) sits at luma
// position (4:2:2: y is the luma row itself)
//               x          y
//     left      2k         2j + 1/2
//     center    2k + 1/2   2j + 1/2
//     topleft   2k         2j
//   ingest  linear interpolation at the luma pixel's position, indices clamped to the plane, k = x >> 1, j = y >> 1:
//     horizontal H(j, x)   co-sited (left, topleft): Ch above
//                          center: 0.75 C[j][k] + 0.25 C[j][max(k-1, 0)] (x even) | 0.75 C[j][k] + 0.25 C[j][min(k+1, Wc-1)] (x odd)
//     vertical (4:2:0)     midway (left, center): 0.75 H(j) + 0.25 H(j -+ 1 clamped) above
//                          co-sited (topleft): H(j, x) (y even) | (H(j, x) + H(min(j+1, Hc-1), x)) / 2 (y odd)
//     (multiples of 1/16 of a level below 2^12: exact in fp32 in any evaluation order)
//   emit    filters centred on the chroma sample's position, indices clamped to the crop, on the per-pixel cb, cr:
//     horizontal           co-sited: [1,2,1]/4 on 2k-1, 2k, 2k+1 above;  center: the mean of columns 2k and min(2k+1, w-1)
//     vertical (4:2:0)     midway: the mean of rows 2j and min(2j+1, h-1) above
//                          co-sited: [1,2,1]/4 on rows max(2j-1, 0), 2j, min(2j+1, h-1)
//   The luma plane does not depend on siting.  What a lane reads beyond the left kernels: ingest center one more chroma column,
//   max(k0-1, 0), per chroma row; ingest topleft chroma rows j and min(j+1, Hc-1) only; emit topleft a third fp32 row,
//   max(y0-1, 0); emit center no left neighbour.  Every SITE_LEFT line is the line it was.  The new instantiations fuse the
//   products of the matrix step by name, as 4:2:2 and 4:4:4 do.
#include <cstdint>

#include "frame_common.h"
#include "frame_sample.h"

namespace dvsr {

constexpr int YUV_X = 64, YUV_Y = 4;   // threads of a workgroup along a row (one wave) / block rows of a workgroup
// the chroma sub-sampling CS of a kernel: the chroma field of a descriptor's format
constexpr int CS_420 = DVSR_YUV_CHROMA_420, CS_422 = DVSR_YUV_CHROMA_422, CS_444 = DVSR_YUV_CHROMA_444;
// the chroma siting SITE of a kernel (kernels.h: YuvFrame::siting)
constexpr int SITE_LEFT = YUV_SITE_LEFT, SITE_CENTER = YUV_SITE_CENTER, SITE_TOPLEFT = YUV_SITE_TOPLEFT;

// (what the 8-bit kernels read comes first and together: their scalar loads of it stay few)
struct YuvCoef {
  float y0, ys, cs;                 // luma offset, luma / chroma scale (levels)
  float kr, kg, kb;
  float r_cr, g_cb, g_cr, b_cb;     // 2(1-Kr), 2 Kb (1-Kb) / Kg, 2 Kr (1-Kr) / Kg, 2(1-Kb)
  float cm, top;                    // chroma mid, 2^d - 1 (levels)
  float inv_ys, inv_cs;             // (double) 1 / ys, 1 / cs
  float inv_r_cr, inv_b_cb;         // (double) 1 / (2(1-Kr)), 1 / (2(1-Kb))
};

struct YuvIngestArgs {
  const unsigned char* p[3];
  long long rs[3];                  // bytes
  float* dst;
  int h, w, Hp, Wp, pad;
  YuvCoef k;
  unsigned shift, mask;             // 16-bit words: level = (word >> shift) & mask
};

struct YuvEmitArgs {
  const float* src;
  unsigned char* p[3];
  long long rs[3];
  int Hs, Ws, h, w;
  float lo, inv_scale, hi;          // inv_scale = (double) 1 / (hi - lo)
  unsigned shift;                   // 16-bit words: word = level << shift
  YuvCoef k;
};

// ---- a sample trait S: the groups of frame_sample.h (B bytes per sample; ld1 / ld2 / ld4, st1 / st2 / st4 in naturally aligned
// pieces) with what a YCbCr level needs: lev(a, group, i), the level of sample i of a loaded group; word(a, level); the chroma
// midpoint; the quotient x / d given d and its reciprocal.

struct Sample8 : Bytes8 {
  // (a literal, as 255 is not: read from the argument struct it costs the planar ingest kernel 35 VGPRs and a wave of occupancy)
  static __device__ __forceinline__ float cm(const YuvCoef&) { return 128.0f; }
  static __device__ __forceinline__ float quot(float x, float d, float) { return x / d; }   // IEEE division
  static __device__ __forceinline__ float lev(const YuvIngestArgs&, unsigned v, int i) { return (float)((v >> (8 * i)) & 0xffu); }
  static __device__ __forceinline__ float lev(const YuvIngestArgs& a, const G4& g, int i) { return lev(a, g.d[0], i); }
  static __device__ __forceinline__ unsigned word(const YuvEmitArgs&, unsigned level) { return level; }
};

struct Sample16 : Words16 {
  static __device__ __forceinline__ float cm(const YuvCoef& k) { return k.cm; }
  static __device__ __forceinline__ float quot(float x, float, float inv) { return x * inv; }
  static __device__ __forceinline__ float lev(const YuvIngestArgs& a, unsigned v, int i) {   // the two words of a dword
    return i ? (float)((v >> (16 + a.shift)) & a.mask) : (float)(((v & 0xffffu) >> a.shift) & a.mask);
  }
  static __device__ __forceinline__ float lev(const YuvIngestArgs& a, const G4& g, int i) { return lev(a, g.d[i >> 1], i & 1); }
  static __device__ __forceinline__ unsigned word(const YuvEmitArgs& a, unsigned level) { return level << a.shift; }
};

// chroma sample (j, k) of both planes
template <class S, bool SEMI>
__device__ __forceinline__ void chroma1(const YuvIngestArgs& a, int j, int k, float& cb, float& cr) {
  if (SEMI) {
    const unsigned v = S::ld2(a.p[1] + (long long)j * a.rs[1] + 2 * S::B * k);
    cb = S::lev(a, v, 0);
    cr = S::lev(a, v, 1);
  } else {
    cb = S::lev(a, S::ld1(a.p[1] + (long long)j * a.rs[1] + S::B * k), 0);
    cr = S::lev(a, S::ld1(a.p[2] + (long long)j * a.rs[2] + S::B * k), 0);
  }
}

// chroma samples (j, k0), (j, k0 + 1), (j, k2) of both planes; k0 is even and k0 + 1 < Wc
template <class S, bool SEMI>
__device__ __forceinline__ void chroma3(const YuvIngestArgs& a, int j, int k0, int k2, float cb[3], float cr[3]) {
  if (SEMI) {
    const typename S::G4 g = S::ld4(a.p[1] + (long long)j * a.rs[1] + 2 * S::B * k0);
    cb[0] = S::lev(a, g, 0);
    cr[0] = S::lev(a, g, 1);
    cb[1] = S::lev(a, g, 2);
    cr[1] = S::lev(a, g, 3);
  } else {
    const unsigned u = S::ld2(a.p[1] + (long long)j * a.rs[1] + S::B * k0), v = S::ld2(a.p[2] + (long long)j * a.rs[2] + S::B * k0);
    cb[0] = S::lev(a, u, 0);
    cb[1] = S::lev(a, u, 1);
    cr[0] = S::lev(a, v, 0);
    cr[1] = S::lev(a, v, 1);
  }
  chroma1<S, SEMI>(a, j, k2, cb[2], cr[2]);
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// the horizontal step of a block inside the frame, SITE_CENTER and SITE_TOPLEFT: chroma columns k0, k0 + 1, k2 (c) and
// max(k0 - 1, 0) (cm, center alone) of one chroma row -> luma columns x0 .. x0 + 3
template <int SITE>
__device__ __forceinline__ void chroma_h4(const float c[3], float cm, float h[4]) {
  if constexpr (SITE == SITE_CENTER) {
    h[0] = 0.75f * c[0] + 0.25f * cm;
    h[1] = 0.75f * c[0] + 0.25f * c[1];
    h[2] = 0.75f * c[1] + 0.25f * c[0];
    h[3] = 0.75f * c[1] + 0.25f * c[2];
  } else {
    h[0] = c[0];
    h[1] = (c[0] + c[1]) * 0.5f;
    h[2] = c[1];
    h[3] = (c[1] + c[2]) * 0.5f;
  }
}

// SITE_CENTER and SITE_TOPLEFT: the second chroma column / row of luma index s whose first is s >> 1 (n: of the plane), and the
// weight of the first -- center and midway 0.75, co-sited 0.5 (an even co-sited index is its own neighbour)
template <bool COSITED>
__device__ __forceinline__ int chroma_other(int s, int n) {
  const int k = s >> 1;
  return (s & 1) ? min(k + 1, n - 1) : (COSITED ? k : max(k - 1, 0));
}
template <bool COSITED>
constexpr float chroma_weight() { return COSITED ? 0.5f : 0.75f; }

// 4:2:0, SITE_CENTER and SITE_TOPLEFT: the chroma of a 4 x 2 block inside the frame, on the luma grid
template <class S, bool SEMI, int SITE>
__device__ __forceinline__ void chroma_block_sited(const YuvIngestArgs& a, int x0, int y0, int Hc, int Wc, float Cb[2][4], float Cr[2][4]) {
  constexpr bool TOP = SITE == SITE_TOPLEFT;
  constexpr int NR = TOP ? 2 : 3;      // chroma rows read: j, j + 1 (co-sited) | j - 1, j, j + 1 (midway), clamped
  const int j = y0 >> 1, k0 = x0 >> 1, k2 = min(k0 + 2, Wc - 1), km = max(k0 - 1, 0);
  float cb[NR][3], cr[NR][3], lb[NR], lr[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int jr = TOP ? min(j + r, Hc - 1) : min(max(j - 1 + r, 0), Hc - 1);
    chroma3<S, SEMI>(a, jr, k0, k2, cb[r], cr[r]);
    if constexpr (SITE == SITE_CENTER) chroma1<S, SEMI>(a, jr, km, lb[r], lr[r]);
    else lb[r] = lr[r] = 0.0f;         // (not read)
  }
  float hb[NR][4], hr[NR][4];          // the horizontal step, per chroma row
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    chroma_h4<SITE>(cb[r], lb[r], hb[r]);
    chroma_h4<SITE>(cr[r], lr[r], hr[r]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (TOP) {
      Cb[0][i] = hb[0][i];
      Cb[1][i] = (hb[0][i] + hb[1][i]) * 0.5f;
      Cr[0][i] = hr[0][i];
      Cr[1][i] = (hr[0][i] + hr[1][i]) * 0.5f;
    } else {
      Cb[0][i] = 0.75f * hb[1][i] + 0.25f * hb[0][i];
      Cb[1][i] = 0.75f * hb[1][i] + 0.25f * hb[2][i];
      Cr[0][i] = 0.75f * hr[1][i] + 0.25f * hr[0][i];
      Cr[1][i] = 0.75f * hr[1][i] + 0.25f * hr[2][i];
    }
  }
}

// 4:2:2 and 4:4:4: the chroma of a 4 x 2 block inside the frame, on the luma grid -- each luma row has its own chroma row
template <class S, bool SEMI, int CS, int SITE>
__device__ __forceinline__ void chroma_rows(const YuvIngestArgs& a, int x0, int y0, float Cb[2][4], float Cr[2][4]) {
  if constexpr (CS == CS_422 && SITE == SITE_CENTER) {
    const int Wc = (a.w + 1) >> 1, k0 = x0 >> 1, k2 = min(k0 + 2, Wc - 1), km = max(k0 - 1, 0);
    float cb[2][3], cr[2][3], lb[2], lr[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      chroma3<S, SEMI>(a, y0 + r, k0, k2, cb[r], cr[r]);
      chroma1<S, SEMI>(a, y0 + r, km, lb[r], lr[r]);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      chroma_h4<SITE>(cb[r], lb[r], Cb[r]);
      chroma_h4<SITE>(cr[r], lr[r], Cr[r]);
    }
  } else if constexpr (CS == CS_422) {
    // columns x0 .. x0 + 3 lie on chroma columns k0, k0 + 1 and reach to k0 + 2 for the last (odd) one
    const int Wc = (a.w + 1) >> 1, k0 = x0 >> 1, k2 = min(k0 + 2, Wc - 1);
    float cb[2][3], cr[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r) chroma3<S, SEMI>(a, y0 + r, k0, k2, cb[r], cr[r]);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      Cb[r][0] = cb[r][0];
      Cb[r][1] = (cb[r][0] + cb[r][1]) * 0.5f;
      Cb[r][2] = cb[r][1];
      Cb[r][3] = (cb[r][1] + cb[r][2]) * 0.5f;
      Cr[r][0] = cr[r][0];
      Cr[r][1] = (cr[r][0] + cr[r][1]) * 0.5f;
      Cr[r][2] = cr[r][1];
      Cr[r][3] = (cr[r][1] + cr[r][2]) * 0.5f;
    }
  } else {
    static_assert(CS == CS_444 && !SEMI, "4:4:4 is planar");
    typename S::G4 gb[2], gr[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      gb[r] = S::ld4(a.p[1] + (long long)(y0 + r) * a.rs[1] + S::B * x0);
      gr[r] = S::ld4(a.p[2] + (long long)(y0 + r) * a.rs[2] + S::B * x0);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Cb[r][i] = S::lev(a, gb[r], i);
        Cr[r][i] = S::lev(a, gr[r], i);
      }
  }
}

template <class S, bool SEMI, int CS, int SITE = SITE_LEFT>
__global__ __launch_bounds__(YUV_X * YUV_Y) void frame_ingest_yuv_kernel(YuvIngestArgs a) {
  static_assert(SITE == SITE_LEFT || CS == CS_420 || (CS == CS_422 && SITE == SITE_CENTER), "a siting of this sub-sampling");
  const int x0 = (blockIdx.x * YUV_X + threadIdx.x) * 4;
  const int y0 = (blockIdx.y * YUV_Y + threadIdx.y) * 2;
  if (x0 >= a.Wp || y0 >= a.Hp) return;
  const int Hc = (a.h + 1) >> 1, Wc = (a.w + 1) >> 1;   // (Hc: of 4:2:0; Wc: of 4:2:0 and 4:2:2)
  float Y[2][4], Cb[2][4], Cr[2][4];   // levels: luma as stored, chroma upsampled to the luma grid
  if constexpr (CS != CS_420) {
    if (x0 + 3 < a.w && y0 + 1 < a.h) {
      typename S::G4 yl[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) yl[r] = S::ld4(a.p[0] + (long long)(y0 + r) * a.rs[0] + S::B * x0);
      chroma_rows<S, SEMI, CS, SITE>(a, x0, y0, Cb, Cr);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) Y[r][i] = S::lev(a, yl[r], i);
    } else {
      // padded rows / columns, the ragged end of a row, the last row of an odd height: sample by sample, every index clamped
      float cbv[2][4][2], crv[2][4][2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int sy = pad_index(min(y0 + r, a.Hp - 1), a.h, a.pad);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int sx = pad_index(x0 + i, a.w, a.pad);
          Y[r][i] = S::lev(a, S::ld1(a.p[0] + (long long)sy * a.rs[0] + S::B * sx), 0);
          // 4:2:2: the two chroma columns of Ch(sy, sx); 4:4:4: the pixel's own sample, as both
          const int ka = CS == CS_422 ? sx >> 1 : sx;
          chroma1<S, SEMI>(a, sy, ka, cbv[r][i][0], crv[r][i][0]);
          if constexpr (CS == CS_422 && SITE == SITE_CENTER) {
            chroma1<S, SEMI>(a, sy, chroma_other<false>(sx, Wc), cbv[r][i][1], crv[r][i][1]);
          } else if constexpr (CS == CS_422) {
            chroma1<S, SEMI>(a, sy, (sx & 1) ? min(ka + 1, Wc - 1) : ka, cbv[r][i][1], crv[r][i][1]);
          } else {
            cbv[r][i][1] = cbv[r][i][0];
            crv[r][i][1] = crv[r][i][0];
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if constexpr (SITE == SITE_CENTER) {
            Cb[r][i] = 0.75f * cbv[r][i][0] + 0.25f * cbv[r][i][1];
            Cr[r][i] = 0.75f * crv[r][i][0] + 0.25f * crv[r][i][1];
          } else {
            Cb[r][i] = (cbv[r][i][0] + cbv[r][i][1]) * 0.5f;   // (4:4:4: (c + c) / 2 = c, exactly)
            Cr[r][i] = (crv[r][i][0] + crv[r][i][1]) * 0.5f;
          }
        }
    }
  } else if (SITE != SITE_LEFT && x0 + 3 < a.w && y0 + 1 < a.h) {
    if constexpr (SITE != SITE_LEFT) {
      typename S::G4 yl[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) yl[r] = S::ld4(a.p[0] + (long long)(y0 + r) * a.rs[0] + S::B * x0);
      chroma_block_sited<S, SEMI, SITE>(a, x0, y0, Hc, Wc, Cb, Cr);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) Y[r][i] = S::lev(a, yl[r], i);
    }
  } else if (SITE != SITE_LEFT) {
    // ... and its blocks with padded rows / columns or a ragged end: sample by sample, every index clamped
    if constexpr (SITE != SITE_LEFT) {
      constexpr bool CO_X = SITE != SITE_CENTER, CO_Y = SITE == SITE_TOPLEFT;   // co-sited with a luma column / row
      constexpr float WX = chroma_weight<CO_X>(), WY = chroma_weight<CO_Y>();
      float cbv[2][4][4], crv[2][4][4];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int sy = pad_index(min(y0 + r, a.Hp - 1), a.h, a.pad);
        const int j = sy >> 1, jn = chroma_other<CO_Y>(sy, Hc);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int sx = pad_index(x0 + i, a.w, a.pad);
          const int ka = sx >> 1, kb = chroma_other<CO_X>(sx, Wc);
          Y[r][i] = S::lev(a, S::ld1(a.p[0] + (long long)sy * a.rs[0] + S::B * sx), 0);
          chroma1<S, SEMI>(a, j, ka, cbv[r][i][0], crv[r][i][0]);
          chroma1<S, SEMI>(a, j, kb, cbv[r][i][1], crv[r][i][1]);
          chroma1<S, SEMI>(a, jn, ka, cbv[r][i][2], crv[r][i][2]);
          chroma1<S, SEMI>(a, jn, kb, cbv[r][i][3], crv[r][i][3]);
        }
      }
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          Cb[r][i] = WY * (WX * cbv[r][i][0] + (1.0f - WX) * cbv[r][i][1]) + (1.0f - WY) * (WX * cbv[r][i][2] + (1.0f - WX) * cbv[r][i][3]);
          Cr[r][i] = WY * (WX * crv[r][i][0] + (1.0f - WX) * crv[r][i][1]) + (1.0f - WY) * (WX * crv[r][i][2] + (1.0f - WX) * crv[r][i][3]);
        }
    }
  } else if (x0 + 3 < a.w && y0 + 1 < a.h) {
    // a block inside the frame: luma rows y0, y0 + 1 share chroma row j; its columns x0 .. x0 + 3 lie on chroma columns
    // k0, k0 + 1 and reach to k0 + 2 for the last (odd) one
    const int j = y0 >> 1, k0 = x0 >> 1, k2 = min(k0 + 2, Wc - 1);
    const int jr[3] = {max(j - 1, 0), j, min(j + 1, Hc - 1)};
    typename S::G4 yl[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) yl[r] = S::ld4(a.p[0] + (long long)(y0 + r) * a.rs[0] + S::B * x0);
    float cb[3][3], cr[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) chroma3<S, SEMI>(a, jr[r], k0, k2, cb[r], cr[r]);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) Y[r][i] = S::lev(a, yl[r], i);
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
      const int sy = pad_index(min(y0 + r, a.Hp - 1), a.h, a.pad);
      const int j = sy >> 1, jn = (sy & 1) ? min(j + 1, Hc - 1) : max(j - 1, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int sx = pad_index(x0 + i, a.w, a.pad);
        const int ka = sx >> 1, kb = (sx & 1) ? min(ka + 1, Wc - 1) : ka;
        Y[r][i] = S::lev(a, S::ld1(a.p[0] + (long long)sy * a.rs[0] + S::B * sx), 0);
        chroma1<S, SEMI>(a, j, ka, cbv[r][i][0], crv[r][i][0]);
        chroma1<S, SEMI>(a, j, kb, cbv[r][i][1], crv[r][i][1]);
        chroma1<S, SEMI>(a, jn, ka, cbv[r][i][2], crv[r][i][2]);
        chroma1<S, SEMI>(a, jn, kb, cbv[r][i][3], crv[r][i][3]);
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
      const float yn = S::quot(Y[r][i] - a.k.y0, a.k.ys, a.k.inv_ys), cb = S::quot(Cb[r][i] - S::cm(a.k), a.k.cs, a.k.inv_cs),
                  cr = S::quot(Cr[r][i] - S::cm(a.k), a.k.cs, a.k.inv_cs);
      if constexpr (CS == CS_420 && SITE == SITE_LEFT) {
        o[r][0][i] = clamp01(yn + a.k.r_cr * cr);
        o[r][1][i] = clamp01(yn - a.k.g_cb * cb - a.k.g_cr * cr);
        o[r][2][i] = clamp01(yn + a.k.b_cb * cb);
      } else {
        // the same lines with every product fused by name: which products the compiler fuses on its own differs between
        // instantiations (packed math), and a planar and a semi-planar frame of the same levels give the same bits
        o[r][0][i] = clamp01(fmaf(a.k.r_cr, cr, yn));
        o[r][1][i] = clamp01(fmaf(-a.k.g_cr, cr, fmaf(-a.k.g_cb, cb, yn)));
        o[r][2][i] = clamp01(fmaf(a.k.b_cb, cb, yn));
      }
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

__device__ __forceinline__ unsigned quant_level(float v, float top) { return (unsigned)(int)fminf(fmaxf(rintf(v), 0.0f), top); }

// this lane's two chroma columns of chroma row j, as they are stored (4:2:0 and 4:2:2)
template <class S, bool SEMI>
__device__ __forceinline__ void store_chroma2(const YuvEmitArgs& a, int j, int x0, const unsigned (&cbw)[2], const unsigned (&crw)[2]) {
  const bool two = x0 + 2 < a.w;        // this lane's second chroma column exists
  if (SEMI) {
    unsigned char* q = a.p[1] + (long long)j * a.rs[1] + S::B * x0;   // pair k0 = x0 / 2 is 2 k0 samples into the row
    const unsigned s[4] = {cbw[0], crw[0], cbw[1], crw[1]};
    if (two) S::st4(q, s);
    else S::st2(q, s);
  } else {
    unsigned char* qb = a.p[1] + (long long)j * a.rs[1] + S::B * (x0 >> 1);
    unsigned char* qr = a.p[2] + (long long)j * a.rs[2] + S::B * (x0 >> 1);
    if (two) {
      S::st2(qb, cbw);
      S::st2(qr, crw);
    } else {
      S::st1(qb, cbw[0]);
      S::st1(qr, crw[0]);
    }
  }
}

template <class S, bool SEMI, int CS, int SITE = SITE_LEFT>
__global__ __launch_bounds__(YUV_X * YUV_Y) void frame_emit_yuv_kernel(YuvEmitArgs a) {
  static_assert(CS != CS_444 || !SEMI, "4:4:4 is planar");
  static_assert(SITE == SITE_LEFT || CS == CS_420 || (CS == CS_422 && SITE == SITE_CENTER), "a siting of this sub-sampling");
  // SITE_TOPLEFT: a third row, max(y0 - 1, 0), for the vertical taps; SITE_CENTER: no left neighbour, as 4:4:4
  constexpr int NR = SITE == SITE_TOPLEFT ? 3 : 2;
  constexpr bool NO_LEFT = CS == CS_444 || SITE == SITE_CENTER;
  const int x0 = (blockIdx.x * YUV_X + threadIdx.x) * 4;
  const int y0 = (blockIdx.y * YUV_Y + threadIdx.y) * 2;
  if (x0 >= a.w || y0 >= a.h) return;
  // rows y0 and min(y0 + 1, h - 1); columns max(x0 - 1, 0) and x0 .. x0 + 3 (x0 + 3 < Ws: Ws is a multiple of 4, x0 < w <= Ws)
  const long long plane = (long long)a.Hs * a.Ws;
  const int yr[3] = {y0, min(y0 + 1, a.h - 1), max(y0 - 1, 0)}, xl = max(x0 - 1, 0);
  f32x4 v[NR][3];
  float l[NR][3];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const float* row = a.src + (long long)yr[r] * a.Ws;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[r][c] = *reinterpret_cast<const f32x4*>(row + c * plane + x0);
      if constexpr (NO_LEFT) l[r][c] = 0.0f;   // (no filter, no left neighbour: what comes of it below is dropped)
      else l[r][c] = row[c * plane + xl];
    }
  }
  const float scale = a.hi - a.lo;
  float yv[NR][4], cbv[NR][5], crv[NR][5];   // column index 0 of cbv / crv is the left neighbour (yv of the third row: dropped)
#pragma unroll
  for (int r = 0; r < NR; ++r)
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
        t[c] = S::quot(fminf(fmaxf(s, a.lo), a.hi) - a.lo, scale, a.inv_scale);
      }
      const float y = a.k.kr * t[0] + a.k.kg * t[1] + a.k.kb * t[2];
      cbv[r][i] = S::quot(t[2] - y, a.k.b_cb, a.k.inv_b_cb);
      crv[r][i] = S::quot(t[0] - y, a.k.r_cr, a.k.inv_r_cr);
      if (i > 0) yv[r][i - 1] = y;
    }
  constexpr int CR = CS == CS_420 ? 1 : 2, CK = CS == CS_444 ? 4 : 2;   // this lane's chroma rows, samples of one
  unsigned yw[2][4], cbw[CR][CK], crw[CR][CK];   // samples as they are stored
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) yw[r][i] = S::word(a, quant_level(a.k.y0 + a.k.ys * yv[r][i], a.k.top));
  if constexpr (CS == CS_420) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = 2 * k;               // columns 2k - 1, 2k, 2k + 1 of this lane's chroma column k
      if constexpr (SITE == SITE_LEFT) {
        const float fb = 0.5f * (0.25f * (cbv[0][i] + 2.0f * cbv[0][i + 1] + cbv[0][i + 2]) +
                                 0.25f * (cbv[1][i] + 2.0f * cbv[1][i + 1] + cbv[1][i + 2]));
        const float fr = 0.5f * (0.25f * (crv[0][i] + 2.0f * crv[0][i + 1] + crv[0][i + 2]) +
                                 0.25f * (crv[1][i] + 2.0f * crv[1][i + 1] + crv[1][i + 2]));
        cbw[0][k] = S::word(a, quant_level(S::cm(a.k) + a.k.cs * fb, a.k.top));
        crw[0][k] = S::word(a, quant_level(S::cm(a.k) + a.k.cs * fr, a.k.top));
      } else {
        float fb, fr;
        if constexpr (SITE == SITE_CENTER) {   // columns 2k, 2k + 1 of rows 2j, 2j + 1
          fb = 0.5f * (0.5f * (cbv[0][i + 1] + cbv[0][i + 2]) + 0.5f * (cbv[1][i + 1] + cbv[1][i + 2]));
          fr = 0.5f * (0.5f * (crv[0][i + 1] + crv[0][i + 2]) + 0.5f * (crv[1][i + 1] + crv[1][i + 2]));
        } else {                               // the same columns of rows 2j - 1 (index 2), 2j, 2j + 1
          float hb[3], hr[3];
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            hb[r] = 0.25f * (cbv[r][i] + 2.0f * cbv[r][i + 1] + cbv[r][i + 2]);
            hr[r] = 0.25f * (crv[r][i] + 2.0f * crv[r][i + 1] + crv[r][i + 2]);
          }
          fb = 0.25f * (hb[2] + 2.0f * hb[0] + hb[1]);
          fr = 0.25f * (hr[2] + 2.0f * hr[0] + hr[1]);
        }
        cbw[0][k] = S::word(a, quant_level(fmaf(a.k.cs, fb, S::cm(a.k)), a.k.top));
        crw[0][k] = S::word(a, quant_level(fmaf(a.k.cs, fr, S::cm(a.k)), a.k.top));
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int k = 0; k < CK; ++k) {
        if constexpr (SITE == SITE_CENTER) {   // 4:2:2: columns 2k, 2k + 1 of row r
          const float fb = 0.5f * (cbv[r][2 * k + 1] + cbv[r][2 * k + 2]), fr = 0.5f * (crv[r][2 * k + 1] + crv[r][2 * k + 2]);
          cbw[r][k] = S::word(a, quant_level(fmaf(a.k.cs, fb, S::cm(a.k)), a.k.top));
          crw[r][k] = S::word(a, quant_level(fmaf(a.k.cs, fr, S::cm(a.k)), a.k.top));
        } else {
          // 4:2:2: the same columns, of row r alone; 4:4:4: the pixel's own
          const float fb = CS == CS_444 ? cbv[r][k + 1] : 0.25f * (cbv[r][2 * k] + 2.0f * cbv[r][2 * k + 1] + cbv[r][2 * k + 2]);
          const float fr = CS == CS_444 ? crv[r][k + 1] : 0.25f * (crv[r][2 * k] + 2.0f * crv[r][2 * k + 1] + crv[r][2 * k + 2]);
          cbw[r][k] = S::word(a, quant_level(S::cm(a.k) + a.k.cs * fb, a.k.top));
          crw[r][k] = S::word(a, quant_level(S::cm(a.k) + a.k.cs * fr, a.k.top));
        }
      }
  }
  // ---- stores
#pragma unroll
  for (int r = 0; r < 2; ++r)
    if (y0 + r < a.h) {
      unsigned char* q = a.p[0] + (long long)(y0 + r) * a.rs[0] + S::B * x0;
      if (x0 + 3 < a.w) {
        S::st4(q, yw[r]);
      } else {
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (x0 + i < a.w) S::st1(q + S::B * i, yw[r][i]);
      }
    }
  if constexpr (CS == CS_444) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if (y0 + r < a.h) {                 // a chroma row is stored like the luma row it belongs to
        unsigned char* qb = a.p[1] + (long long)(y0 + r) * a.rs[1] + S::B * x0;
        unsigned char* qr = a.p[2] + (long long)(y0 + r) * a.rs[2] + S::B * x0;
        if (x0 + 3 < a.w) {
          S::st4(qb, cbw[r]);
          S::st4(qr, crw[r]);
        } else {
#pragma unroll
          for (int i = 0; i < 3; ++i)
            if (x0 + i < a.w) {
              S::st1(qb + S::B * i, cbw[r][i]);
              S::st1(qr + S::B * i, crw[r][i]);
            }
        }
      }
  } else if constexpr (CS == CS_422) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if (y0 + r < a.h) store_chroma2<S, SEMI>(a, y0 + r, x0, cbw[r], crw[r]);   // the chroma row of luma row y0 + r
  } else {
    store_chroma2<S, SEMI>(a, y0 >> 1, x0, cbw[0], crw[0]);
  }
}

// ---- the host side, on the one internal frame (kernels.h: YuvFrame)

// format = base | chroma << 4: a known pair (base 0 is the semi-planar form of either descriptor, 1 the planar one)?  The chroma
// field names a sub-sampling and a siting: 3, 7 and above and any bit above bit 7 name none.
static bool yuv_format_known(int format) {
  const int base = format & 15, chroma = format >> 4;
  return format >= 0 && base <= 1 && chroma <= DVSR_YUV_CHROMA_422_CENTER && chroma != 3;
}

// the sub-sampling / the siting of the chroma field of a known format
static int yuv_chroma_of(int format) {
  const int c = format >> 4;
  if (c == DVSR_YUV_CHROMA_420_CENTER || c == DVSR_YUV_CHROMA_420_TOPLEFT) return DVSR_YUV_CHROMA_420;
  return c == DVSR_YUV_CHROMA_422_CENTER ? DVSR_YUV_CHROMA_422 : c;
}
static int yuv_siting_of(int format) {
  const int c = format >> 4;
  if (c == DVSR_YUV_CHROMA_420_CENTER || c == DVSR_YUV_CHROMA_422_CENTER) return YUV_SITE_CENTER;
  return c == DVSR_YUV_CHROMA_420_TOPLEFT ? YUV_SITE_TOPLEFT : YUV_SITE_LEFT;
}

int yuv_frame_from(const char* what, const dvsr_yuv_desc* d, YuvFrame* f) {
  DVSR_REQUIRE(d, DVSR_ERR_INVALID, "%s: null descriptor", what);
  DVSR_REQUIRE(yuv_format_known(d->format), DVSR_ERR_INVALID, "%s: unknown YUV format %d", what, d->format);
  DVSR_REQUIRE(d->format != DVSR_YUV_FORMAT(DVSR_YUV_NV12, DVSR_YUV_CHROMA_444), DVSR_ERR_INVALID,
               "%s: YUV format %d, semi-planar 4:4:4, is not provided", what, d->format);
  *f = YuvFrame{{d->plane[0], d->plane[1], d->plane[2]}, {d->row_stride[0], d->row_stride[1], d->row_stride[2]},
                d->h, d->w, d->matrix, d->range, (d->format & 15) == DVSR_YUV_NV12, 1, 8, yuv_chroma_of(d->format), yuv_siting_of(d->format)};
  return DVSR_OK;
}

int yuv_frame_from(const char* what, const dvsr_yuv16_desc* d, YuvFrame* f) {
  DVSR_REQUIRE(d, DVSR_ERR_INVALID, "%s: null descriptor", what);
  DVSR_REQUIRE(yuv_format_known(d->format), DVSR_ERR_INVALID, "%s: unknown 16-bit YUV format %d", what, d->format);
  DVSR_REQUIRE(d->format != DVSR_YUV_FORMAT(DVSR_YUV16_SEMI_MSB, DVSR_YUV_CHROMA_444), DVSR_ERR_INVALID,
               "%s: 16-bit YUV format %d, semi-planar 4:4:4, is not provided", what, d->format);
  DVSR_REQUIRE(d->depth == 10 || d->depth == 12, DVSR_ERR_INVALID, "%s: unknown depth %d (10 or 12)", what, d->depth);
  *f = YuvFrame{{d->plane[0], d->plane[1], d->plane[2]}, {d->row_stride[0], d->row_stride[1], d->row_stride[2]},
                d->h, d->w, d->matrix, d->range, (d->format & 15) == DVSR_YUV16_SEMI_MSB, 2, d->depth, yuv_chroma_of(d->format),
                yuv_siting_of(d->format)};
  return DVSR_OK;
}

// (arguments checked by yuv_frame_check)
static YuvCoef yuv_coef(const YuvFrame& f) {
  const bool bt709 = f.matrix == DVSR_YUV_BT709, bt2020 = f.matrix == DVSR_YUV_BT2020NC, full = f.range == DVSR_YUV_FULL;
  const double kr = bt2020 ? 0.2627 : bt709 ? 0.2126 : 0.299, kb = bt2020 ? 0.0593 : bt709 ? 0.0722 : 0.114, kg = 1.0 - kr - kb;
  const double s = (double)(1 << (f.depth - 8)), top = (double)((1 << f.depth) - 1);
  const double y0 = full ? 0.0 : 16.0 * s, ys = full ? top : 219.0 * s, cs = full ? top : 224.0 * s, cm = 128.0 * s;
  const double r_cr = 2.0 * (1.0 - kr), b_cb = 2.0 * (1.0 - kb);
  return YuvCoef{(float)y0, (float)ys, (float)cs, (float)kr, (float)kg, (float)kb, (float)r_cr,
                 (float)(2.0 * kb * (1.0 - kb) / kg), (float)(2.0 * kr * (1.0 - kr) / kg), (float)b_cb, (float)cm, (float)top,
                 (float)(1.0 / ys), (float)(1.0 / cs), (float)(1.0 / r_cr), (float)(1.0 / b_cb)};
}

// the frame on the "any address, any pitch" side, against the h x w it may have at most
static int yuv_frame_check(const char* what, const YuvFrame& f, int Ht, int Wt) {
  DVSR_REQUIRE(f.matrix == DVSR_YUV_BT601 || f.matrix == DVSR_YUV_BT709 || f.matrix == DVSR_YUV_BT2020NC, DVSR_ERR_INVALID,
               "%s: unknown YUV matrix %d", what, f.matrix);
  DVSR_REQUIRE(f.range == DVSR_YUV_LIMITED || f.range == DVSR_YUV_FULL, DVSR_ERR_INVALID, "%s: unknown YUV range %d", what,
               f.range);
  DVSR_REQUIRE(f.h >= 1 && f.w >= 1 && f.h <= Ht && f.w <= Wt, DVSR_ERR_INVALID,
               "%s: frame size h=%d w=%d outside [1, %d] x [1, %d]", what, f.h, f.w, Ht, Wt);
  const long long Wc = f.chroma == DVSR_YUV_CHROMA_444 ? f.w : (f.w + 1) / 2;   // samples of a chroma row, per plane
  for (int i = 0; i < (f.semi ? 2 : 3); ++i) {   // (the two "16-bit samples" checks cannot fail for bytes: % 1)
    DVSR_REQUIRE(f.plane[i], DVSR_ERR_INVALID, "%s: null plane %d", what, i);
    DVSR_REQUIRE(reinterpret_cast<uintptr_t>(f.plane[i]) % f.bytes == 0, DVSR_ERR_INVALID,
                 "%s: odd address of plane %d (16-bit samples)", what, i);
    const long long need = f.bytes * (i == 0 ? f.w : (f.semi ? 2 * Wc : Wc));
    DVSR_REQUIRE(f.rs[i] >= need, DVSR_ERR_INVALID, "%s: row stride %lld of plane %d shorter than a row of %lld bytes", what,
                 f.rs[i], i, need);
    DVSR_REQUIRE(f.rs[i] % f.bytes == 0, DVSR_ERR_INVALID, "%s: odd row stride %lld of plane %d (16-bit samples)", what, f.rs[i], i);
  }
  return DVSR_OK;
}

// a workgroup covers 2 * YUV_Y rows
static dim3 yuv_grid(int h, int w) { return dim3(ceil_div(ceil_div(w, 4), YUV_X), ceil_div(ceil_div(h, 2), YUV_Y)); }

// the instantiation that takes a frame
template <int CS, int SITE = SITE_LEFT>
static auto ingest_kernel_of(const YuvFrame& f) {
  if (f.bytes == 2)
    return f.semi ? frame_ingest_yuv_kernel<Sample16, true, CS, SITE> : frame_ingest_yuv_kernel<Sample16, false, CS, SITE>;
  return f.semi ? frame_ingest_yuv_kernel<Sample8, true, CS, SITE> : frame_ingest_yuv_kernel<Sample8, false, CS, SITE>;
}
template <int CS, int SITE = SITE_LEFT>
static auto emit_kernel_of(const YuvFrame& f) {
  if (f.bytes == 2) return f.semi ? frame_emit_yuv_kernel<Sample16, true, CS, SITE> : frame_emit_yuv_kernel<Sample16, false, CS, SITE>;
  return f.semi ? frame_emit_yuv_kernel<Sample8, true, CS, SITE> : frame_emit_yuv_kernel<Sample8, false, CS, SITE>;
}
// (the pairs of sub-sampling and siting that yuv_frame_from lets through: 4:2:0 x 3, 4:2:2 x {left, center}, 4:4:4)
static auto ingest_kernel(const YuvFrame& f) {
  if (f.chroma == CS_444)   // (planar alone: yuv_frame_from)
    return f.bytes == 2 ? frame_ingest_yuv_kernel<Sample16, false, CS_444> : frame_ingest_yuv_kernel<Sample8, false, CS_444>;
  if (f.chroma == CS_422) return f.siting == SITE_CENTER ? ingest_kernel_of<CS_422, SITE_CENTER>(f) : ingest_kernel_of<CS_422>(f);
  if (f.siting == SITE_CENTER) return ingest_kernel_of<CS_420, SITE_CENTER>(f);
  return f.siting == SITE_TOPLEFT ? ingest_kernel_of<CS_420, SITE_TOPLEFT>(f) : ingest_kernel_of<CS_420>(f);
}
static auto emit_kernel(const YuvFrame& f) {
  if (f.chroma == CS_444)
    return f.bytes == 2 ? frame_emit_yuv_kernel<Sample16, false, CS_444> : frame_emit_yuv_kernel<Sample8, false, CS_444>;
  if (f.chroma == CS_422) return f.siting == SITE_CENTER ? emit_kernel_of<CS_422, SITE_CENTER>(f) : emit_kernel_of<CS_422>(f);
  if (f.siting == SITE_CENTER) return emit_kernel_of<CS_420, SITE_CENTER>(f);
  return f.siting == SITE_TOPLEFT ? emit_kernel_of<CS_420, SITE_TOPLEFT>(f) : emit_kernel_of<CS_420>(f);
}

int frame_ingest_yuv_check(const char* what, const YuvFrame& f, const float* dst, int Hp, int Wp, int pad_mode) {
  int rc = frame_planar_check(what, dst, Hp, Wp, 2 * YUV_Y);
  if (rc != DVSR_OK) return rc;
  rc = yuv_frame_check(what, f, Hp, Wp);
  if (rc != DVSR_OK) return rc;
  return frame_pad_check(what, pad_mode, f.h, f.w, Hp, Wp);
}

// (arguments checked by frame_ingest_yuv_check)
int frame_ingest_yuv_launch(const YuvFrame& f, float* dst, int Hp, int Wp, int pad_mode, hipStream_t st) {
  YuvIngestArgs a{};
  for (int i = 0; i < 3; ++i) {
    a.p[i] = static_cast<const unsigned char*>(f.plane[i]);
    a.rs[i] = f.rs[i];
  }
  a.dst = dst;
  a.h = f.h, a.w = f.w, a.Hp = Hp, a.Wp = Wp, a.pad = pad_mode;
  a.shift = f.semi ? 16u - (unsigned)f.depth : 0u;   // (bytes: unused)
  a.mask = (1u << f.depth) - 1u;
  a.k = yuv_coef(f);
  hipLaunchKernelGGL(ingest_kernel(f), yuv_grid(Hp, Wp), dim3(YUV_X, YUV_Y), 0, st, a);
  return check_launch(f.bytes == 2 ? "frame_ingest_yuv16_kernel" : "frame_ingest_yuv_kernel");
}

static int frame_ingest_yuv(const char* what, const YuvFrame& f, float* dst, int Hp, int Wp, int pad_mode, hipStream_t st) {
  int rc = frame_ingest_yuv_check(what, f, dst, Hp, Wp, pad_mode);
  if (rc != DVSR_OK) return rc;
  return frame_ingest_yuv_launch(f, dst, Hp, Wp, pad_mode, st);
}

static int frame_emit_yuv(const char* what, const YuvFrame& f, const float* src, int Hs, int Ws, float lo, float hi, hipStream_t st) {
  int rc = frame_planar_check(what, src, Hs, Ws, 2 * YUV_Y);
  if (rc != DVSR_OK) return rc;
  rc = yuv_frame_check(what, f, Hs, Ws);
  if (rc != DVSR_OK) return rc;
  DVSR_REQUIRE(hi > lo, DVSR_ERR_INVALID, "%s: range [%g, %g]", what, (double)lo, (double)hi);
  YuvEmitArgs a{};
  a.src = src;
  for (int i = 0; i < 3; ++i) {
    a.p[i] = static_cast<unsigned char*>(f.plane[i]);
    a.rs[i] = f.rs[i];
  }
  a.Hs = Hs, a.Ws = Ws, a.h = f.h, a.w = f.w, a.lo = lo, a.hi = hi;
  a.inv_scale = (float)(1.0 / ((double)hi - (double)lo));
  a.shift = f.semi ? 16u - (unsigned)f.depth : 0u;
  a.k = yuv_coef(f);
  hipLaunchKernelGGL(emit_kernel(f), yuv_grid(f.h, f.w), dim3(YUV_X, YUV_Y), 0, st, a);
  return check_launch(f.bytes == 2 ? "frame_emit_yuv16_kernel" : "frame_emit_yuv_kernel");
}

}  // namespace dvsr

using namespace dvsr;

extern "C" int dvsr_frame_ingest_yuv(const dvsr_yuv_desc* sd, float* dst, int Hp, int Wp, int pad_mode, dvsr_stream_t stream) {
  YuvFrame f;
  int rc = yuv_frame_from("frame_ingest_yuv", sd, &f);
  return rc != DVSR_OK ? rc : frame_ingest_yuv("frame_ingest_yuv", f, dst, Hp, Wp, pad_mode, (hipStream_t)stream);
}

extern "C" int dvsr_frame_ingest_yuv16(const dvsr_yuv16_desc* sd, float* dst, int Hp, int Wp, int pad_mode, dvsr_stream_t stream) {
  YuvFrame f;
  int rc = yuv_frame_from("frame_ingest_yuv16", sd, &f);
  return rc != DVSR_OK ? rc : frame_ingest_yuv("frame_ingest_yuv16", f, dst, Hp, Wp, pad_mode, (hipStream_t)stream);
}

extern "C" int dvsr_frame_emit_yuv(const float* src, int Hs, int Ws, const dvsr_yuv_desc* dd, float lo, float hi,
                                   dvsr_stream_t stream) {
  YuvFrame f;
  int rc = yuv_frame_from("frame_emit_yuv", dd, &f);
  return rc != DVSR_OK ? rc : frame_emit_yuv("frame_emit_yuv", f, src, Hs, Ws, lo, hi, (hipStream_t)stream);
}

extern "C" int dvsr_frame_emit_yuv16(const float* src, int Hs, int Ws, const dvsr_yuv16_desc* dd, float lo, float hi,
                                     dvsr_stream_t stream) {
  YuvFrame f;
  int rc = yuv_frame_from("frame_emit_yuv16", dd, &f);
  return rc != DVSR_OK ? rc : frame_emit_yuv("frame_emit_yuv16", f, src, Hs, Ws, lo, hi, (hipStream_t)stream);
}
