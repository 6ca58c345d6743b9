// PSNR / SSIM of an emitted frame against its ground truth, each where and as it lies (dvsr_frame_score; frames.py: score,
// adapt.py: the gt= argument of super_resolve_frames).
//
// The reference ends every evaluation in tensor2img -> [bgr2ycbcr(only_y=True)] -> crop_border -> calculate_psnr /
// calculate_ssim (codes/utils/util.py, codes/data/util.py).  dvsr_frame_metrics (metrics.hip) does that for two fp32 planar RGB
// frames in three launches with two quantised staging planes; here the two frames are described by a dvsr_frame_desc each --
// any address, any pitch, their own format -- and one tile kernel plus a fixed-order finalize give {mse, mean ssim}.
//
// Samples of a pixel (channel rgb: 3 samples, channel y: 1 sample):
//   U8_HWC_RGB / _BGR (pixel stride 3 | 4)   rgb: the bytes, in RGB order            y: Y8(R, G, B)
//   F32_CHW (3 planes)                       rgb: quant_u8(v, lo, hi) per channel    y: Y8 of those (quant.h: the one quantiser)
//   U8_Y                                     rgb: refused                            y: the byte
//   U16_Y_MSB / _10 / _12, depth d = 10 | 12 rgb: refused                            y: the d-bit level, word >> (16 - d) (MSB)
//                                                                                       or word & (2^d - 1) (_10 / _12)
//   U16_HWC_RGB / _BGR, depth 16             rgb: the words, in RGB order            y: refused (no Y from RGB above 8 bits)
//   U8_CHW_RGB / _GBR                        rgb: the bytes of the planes, as R G B  y: Y8(R, G, B)
//   U16_CHW_RGB / _GBR, d = 10 | 12 | 16     rgb: word & (2^d - 1), as R G B         y: refused
//   (with one of these on the other side an F32_CHW frame is quantised at its depth: quant_levels(v, lo, hi, 2^d - 1))
// Y8 is the reference's rgb2ycbcr(only_y=True), (65.481 R + 128.553 G + 24.966 B) / 255 + 16 rounded half to even, evaluated
// exactly in integers: num = 65481 R + 128553 G + 24966 B + 16 * 255000 (< 2^26), q = num / 255000, one more when the remainder
// is above 127500 or equals it with q odd.  Both frames reduce to one sample domain (8-bit with 8-bit, depth d with depth d).
// Region: crop_border = k removes k pixels on every side first (util.crop_border), H' x W' = (H - 2k) x (W - 2k); the SSIM
// "valid" region, (H' - 10) x (W' - 10), lies inside the crop.
//   out[0] = sum of squared sample differences over the crop (an exact 64-bit integer) / (samples), divided once
//   out[1] = mean of the SSIM map over channels and valid pixels, C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = 255 or 2^d - 1;
//            NaN without a valid region (H' <= 10 or W' <= 10), as in dvsr_frame_metrics and numpy
//
// score_tile_kernel: a workgroup covers a 32 x 16 tile of SSIM outputs of one channel.  It stages the 42 x 26 footprint of both
// frames into the LDS as 16-bit integer samples, converting on the way in, and then does what ssim_tile_kernel does (separable
// 11-tap Gaussian in float64 of x, y, x^2, y^2, xy; one partial per workgroup).  While staging, a thread adds the squared
// difference of every pixel its tile OWNS: the tile's 32 x 16 origin block, and for the last tile of a row / column also the <= 10
// remaining columns / rows, which its footprint already holds -- every pixel of the crop exactly once.  Without a valid region
// the grid is ceil(max(W' - 10, 1) / 32) x ceil(max(H' - 10, 1) / 16), which still covers the crop, and the SSIM part is skipped.
// No quantised plane goes to global memory, nothing is read in a second pass, and there are no floating-point atomics:
// score_finalize_kernel adds the partials in a fixed order, so a result is bit-identical from run to run.
#include <cmath>
#include <cstdint>

#include "common.h"
#include "kernels.h"
#include "quant.h"

namespace dvsr {

constexpr int SC_W = 32, SC_H = 16, SC_IW = SC_W + 10, SC_IH = SC_H + 10;
enum : int { SC_F32 = 0, SC_HWC = 1, SC_Y8 = 2, SC_Y16_MSB = 3, SC_Y16_LSB = 4,
             SC_HWC16 = 5, SC_CHW8 = 6, SC_CHW16 = 7 };   // frame_rgb.hip's formats (swap: BGR words / G, B, R planes)

struct ScoreSide {
  const unsigned char* p;              // pixel (0, 0) of the CROP
  long long row_bytes, plane_bytes;
  int kind, pixel_stride, swap;
};

struct ScoreArgs {
  ScoreSide a, b;
  int h, w;                            // the crop
  int luma, depth, valid;              // channel y; 8 | 10 | 12 | 16; the crop has a valid SSIM region
  float lo, hi, top;                   // top = 2^depth - 1: an fp32 side is quantised at the depth of the comparison
  double c1, c2;
  double g[11];
  unsigned long long* sse_partials;
  double* partials;
};

__device__ __forceinline__ unsigned score_y8(unsigned r, unsigned g, unsigned b) {
  const unsigned num = 65481u * r + 128553u * g + 24966u * b + 16u * 255000u;
  const unsigned q = num / 255000u, rem = num - q * 255000u;
  return q + ((rem > 127500u || (rem == 127500u && (q & 1u))) ? 1u : 0u);
}

constexpr int SC_NL = (SC_IH * SC_IW + 255) / 256;   // samples of a footprint per thread

// sample c of pixel (y, x) of the crop (c is ignored for channel y: LUMA)
template <int KIND, bool LUMA>
__device__ __forceinline__ unsigned score_sample(const ScoreSide& s, int y, int x, int c, const ScoreArgs& A) {
  const unsigned char* row = s.p + (long long)y * s.row_bytes;
  if constexpr (KIND == SC_F32) {
    const unsigned char* px = row + 4ll * x;
    if constexpr (!LUMA) {
      return (unsigned)quant_levels(*reinterpret_cast<const float*>(px + c * s.plane_bytes), A.lo, A.hi, A.top);
    } else {
      const float r = *reinterpret_cast<const float*>(px), g = *reinterpret_cast<const float*>(px + s.plane_bytes);
      const float b = *reinterpret_cast<const float*>(px + 2 * s.plane_bytes);
      return score_y8((unsigned)quant_u8(r, A.lo, A.hi), (unsigned)quant_u8(g, A.lo, A.hi), (unsigned)quant_u8(b, A.lo, A.hi));
    }
  } else if constexpr (KIND == SC_HWC) {
    const unsigned char* px = row + (long long)x * s.pixel_stride;
    if constexpr (!LUMA) {
      return px[s.swap ? 2 - c : c];
    } else {
      const unsigned p0 = px[0], p1 = px[1], p2 = px[2];
      return score_y8(s.swap ? p2 : p0, p1, s.swap ? p0 : p2);
    }
  } else if constexpr (KIND == SC_Y8) {
    return row[x];
  } else if constexpr (KIND == SC_Y16_MSB) {
    return (unsigned)reinterpret_cast<const unsigned short*>(row)[x] >> (16 - A.depth);
  } else if constexpr (KIND == SC_HWC16) {          // (channel rgb alone)
    return reinterpret_cast<const unsigned short*>(row + (long long)x * s.pixel_stride)[s.swap ? 2 - c : c];
  } else if constexpr (KIND == SC_CHW8) {
    const unsigned char* px = row + x;
    if constexpr (!LUMA) {
      return px[(s.swap ? (c + 2) % 3 : c) * s.plane_bytes];
    } else {
      return score_y8(px[(s.swap ? 2 : 0) * s.plane_bytes], px[(s.swap ? 0 : 1) * s.plane_bytes], px[(s.swap ? 1 : 2) * s.plane_bytes]);
    }
  } else if constexpr (KIND == SC_CHW16) {          // (channel rgb alone)
    const unsigned char* px = row + 2ll * x + (s.swap ? (c + 2) % 3 : c) * s.plane_bytes;
    return (unsigned)*reinterpret_cast<const unsigned short*>(px) & ((1u << A.depth) - 1u);
  } else {
    return (unsigned)reinterpret_cast<const unsigned short*>(row)[x] & ((1u << A.depth) - 1u);
  }
}

// the thread's SC_NL samples of the footprint at (oy0, ox0) of one frame, 0 outside the crop.  Straight-line code: every load
// of a side is issued before the first is used (one latency, not SC_NL); a sample outside the crop reads pixel (0, 0) instead.
template <int KIND, bool LUMA>
__device__ __forceinline__ void score_stage(const ScoreSide& s, int oy0, int ox0, int c, const ScoreArgs& A, unsigned v[SC_NL]) {
#pragma unroll
  for (int k = 0; k < SC_NL; ++k) {
    const int i = threadIdx.x + 256 * k;
    const int r = i / SC_IW, col = i - r * SC_IW;
    const int gy = oy0 + r, gx = ox0 + col;
    const bool ok = i < SC_IH * SC_IW && gy < A.h && gx < A.w;
    const unsigned t = score_sample<KIND, LUMA>(s, ok ? gy : 0, ok ? gx : 0, c, A);
    v[k] = ok ? t : 0u;
  }
}

// the format is uniform over the grid: one branch per side, outside the loads
__device__ __forceinline__ void score_stage_any(const ScoreSide& s, int oy0, int ox0, int c, const ScoreArgs& A, unsigned v[SC_NL]) {
  switch (s.kind) {
    case SC_F32:
      if (A.luma) score_stage<SC_F32, true>(s, oy0, ox0, c, A, v);
      else score_stage<SC_F32, false>(s, oy0, ox0, c, A, v);
      break;
    case SC_HWC:
      if (A.luma) score_stage<SC_HWC, true>(s, oy0, ox0, c, A, v);
      else score_stage<SC_HWC, false>(s, oy0, ox0, c, A, v);
      break;
    case SC_Y8: score_stage<SC_Y8, true>(s, oy0, ox0, c, A, v); break;
    case SC_Y16_MSB: score_stage<SC_Y16_MSB, true>(s, oy0, ox0, c, A, v); break;
    case SC_HWC16: score_stage<SC_HWC16, false>(s, oy0, ox0, c, A, v); break;
    case SC_CHW8:
      if (A.luma) score_stage<SC_CHW8, true>(s, oy0, ox0, c, A, v);
      else score_stage<SC_CHW8, false>(s, oy0, ox0, c, A, v);
      break;
    case SC_CHW16: score_stage<SC_CHW16, false>(s, oy0, ox0, c, A, v); break;
    default: score_stage<SC_Y16_LSB, true>(s, oy0, ox0, c, A, v); break;
  }
}

// (4 waves per SIMD, the 4 workgroups per CU that the LDS admits: without the bound the kernel takes 132 VGPRs and runs 3)
__global__ __launch_bounds__(256, 4) void score_tile_kernel(ScoreArgs A) {
  __shared__ unsigned short s_x[SC_IH][SC_IW + 2], s_y[SC_IH][SC_IW + 2];
  __shared__ double s_h[5][SC_IH][SC_W];  // horizontal pass of x, y, xx, yy, xy
  __shared__ double s_red[4];
  __shared__ unsigned long long s_sse[4];
  const int c = blockIdx.z;
  const int ox0 = blockIdx.x * SC_W, oy0 = blockIdx.y * SC_H;  // first valid-output pixel of the tile = input origin
  const bool last_x = blockIdx.x == gridDim.x - 1, last_y = blockIdx.y == gridDim.y - 1;
  unsigned long long sse = 0;
  {
    constexpr int NL = SC_NL;
    unsigned vx[NL], vy[NL];
    score_stage_any(A.a, oy0, ox0, c, A, vx);
    score_stage_any(A.b, oy0, ox0, c, A, vy);
    unsigned long long own = 0;          // (5 x 65535^2 is beyond 32 bits)
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const int i = threadIdx.x + 256 * k;
      const int r = i / SC_IW, col = i - r * SC_IW;
      // a pixel this tile owns (outside the crop both samples are 0)
      if (i < SC_IH * SC_IW && (r < SC_H || last_y) && (col < SC_W || last_x)) {
        const unsigned d = vx[k] > vy[k] ? vx[k] - vy[k] : vy[k] - vx[k];
        own += d * d;                    // (65535^2 < 2^32)
      }
    }
    sse = own;
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const int i = threadIdx.x + 256 * k;
      const int r = i / SC_IW, col = i - r * SC_IW;
      if (i < SC_IH * SC_IW) { s_x[r][col] = (unsigned short)vx[k]; s_y[r][col] = (unsigned short)vy[k]; }
    }
  }
  for (int off = 32; off > 0; off >>= 1) sse += __shfl_down(sse, off, 64);
  if ((threadIdx.x & 63) == 0) s_sse[threadIdx.x >> 6] = sse;
  __syncthreads();
  const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  if (threadIdx.x == 0) A.sse_partials[wg] = (s_sse[0] + s_sse[1]) + (s_sse[2] + s_sse[3]);
  if (!A.valid) {                       // (uniform over the grid) no SSIM output anywhere: the finalize writes NaN
    if (threadIdx.x == 0) A.partials[wg] = 0.0;
    return;
  }
  // horizontal pass: one thread = 4 consecutive columns of a row (14 samples of each frame converted once)
  for (int i = threadIdx.x; i < SC_IH * (SC_W / 4); i += 256) {
    const int r = i / (SC_W / 4), col = (i - r * (SC_W / 4)) * 4;
    double a[14], b[14];
#pragma unroll
    for (int t = 0; t < 14; ++t) { a[t] = (double)s_x[r][col + t]; b[t] = (double)s_y[r][col + t]; }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
      for (int t = 0; t < 11; ++t) {
        const double w = A.g[t], u = a[o + t], v = b[o + t];
        sx += w * u; sy += w * v; sxx += w * (u * u); syy += w * (v * v); sxy += w * (u * v);
      }
      s_h[0][r][col + o] = sx; s_h[1][r][col + o] = sy; s_h[2][r][col + o] = sxx; s_h[3][r][col + o] = syy;
      s_h[4][r][col + o] = sxy;
    }
  }
  __syncthreads();
  double acc = 0;
  {  // vertical pass: one thread = 2 consecutive rows of a column (12 rows of the 5 maps read once)
    const int col = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 2;
    double m[2][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
#pragma unroll
    for (int t = 0; t < 12; ++t) {
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        const double v = s_h[q][r0 + t][col];
        if (t < 11) m[0][q] += A.g[t] * v;
        if (t > 0) m[1][q] += A.g[t - 1] * v;
      }
    }
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      if (oy0 + r0 + o >= A.h - 10 || ox0 + col >= A.w - 10) continue;  // outside the "valid" region
      const double mu1 = m[o][0], mu2 = m[o][1];
      const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
      const double s1 = m[o][2] - mu1_sq, s2 = m[o][3] - mu2_sq, s12 = m[o][4] - mu12;
      acc += ((2 * mu12 + A.c1) * (2 * s12 + A.c2)) / ((mu1_sq + mu2_sq + A.c1) * (s1 + s2 + A.c2));
    }
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) A.partials[wg] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ __launch_bounds__(256) void score_finalize_kernel(const double* __restrict__ partials,
                                                             const unsigned long long* __restrict__ sse_partials, int n,
                                                             double n_samples, double n_valid, double* __restrict__ out) {
  __shared__ double s[256];
  __shared__ unsigned long long si[256];
  double acc = 0;
  unsigned long long iacc = 0;
  // fixed order per thread; eight loads of each kind in flight at a time (one at a time, 5400 partials took 8 us)
  constexpr int U = 8;
  for (int base = threadIdx.x; base < n; base += 256 * U) {
    double v[U];
    unsigned long long q[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + 256 * u;
      v[u] = i < n ? partials[i] : 0.0;
      q[u] = i < n ? sse_partials[i] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) { acc += v[u]; iacc += q[u]; }
  }
  s[threadIdx.x] = acc;
  si[threadIdx.x] = iacc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) { s[threadIdx.x] += s[threadIdx.x + off]; si[threadIdx.x] += si[threadIdx.x + off]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (double)si[0] / n_samples;
    out[1] = n_valid > 0 ? s[0] / n_valid : nan("");  // numpy: mean of an empty map
  }
}

static size_t score_align256(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr int SCORE_MAX_SIDE = 32768;

static size_t score_tiles(int channels, int h, int w) {
  return (size_t)ceil_div(w > 10 ? w - 10 : 1, SC_W) * ceil_div(h > 10 ? h - 10 : 1, SC_H) * channels;
}

// one side of the pair: its checks, and its ScoreSide with p at pixel (k, k)
static int score_side(const char* which, const void* p, const dvsr_frame_desc* d, const dvsr_score_args* args, ScoreSide* s) {
  const int k = args->crop_border;
  const bool luma = args->channel == DVSR_SCORE_Y;
  s->swap = 0;
  s->pixel_stride = 0;
  s->plane_bytes = 0;
  switch (d->format) {
    case DVSR_FRAME_F32_CHW:
      // (channel rgb: quantised at the depth of the comparison; the Y8 of channel y is defined on the 8-bit image alone)
      DVSR_REQUIRE(!luma || args->depth == 8, DVSR_ERR_INVALID, "frame_score: the Y of fp32 frame %s has 8-bit samples, depth is %d",
                   which, args->depth);
      DVSR_REQUIRE(args->hi > args->lo, DVSR_ERR_INVALID, "frame_score: range [%g, %g] of an fp32 frame", (double)args->lo,
                   (double)args->hi);
      DVSR_REQUIRE(d->row_stride >= d->w, DVSR_ERR_INVALID, "frame_score: row stride %lld of frame %s shorter than a row of %d floats",
                   d->row_stride, which, d->w);
      DVSR_REQUIRE(d->plane_stride >= (long long)(d->h - 1) * d->row_stride + d->w, DVSR_ERR_INVALID,
                   "frame_score: plane stride %lld of frame %s shorter than a plane of %d rows", d->plane_stride, which, d->h);
      DVSR_REQUIRE(reinterpret_cast<uintptr_t>(p) % 4 == 0, DVSR_ERR_INVALID, "frame_score: misaligned fp32 frame %s (4 bytes)", which);
      s->kind = SC_F32;
      s->row_bytes = 4 * d->row_stride;
      s->plane_bytes = 4 * d->plane_stride;
      s->p = static_cast<const unsigned char*>(p) + k * s->row_bytes + 4ll * k;
      return DVSR_OK;
    case DVSR_FRAME_U8_HWC_RGB:
    case DVSR_FRAME_U8_HWC_BGR:
      DVSR_REQUIRE(args->depth == 8, DVSR_ERR_INVALID, "frame_score: frame %s has 8-bit samples, depth is %d", which, args->depth);
      DVSR_REQUIRE(d->pixel_stride == 3 || d->pixel_stride == 4, DVSR_ERR_INVALID, "frame_score: pixel stride %d of frame %s (3 or 4)",
                   d->pixel_stride, which);
      s->kind = SC_HWC;
      s->pixel_stride = d->pixel_stride;
      s->swap = d->format == DVSR_FRAME_U8_HWC_BGR;
      break;
    case DVSR_FRAME_U8_Y:
      DVSR_REQUIRE(luma, DVSR_ERR_INVALID, "frame_score: channel rgb on a Y plane (frame %s)", which);
      DVSR_REQUIRE(args->depth == 8, DVSR_ERR_INVALID, "frame_score: frame %s has 8-bit samples, depth is %d", which, args->depth);
      DVSR_REQUIRE(d->pixel_stride == 1, DVSR_ERR_INVALID, "frame_score: pixel stride %d of a Y plane (1)", d->pixel_stride);
      s->kind = SC_Y8;
      s->pixel_stride = 1;
      break;
    case DVSR_FRAME_U16_Y_MSB:
    case DVSR_FRAME_U16_Y_10:
    case DVSR_FRAME_U16_Y_12: {
      DVSR_REQUIRE(luma, DVSR_ERR_INVALID, "frame_score: channel rgb on a Y plane (frame %s)", which);
      const bool ok = d->format == DVSR_FRAME_U16_Y_MSB ? (args->depth == 10 || args->depth == 12)
                                                        : args->depth == (d->format == DVSR_FRAME_U16_Y_10 ? 10 : 12);
      DVSR_REQUIRE(ok, DVSR_ERR_INVALID, "frame_score: frame %s (format %d) does not hold %d-bit samples", which, d->format, args->depth);
      DVSR_REQUIRE(d->pixel_stride == 2, DVSR_ERR_INVALID, "frame_score: pixel stride %d of a 16-bit Y plane (2)", d->pixel_stride);
      DVSR_REQUIRE(reinterpret_cast<uintptr_t>(p) % 2 == 0 && d->row_stride % 2 == 0, DVSR_ERR_INVALID,
                   "frame_score: odd address or row stride %lld of the 16-bit Y plane %s", d->row_stride, which);
      s->kind = d->format == DVSR_FRAME_U16_Y_MSB ? SC_Y16_MSB : SC_Y16_LSB;
      s->pixel_stride = 2;
      break;
    }
    default: {
      RgbFormat f;                       // frame_rgb.hip's formats
      DVSR_REQUIRE(frame_rgb_format(d->format, &f), DVSR_ERR_INVALID, "frame_score: unknown format %d of frame %s", d->format, which);
      const int rc = frame_rgb_check("frame_score", p, d, d->h, d->w, false);
      if (rc != DVSR_OK) return rc;
      DVSR_REQUIRE(args->depth == f.depth, DVSR_ERR_INVALID, "frame_score: frame %s has %d-bit samples, depth is %d", which, f.depth,
                   args->depth);
      DVSR_REQUIRE(!luma || f.depth == 8, DVSR_ERR_INVALID, "frame_score: channel y on the %d-bit RGB frame %s (rgb alone)", f.depth,
                   which);
      s->kind = f.planar ? (f.bytes == 1 ? SC_CHW8 : SC_CHW16) : SC_HWC16;
      s->pixel_stride = d->pixel_stride;
      s->swap = f.reorder;
      s->plane_bytes = f.planar ? d->plane_stride : 0;
      break;
    }
  }
  DVSR_REQUIRE(d->row_stride >= (long long)d->w * s->pixel_stride, DVSR_ERR_INVALID,
               "frame_score: row stride %lld of frame %s shorter than a row of %lld bytes", d->row_stride, which,
               (long long)d->w * s->pixel_stride);
  s->row_bytes = d->row_stride;
  s->p = static_cast<const unsigned char*>(p) + k * s->row_bytes + (long long)k * s->pixel_stride;
  return DVSR_OK;
}

}  // namespace dvsr

using namespace dvsr;

extern "C" size_t dvsr_frame_score_workspace_bytes(int channels, int h, int w) {
  if (channels < 1 || channels > 3 || h < 1 || w < 1 || h > SCORE_MAX_SIDE || w > SCORE_MAX_SIDE) return 0;
  const size_t n = score_tiles(channels, h, w);
  return score_align256(n * sizeof(unsigned long long)) + score_align256(n * sizeof(double));
}

extern "C" int dvsr_frame_score(const void* a, const dvsr_frame_desc* da, const void* b, const dvsr_frame_desc* db,
                                const dvsr_score_args* args, double* out, void* workspace, size_t workspace_bytes,
                                dvsr_stream_t stream) {
  DVSR_REQUIRE(a && da && b && db && args && out && workspace, DVSR_ERR_INVALID,
               "frame_score: null frame / descriptor / arguments / result / workspace");
  DVSR_REQUIRE(args->channel == DVSR_SCORE_RGB || args->channel == DVSR_SCORE_Y, DVSR_ERR_INVALID,
               "frame_score: unknown channel %d", args->channel);
  DVSR_REQUIRE(args->depth == 8 || args->depth == 10 || args->depth == 12 || args->depth == 16, DVSR_ERR_INVALID,
               "frame_score: depth %d (8, 10, 12 or 16)", args->depth);
  DVSR_REQUIRE(da->h >= 1 && da->w >= 1 && da->h <= SCORE_MAX_SIDE && da->w <= SCORE_MAX_SIDE, DVSR_ERR_INVALID,
               "frame_score: frame size h=%d w=%d outside [1, %d]", da->h, da->w, SCORE_MAX_SIDE);
  DVSR_REQUIRE(da->h == db->h && da->w == db->w, DVSR_ERR_INVALID, "frame_score: frame a is %d x %d, frame b is %d x %d", da->h,
               da->w, db->h, db->w);
  const int k = args->crop_border;
  DVSR_REQUIRE(k >= 0 && k <= (da->h - 1) / 2 && k <= (da->w - 1) / 2, DVSR_ERR_INVALID,
               "frame_score: crop_border %d leaves nothing of %d x %d", k, da->h, da->w);
  DVSR_REQUIRE(reinterpret_cast<uintptr_t>(out) % 8 == 0, DVSR_ERR_INVALID, "frame_score: misaligned result (8 bytes)");
  ScoreArgs A;
  int rc = score_side("a", a, da, args, &A.a);
  if (rc != DVSR_OK) return rc;
  rc = score_side("b", b, db, args, &A.b);
  if (rc != DVSR_OK) return rc;
  A.h = da->h - 2 * k;
  A.w = da->w - 2 * k;
  A.luma = args->channel == DVSR_SCORE_Y;
  A.depth = args->depth;
  A.valid = A.h > 10 && A.w > 10;
  A.lo = args->lo;
  A.hi = args->hi;
  A.top = (float)((1 << args->depth) - 1);
  const int nch = A.luma ? 1 : 3;
  const size_t need = dvsr_frame_score_workspace_bytes(nch, A.h, A.w);
  DVSR_REQUIRE(workspace_bytes >= need, DVSR_ERR_WORKSPACE, "frame_score: workspace %zu < %zu bytes", workspace_bytes, need);
  DVSR_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, DVSR_ERR_INVALID, "frame_score: misaligned workspace (8 bytes)");
  const double L = (double)((1 << args->depth) - 1);
  A.c1 = (0.01 * L) * (0.01 * L);
  A.c2 = (0.03 * L) * (0.03 * L);
  double sum = 0;  // cv2.getGaussianKernel(11, 1.5): exp(-(i - 5)^2 / (2 sigma^2)), normalised to sum 1
  for (int i = 0; i < 11; ++i) { A.g[i] = std::exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); sum += A.g[i]; }
  for (int i = 0; i < 11; ++i) A.g[i] /= sum;
  const size_t n = score_tiles(nch, A.h, A.w);
  A.sse_partials = static_cast<unsigned long long*>(workspace);
  A.partials = reinterpret_cast<double*>(static_cast<unsigned char*>(workspace) + score_align256(n * sizeof(unsigned long long)));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ceil_div(A.w > 10 ? A.w - 10 : 1, SC_W), ceil_div(A.h > 10 ? A.h - 10 : 1, SC_H), nch);
  hipLaunchKernelGGL(score_tile_kernel, grid, dim3(256), 0, st, A);
  rc = check_launch("score_tile_kernel");
  if (rc != DVSR_OK) return rc;
  const double n_valid = A.valid ? (double)(A.h - 10) * (A.w - 10) * nch : 0.0;
  hipLaunchKernelGGL(score_finalize_kernel, dim3(1), dim3(256), 0, st, A.partials, A.sse_partials, (int)n,
                     (double)nch * A.h * A.w, n_valid, out);
  return check_launch("score_finalize_kernel");
}
