// SR frames at a target output size (dvsr_frame_resize_taps / _table / dvsr_frame_resize).
//
// The resampler is separable antialiased bicubic -- Keys' kernel with a = -0.5, half-pixel centres, the support widened by
// the down-scale ratio: torch.nn.functional.interpolate(x, size, mode='bicubic', antialias=True, align_corners=False).  Per
// axis, n_in -> n_out:  scale = n_in / n_out, support = 2 scale (scale >= 1) or 2, inv = 1 / scale (scale >= 1) or 1; output
// i has its centre at c = scale (i + 0.5) and takes the source samples j in [first, end), first = max(0, int(c - support +
// 0.5)), end = min(n_in, int(c + support + 0.5)), with weights k((j - c + 0.5) inv) divided by their sum.  The window is cut
// at the edge of the image and renormalised: nothing outside the image is read.  The table of an axis (first[n_out],
// weights[n_out][taps], computed in double, rounded to fp32, zero-padded) is built on the host once per size pair.
//
//   frame_resize_kernel   fp32 planar [3][Hs][Ws], of which the top-left h x w is the image  ->  fp32 planar [3][Ho][Wo],
//                         rows 0 .. oh-1: columns 0 .. ow-1 resampled, columns ow .. Wo-1 zero (what the emit kernels'
//                         16-byte loads read)
// A workgroup of 256 threads owns TW x TH outputs of ONE plane (grid z = plane).  It stages the tile's source footprint,
// FH <= 64 rows x FW columns, in the LDS (16-byte global loads: the rows of src are 16-byte aligned and the footprint starts
// on a multiple of 4 columns; whatever lies outside the h x w image is staged as 0, never loaded), runs the horizontal pass
// into a second LDS image [FH][TW], and the vertical pass into registers.  All global loads -- the footprint and the tables of
// the tile -- are issued ahead of the first global store; there is no grid-stride loop and no atomic.
// Both passes keep the LDS free of bank conflicts by what they map to the lanes of a wave:
//   horizontal   a wave takes ONE output column at a time and its 64 lanes are the staged ROWS: the window start and the
//                weights are wave-uniform (they sit in lanes 0 .. 17 and 32 of one register loaded at the start, read with
//                v_readlane), lane r reads img[r * (FW + 1) + j] -- an odd row pitch, so 32 consecutive rows fall on 32
//                different banks whatever the ratio is -- and writes mid[r * (TW + 1) + column], conflict-free as well.
//                (Lanes along the output columns would start `ratio` floats apart: a ratio-way conflict at integer ratios.)
//   vertical     a wave takes ONE output row at a time, its lanes are the tile's columns: consecutive addresses.
// What the odd pitch costs is on the staging side: a lane's four floats go out as four ds_write_b32, whose lanes are 4 banks
// apart (4-way, twice the cycles of a conflict-free dword store).  The footprint is written once and read taps / ratio >= 4
// times, so the reads were given the conflict-free layout.
// TH is the largest number of rows whose footprint fits the 64 lanes (at most 32), TW the largest of 64, 32, 16, 8 whose
// two images fit 64 KB and 12 16-byte loads per thread: two workgroups share a CU at any accepted ratio.
// No table content can make the kernel read outside the image or the LDS images: every window start is clamped into the
// image, every staged index into the footprint; a table that is not dvsr_frame_resize_table's gives a wrong picture, no fault.
// A tap whose weight is 0 (the zero-padding of a row of the table) contributes 0, not 0 x the value it would have read.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "frame_resample.h"
#include "kernels.h"

namespace dvsr {

struct ResizeArgs {
  const float* src;
  float* dst;
  int Hs, Ws, h, w, Ho, Wo, oh, ow;
  const int* first_r;
  const float* w_r;
  int taps_r;
  const int* first_c;
  const float* w_c;
  int taps_c;
  int TW, TH, FH, FW;   // tile; staged rows (<= RS_ROWS) and columns (a multiple of 4)
};

template <int TAPS>
__global__ __launch_bounds__(RS_THREADS) void frame_resize_kernel(ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ox0 = blockIdx.x * a.TW, oy0 = blockIdx.y * a.TH;
  const int tw = min(a.TW, a.Wo - ox0);     // columns of dst that this tile writes, the zero columns included
  const int twv = min(a.TW, a.ow - ox0);    // ... of which resampled (<= 0: the tile lies in the zero columns)
  const int th = min(a.TH, a.oh - oy0);
  float* dst = a.dst + (size_t)blockIdx.z * a.Ho * a.Wo + (size_t)oy0 * a.Wo + ox0;
  if (twv <= 0) {
#pragma unroll
    for (int k = 0; k < RS_OUTS; ++k) {
      const int oyl = wv + 4 * k;
      if (oyl < th && lane < tw) dst[(size_t)oyl * a.Wo + lane] = 0.f;
    }
    return;
  }
  const float* src = a.src + (size_t)blockIdx.z * a.Hs * a.Ws;
  const int pitch1 = a.FW + 1, pitch2 = a.TW + 1;
  float* img = rs_lds;                       // [FH][FW + 1]  the source footprint
  float* mid = rs_lds + a.FH * pitch1;       // [FH][TW + 1]  after the horizontal pass
  const int y_lo = clampi(a.first_r[oy0], 0, a.h - 1);
  const int x_lo = clampi(a.first_c[ox0], 0, a.w - 1) & ~3;

  // ---- every global load of the workgroup: the footprint ...
  const int fw4 = a.FW >> 2, n4 = a.FH * fw4;
  f32x4 v[RS_MAXV];
  int sr[RS_MAXV], sc[RS_MAXV];
#pragma unroll
  for (int k = 0; k < RS_MAXV; ++k) {
    if (k * RS_THREADS < n4) {               // (uniform)
      const int q = min(k * RS_THREADS + tid, n4 - 1);
      sr[k] = q / fw4;
      sc[k] = 4 * (q - sr[k] * fw4);
      const int y = min(y_lo + sr[k], a.h - 1), x = min(x_lo + sc[k], (a.w - 1) & ~3);   // inside the image; x + 3 < Ws
      v[k] = *reinterpret_cast<const f32x4*>(src + (size_t)y * a.Ws + x);
    }
  }
  // ... and the table rows of the columns and rows that this wave will compute
  float gc[RS_COLS], gr[RS_OUTS];
#pragma unroll
  for (int k = 0; k < RS_COLS; ++k) gc[k] = table_row(a.first_c, a.w_c, a.taps_c, min(ox0 + wv + 4 * k, a.ow - 1), lane);
#pragma unroll
  for (int k = 0; k < RS_OUTS; ++k) gr[k] = table_row(a.first_r, a.w_r, a.taps_r, min(oy0 + wv + 4 * k, a.oh - 1), lane);

  // ---- stage: outside the image is 0
#pragma unroll
  for (int k = 0; k < RS_MAXV; ++k) {
    if (k * RS_THREADS < n4 && k * RS_THREADS + tid < n4) {
      const bool row_in = y_lo + sr[k] < a.h;
      float* p = img + sr[k] * pitch1 + sc[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) p[e] = (row_in && x_lo + sc[k] + e < a.w) ? v[k][e] : 0.f;
    }
  }
  __syncthreads();

  // ---- horizontal: one output column per wave and step, lanes = staged rows
  const float* my_row = img + min(lane, a.FH - 1) * pitch1;
#pragma unroll
  for (int k = 0; k < RS_COLS; ++k) {
    const int oxl = wv + 4 * k;
    if (oxl < twv) {                         // (uniform)
      const int f = __builtin_amdgcn_readlane(__builtin_bit_cast(int, gc[k]), RS_FIRST_LANE);
      const int b = clampi(clampi(f, 0, a.w - 1) - x_lo, 0, a.FW - 1);
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < TAPS; ++t) {
        const float g = lane_value(gc[k], t);
        const float x = my_row[min(b + t, a.FW - 1)];
        acc = fmaf(g, g != 0.f ? x : 0.f, acc);
      }
      if (lane < a.FH) mid[lane * pitch2 + oxl] = acc;
    }
  }
  __syncthreads();

  // ---- vertical: one output row per wave and step, lanes = the tile's columns
  const float* my_col = mid + min(lane, a.TW - 1);
  float res[RS_OUTS];
#pragma unroll
  for (int k = 0; k < RS_OUTS; ++k) {
    const int oyl = wv + 4 * k;
    res[k] = 0.f;
    if (oyl < th) {                          // (uniform)
      const int f = __builtin_amdgcn_readlane(__builtin_bit_cast(int, gr[k]), RS_FIRST_LANE);
      const int b = clampi(clampi(f, 0, a.h - 1) - y_lo, 0, a.FH - 1);
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < TAPS; ++t) {
        const float g = lane_value(gr[k], t);
        const float x = my_col[min(b + t, a.FH - 1) * pitch2];
        acc = fmaf(g, g != 0.f ? x : 0.f, acc);
      }
      res[k] = lane < twv ? acc : 0.f;       // columns ow .. Wo-1 are stored as 0
    }
  }
#pragma unroll
  for (int k = 0; k < RS_OUTS; ++k) {
    const int oyl = wv + 4 * k;
    if (oyl < th && lane < tw) dst[(size_t)oyl * a.Wo + lane] = res[k];
  }
}

// ---- the definition, on the host -----------------------------------------------------------------
static bool axis_ok(int n_in, int n_out) {
  return n_in >= 1 && n_out >= 1 && (long long)n_in <= 4LL * n_out && (long long)n_out <= 2LL * n_in;
}

static double keys(double x) {
  const double a = -0.5;
  x = std::fabs(x);
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return a * (((x - 5.0) * x + 8.0) * x - 4.0);
  return 0.0;
}

struct AxisWindow {
  int first, end;
  double c, inv;
};

static AxisWindow axis_window(int n_in, int n_out, int i) {
  const double scale = (double)n_in / (double)n_out;
  const double support = scale >= 1.0 ? 2.0 * scale : 2.0;
  AxisWindow win;
  win.inv = scale >= 1.0 ? 1.0 / scale : 1.0;
  win.c = scale * (i + 0.5);
  win.first = std::max(0, (int)(win.c - support + 0.5));
  win.end = std::min(n_in, (int)(win.c + support + 0.5));
  return win;
}

static int axis_taps(int n_in, int n_out) {
  int taps = 0;
  for (int i = 0; i < n_out; ++i) {
    const AxisWindow win = axis_window(n_in, n_out, i);
    taps = std::max(taps, win.end - win.first);
  }
  return taps;
}

// the longest source footprint of a tile of `tile` outputs: from the first window's start, rounded down to `align`, to the
// last window's end
static int axis_span(int n_in, int n_out, int tile, int align) {
  int span = 0;
  for (int i0 = 0; i0 < n_out; i0 += tile) {
    const int lo = axis_window(n_in, n_out, i0).first / align * align;
    span = std::max(span, axis_window(n_in, n_out, std::min(i0 + tile, n_out) - 1).end - lo);
  }
  return span;
}

static int resize_check(const float* src, int Hs, int Ws, int h, int w, const float* dst, int Ho, int Wo, int oh, int ow,
                        const dvsr_resize_axis* rows, const dvsr_resize_axis* cols) {
  DVSR_REQUIRE(src && dst && rows && cols, DVSR_ERR_INVALID, "frame_resize: null tensor / axis table");
  DVSR_REQUIRE(rows->first && rows->weights && cols->first && cols->weights, DVSR_ERR_INVALID,
               "frame_resize: null pointer in an axis table");
  DVSR_REQUIRE(Hs >= 1 && Ws >= 4 && Ws % 4 == 0 && h >= 1 && w >= 1 && h <= Hs && w <= Ws, DVSR_ERR_INVALID,
               "frame_resize: image %d x %d in a source of Hs=%d Ws=%d (Ws must be a positive multiple of 4)", h, w, Hs, Ws);
  DVSR_REQUIRE(Ho >= 1 && Wo >= 4 && Wo % 4 == 0 && oh >= 1 && ow >= 1 && oh <= Ho && ow <= Wo, DVSR_ERR_INVALID,
               "frame_resize: result %d x %d in a destination of Ho=%d Wo=%d (Wo must be a positive multiple of 4)", oh, ow, Ho,
               Wo);
  DVSR_REQUIRE(axis_ok(h, oh) && axis_ok(w, ow), DVSR_ERR_INVALID,
               "frame_resize: %d x %d -> %d x %d is outside the accepted ratios (n_in / n_out <= 4, n_out / n_in <= 2)", h, w, oh,
               ow);
  DVSR_REQUIRE(rows->taps >= 1 && rows->taps <= RS_MAX_TAPS && cols->taps >= 1 && cols->taps <= RS_MAX_TAPS, DVSR_ERR_INVALID,
               "frame_resize: taps %d (rows) / %d (columns) outside [1, %d]", rows->taps, cols->taps, RS_MAX_TAPS);
  DVSR_REQUIRE(reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0, DVSR_ERR_INVALID,
               "frame_resize: misaligned planar fp32 tensor (16 bytes)");
  DVSR_REQUIRE(reinterpret_cast<uintptr_t>(rows->first) % 4 == 0 && reinterpret_cast<uintptr_t>(rows->weights) % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(cols->first) % 4 == 0 && reinterpret_cast<uintptr_t>(cols->weights) % 4 == 0,
               DVSR_ERR_INVALID, "frame_resize: misaligned axis table (4 bytes)");
  return DVSR_OK;
}

}  // namespace dvsr

using namespace dvsr;

extern "C" int dvsr_frame_resize_taps(int n_in, int n_out) {
  DVSR_REQUIRE(axis_ok(n_in, n_out), DVSR_ERR_INVALID,
               "frame_resize_taps: %d -> %d is outside the accepted ratios (n_in / n_out <= 4, n_out / n_in <= 2)", n_in, n_out);
  return axis_taps(n_in, n_out);
}

extern "C" int dvsr_frame_resize_table(int n_in, int n_out, int taps, int* first, float* weights) {
  DVSR_REQUIRE(first && weights, DVSR_ERR_INVALID, "frame_resize_table: null table");
  DVSR_REQUIRE(axis_ok(n_in, n_out), DVSR_ERR_INVALID,
               "frame_resize_table: %d -> %d is outside the accepted ratios (n_in / n_out <= 4, n_out / n_in <= 2)", n_in, n_out);
  DVSR_REQUIRE(taps >= axis_taps(n_in, n_out) && taps <= RS_MAX_TAPS, DVSR_ERR_INVALID,
               "frame_resize_table: taps=%d outside [%d, %d]", taps, axis_taps(n_in, n_out), RS_MAX_TAPS);
  for (int i = 0; i < n_out; ++i) {
    const AxisWindow win = axis_window(n_in, n_out, i);
    double k[RS_MAX_TAPS], sum = 0.0;
    const int n = win.end - win.first;
    for (int t = 0; t < n; ++t) {
      k[t] = keys((win.first + t - win.c + 0.5) * win.inv);
      sum += k[t];
    }
    first[i] = win.first;
    for (int t = 0; t < taps; ++t) weights[(size_t)i * taps + t] = t < n ? (float)(k[t] / sum) : 0.f;
  }
  return DVSR_OK;
}

extern "C" int dvsr_frame_resize(const float* src, int Hs, int Ws, int h, int w, float* dst, int Ho, int Wo, int oh, int ow,
                                 const dvsr_resize_axis* rows, const dvsr_resize_axis* cols, dvsr_stream_t stream) {
  int rc = resize_check(src, Hs, Ws, h, w, dst, Ho, Wo, oh, ow, rows, cols);
  if (rc != DVSR_OK) return rc;
  DVSR_REQUIRE(rows->taps >= axis_taps(h, oh) && cols->taps >= axis_taps(w, ow), DVSR_ERR_INVALID,
               "frame_resize: taps %d (rows) / %d (columns) shorter than the windows of %d -> %d / %d -> %d", rows->taps,
               cols->taps, h, oh, w, ow);
  // the tile: as many rows as the 64 lanes of the horizontal pass can stage, then as many columns as the LDS and the staging
  // registers take
  const double sy = (double)h / oh;
  int TH = (int)((RS_ROWS - 2.0 * (sy >= 1.0 ? 2.0 * sy : 2.0) - 2.0) / sy) + 1;
  TH = std::max(1, std::min(TH, RS_MAX_TH));
  while (TH > 1 && axis_span(h, oh, TH, 1) > RS_ROWS) --TH;
  const int FH = axis_span(h, oh, TH, 1);
  int TW = RS_MAX_TW, FW = 0;
  size_t lds = 0;
  for (;; TW /= 2) {
    FW = (axis_span(w, ow, TW, 4) + 3) / 4 * 4;
    lds = ((size_t)FH * (FW + 1) + (size_t)FH * (TW + 1)) * sizeof(float);
    if ((FH * (FW / 4) <= RS_MAXV * RS_THREADS && lds <= RS_LDS_BYTES) || TW == 8) break;
  }
  DVSR_REQUIRE(FH <= RS_ROWS && FH * (FW / 4) <= RS_MAXV * RS_THREADS && lds <= RS_LDS_BYTES, DVSR_ERR_UNSUPPORTED,
               "frame_resize: no tile for %d x %d -> %d x %d (footprint %d x %d)", h, w, oh, ow, FH, FW);
  const int gy = ceil_div(oh, TH);
  DVSR_REQUIRE(gy <= 65535, DVSR_ERR_INVALID, "frame_resize: %d output rows are too many", oh);
  ResizeArgs a{src, dst, Hs, Ws, h, w, Ho, Wo, oh, ow, rows->first, rows->weights, rows->taps,
               cols->first, cols->weights, cols->taps, TW, TH, FH, FW};
  const dim3 grid(ceil_div(Wo, TW), gy, 3), block(RS_THREADS);
  const int taps = std::max(rows->taps, cols->taps);
  hipStream_t st = (hipStream_t)stream;
  if (taps <= 4) hipLaunchKernelGGL(frame_resize_kernel<4>, grid, block, lds, st, a);
  else if (taps <= 8) hipLaunchKernelGGL(frame_resize_kernel<8>, grid, block, lds, st, a);
  else if (taps <= 12) hipLaunchKernelGGL(frame_resize_kernel<12>, grid, block, lds, st, a);
  else hipLaunchKernelGGL(frame_resize_kernel<RS_MAX_TAPS>, grid, block, lds, st, a);
  return check_launch("frame_resize_kernel");
}
