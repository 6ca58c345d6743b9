// MATLAB's imresize(img, scale, 'bicubic') on the device (dvsr_frame_imresize_taps / _table / dvsr_frame_imresize):
// the BI degradation of the SR literature and the "Bicubic" row of its tables, codes/data/util.py:323-524 of the reference
// (calculate_weights_indices, imresize, imresize_np).
//
// The definition, per axis, n_in -> n_out = ceil(n_in scale), scale = num / den out of {1/2, 1/3, 1/4, 2, 3, 4}, in double:
//   kw = 4, or 4 / scale when down-scaling with antialiasing;  P = ceil(kw) + 2 taps
//   output i (0-based):  u = (i + 1) / scale + 0.5 (1 - 1 / scale),  left = floor(u - kw / 2)
//   tap t reads the 1-based sample left + t with weight cubic(u - left - t), or scale cubic((u - left - t) scale) when
//   down-scaling with antialiasing, divided by the sum of the P weights;  cubic(x) = 1.5 |x|^3 - 2.5 |x|^2 + 1 for |x| <= 1,
//   -0.5 |x|^3 + 2.5 |x|^2 - 4 |x| + 2 for 1 < |x| <= 2, 0 otherwise.
//   A 0-based sample index j outside [0, n_in) is folded back by MATLAB's periodic symmetric rule (-k -> k - 1,
//   n_in - 1 + k -> n_in - k, with period 2 n_in) and its weight added, in tap order, to the tap it lands on.  The taps with a
//   non-zero weight then form ONE contiguous window [first, first + len): the table of the axis is first[n_out] and
//   weights[n_out][taps], rounded to fp32 and zero-padded, the form dvsr_frame_resize's tables have.  len is at most 16 (1/4),
//   11 (1/3), 8 (1/2), 4 (up-scaling).  The reference evaluates the same rule in fp32 and copies a symmetric border that is
//   longer than the image for 2 <= n_in <= 6 at 1/4 (it raises); the periodic rule is defined for every n_in >= 1.
//
// frame_imresize_kernel is frame_resize_kernel's plan (frame_resize.hip: a workgroup of 256 threads owns TW x TH outputs of one
// plane, stages their source footprint FH <= 64 rows x FW columns in the LDS at an odd row pitch, runs the horizontal pass with
// the 64 lanes on the staged rows -- conflict-free at the integer ratios 2, 3, 4 that are the whole point here -- into a
// second LDS image, and the vertical pass with the lanes on the tile's columns) with the two ends exchanged:
//   source       a frame as it arrives, through a source policy of frame_source.h: fp32 planes or interleaved bytes at ANY
//                address and pitch, so the staging is scalar loads -- a wave per staged row, its lanes on consecutive columns,
//                up to sixteen rows in flight per lane -- and bytes become v / 255.0f through a 256-entry table in the LDS.
//                Only the top-left h x w crop is read (modcrop costs nothing); loads are clamped into it.
//   destination  fp32 planes by row and plane stride; rows >= oh and columns >= ow are not written; with `quantise` a value
//                leaves as rintf(fminf(fmaxf(255 y, 0), 255)) / 255, the library's one quantiser.
// No table content can make the kernel read outside the crop or the LDS images or write outside oh x ow: every window start
// is clamped into the crop, every staged index into the footprint.  A tap whose weight is 0 contributes 0.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include "common.h"
#include "frame_resample.h"
#include "frame_source.h"
#include "kernels.h"

namespace dvsr {

constexpr int IR_STAGE_ROWS = RS_ROWS / 4;   // staged rows of one wave at most: that many loads in flight per lane

struct ImresizeArgs {
  float* dst;
  long long dst_row, dst_plane;   // floats
  int h, w, oh, ow;
  const int* first_r;
  const float* w_r;
  int taps_r;
  const int* first_c;
  const float* w_c;
  int taps_c;
  int TW, TH, FH, FW;             // tile; staged rows (<= RS_ROWS) and columns
  int quantise;
};

// min of first[i0 .. i0 + n), n <= 64, in every lane of the wave
__device__ __forceinline__ int tile_min(const int* first, int i0, int n, int lane) {
  int v = first[i0 + min(lane, n - 1)];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  return __builtin_amdgcn_readfirstlane(v);
}

template <int TAPS, class Src>
__global__ __launch_bounds__(RS_THREADS) void frame_imresize_kernel(Src src, ImresizeArgs a) {
  extern __shared__ float ir_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int plane = blockIdx.z;
  const int ox0 = blockIdx.x * a.TW, oy0 = blockIdx.y * a.TH;   // < ow, < oh: the grid covers oh x ow
  const int tw = min(a.TW, a.ow - ox0), th = min(a.TH, a.oh - oy0);
  const int pitch1 = a.FW | 1, pitch2 = a.TW + 1;               // odd: 32 consecutive rows fall on 32 banks
  float* img = ir_lds;                       // [FH][pitch1]  the source footprint
  float* mid = img + a.FH * pitch1;          // [FH][pitch2]  after the horizontal pass
  float* lut = mid + a.FH * pitch2;          // [Src::LUT]
  // the origin of the staged image: the smallest window start of the tile's rows / columns (a x3 window of one tap starts
  // behind its neighbours')
  const int y_lo = clampi(tile_min(a.first_r, oy0, th, lane), 0, a.h - 1);
  const int x_lo = clampi(tile_min(a.first_c, ox0, tw, lane), 0, a.w - 1);
  src.fill(lut, tid, RS_THREADS);

  // ---- the table rows of the columns and rows that this wave will compute
  float gc[RS_COLS], gr[RS_OUTS];
#pragma unroll
  for (int k = 0; k < RS_COLS; ++k) gc[k] = table_row(a.first_c, a.w_c, a.taps_c, min(ox0 + wv + 4 * k, a.ow - 1), lane);
#pragma unroll
  for (int k = 0; k < RS_OUTS; ++k) gr[k] = table_row(a.first_r, a.w_r, a.taps_r, min(oy0 + wv + 4 * k, a.oh - 1), lane);
  if (Src::LUT) __syncthreads();

  // ---- stage the footprint: wave wv takes the rows wv, wv + 4, ..; 64 consecutive columns per pass
  for (int c0 = 0; c0 < a.FW; c0 += 64) {
    const int c = c0 + lane;
    const int cx = src.col(min(x_lo + c, a.w - 1));                // inside the crop
    float v[IR_STAGE_ROWS];
#pragma unroll
    for (int k = 0; k < IR_STAGE_ROWS; ++k) {
      const int r = wv + 4 * k;
      if (r < a.FH) v[k] = src.row(plane, min(y_lo + r, a.h - 1), lut)[cx];   // (uniform)
    }
#pragma unroll
    for (int k = 0; k < IR_STAGE_ROWS; ++k) {
      const int r = wv + 4 * k;
      if (r < a.FH && c < a.FW) img[r * pitch1 + c] = v[k];
    }
  }
  __syncthreads();

  // ---- horizontal: one output column per wave and step, lanes = staged rows
  const float* my_row = img + min(lane, a.FH - 1) * pitch1;
#pragma unroll
  for (int k = 0; k < RS_COLS; ++k) {
    const int oxl = wv + 4 * k;
    if (oxl < tw) {                          // (uniform)
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
  float* dst = a.dst + plane * a.dst_plane + oy0 * a.dst_row + ox0;
#pragma unroll
  for (int k = 0; k < RS_OUTS; ++k) {
    const int oyl = wv + 4 * k;
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
      if (a.quantise) acc = rintf(fminf(fmaxf(acc * 255.f, 0.f), 255.f)) / 255.f;
      if (lane < tw) dst[oyl * a.dst_row + lane] = acc;
    }
  }
}

// ---- the definition, on the host -----------------------------------------------------------------
static double cubic(double x) {
  const double ax = std::fabs(x), ax2 = ax * ax, ax3 = ax2 * ax;
  if (ax <= 1.0) return 1.5 * ax3 - 2.5 * ax2 + 1.0;
  if (ax <= 2.0) return -0.5 * ax3 + 2.5 * ax2 - 4.0 * ax + 2.0;
  return 0.0;
}

static bool scale_ok(int num, int den) {
  return (num == 1 && den >= 2 && den <= 4) || (den == 1 && num >= 2 && num <= 4);
}

static long long imresize_n_out(int n_in, int num, int den) { return ((long long)n_in * num + den - 1) / den; }

// output i of an axis: its folded window [first, first + len) and the len weights, in double (len <= RS_MAX_TAPS)
static void axis_row(int n_in, int num, int den, int antialias, int i, int* first, int* len, double* w) {
  const double scale = (double)num / (double)den;
  const bool wide = num < den && antialias;
  const double kw = wide ? 4.0 / scale : 4.0;
  const int P = (int)std::ceil(kw) + 2;                         // <= 18
  const double u = (i + 1) / scale + 0.5 * (1.0 - 1.0 / scale);
  const double left = std::floor(u - kw / 2.0);
  double k[RS_MAX_TAPS], sum = 0.0;
  int j[RS_MAX_TAPS];
  for (int t = 0; t < P; ++t) {
    const double d = u - (left + t);
    k[t] = wide ? scale * cubic(d * scale) : cubic(d);
    sum += k[t];
    const long long period = 2LL * n_in;
    const long long m = ((((long long)left + t - 1) % period) + period) % period;
    j[t] = (int)(m < n_in ? m : period - 1 - m);
  }
  int lo = INT_MAX, hi = -1;
  for (int t = 0; t < P; ++t) {
    k[t] = k[t] / sum;
    if (k[t] != 0.0) lo = std::min(lo, j[t]), hi = std::max(hi, j[t]);
  }
  if (hi < 0) lo = hi = j[P / 2];                               // (no weight at all: cannot happen for the cubic)
  *first = lo;
  *len = std::min(hi - lo + 1, RS_MAX_TAPS);
  for (int t = 0; t < *len; ++t) w[t] = 0.0;
  for (int t = 0; t < P; ++t)
    if (k[t] != 0.0 && j[t] - lo < *len) w[j[t] - lo] += k[t];
}

// the windows of an axis, kept per (n_in, scale, antialias): what dvsr_frame_imresize checks `taps` against and sizes its tile by
struct AxisDef {
  int n_in, num, den, antialias, longest;
  std::vector<int> first, end;
};

static std::shared_ptr<const AxisDef> axis_def(int n_in, int num, int den, int antialias) {
  static std::mutex mu;
  static std::vector<std::shared_ptr<const AxisDef>> kept;
  static size_t next = 0;
  antialias = antialias ? 1 : 0;
  std::lock_guard<std::mutex> lock(mu);
  for (const auto& d : kept)
    if (d->n_in == n_in && d->num == num && d->den == den && d->antialias == antialias) return d;
  auto d = std::make_shared<AxisDef>();
  d->n_in = n_in, d->num = num, d->den = den, d->antialias = antialias, d->longest = 0;
  const int n_out = (int)imresize_n_out(n_in, num, den);
  d->first.resize(n_out), d->end.resize(n_out);
  double w[RS_MAX_TAPS];
  for (int i = 0; i < n_out; ++i) {
    int len;
    axis_row(n_in, num, den, antialias, i, &d->first[i], &len, w);
    d->end[i] = d->first[i] + len;
    d->longest = std::max(d->longest, len);
  }
  if (kept.size() < 16) kept.push_back(d);
  else kept[next++ % kept.size()] = d;
  return d;
}

// the longest source footprint of a tile of `tile` outputs: from the smallest window start -- where the kernel puts the origin
// of its staged image -- to the furthest window end
static int axis_span(const AxisDef& d, int tile) {
  const int n_out = (int)d.first.size();
  int span = 0;
  for (int i0 = 0; i0 < n_out; i0 += tile) {
    int lo = INT_MAX, hi = 0;
    for (int i = i0; i < std::min(i0 + tile, n_out); ++i) lo = std::min(lo, d.first[i]), hi = std::max(hi, d.end[i]);
    span = std::max(span, hi - lo);
  }
  return span;
}

static int imresize_axis_check(const char* what, int n_in, int num, int den) {
  DVSR_REQUIRE(scale_ok(num, den), DVSR_ERR_UNSUPPORTED, "%s: scale %d/%d is not one of 1/2, 1/3, 1/4, 2/1, 3/1, 4/1", what, num,
               den);
  DVSR_REQUIRE(n_in >= 1 && imresize_n_out(n_in, num, den) <= INT_MAX / 4, DVSR_ERR_INVALID, "%s: n_in=%d", what, n_in);
  return DVSR_OK;
}

template <class Src>
static int imresize_launch(const Src& src, const ImresizeArgs& a, size_t lds, hipStream_t st) {
  const dim3 grid(ceil_div(a.ow, a.TW), ceil_div(a.oh, a.TH), 3), block(RS_THREADS);
  lds += Src::LUT * sizeof(float);
  const int taps = std::max(a.taps_r, a.taps_c);
  if (taps <= 4) hipLaunchKernelGGL((frame_imresize_kernel<4, Src>), grid, block, lds, st, src, a);
  else if (taps <= 8) hipLaunchKernelGGL((frame_imresize_kernel<8, Src>), grid, block, lds, st, src, a);
  else if (taps <= 12) hipLaunchKernelGGL((frame_imresize_kernel<12, Src>), grid, block, lds, st, src, a);
  else if (taps <= 16) hipLaunchKernelGGL((frame_imresize_kernel<16, Src>), grid, block, lds, st, src, a);
  else hipLaunchKernelGGL((frame_imresize_kernel<RS_MAX_TAPS, Src>), grid, block, lds, st, src, a);
  return check_launch("frame_imresize_kernel");
}

}  // namespace dvsr

using namespace dvsr;

extern "C" int dvsr_frame_imresize_taps(int n_in, int num, int den, int antialias, int* n_out) {
  int rc = imresize_axis_check("frame_imresize_taps", n_in, num, den);
  if (rc != DVSR_OK) return rc;
  if (n_out) *n_out = (int)imresize_n_out(n_in, num, den);
  return axis_def(n_in, num, den, antialias)->longest;
}

extern "C" int dvsr_frame_imresize_table(int n_in, int num, int den, int antialias, int taps, int* first, float* weights) {
  DVSR_REQUIRE(first && weights, DVSR_ERR_INVALID, "frame_imresize_table: null table");
  int rc = imresize_axis_check("frame_imresize_table", n_in, num, den);
  if (rc != DVSR_OK) return rc;
  const int longest = axis_def(n_in, num, den, antialias)->longest;
  DVSR_REQUIRE(taps >= longest && taps <= RS_MAX_TAPS, DVSR_ERR_INVALID, "frame_imresize_table: taps=%d outside [%d, %d]", taps,
               longest, RS_MAX_TAPS);
  const int n_out = (int)imresize_n_out(n_in, num, den);
  for (int i = 0; i < n_out; ++i) {
    double w[RS_MAX_TAPS];
    int len;
    axis_row(n_in, num, den, antialias, i, &first[i], &len, w);
    for (int t = 0; t < taps; ++t) weights[(size_t)i * taps + t] = t < len ? (float)w[t] : 0.f;
  }
  return DVSR_OK;
}

extern "C" int dvsr_frame_imresize(const void* src, const dvsr_frame_desc* sd, int h, int w, int num, int den, int antialias,
                                   float* dst, long long dst_row_stride, long long dst_plane_stride, int oh, int ow,
                                   const dvsr_resize_axis* rows, const dvsr_resize_axis* cols, int quantise,
                                   dvsr_stream_t stream) {
  DVSR_REQUIRE(dst && rows && cols, DVSR_ERR_INVALID, "frame_imresize: null dst / axis table");
  DVSR_REQUIRE(rows->first && rows->weights && cols->first && cols->weights, DVSR_ERR_INVALID,
               "frame_imresize: null pointer in an axis table");
  int rc = frame_desc_check("frame_imresize", src, sd, INT_MAX, INT_MAX, false);
  if (rc != DVSR_OK) return rc;
  DVSR_REQUIRE(h >= 1 && w >= 1 && h <= sd->h && w <= sd->w, DVSR_ERR_INVALID, "frame_imresize: crop %d x %d of a %d x %d frame", h,
               w, sd->h, sd->w);
  rc = imresize_axis_check("frame_imresize", h, num, den);
  if (rc == DVSR_OK) rc = imresize_axis_check("frame_imresize", w, num, den);
  if (rc != DVSR_OK) return rc;
  DVSR_REQUIRE(oh == imresize_n_out(h, num, den) && ow == imresize_n_out(w, num, den), DVSR_ERR_INVALID,
               "frame_imresize: %d x %d at %d/%d gives %lld x %lld, not %d x %d", h, w, num, den, imresize_n_out(h, num, den),
               imresize_n_out(w, num, den), oh, ow);
  const auto dr = axis_def(h, num, den, antialias), dc = axis_def(w, num, den, antialias);
  DVSR_REQUIRE(rows->taps >= dr->longest && rows->taps <= RS_MAX_TAPS && cols->taps >= dc->longest && cols->taps <= RS_MAX_TAPS,
               DVSR_ERR_INVALID, "frame_imresize: taps %d (rows) / %d (columns) outside [%d, %d] / [%d, %d]", rows->taps, cols->taps,
               dr->longest, RS_MAX_TAPS, dc->longest, RS_MAX_TAPS);
  DVSR_REQUIRE(dst_row_stride >= ow && dst_plane_stride >= (long long)(oh - 1) * dst_row_stride + ow, DVSR_ERR_INVALID,
               "frame_imresize: destination row stride %lld / plane stride %lld shorter than a row of %d / a plane of %d rows",
               dst_row_stride, dst_plane_stride, ow, oh);
  DVSR_REQUIRE(reinterpret_cast<uintptr_t>(dst) % 4 == 0, DVSR_ERR_INVALID, "frame_imresize: misaligned fp32 destination (4 bytes)");
  DVSR_REQUIRE(reinterpret_cast<uintptr_t>(rows->first) % 4 == 0 && reinterpret_cast<uintptr_t>(rows->weights) % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(cols->first) % 4 == 0 && reinterpret_cast<uintptr_t>(cols->weights) % 4 == 0,
               DVSR_ERR_INVALID, "frame_imresize: misaligned axis table (4 bytes)");
  // the tile: as many rows as the 64 lanes of the horizontal pass can stage, then as many columns as the LDS takes
  int TH = RS_MAX_TH;
  while (TH > 1 && axis_span(*dr, TH) > RS_ROWS) --TH;
  const int FH = axis_span(*dr, TH);
  const size_t lut = sd->format == DVSR_FRAME_F32_CHW ? SrcPlanarF32::LUT : SrcBytesHWC::LUT;
  int TW = RS_MAX_TW, FW = 0;
  size_t lds = 0;
  for (;; TW /= 2) {
    FW = axis_span(*dc, TW);
    lds = ((size_t)FH * (FW | 1) + (size_t)FH * (TW + 1)) * sizeof(float);
    if (lds + lut * sizeof(float) <= RS_LDS_BYTES || TW == 8) break;
  }
  DVSR_REQUIRE(FH <= RS_ROWS && lds + lut * sizeof(float) <= RS_LDS_BYTES, DVSR_ERR_UNSUPPORTED,
               "frame_imresize: no tile for %d x %d -> %d x %d (footprint %d x %d)", h, w, oh, ow, FH, FW);
  DVSR_REQUIRE(ceil_div(oh, TH) <= 65535, DVSR_ERR_INVALID, "frame_imresize: %d output rows are too many", oh);
  const ImresizeArgs a{dst, dst_row_stride, dst_plane_stride, h, w, oh, ow, rows->first, rows->weights, rows->taps,
                       cols->first, cols->weights, cols->taps, TW, TH, FH, FW, quantise ? 1 : 0};
  if (sd->format == DVSR_FRAME_F32_CHW)
    return imresize_launch(SrcPlanarF32{static_cast<const float*>(src), sd->row_stride, sd->plane_stride}, a, lds,
                           (hipStream_t)stream);
  return imresize_launch(SrcBytesHWC{static_cast<const unsigned char*>(src), sd->row_stride, sd->pixel_stride,
                                     sd->format == DVSR_FRAME_U8_HWC_BGR},
                         a, lds, (hipStream_t)stream);
}
