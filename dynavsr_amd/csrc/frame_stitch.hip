// Frames in overlapping tiles, the seams blended on the device (dvsr_frame_stitch_origins / _cover / _table / dvsr_frame_stitch;
// DESIGN 3.2r).
//
// A frame too large for one plan is cut into tiles of one size, tile x tile LR pixels `overlap` apart, the last one anchored at
// the edge (stitch_origins); every tile is super-resolved on its own and the SR tiles are blended into the SR frame.  Per axis, in
// SR pixels (L = s tile, O_k = s origin_k): the raw weight of tile k at position r in [O_k, O_k + L) is u_k(r) = min(dl, dr),
// dl = r - O_k + 0.5 (L for the first tile), dr = O_k + L - r - 0.5 (L for the last tile), and w_k(r) = u_k(r) / sum_j u_j(r): a
// linear cross-fade inside an overlap, exactly 1 outside.  The table of an axis (first[s n]: the first tile that covers a
// position; weights[s n][K], K = the largest number of tiles over one position, computed in double, rounded to fp32, zero-padded)
// is built on the host once per geometry.
//
//   frame_stitch_kernel   fp32 [ny nx][planes][Ht][Wt] -> fp32 [planes][H][W]:
//                         dst[p][r][c] = sum_a sum_b (wy[r][a] wx[c][b]) tile(first_y[r] + a, first_x[c] + b)[p][r - O_y][c - O_x]
//
// Wt % 4 == 0, W % 4 == 0, every origin is a multiple of 4 and every pointer is 16-byte aligned, so a row is W / 4 chunks of one
// float4 and a chunk never straddles a tile edge: a thread owns one chunk of ST_ROWS = 4 consecutive rows of dst (H % 4 == 0), and
// every load and store is a 16-byte access, consecutive lanes at consecutive addresses.  The grid is (chunks of a row, H / 4,
// planes): the rows and the plane are uniform over a workgroup, so the rows' table entries are scalar loads and there is no
// division.  The column tables -- first_x at the chunk's first column (origins are multiples of 4: the four columns of a chunk
// have one set of covering tiles), the weights as KX float4 loads (4 KX consecutive floats of the table), the origins -- are
// loaded once for the four rows.  The first entry of each of the four rows is loaded ahead of everything else (4 KX 16-byte
// loads in flight); further row entries exist in overlap rows alone and come under a uniform branch.  One row per thread
// measured 47.7 us for a 3 x 2160 x 3840 frame, four rows 38.0 us.  No LDS, no atomics, one launch; every element of dst is
// written once and nothing else is.
// The sum runs a outer, b inner; the product of the two weights comes first, then the product with the value; the accumulator
// starts as the first term; fp32, never contracted: the result equals the same loop written in torch bit for bit.  An entry
// whose row or column weight is exactly 0 (the zero-padding of the table) is neither read nor added -- a NaN in a tile that
// does not cover a pixel never reaches it -- and where one tile covers, 1.0f * 1.0f * v is v.
// No table content can make the kernel read outside `tiles` or write outside dst: tile indices, rows and chunks are clamped;
// a table that is not dvsr_frame_stitch_table's gives a wrong picture, no fault.
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace dvsr {

constexpr int ST_MAX_COVER = 3;

struct StitchArgs {
  const f32x4* tiles;
  f32x4* dst;
  int ny, nx, planes, Ht, wt4, H, w4;
  const int* first_y;
  const float* w_y;
  const int* o_y;
  int ky;
  const int* first_x;
  const f32x4* w_x;
  const int* o_x;
};

__device__ __forceinline__ int st_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

constexpr int ST_ROWS = 4;   // rows of a thread: H % 4 == 0; the column tables are loaded once for them

template <int KX>
__global__ __launch_bounds__(256) void frame_stitch_kernel(StitchArgs a) {
#pragma clang fp contract(off)
  const int r0 = blockIdx.y * ST_ROWS, p = blockIdx.z;            // (uniform: the rows' tables come by scalar loads)
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int c4 = min(q, a.w4 - 1), c = 4 * c4;                    // spare threads of the last workgroup load the last chunk
  const int fx = st_clamp(a.first_x[c], 0, a.nx - 1);
  // the column weights of the chunk: floats [c KX, (c + 4) KX) of the table; column c + e, entry b is element e KX + b
  f32x4 wq[KX];
#pragma unroll
  for (int b = 0; b < KX; ++b) wq[b] = a.w_x[(size_t)c4 * KX + b];
  float wx[KX][4];
#pragma unroll
  for (int b = 0; b < KX; ++b)
#pragma unroll
    for (int e = 0; e < 4; ++e) wx[b][e] = wq[(e * KX + b) >> 2][(e * KX + b) & 3];
  size_t col[KX];                                                 // tile (., fx + b): its first image and the chunk inside a row
  bool any[KX];
#pragma unroll
  for (int b = 0; b < KX; ++b) {
    const int tx = min(fx + b, a.nx - 1);
    const int lc4 = st_clamp(c - a.o_x[tx], 0, 4 * (a.wt4 - 1)) >> 2;
    col[b] = (size_t)tx * a.planes * a.Ht * a.wt4 + lc4;
    any[b] = wx[b][0] != 0.f || wx[b][1] != 0.f || wx[b][2] != 0.f || wx[b][3] != 0.f;
  }
  // entry k of row r0 + j: its weight and the row of tile (fy + k, .) it reads
  auto row_of = [&](int j, int k, float* w) -> size_t {
    const int r = r0 + j;
    const int fy = st_clamp(a.first_y[r], 0, a.ny - 1);
    *w = a.w_y[(size_t)r * a.ky + k];
    const int ty = min(fy + k, a.ny - 1);
    const int lr = st_clamp(r - a.o_y[ty], 0, a.Ht - 1);
    return (((size_t)ty * a.nx * a.planes + p) * a.Ht + lr) * a.wt4;
  };
  auto add = [&](f32x4& acc, bool* have, float wy, const f32x4* v) {
#pragma unroll
    for (int b = 0; b < KX; ++b)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (wx[b][e] != 0.f) {
          const float w = wy * wx[b][e];
          const float t = w * v[b][e];
          acc[e] = have[e] ? acc[e] + t : t;
          have[e] = true;
        }
  };
  // the first entry of every row: ST_ROWS x KX loads in flight
  float wy0[ST_ROWS];
  f32x4 v0[ST_ROWS][KX];
#pragma unroll
  for (int j = 0; j < ST_ROWS; ++j) {
    const size_t row = row_of(j, 0, &wy0[j]);
#pragma unroll
    for (int b = 0; b < KX; ++b) {
      v0[j][b] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (wy0[j] != 0.f && any[b]) v0[j][b] = a.tiles[row + col[b]];
    }
  }
  f32x4 acc[ST_ROWS];
#pragma unroll
  for (int j = 0; j < ST_ROWS; ++j) {
    acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bool have[4] = {false, false, false, false};
    if (wy0[j] != 0.f) add(acc[j], have, wy0[j], v0[j]);          // (uniform)
    for (int k = 1; k < a.ky; ++k) {                              // (uniform; rows inside an overlap alone)
      float wy;
      const size_t row = row_of(j, k, &wy);
      if (wy != 0.f) {
        f32x4 v[KX];
#pragma unroll
        for (int b = 0; b < KX; ++b) {
          v[b] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (any[b]) v[b] = a.tiles[row + col[b]];
        }
        add(acc[j], have, wy, v);
      }
    }
  }
  if (q < a.w4) {
#pragma unroll
    for (int j = 0; j < ST_ROWS; ++j) a.dst[((size_t)p * a.H + r0 + j) * a.w4 + c4] = acc[j];
  }
}

// ---- the definition, on the host -----------------------------------------------------------------
static bool stitch_axis_ok(int n, int tile, int overlap) {
  return n >= 4 && n % 4 == 0 && tile >= 4 && tile % 4 == 0 && overlap >= 0 && overlap % 4 == 0 && 2LL * overlap <= tile;
}

// the tiles of an axis of (padded) length n: origins k step for k step < n - tile, then n - tile; one tile of length n if tile >= n
static int stitch_count(int n, int tile, int overlap) {
  if (tile >= n) return 1;
  const int step = tile - overlap;
  return (n - tile + step - 1) / step + 1;
}

static int stitch_origin(int n, int tile, int overlap, int k) {
  if (tile >= n) return 0;
  return (int)std::min<long long>((long long)k * (tile - overlap), n - tile);
}

static int stitch_scale_ok(int scale) { return scale >= 1 && scale <= 16; }

// the tiles [k0, k1) that cover position r (SR pixels) and their raw weights; returns k1 - k0
static int stitch_cover_at(int n, int tile, int overlap, int scale, int r, int* k0, double* u) {
  const int cnt = stitch_count(n, tile, overlap);
  const long long L = (long long)scale * std::min(tile, n);
  int m = 0;
  *k0 = 0;
  for (int k = 0; k < cnt; ++k) {
    const long long O = (long long)scale * stitch_origin(n, tile, overlap, k);
    if (r < O) break;
    if (r >= O + L) continue;
    if (m == 0) *k0 = k;
    const double dl = k == 0 ? (double)L : (double)(r - O) + 0.5;
    const double dr = k == cnt - 1 ? (double)L : (double)(O + L - r) - 0.5;
    if (m < ST_MAX_COVER + 1) u[m] = std::min(dl, dr);
    ++m;
  }
  return m;
}

static int stitch_axis_cover(int n, int tile, int overlap) {
  // (coverage changes at tile edges alone: scale 1 and every fourth position decide it)
  int cover = 0, k0;
  double u[ST_MAX_COVER + 1];
  for (int r = 0; r < n; r += 4) cover = std::max(cover, stitch_cover_at(n, tile, overlap, 1, r, &k0, u));
  return cover;
}

static bool aligned_to(const void* p, int a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// host origins (SR pixels) of an axis of `tiles` tiles of length L over N: from 0 to N - L, ascending, multiples of 4, no gap
static bool origins_ok(const int* o, int tiles, int L, int N) {
  if (o[0] != 0 || o[tiles - 1] != N - L) return false;
  for (int k = 0; k < tiles; ++k) {
    if (o[k] % 4) return false;
    if (k && (o[k] <= o[k - 1] || o[k] - o[k - 1] > L)) return false;
  }
  return true;
}

}  // namespace dvsr

using namespace dvsr;

#define STITCH_AXIS_REQUIRE(what)                                                                                              \
  DVSR_REQUIRE(stitch_axis_ok(n, tile, overlap), DVSR_ERR_INVALID,                                                             \
               what ": n=%d, tile=%d, overlap=%d (n, tile multiples of 4 and >= 4; overlap a multiple of 4, 0 <= overlap <= "  \
               "tile / 2)", n, tile, overlap)

extern "C" int dvsr_frame_stitch_origins(int n, int tile, int overlap, int* origins, int capacity) {
  STITCH_AXIS_REQUIRE("frame_stitch_origins");
  const int cnt = stitch_count(n, tile, overlap);
  if (origins) {
    DVSR_REQUIRE(capacity >= cnt, DVSR_ERR_INVALID, "frame_stitch_origins: room for %d origins, the axis has %d", capacity, cnt);
    for (int k = 0; k < cnt; ++k) origins[k] = stitch_origin(n, tile, overlap, k);
  }
  return cnt;
}

extern "C" int dvsr_frame_stitch_cover(int n, int tile, int overlap) {
  STITCH_AXIS_REQUIRE("frame_stitch_cover");
  return stitch_axis_cover(n, tile, overlap);
}

extern "C" int dvsr_frame_stitch_table(int n, int tile, int overlap, int scale, int cover, int* first, float* weights) {
  DVSR_REQUIRE(first && weights, DVSR_ERR_INVALID, "frame_stitch_table: null table");
  STITCH_AXIS_REQUIRE("frame_stitch_table");
  DVSR_REQUIRE(stitch_scale_ok(scale), DVSR_ERR_INVALID, "frame_stitch_table: scale=%d outside [1, 16]", scale);
  const int need = stitch_axis_cover(n, tile, overlap);
  DVSR_REQUIRE(cover >= need && cover <= ST_MAX_COVER, DVSR_ERR_INVALID, "frame_stitch_table: cover=%d outside [%d, %d]", cover, need,
               ST_MAX_COVER);
  const long long N = (long long)scale * n;
  DVSR_REQUIRE(N <= 0x7FFFFFFFLL / ST_MAX_COVER, DVSR_ERR_INVALID, "frame_stitch_table: %lld positions are too many", N);
  for (int r = 0; r < (int)N; ++r) {
    int k0 = 0;
    double u[ST_MAX_COVER + 1], sum = 0.0;
    const int m = stitch_cover_at(n, tile, overlap, scale, r, &k0, u);
    for (int t = 0; t < m; ++t) sum += u[t];
    first[r] = k0;
    for (int t = 0; t < cover; ++t) weights[(size_t)r * cover + t] = t < m ? (float)(u[t] / sum) : 0.f;
  }
  return DVSR_OK;
}

static int stitch_axis_check(const char* axis, const dvsr_stitch_axis* t, const int* origins, int tiles, int L, int N) {
  DVSR_REQUIRE(t->first && t->weights && t->origins, DVSR_ERR_INVALID, "frame_stitch: null pointer in the table of the %s", axis);
  DVSR_REQUIRE(t->cover >= 1 && t->cover <= ST_MAX_COVER, DVSR_ERR_INVALID, "frame_stitch: cover=%d of the %s outside [1, %d]",
               t->cover, axis, ST_MAX_COVER);
  DVSR_REQUIRE(aligned_to(t->first, 4) && aligned_to(t->origins, 4) && aligned_to(t->weights, 16), DVSR_ERR_INVALID,
               "frame_stitch: misaligned table of the %s (first, origins: 4 bytes; weights: 16 bytes)", axis);
  DVSR_REQUIRE(L <= N && origins_ok(origins, tiles, L, N), DVSR_ERR_INVALID,
               "frame_stitch: the origins of the %d tiles of length %d do not tile the %s of length %d (0 first, %d last, "
               "ascending multiples of 4, no gap)", tiles, L, axis, N, N - L);
  return DVSR_OK;
}

extern "C" int dvsr_frame_stitch(const float* tiles, int ny, int nx, int planes, int Ht, int Wt, float* dst, int H, int W,
                                 const dvsr_stitch_axis* rows, const dvsr_stitch_axis* cols, const int* origins_y,
                                 const int* origins_x, dvsr_stream_t stream) {
  DVSR_REQUIRE(tiles && dst && rows && cols && origins_y && origins_x, DVSR_ERR_INVALID,
               "frame_stitch: null tensor / axis table / origins");
  DVSR_REQUIRE(ny >= 1 && nx >= 1 && planes >= 1, DVSR_ERR_INVALID, "frame_stitch: ny=%d, nx=%d, planes=%d must be positive", ny, nx,
               planes);
  DVSR_REQUIRE(Ht >= 4 && Wt >= 4 && Ht % 4 == 0 && Wt % 4 == 0 && H >= 4 && W >= 4 && H % 4 == 0 && W % 4 == 0, DVSR_ERR_INVALID,
               "frame_stitch: tiles of %d x %d, a frame of %d x %d (positive multiples of 4)", Ht, Wt, H, W);
  DVSR_REQUIRE(H <= 65535 && planes <= 65535, DVSR_ERR_INVALID, "frame_stitch: H=%d, planes=%d (at most 65535 each)", H, planes);
  DVSR_REQUIRE((long long)ny * nx <= 0x7FFFFFFFLL / planes, DVSR_ERR_INVALID, "frame_stitch: %d x %d tiles of %d planes are too many",
               ny, nx, planes);
  int rc = stitch_axis_check("rows", rows, origins_y, ny, Ht, H);
  if (rc != DVSR_OK) return rc;
  rc = stitch_axis_check("columns", cols, origins_x, nx, Wt, W);
  if (rc != DVSR_OK) return rc;
  DVSR_REQUIRE(aligned_to(tiles, 16) && aligned_to(dst, 16), DVSR_ERR_INVALID, "frame_stitch: misaligned fp32 tensor (16 bytes)");
  const uintptr_t t0 = reinterpret_cast<uintptr_t>(tiles), d0 = reinterpret_cast<uintptr_t>(dst);
  const uintptr_t t1 = t0 + (uintptr_t)ny * nx * planes * Ht * Wt * sizeof(float), d1 = d0 + (uintptr_t)planes * H * W * sizeof(float);
  DVSR_REQUIRE(d1 <= t0 || t1 <= d0, DVSR_ERR_INVALID, "frame_stitch: dst overlaps tiles (stitching in place is not provided)");
  StitchArgs a{reinterpret_cast<const f32x4*>(tiles), reinterpret_cast<f32x4*>(dst), ny, nx, planes, Ht, Wt / 4, H, W / 4,
               rows->first, rows->weights, rows->origins, rows->cover,
               cols->first, reinterpret_cast<const f32x4*>(cols->weights), cols->origins};
  // whole waves per workgroup, as few idle lanes in a row's last workgroup as 64 .. 256 threads allow
  int threads = 256, best = -1;
  for (int t = 256; t >= 64; t -= 64) {
    const int padded = ceil_div(a.w4, t) * t;
    if (best < 0 || padded < best) { best = padded; threads = t; }
  }
  const dim3 grid(ceil_div(a.w4, threads), H / ST_ROWS, planes), block(threads);
  hipStream_t st = (hipStream_t)stream;
  if (cols->cover == 1) hipLaunchKernelGGL(frame_stitch_kernel<1>, grid, block, 0, st, a);
  else if (cols->cover == 2) hipLaunchKernelGGL(frame_stitch_kernel<2>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(frame_stitch_kernel<3>, grid, block, 0, st, a);
  return check_launch("frame_stitch_kernel");
}
