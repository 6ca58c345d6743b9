// Weight / bias gradient of the dense convolutions (backward of conv2d.hip) on
// v_mfma_f32_32x32x2_f32:   dW[o][c][tap] = sum_{n,y,x} gy[n][o][y][x] * x[n][c][y*S+ty-pad][x*S+tx-pad]
//
// GEMM view per workgroup: D[o 64][c 64] (one D per tap) with K = pixels.  Each of the 4 waves owns
// one (o-half, c-half) 32x32 tile for ALL taps (9 accumulators = 144 VGPRs) and walks a strided
// list of 2x32-pixel tiles, so the pixel reduction stays in registers.  The per-workgroup sums are
// folded into NSLOT (<= 8) zero-initialised [tap][o][c] slots with coalesced hardware fp32 atomics
// (workgroup s -> slot s % NSLOT) and a second kernel sums the slots and transposes to OIHW; this
// keeps the flush traffic at NSLOT x 147 KB instead of nsplit x 147 KB (the r01 profile had the
// slot-less reduce at 51 us per call on the 44x80 inner-step shapes).  Summation order across
// workgroups is therefore not fixed (1e-7-level run-to-run differences, like cuDNN's wgrad).
// Operand reads are conflict-free: both LDS images use an odd plane stride.
//   A (lane l): gy[o = l&31][px = 2kk + (l>>5)]   <- s_g[o*65 + px]
//   B (lane l): x [c = l&31][px shifted by tap]   <- s_x[c*PLANEP + (py*S+ty)*IW + px*S+tx]
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "small_grid.h"

namespace dvsr {

#ifdef DVSR_CONV_TRACE
static long long* g_wgrad_trace = nullptr;
// every weight-gradient launch from now on stamps its timeline into buf (tools/wgrad_trace.py)
extern "C" int dvsr_debug_wgrad_trace(void* buf) { g_wgrad_trace = (long long*)buf; return 0; }
#endif

template <int KS, int S>
struct WgShape {
  static constexpr int TH = 2, TW = 32, NPX = TH * TW, KK = KS * KS;
  static constexpr int IH = (TH - 1) * S + KS, IW = (TW - 1) * S + KS;
  static constexpr int PLANE = IH * IW, PLANEP = PLANE | 1, GROW = NPX + 1;
  static constexpr size_t LDS_BYTES = (size_t)(64 * GROW + 64 * PLANEP) * sizeof(float);
};

template <int KS, int S>
__global__ __launch_bounds__(256, 2) void conv2d_wgrad_kernel(WgradK a) {
  using Sh = WgShape<KS, S>;
  constexpr int KK = Sh::KK, IW = Sh::IW, PLANE = Sh::PLANE, PLANEP = Sh::PLANEP, GROW = Sh::GROW,
                NPX = Sh::NPX;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* s_g = smem;
  float* s_x = smem + 64 * GROW;

  const int split = blockIdx.x, ob = blockIdx.y, cbk = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = lane & 31, hi = lane >> 5;
  const int ot = wave >> 1, ct = wave & 1;
  const size_t HW = (size_t)a.H * a.W, HWo = (size_t)a.Ho * a.Wo;

  f32x16 acc[KK];
#pragma unroll
  for (int t = 0; t < KK; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float db = 0.f;

  const WgSpan sp = wg_span(a, split);
  for (int tile = sp.tile0; tile < sp.tile_end; tile += a.nsplit) {
    const int tx_ = tile % a.tiles_x;
    const int t2 = tile / a.tiles_x;
    const int ty_ = t2 % a.tiles_y;
    const int n = t2 / a.tiles_y;
    const int oy0 = ty_ * Sh::TH, ox0 = tx_ * Sh::TW;
    const int iy0 = oy0 * S - a.pad, ix0 = ox0 * S - a.pad;
    __syncthreads();
    // ---- gy tile: s_g[o][p]
    for (int idx = tid; idx < 64 * NPX; idx += 256) {
      const int o = idx / NPX, p = idx - o * NPX;
      const int oy = oy0 + (p >> 5), ox = ox0 + (p & 31), co = ob * 64 + o;
      float v = 0.f;
      if (co < a.Cout && oy < a.Ho && ox < a.Wo) {
        if (a.gy_ps)
          v = a.gy[(((size_t)n * (a.Cout >> 2) + (co >> 2)) * (2 * a.Ho) + 2 * oy + ((co >> 1) & 1)) *
                       (size_t)(2 * a.Wo) + 2 * ox + (co & 1)];
        else
          v = a.gy[((size_t)n * a.Cout + co) * HWo + (size_t)oy * a.Wo + ox];
      }
      s_g[o * GROW + p] = v;
    }
    // ---- x halo tile: s_x[c][iy][ix]
    const float* xn = a.x + (size_t)(n / a.x_bdiv) * a.x_bs;
    for (int idx = tid; idx < 64 * PLANE; idx += 256) {
      const int c = idx / PLANE, r = idx - c * PLANE;
      const int iy = r / IW, ix = r - iy * IW;
      const int gy_ = iy0 + iy, gx_ = ix0 + ix, ci = cbk * 64 + c;
      float v = 0.f;
      if (ci < a.Cin && (unsigned)gy_ < (unsigned)a.H && (unsigned)gx_ < (unsigned)a.W)
        v = xn[(size_t)ci * HW + (size_t)gy_ * a.W + gx_];
      s_x[c * PLANEP + r] = v;
    }
    __syncthreads();
    if (cbk == 0 && tid < 64) {
      float s = 0.f;
#pragma unroll 8
      for (int p = 0; p < NPX; ++p) s += s_g[tid * GROW + p];
      db += s;
    }
#pragma unroll 4
    for (int kk = 0; kk < NPX / 2; ++kk) {
      const int p = 2 * kk + hi;
      const int py = p >> 5, px = p & 31;
      const float av = s_g[(ot * 32 + lo) * GROW + p];
      const float* bx = s_x + (ct * 32 + lo) * PLANEP + (py * S) * IW + px * S;
#pragma unroll
      for (int t = 0; t < KK; ++t) {
        const int ty = t / KS, tx = t - ty * KS;
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bx[ty * IW + tx], acc[t], 0, 0, 0);
      }
    }
  }

  // ---- partial[slot][tap][o][c]  (o, c padded to the 64-blocks of the grid), slot = split % nslot
  const int OP = a.nob * 64, CP = a.ncb * 64;
  const int slot = sp.slot;
#pragma unroll
  for (int t = 0; t < KK; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = ob * 64 + ot * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      const int c = cbk * 64 + ct * 32 + lo;
      unsafeAtomicAdd(a.partial + (((size_t)slot * KK + t) * OP + o) * CP + c, acc[t][r]);
    }
  if (cbk == 0 && tid < 64) unsafeAtomicAdd(a.dbp + (size_t)slot * OP + ob * 64 + tid, db);
}

// -------------------------------------------------------------------------------------------------
// Pipelined variant for the stride-1 layers (3x3: all but two of EDVR's convolutions; 2x2 and 1x1: the
// estimator's re-expressed 4x4 convs, the TSA / fusion 1x1s and the DCN weight gradient).  Same
// decomposition and flush as above; what changes is how a tile gets into LDS:
//   * the tile of the NEXT iteration is fetched into registers before the MFMAs of the current one
//     (64 loads per lane, all in flight together) and written to the other LDS buffer after 3/4 of
//     them -- the simple kernel above pays a full memory latency per loop iteration of its staging
//     loops (measured: ~55 us per 64-pixel tile at 44x80, against 8.5 us of MFMA work);
//   * every wave stages whole channels (wave w: channels 16w..16w+15 of both operands), so a load's
//     address is a scalar channel-plane base plus a per-lane 32-bit offset that is fixed for the tile;
//   * the bias gradient falls out of the A operands the MFMA loop reads anyway (one v_add per k-step).
// 2 x 51.7 KB of LDS: one workgroup per CU, which is also what the pixel split produces.
// -------------------------------------------------------------------------------------------------
template <int KS, bool KYS = false>
__global__ __launch_bounds__(256, KYS ? 2 : 1) void conv2d_wgrad_pipe_kernel(WgradK a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // (7x7 / 9x9 kernel rows: 112 / 144 accumulators at two workgroups per CU leave no room for the fast path's operand ring)
  if constexpr (KS <= 3) {
    if (a.Cin - (int)blockIdx.z * 64 > 32 && a.Cout - (int)blockIdx.y * 64 > 32) {
      if (a.vx == 4) conv2d_wgrad_wide_item<KS, KYS, 4>(a, blockIdx.x, blockIdx.y, blockIdx.z, smem);
      else if (a.vx == 2) conv2d_wgrad_wide_item<KS, KYS, 2>(a, blockIdx.x, blockIdx.y, blockIdx.z, smem);
      else conv2d_wgrad_pipe_item<KS, KYS, true>(a, blockIdx.x, blockIdx.y, blockIdx.z, smem);
      return;
    }
  }
  conv2d_wgrad_pipe_item<KS, KYS, false>(a, blockIdx.x, blockIdx.y, blockIdx.z, smem);
}

// dW[o][c_off + c][tap] = sum_s partial[s][tap][o][c];  db[o] = sum_s dbp[s][o], for a table of layers in ONE launch
// (blockIdx.y = layer): on the small inner-step clips a per-layer reduce is a 6 us kernel plus a launch gap behind every 44 us
// weight-gradient kernel.  The slots are zeroed again while they are read, so the next wgrad launch on the same scratch can
// accumulate into them without a memset of its own (conv2d_wgrad_run's `scratch_is_zero` contract).
__global__ void wgrad_reduce_batch_kernel(WgradReduceTable t) {
  const WgradReduceEntry& e = t.e[blockIdx.y];
  const int g = blockIdx.z;   // group of a per-group gradient (launch: z = the largest group count of the table)
  if (g >= e.ngroups) return;
  float* const partial = e.partial + (size_t)g * e.nslot * e.KK * e.OP * e.CP;
  float* const dbp = e.dbp + (size_t)g * e.nslot * e.OP;
  float* const dW = e.dW + (size_t)g * e.dW_gs;
  float* const db = e.db ? e.db + (size_t)g * e.db_gs : nullptr;
  const int total = e.Cout * e.Cin * e.KK;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int c = i % e.Cin;
    const int t2 = i / e.Cin;
    const int o = t2 % e.Cout;
    const int tp = t2 / e.Cout;
    float s = 0.f;
    for (int sp = 0; sp < e.nslot; ++sp) {
      float* q = partial + (((size_t)sp * e.KK + tp) * e.OP + o) * e.CP + c;
      s += *q;
      *q = 0.f;
    }
    dW[((size_t)o * e.Ctot + e.c_off + c) * e.KK + tp] = s;
  }
  for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < e.OP; o += gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int sp = 0; sp < e.nslot; ++sp) {
      s += dbp[(size_t)sp * e.OP + o];
      dbp[(size_t)sp * e.OP + o] = 0.f;
    }
    if (db && o < e.Cout) db[o] = s;
  }
}

int wgrad_reduce_batch(const WgradReduceEntry* entries, int n, hipStream_t st, int blocks) {
  for (int base = 0; base < n; base += WGRAD_REDUCE_BATCH) {
    WgradReduceTable t;
    t.n = n - base < WGRAD_REDUCE_BATCH ? n - base : WGRAD_REDUCE_BATCH;
    int gmax = 1;
    for (int i = 0; i < t.n; ++i) { t.e[i] = entries[base + i]; gmax = t.e[i].ngroups > gmax ? t.e[i].ngroups : gmax; }
    hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3(blocks, t.n, gmax), dim3(256), 0, st, t);
    int rc = check_launch("wgrad_reduce_batch_kernel");
    if (rc) return rc;
  }
  return DVSR_OK;
}

// ---- launch geometry ----------------------------------------------------------------------------------------
// One function per decision; conv2d_wgrad_choose below lists them in priority order.

// The rule's A/B switches are the DVSR_WGRAD_* rows of switches.h; every other figure is a named constant beside its decision.
bool wgrad_split3_default() { return sw(Sw::WGRAD_SPLIT3); }

// The kernel argument without the rule's answers and the slot pointers: the descriptor's defaults resolved, and the tiling every
// kernel shares (2 x 32-pixel tiles, 64 x 64 (cout, cin) blocks)
static WgradK wgrad_shape(const WgradDesc& d) {
  WgradK k = {};
  k.x = d.x; k.gy = d.gy; k.x_bs = d.x_bs > 0 ? d.x_bs : (long long)d.Cin * d.H * d.W; k.x_bdiv = d.x_bdiv > 0 ? d.x_bdiv : 1;
  k.N = d.N; k.Cin = d.Cin; k.H = d.H; k.W = d.W; k.Cout = d.Cout; k.pad = d.pad < 0 ? d.ks / 2 : d.pad; k.gy_ps = d.gy_ps;
  k.Ho = (d.H + 2 * k.pad - d.ks) / d.stride + 1;
  k.Wo = (d.W + 2 * k.pad - d.ks) / d.stride + 1;
  k.tiles_x = ceil_div(k.Wo, 32); k.tiles_y = ceil_div(k.Ho, 2);
  k.ngroups = d.groups < 1 ? 1 : d.groups; k.gtiles = k.tiles_x * k.tiles_y * (d.N / k.ngroups); k.ntiles = k.gtiles * k.ngroups;
  k.nob = ceil_div(d.Cout, 64); k.ncb = ceil_div(d.Cin, 64);
  return k;
}
static long long work(const WgradK& k) { return (long long)k.ntiles * k.nob * k.ncb; }
// a launch-wide split count -> per group (rounded DOWN: the un-split kernel runs one workgroup per CU, and 12 groups x
// ceil(256 / 12) = 264 workgroups are two rounds on 256 CUs -- the batched inner step measured 6.07 ms per frame at 12 frames
// against 5.38 at 8 and 5.09 at 16), never more than a group has tiles
static int per_group(const WgradK& k, int s) {
  s = k.ngroups > 1 ? s / k.ngroups : s;
  return s > k.gtiles ? k.gtiles : (s < 1 ? 1 : s);
}

// Pixel splits of the fp32 kernels: one workgroup per CU for the pipelined kernel (its LDS allows no more; latency-bound on small
// grids: every extra tile per workgroup is serial time), two per CU for the simple kernel on big grids.  The launch as a whole
// (groups x splits x cout blocks x cin blocks) aims at the same number of workgroups as an ungrouped one over the same tensor.
// (the estimator's 4x4 stride-2 convs, ks == 2 here: 128 / 256 / 512 / 1024 workgroups per launch measured 2.79 / 2.51 /
// 2.54 / 2.56 ms per MFDN forward+backward -- the kernel is staging-bound, 16 accumulator tiles per staged tile against
// 36 for 3x3, not parallelism-bound)
static int base_splits(const WgradDesc& d, const WgradK& k) {
  int s = ceil_div((k.ntiles >= 2048 && d.stride != 1) ? 512 : 256, k.nob * k.ncb);
  if (s > k.ntiles) s = k.ntiles;
  return per_group(k, s < 1 ? 1 : s);
}
// The flush slots, and what conv2d_wgrad_workspace_bytes sizes: the later decisions only lower the split count.
constexpr int WGRAD_MAX_SLOTS = 8;
static int max_slots(const WgradDesc& d, const WgradK& k) { return std::min(base_splits(d, k), WGRAD_MAX_SLOTS); }

// The operands the launch gets: the bf16 kernels are 3x3 stride 1; the split kernel also has a 2x2 form.  0: fp32.
static int operand_mode(const WgradDesc& d) {
  return (d.mode && d.stride == 1 && (d.ks == 3 || (d.ks == 2 && d.mode == 2))) ? d.mode : 0;
}

// The bf16 kernels are staging- and flush-bound (36 MFMAs per tile): fewer workgroups, each with more tiles, keep the
// 147 KB-per-workgroup atomic flush small.  128 at the 64x64 tiles of configs[4] -- sweep in profiles/r02_z_bf16_wgrad.txt --
// growing with the pixel grid: about eight tiles per workgroup, at most 512 workgroups.
constexpr int BF_MIN_WGS = 128, BF_MAX_WGS = 512, BF_TILES_PER_WG = 8;
static int bf_splits(const WgradK& k) {
  const int target = std::max(BF_MIN_WGS, std::min(BF_MAX_WGS, k.ntiles / BF_TILES_PER_WG));
  return per_group(k, ceil_div(target, k.nob * k.ncb));
}

// fp32, small pixel grids: one kernel row per workgroup (conv2d_wgrad_pipe_kernel<3, true>), the pixel split sized for ~two
// workgroups per CU over the three rows; 7x7 / 9x9 always (their 49 / 81 accumulators would not fit the register file).
// 1024 (r03; 4096 before): the row split pays when a workgroup would otherwise get less than ~4 tiles; above that its three-fold
// re-staging of x costs more than the parallelism gives -- the batched inner step (8 frames, 40 x 44x80 = 2640 tiles per layer)
// measured 5.96 ms per frame with the row split on those layers and 5.45 without (profiles/r03_inner_batch_sweeps.txt).
constexpr long long PIPE_ROW_SPLIT_BELOW = 1024;   // tiles x cout blocks x cin blocks
constexpr int PIPE_ROW_SPLIT_WGS = 288, PIPE_ROW_SPLIT_WGS_7_9 = 512;
static bool pipe_row_split(const WgradDesc& d, const WgradK& k) {
  return (d.ks == 3 && d.stride == 1 && work(k) < PIPE_ROW_SPLIT_BELOW) || d.ks == 7 || d.ks == 9;
}
static int pipe_row_splits(const WgradDesc& d, const WgradK& k) {
  return per_group(k, ceil_div(d.ks == 3 ? PIPE_ROW_SPLIT_WGS : PIPE_ROW_SPLIT_WGS_7_9, d.ks * k.nob * k.ncb));
}

// Wide staging: gy rows as float4 (Wo % 4 == 0, not pixel-shuffled), x as float4 / float2 when the row pitch, the batch stride
// and the pointers allow it.  The fp32 pipelined kernel and the split kernel have the same two vector forms; plain bf16 has none.
static int vector_width(const WgradDesc& d, const WgradK& k, int bf) {
  const bool gy_ok = !k.gy_ps && k.Wo % 4 == 0 && ((uintptr_t)k.gy & 15) == 0;
  if (!sw(Sw::WGRAD_WIDE) || !gy_ok || d.stride != 1 || d.ks > 3 || bf == 1) return 0;
  if (k.W % 4 == 0 && k.x_bs % 4 == 0 && ((uintptr_t)k.x & 15) == 0) return 4;
  if (k.W % 2 == 0 && k.x_bs % 2 == 0 && ((uintptr_t)k.x & 7) == 0) return 2;
  return 0;
}

// The split's vector-staging kernels exist for 3x3 with pad 0 / 1 and for the 2x2 form with pad 0 (any other pad runs the
// scalar-staging kernel), and address a sample with 32-bit byte offsets.
static bool split_vector_staging(const WgradDesc& d, const WgradK& k, int vx) {
  const bool vec_form = (d.ks == 3 && (k.pad == 0 || k.pad == 1)) || (d.ks == 2 && k.pad == 0);
  const bool fits = (unsigned long long)k.Cin * k.H * k.W < (1ull << 30) && (unsigned long long)k.Cout * k.Ho * k.Wo < (1ull << 30);
  return sw(Sw::WGRAD_S3V) && vx != 0 && vec_form && fits;
}
// The vector-staging form can run one kernel ROW per workgroup, two workgroups per CU (conv2d_wgrad_bf16.hip:
// conv2d_wgrad_split3v_kernel<.., KYS>).  It stages gy three times and x one and a half times, so it pays where a workgroup has
// few tiles and the fixed costs (first loads, flush, the tail of the last round) weigh most -- measured (tools/wgrad_bench.py,
// us with / without): 40 x 44x80 93 / 102, 8 x 44x80 40 / 51, 40 x 22x40 47 / 61, 1 x 176x320 52 / 63, but 40 x 176x320
// 1046 / 941, 64 -> 216 at 40 x 44x80 290 / 264.
static bool split_row_split(const WgradK& k) { return work(k) < sw(Sw::WGRAD_S3_KYS_BELOW); }
// two workgroups per CU from ~1000 tiles, one below; rounded DOWN (one workgroup more than the CUs hold at once is a second
// round with one workgroup in it)
static int split_row_splits(const WgradDesc& d, const WgradK& k) {
  const int wgs = sw(Sw::WGRAD_S3_WGS) > 0 ? sw(Sw::WGRAD_S3_WGS) : (work(k) >= 1000 ? 512 : 256);
  return per_group(k, wgs / (d.ks * k.nob * k.ncb));
}
// The eight-wave form (two waves per SIMD, 16x16x32 MFMAs) for the float4-staged launches that are not row-split: 7 - 14 % per
// launch over the four-wave form (profiles/r05_wgrad_s3w.txt); the float2 forms spill there and stay on four waves.
static bool split_eight_waves(int vx) { return sw(Sw::WGRAD_S3W) && vx == 4; }

static WgradGeo choose(const WgradDesc& d, const WgradK& k) {
  WgradGeo g;
  const int bf = operand_mode(d);
  g.nsplit = base_splits(d, k);
  g.vx = vector_width(d, k, bf);
  if (bf == 2) {
    g.nsplit = std::min(g.nsplit, bf_splits(k));
    const bool vec = split_vector_staging(d, k, g.vx);
    g.row_split = vec && split_row_split(k);
    if (g.row_split) g.nsplit = split_row_splits(d, k);
    g.kernel = !vec ? WgradKernel::SPLIT_SCALAR
                    : (!g.row_split && split_eight_waves(g.vx) ? WgradKernel::SPLIT_WAVE8 : WgradKernel::SPLIT_VECTOR);
  } else if (bf == 1) {
    g.nsplit = std::min(g.nsplit, bf_splits(k));
    g.kernel = WgradKernel::BF16;
  } else {
    g.row_split = pipe_row_split(d, k);
    if (g.row_split) g.nsplit = pipe_row_splits(d, k);
    g.kernel = d.stride == 1 ? WgradKernel::PIPE : WgradKernel::SIMPLE;
  }
  g.nslot = std::min(max_slots(d, k), g.nsplit);
  g.grid = dim3((g.row_split ? d.ks : 1) * k.ngroups * g.nsplit, k.nob, k.ncb);
  g.block = g.kernel == WgradKernel::SPLIT_WAVE8 ? 512 : 256;
  return g;
}
WgradGeo conv2d_wgrad_choose(const WgradDesc& d) { return choose(d, wgrad_shape(d)); }

// slot regions: [group][slot][tap][o][c] partial sums, then [group][slot][o] bias sums
static size_t partial_floats(const WgradDesc& d, const WgradK& k, int nslot) {
  return (size_t)k.ngroups * nslot * d.ks * d.ks * k.nob * 64 * k.ncb * 64;
}
static size_t slot_bytes(const WgradDesc& d, const WgradK& k, int nslot) {
  return (partial_floats(d, k, nslot) + (size_t)k.ngroups * nslot * k.nob * 64) * sizeof(float);
}
size_t conv2d_wgrad_workspace_bytes(const WgradDesc& d) {
  const WgradK k = wgrad_shape(d);
  return slot_bytes(d, k, max_slots(d, k));
}

static int wgrad_check(const WgradDesc& d) {
  DVSR_REQUIRE(((d.ks == 1 || d.ks == 2 || d.ks == 7 || d.ks == 9) && d.stride == 1) || (d.ks == 3 && (d.stride == 1 || d.stride == 2)),
               DVSR_ERR_UNSUPPORTED, "conv2d_wgrad: ks=%d stride=%d unsupported", d.ks, d.stride);
  DVSR_REQUIRE(d.N % (d.groups < 1 ? 1 : d.groups) == 0, DVSR_ERR_INVALID, "conv2d_wgrad: N=%d is not a multiple of groups=%d", d.N,
               d.groups);
  return DVSR_OK;
}

int conv2d_wgrad_prepare(const WgradDesc& d, void* ws, size_t ws_bytes, hipStream_t st, int scratch_is_zero, WgradReduceEntry* entry,
                         WgradLaunch* out) {
  DVSR_REQUIRE(d.x && d.gy && d.dW && ws, DVSR_ERR_INVALID, "conv2d_wgrad: null pointer");
  int rc = wgrad_check(d);
  if (rc) return rc;
  WgradK& k = out->k;
  k = wgrad_shape(d);
  const size_t need = slot_bytes(d, k, max_slots(d, k));
  DVSR_REQUIRE(ws_bytes >= need, DVSR_ERR_WORKSPACE, "conv2d_wgrad: workspace %zu < %zu", ws_bytes, need);
  const WgradGeo g = choose(d, k);
  k.nsplit = g.nsplit; k.nslot = g.nslot; k.vx = g.vx;
  out->geo = g; out->ks = d.ks;
#ifdef DVSR_CONV_TRACE
  { static const int nf = sw(Sw::WGRAD_NOFLUSH); k.noflush = nf; }
  k.trace = g_wgrad_trace;
#endif
  k.partial = (float*)ws;
  k.dbp = k.partial + partial_floats(d, k, k.nslot);
  if (!scratch_is_zero)
    DVSR_REQUIRE(hipMemsetAsync(ws, 0, slot_bytes(d, k, k.nslot), st) == hipSuccess, DVSR_ERR_HIP, "conv2d_wgrad: memset failed");
  *entry = WgradReduceEntry{k.partial, k.dbp, d.dW, d.db, k.nslot, d.ks * d.ks, k.nob * 64, k.ncb * 64, d.Cout, d.Cin, d.Ctot, d.c_off};
  entry->ngroups = k.ngroups; entry->dW_gs = d.dW_gs; entry->db_gs = d.db_gs;
  return DVSR_OK;
}

template <int KS, bool KYS>
static void launch_pipe(const WgradLaunch& l, hipStream_t st) {
  constexpr size_t lds_a = WgPipeShape<KS, KYS>::LDS_BYTES;
  constexpr size_t lds_b = KS <= 3 ? (WgWideShape<KS, KYS, 4>::LDS_BYTES > WgWideShape<KS, KYS, 2>::LDS_BYTES
                                          ? WgWideShape<KS, KYS, 4>::LDS_BYTES : WgWideShape<KS, KYS, 2>::LDS_BYTES) : 0;
  constexpr size_t lds = lds_a > lds_b ? lds_a : lds_b;
  static PerDeviceOnce attr_once;
  set_dyn_lds_once(attr_once, (const void*)conv2d_wgrad_pipe_kernel<KS, KYS>, lds);
  hipLaunchKernelGGL((conv2d_wgrad_pipe_kernel<KS, KYS>), l.geo.grid, dim3(l.geo.block), lds, st, l.k);
}

int conv2d_wgrad_launch(const WgradLaunch& l, hipStream_t st) {
  switch (l.geo.kernel) {
    case WgradKernel::BF16: return conv2d_wgrad_bf16_launch(l, st);
    case WgradKernel::SPLIT_SCALAR: case WgradKernel::SPLIT_VECTOR: case WgradKernel::SPLIT_WAVE8:
      return conv2d_wgrad_split3_launch(l, st);
    case WgradKernel::SIMPLE: {   // 3x3 stride 2 (wgrad_check)
      using Sh = WgShape<3, 2>;
      static PerDeviceOnce attr_once;
      set_dyn_lds_once(attr_once, (const void*)conv2d_wgrad_kernel<3, 2>, Sh::LDS_BYTES);
      hipLaunchKernelGGL((conv2d_wgrad_kernel<3, 2>), l.geo.grid, dim3(l.geo.block), Sh::LDS_BYTES, st, l.k);
      break;
    }
    case WgradKernel::PIPE:
      if (l.ks == 7) launch_pipe<7, true>(l, st);
      else if (l.ks == 9) launch_pipe<9, true>(l, st);
      else if (l.ks == 3 && l.geo.row_split) launch_pipe<3, true>(l, st);
      else if (l.ks == 3) launch_pipe<3, false>(l, st);
      else if (l.ks == 2) launch_pipe<2, false>(l, st);
      else launch_pipe<1, false>(l, st);
      break;
  }
  return check_launch("conv2d_wgrad_kernel");
}

int conv2d_wgrad_run(const WgradDesc& d, void* ws, size_t ws_bytes, hipStream_t st, int scratch_is_zero, WgradReduceEntry* defer) {
  WgradLaunch l;
  WgradReduceEntry own;
  int rc = conv2d_wgrad_prepare(d, ws, ws_bytes, st, scratch_is_zero, defer ? defer : &own, &l);
  if (rc) return rc;
  rc = conv2d_wgrad_launch(l, st);
  if (rc || defer) return rc;
  return wgrad_reduce_batch(&own, 1, st, ceil_div(d.Cout * d.Cin * d.ks * d.ks, 256));   // (alone on the stream: a thread per element)
}

// The weight gradient of a C-ABI descriptor's first input (plain layout, dense dW)
static WgradDesc wgrad_desc_of(const dvsr_conv2d_desc& d, const float* gy, float* gw, float* gb) {
  WgradDesc w;
  w.x = d.x0; w.x_bs = d.x0_bstride; w.gy = gy; w.gy_ps = d.pixel_shuffle ? 1 : 0; w.dW = gw; w.db = gb;
  w.N = d.N; w.Cin = d.c0; w.H = d.H; w.W = d.W; w.Cout = d.Cout; w.Ctot = d.c0 + d.c1; w.c_off = 0;
  w.ks = d.ks; w.stride = d.stride; w.pad = d.pad;
  return w;
}

}  // namespace dvsr

extern "C" size_t dvsr_conv2d_backward_workspace_bytes(const dvsr_conv2d_desc* d) {
  if (!d) return 0;
  dvsr::WgradDesc w = dvsr::wgrad_desc_of(*d, nullptr, nullptr, nullptr);
  w.Cin = d->c0 > d->c1 ? d->c0 : d->c1; w.pad = d->ks / 2;
  return dvsr::conv2d_wgrad_workspace_bytes(w);
}

// What dvsr_conv2d_wgrad_bf16 / _split3 (mode 1 / 2) or dvsr_conv2d_backward (mode 0; it pads by ks / 2) launch for d's first
// input, gy at an address aligned like d->y, `groups` per-group gradients: geo = {WgradKernel, row_split, vx, nsplit, nslot,
// grid x, y, z}.  Launches nothing and needs no device.
extern "C" int dvsr_conv2d_wgrad_geometry(const dvsr_conv2d_desc* d, int mode, int groups, int geo[8]) {
  DVSR_REQUIRE(d && geo && mode >= 0 && mode <= 2 && groups >= 1, DVSR_ERR_INVALID, "conv2d_wgrad_geometry: invalid argument");
  dvsr::WgradDesc w = dvsr::wgrad_desc_of(*d, d->y, nullptr, nullptr);
  w.mode = mode; w.groups = groups;
  int rc = dvsr::wgrad_check(w);
  if (rc) return rc;
  const dvsr::WgradGeo g = dvsr::conv2d_wgrad_choose(w);
  geo[0] = static_cast<int>(g.kernel); geo[1] = g.row_split; geo[2] = g.vx; geo[3] = g.nsplit; geo[4] = g.nslot;
  geo[5] = (int)g.grid.x; geo[6] = (int)g.grid.y; geo[7] = (int)g.grid.z;
  return DVSR_OK;
}
// The workspace of that launch (dvsr_conv2d_backward_workspace_bytes is the groups = 1, pad = ks / 2 case over the wider input)
extern "C" size_t dvsr_conv2d_wgrad_workspace_bytes(const dvsr_conv2d_desc* d, int groups) {
  if (!d) return 0;
  dvsr::WgradDesc w = dvsr::wgrad_desc_of(*d, nullptr, nullptr, nullptr);
  w.groups = groups;
  return dvsr::conv2d_wgrad_workspace_bytes(w);
}

// Backward of dvsr_conv2d_forward for the plain layout (no pixel shuffle): `gy` is the gradient
// w.r.t. the PRE-activation output (the caller multiplies by act' first).  Any of gx0/gx1/gw/gb
// may be NULL to skip it.  gx1 has the shape of x1 only when x1_bdiv == 1.
extern "C" int dvsr_conv2d_backward(const dvsr_conv2d_desc* d, const float* gy, float* gx0, float* gx1,
                                    float* gw, float* gb, void* workspace, size_t workspace_bytes,
                                    dvsr_stream_t stream) {
  using namespace dvsr;
  DVSR_REQUIRE(d && gy, DVSR_ERR_INVALID, "conv2d_backward: null argument");
  DVSR_REQUIRE(d->pixel_shuffle == 0 && d->x1_bdiv <= 1, DVSR_ERR_UNSUPPORTED,
               "conv2d_backward: pixel_shuffle / broadcast x1 are handled by the EDVR engine only");
  hipStream_t st = (hipStream_t)stream;
  const int pad = d->ks / 2, ctot = d->c0 + d->c1;
  const int Ho = (d->H + 2 * pad - d->ks) / d->stride + 1, Wo = (d->W + 2 * pad - d->ks) / d->stride + 1;
  int rc;
  if (gw) {
    WgradDesc w = wgrad_desc_of(*d, gy, gw, gb);
    w.pad = pad;
    rc = conv2d_wgrad_run(w, workspace, workspace_bytes, st);
    if (rc) return rc;
    if (d->c1) {
      w.x = d->x1; w.x_bs = d->x1_bstride; w.Cin = d->c1; w.c_off = d->c0; w.db = nullptr;
      rc = conv2d_wgrad_run(w, workspace, workspace_bytes, st);
      if (rc) return rc;
    }
  }
  for (int which = 0; which < 2; ++which) {
    float* gx = which ? gx1 : gx0;
    const int ci = which ? d->c1 : d->c0;
    if (!gx || !ci) continue;
    dvsr_conv2d_desc g = {};
    g.x0 = gy; g.w = d->w; g.y = gx; g.N = d->N; g.c0 = d->Cout; g.Cout = ci; g.ks = d->ks; g.stride = 1;
    g.pad = pad; g.act = ACT_NONE; g.x1_bdiv = 1;
    ConvExtra ex;
    ex.wt = 1; ex.w_ctot = ctot; ex.w_coff = which ? d->c0 : 0;
    if (d->stride == 2) { ex.in_dil = 2; ex.Hs = Ho; ex.Ws = Wo; g.H = d->H; g.W = d->W; }
    else { g.H = Ho; g.W = Wo; }
    rc = conv2d_run(g, ex, st);
    if (rc) return rc;
  }
  return DVSR_OK;
}

// Weight / bias gradient of a single-input 3x3 stride-1 conv with bf16 operands on the bf16 MFMA (fp32 accumulate):
// the op-level face of conv2d_wgrad_bf16.hip (the EDVR plan uses it when network_G.bf16_mfma = 1).  Workspace:
// dvsr_conv2d_backward_workspace_bytes.
static int wgrad_bf_mode(const dvsr_conv2d_desc* d, const float* gy, float* gw, float* gb, void* workspace,
                         size_t workspace_bytes, dvsr_stream_t stream, int mode) {
  using namespace dvsr;
  DVSR_REQUIRE(d && gy && gw && d->x0, DVSR_ERR_INVALID, "conv2d_wgrad_bf16: null argument");
  DVSR_REQUIRE(d->ks == 3 && d->stride == 1 && d->c1 == 0 && d->pixel_shuffle == 0, DVSR_ERR_UNSUPPORTED,
               "conv2d_wgrad_bf16: 3x3 stride-1 single-input convolutions only");
  WgradDesc w = wgrad_desc_of(*d, gy, gw, gb);
  w.mode = mode;
  return conv2d_wgrad_run(w, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int dvsr_conv2d_wgrad_bf16(const dvsr_conv2d_desc* d, const float* gy, float* gw, float* gb, void* workspace,
                                      size_t workspace_bytes, dvsr_stream_t stream) {
  return wgrad_bf_mode(d, gy, gw, gb, workspace, workspace_bytes, stream, 1);
}

// The same on the exact 3-way bf16 split of both operands (fp32 accuracy; what the plans run for their 3x3 stride-1 weight
// gradients unless DVSR_WGRAD_SPLIT3=0).
extern "C" int dvsr_conv2d_wgrad_split3(const dvsr_conv2d_desc* d, const float* gy, float* gw, float* gb, void* workspace,
                                        size_t workspace_bytes, dvsr_stream_t stream) {
  return wgrad_bf_mode(d, gy, gw, gb, workspace, workspace_bytes, stream, 2);
}

