// Window gather of the streaming EDVR forward (engine.hip: dvsr_edvr_stream_fuse).
//
// The frame cache keeps every frame's L1 / L2 / L3 features in one slot; a window of `nframes` frames names its slots in
// window order, and ONE launch copies the nframes x 3 feature planes into the contiguous [nframes][C][h][w] tensors the
// fuse tape reads.  The slot list travels by value in the kernel arguments: no device-side table, no host sync.
//
// Pure HBM streaming (at 5 x 64 x 180 x 320: 97 MB in, 97 MB out), so: 16-byte loads and stores, GATHER_U loads in flight
// per lane, all of a lane's loads issued before its first store, and every lane touches its elements ONCE -- there is no
// grid-stride loop, because a loop's next loads would queue behind this iteration's stores (gfx9 counts both in vmcnt, in
// order: `store ... load ... s_waitcnt vmcnt(0)` waits for the store's acknowledge as well).  Whole chunks take a
// straight-line path without predicated stores; only the last workgroup of a frame runs the predicated one.
#include "common.h"
#include "kernels.h"

namespace dvsr {

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_U = 4;                                  // float4 per lane
constexpr int GATHER_CHUNK = GATHER_THREADS * GATHER_U;      // float4 per workgroup

struct GatherArgs {
  const float* cache;
  float* dst[3];            // L1 / L2 / L3 tensors of the fuse tape, [nframes][n4 * 4]
  long long slot_floats;    // floats between two slots of the cache
  long long src_off[3];     // floats from a slot's start to its level-l features
  long long n4[3];          // float4 per frame at level l
  int slot[DVSR_STREAM_MAX_FRAMES];
};

// element r (in float4) of a frame's concatenated [L1 | L2 | L3] features -> its address, given the three levels' wave-uniform
// bases.  (Plain scalars, not arrays: indexing the kernel-argument arrays -- or a local array -- by a per-lane level makes every
// lane fetch the bases from memory.)
template <class P>
__device__ __forceinline__ P* gather_addr(P* b0, P* b1, P* b2, long long n0, long long n1, long long r) {
  const long long r1 = r - n0, r2 = r1 - n1;
  return r1 < 0 ? b0 + r : (r2 < 0 ? b1 + r1 : b2 + r2);
}

__global__ __launch_bounds__(GATHER_THREADS) void stream_gather_kernel(GatherArgs a) {
  const int f = blockIdx.y;
  const float* slot_base = a.cache + (long long)a.slot[f] * a.slot_floats;
  const long long n0 = a.n4[0], n1 = a.n4[1], n2 = a.n4[2];
  const f32x4* s0 = reinterpret_cast<const f32x4*>(slot_base + a.src_off[0]);
  const f32x4* s1 = reinterpret_cast<const f32x4*>(slot_base + a.src_off[1]);
  const f32x4* s2 = reinterpret_cast<const f32x4*>(slot_base + a.src_off[2]);
  f32x4* d0 = reinterpret_cast<f32x4*>(a.dst[0]) + f * n0;
  f32x4* d1 = reinterpret_cast<f32x4*>(a.dst[1]) + f * n1;
  f32x4* d2 = reinterpret_cast<f32x4*>(a.dst[2]) + f * n2;
  const long long per = n0 + n1 + n2;
  const long long base = (long long)blockIdx.x * GATHER_CHUNK + threadIdx.x;
  if ((long long)(blockIdx.x + 1) * GATHER_CHUNK <= per) {
    f32x4 v[GATHER_U];
#pragma unroll
    for (int j = 0; j < GATHER_U; ++j) v[j] = *gather_addr(s0, s1, s2, n0, n1, base + j * GATHER_THREADS);
#pragma unroll
    for (int j = 0; j < GATHER_U; ++j) *gather_addr(d0, d1, d2, n0, n1, base + j * GATHER_THREADS) = v[j];
  } else {
#pragma unroll
    for (int j = 0; j < GATHER_U; ++j) {
      const long long r = base + j * GATHER_THREADS;
      if (r < per) *gather_addr(d0, d1, d2, n0, n1, r) = *gather_addr(s0, s1, s2, n0, n1, r);
    }
  }
}

int stream_gather_run(const float* cache, size_t slot_floats, const size_t src_off[3], float* const dst[3],
                      const size_t level_floats[3], int nframes, const int* slots, hipStream_t st) {
  DVSR_REQUIRE(cache && slots && nframes > 0 && nframes <= DVSR_STREAM_MAX_FRAMES, DVSR_ERR_INVALID,
               "stream_gather: bad argument (nframes=%d, at most %d)", nframes, DVSR_STREAM_MAX_FRAMES);
  GatherArgs a;
  a.cache = cache;
  a.slot_floats = (long long)slot_floats;
  long long per = 0;
  // 16-byte accesses: every base, offset and length a multiple of 4 floats (arena and cache sections are 64-float aligned)
  DVSR_REQUIRE((uintptr_t)cache % 16 == 0 && slot_floats % 4 == 0, DVSR_ERR_INVALID, "stream_gather: cache not 16-byte aligned");
  for (int l = 0; l < 3; ++l) {
    DVSR_REQUIRE(dst[l] && (uintptr_t)dst[l] % 16 == 0 && src_off[l] % 4 == 0 && level_floats[l] % 4 == 0 && level_floats[l] > 0,
                 DVSR_ERR_INVALID, "stream_gather: level %d is not 16-byte aligned", l);
    a.dst[l] = dst[l];
    a.src_off[l] = (long long)src_off[l];
    a.n4[l] = (long long)(level_floats[l] / 4);
    per += a.n4[l];
  }
  for (int f = 0; f < DVSR_STREAM_MAX_FRAMES; ++f) a.slot[f] = f < nframes ? slots[f] : 0;
  const long long gx = (per + GATHER_CHUNK - 1) / GATHER_CHUNK;
  DVSR_REQUIRE(gx <= 0x7fffffffLL, DVSR_ERR_UNSUPPORTED, "stream_gather: frame too large");
  hipLaunchKernelGGL(stream_gather_kernel, dim3((unsigned)gx, (unsigned)nframes), dim3(GATHER_THREADS), 0, st, a);
  return check_launch("stream_gather_kernel");
}

}  // namespace dvsr
