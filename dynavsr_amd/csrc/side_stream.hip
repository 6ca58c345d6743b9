// The weight-gradient side-stream pool and the probe that tells which of its streams runs beside a launch stream.
#include <cstdlib>
#include <mutex>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace dvsr {

// The weight-gradient side streams: a small pool per device for the whole process (never destroyed).  Plans on different
// launch streams share it: their weight gradients then queue behind each other, ordered by the plans' own fork / join events.
// Candidate 0 is THE side stream whenever it runs beside the launch stream; the others exist only for launch streams it
// shares a hardware queue with (side_stream_for).
constexpr int SIDE_POOL = 4;
static hipStream_t pool_side_stream(int i) {
  static std::mutex mu;
  static hipStream_t streams[64][SIDE_POOL] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || i < 0 || i >= SIDE_POOL) { (void)hipGetLastError(); return nullptr; }
  std::lock_guard<std::mutex> lock(mu);
  if (!streams[dev][i] && hipStreamCreateWithFlags(&streams[dev][i], hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    streams[dev][i] = nullptr;
  }
  return streams[dev][i];
}
static hipStream_t shared_side_stream() { return pool_side_stream(0); }

// ---- does work on the side stream run BESIDE work on a launch stream?
// ROCm maps HIP streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default) and two streams that land on one queue run
// behind each other: a plan whose weight gradients sit on such a side stream pays the fork / join events and gets no
// overlap (the inner step measured 10.0 instead of 8.2 ms with an RCCL communicator's streams in the process, r02-r04).
// Which queue a stream gets depends on every stream the process created before -- nothing a plan can know -- so it is
// MEASURED, once per (device, launch stream): a kernel that spins for 150 us on the launch stream, a marker kernel on the
// side stream behind it; the marker's start time tells whether it waited for the spinner.  dvsr_edvr_backward falls back to
// single-stream weight gradients for a launch stream that fails the probe.  DVSR_BWD_PROBE=0 skips it (assume overlap).
__global__ void probe_spin_kernel(long long* out, long long ticks) {
  const long long t0 = __builtin_amdgcn_s_memrealtime();
  long long t = t0;
  while (t - t0 < ticks) { __builtin_amdgcn_s_sleep(8); t = __builtin_amdgcn_s_memrealtime(); }
  out[0] = t0;
  out[1] = t;
}
__global__ void probe_mark_kernel(long long* out) { out[2] = __builtin_amdgcn_s_memrealtime(); }

// 1: overlaps, 0: serialised, -1: could not tell (capturing, allocation failure, probe disabled by the caller)
static int probe_side_overlap(hipStream_t st, hipStream_t side) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return -1; }
  long long* d = nullptr;
  if (hipMalloc(&d, 4 * sizeof(long long)) != hipSuccess) { (void)hipGetLastError(); return -1; }
  int res = -1;
  long long h[4] = {0, 0, 0, 0};
  // (the streams are drained first: what is still queued on either would be measured instead)
  if (hipStreamSynchronize(st) == hipSuccess && hipStreamSynchronize(side) == hipSuccess &&
      hipMemsetAsync(d, 0, sizeof(h), st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess) {
    // (one untimed marker first: the first launch on a fresh stream costs its queue set-up, > 100 us at times -- timed, that is a
    // false "serialised")
    hipLaunchKernelGGL(probe_mark_kernel, dim3(1), dim3(64), 0, side, d);
    (void)hipStreamSynchronize(side);
    (void)hipMemsetAsync(d, 0, sizeof(h), st);
    (void)hipStreamSynchronize(st);
    hipLaunchKernelGGL(probe_spin_kernel, dim3(1), dim3(64), 0, st, d, 15000LL);   // 150 us of the 100 MHz counter
    hipLaunchKernelGGL(probe_mark_kernel, dim3(1), dim3(64), 0, side, d);
    if (hipStreamSynchronize(side) == hipSuccess && hipStreamSynchronize(st) == hipSuccess &&
        hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess && h[1] > h[0] && h[2] > 0)
      res = h[2] < h[1] - 5000 ? 1 : 0;   // the marker started at least 50 us before the spinner ended
  }
  (void)hipGetLastError();
  (void)hipFree(d);
  return res;
}

// The side stream to use beside launch stream `st`: the first of the pool that the probe finds running concurrently with
// it (a new stream lands on another hardware queue than its predecessor, so one of four consecutive candidates is off the
// launch stream's queue unless everything is on one), cached per (device, launch stream).  nullptr: none overlaps -- the
// caller keeps its weight gradients on `st`.  *known = false: the probe could not run (stream capture): candidate 0, unprobed.
hipStream_t side_stream_for(hipStream_t st, bool* known) {
  const bool probe_on = sw(Sw::BWD_PROBE);
  if (known) *known = probe_on;
  if (!probe_on) return shared_side_stream();
  // (a NEGATIVE answer is not kept for ever: the stream -> hardware-queue mapping moves as the process creates streams, and a
  // destroyed stream's handle can come back as another stream -- it is asked again every 64th use)
  struct Entry { int dev; hipStream_t st, side; int uses; };
  static std::mutex mu;
  static std::vector<Entry> cache;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  for (size_t i = 0; i < cache.size(); ++i) {
    Entry& e = cache[i];
    if (e.dev != dev || e.st != st) continue;
    if (e.side || ++e.uses < 64) return e.side;
    cache.erase(cache.begin() + i);   // re-probe below
    break;
  }
  for (int i = 0; i < SIDE_POOL; ++i) {
    hipStream_t cand = pool_side_stream(i);
    if (!cand) break;
    const int r = probe_side_overlap(st, cand);
    if (r < 0) {   // (capturing: no measurement possible, nothing cached)
      if (known) *known = false;
      return shared_side_stream();
    }
    if (r == 1) {
      cache.push_back({dev, st, cand, 0});
      return cand;
    }
  }
  cache.push_back({dev, st, nullptr, 0});
  return nullptr;
}

// 1: a side stream of the pool runs beside `stream` on this device (the plans fork their weight gradients onto it), 0: none
// does (they stay on `stream`), -1: unknown (see probe_side_overlap)
extern "C" int dvsr_side_stream_overlaps(dvsr_stream_t stream) {
  bool known = true;
  hipStream_t side = side_stream_for((hipStream_t)stream, &known);
  if (!known) return -1;
  return side ? 1 : 0;
}

}  // namespace dvsr
