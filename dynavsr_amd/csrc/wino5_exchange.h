// Index arithmetic of conv2d_wino5_kernel's epilogue exchange (conv2d_wino5.hip), kept apart so that the compiler checks it on
// the host: which 16-byte record of the LDS image a consumer wave writes, which reader wave picks it up, and which cout it is.
//
// A consumer wave (xi, mh) leaves the column transform with Z[j][r], j = 0..3, r = 0..15: MFMA accumulator register r of lane
// (tile, hi) is cout 32 mh + 8 (r / 4) + 4 hi + (r % 4) of the 64-cout block.  rq = r / 4 is the register QUAD, c = r % 4 the
// register inside it.  A record holds the four j of ONE cout -- {Z[0][r], Z[1][r], Z[2][r], Z[3][r]} -- so a reader fetches a
// cout's 6 x 4 values with six conflict-free 16-byte reads and the row transform's result IS the 16-byte output row.
//   unit(mh, rq) = [xi 6][c 4][lane 64] x 16 B = 24 576 B
//   round t (0, 1) carries the units (mh, 2 t) and (mh, 2 t + 1) of BOTH cout halves: four units, 96 KB; all twelve consumer
//   waves write in both rounds (eight records per lane and round).
#pragma once

namespace dvsr {
namespace w5x {

constexpr int NXI = 6, NC = 4, NLANE = 64, REC_F = 4;     // REC_F: floats of a record
constexpr int UNIT_F = NXI * NC * NLANE * REC_F;          // floats of a unit (6144)
constexpr int ROUND_UNITS = 4, ROUNDS = 2;
constexpr int IMG_F = ROUND_UNITS * UNIT_F;               // floats of the exchange image (24 576 = 96 KB)

__host__ __device__ constexpr int round_of(int rq) { return rq >> 1; }
__host__ __device__ constexpr int unit_pos(int mh, int rq) { return 2 * mh + (rq & 1); }   // place of unit (mh, rq) in its round
// float index of the record (xi, c, lane) of unit (mh, rq) -- writer and reader both address through this
__host__ __device__ constexpr int rec(int mh, int rq, int xi, int c, int lane) {
  return unit_pos(mh, rq) * UNIT_F + ((xi * NC + c) * NLANE + lane) * REC_F;
}
// cout (inside the 64-cout block) of accumulator register 4 rq + c in lane half hi of cout half mh: the MFMA's row layout
__host__ __device__ constexpr int cout_of(int mh, int rq, int hi, int c) { return 32 * mh + 8 * rq + 4 * hi + c; }

// sixteen readers (residual / addend instantiations): wave -> one cout of one unit per round
__host__ __device__ constexpr int r16_mh(int wave) { return wave >> 3; }
__host__ __device__ constexpr int r16_rq(int wave, int t) { return 2 * t + ((wave >> 2) & 1); }
__host__ __device__ constexpr int r16_c(int wave) { return wave & 3; }
// eight pair readers (plain instantiation, PixelShuffle(2) included): waves 0..7 -> the couts c, c + 1 of one unit per round
__host__ __device__ constexpr int r8_mh(int wave) { return wave >> 2; }
__host__ __device__ constexpr int r8_rq(int wave, int t) { return 2 * t + ((wave >> 1) & 1); }
__host__ __device__ constexpr int r8_c(int wave) { return 2 * (wave & 1); }

namespace check {
// every record of a round is written exactly once, inside the image: the units of a round neither overlap nor leave it
constexpr bool round_is_a_partition(int t) {
  bool seen[IMG_F / REC_F] = {};
  for (int mh = 0; mh < 2; ++mh)
    for (int rq = 2 * t; rq < 2 * t + 2; ++rq)
      for (int xi = 0; xi < NXI; ++xi)
        for (int c = 0; c < NC; ++c)
          for (int lane = 0; lane < NLANE; ++lane) {
            const int f = rec(mh, rq, xi, c, lane);
            if (round_of(rq) != t || f < 0 || f % REC_F || f + REC_F > IMG_F || seen[f / REC_F]) return false;
            seen[f / REC_F] = true;
          }
  for (bool s : seen)
    if (!s) return false;
  return true;
}
// the readers of a round pick every (mh, rq, c) of that round up exactly once, so every cout 0..63 is stored exactly once over
// the two rounds and lane halves -- and it is the cout the writer's register held
constexpr bool readers_cover(bool pairs) {
  int hits[64] = {};
  for (int t = 0; t < ROUNDS; ++t) {
    bool unit_c[2][4][NC] = {};
    for (int wave = 0; wave < (pairs ? 8 : 16); ++wave)
      for (int k = 0; k < (pairs ? 2 : 1); ++k) {
        const int mh = pairs ? r8_mh(wave) : r16_mh(wave), rq = pairs ? r8_rq(wave, t) : r16_rq(wave, t);
        const int c = (pairs ? r8_c(wave) : r16_c(wave)) + k;
        if (mh > 1 || rq > 3 || c >= NC || round_of(rq) != t || unit_c[mh][rq][c]) return false;
        unit_c[mh][rq][c] = true;
        for (int hi = 0; hi < 2; ++hi) ++hits[cout_of(mh, rq, hi, c)];
      }
  }
  for (int h : hits)
    if (h != 1) return false;
  return true;
}
static_assert(round_is_a_partition(0) && round_is_a_partition(1), "a round's four units tile the exchange image exactly");
static_assert(readers_cover(false), "sixteen readers: every cout of the block exactly once");
static_assert(readers_cover(true), "eight pair readers: every cout of the block exactly once");
static_assert(r8_c(0) % 2 == 0 && r8_c(1) % 2 == 0, "a pair is (even cout, odd cout): PixelShuffle(2)'s dx");
static_assert(cout_of(1, 3, 1, 3) == 63 && cout_of(0, 0, 0, 0) == 0, "MFMA row layout");
}  // namespace check

}  // namespace w5x
}  // namespace dvsr
