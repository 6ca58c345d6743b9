// The sample side of the frame kernels (frame_yuv.hip, frame_rgb.hip, frame_cut.hip): little-endian groups of 8-bit or 16-bit
// samples at any sample-aligned address, loaded and stored in naturally aligned pieces.  No access is wider than its address is
// aligned (relaxed atomics of wavefront scope: plain accesses that are never merged into wider, possibly misaligned ones) and
// none is narrower than a sample.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace dvsr {

template <typename T>
__device__ __forceinline__ T ld_plain(const unsigned char* p) {
  return __hip_atomic_load(reinterpret_cast<const T*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
template <typename T>
__device__ __forceinline__ void st_plain(unsigned char* p, T v) {
  __hip_atomic_store(reinterpret_cast<T*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// ---- B bytes per sample; groups of 1, 2, 4 samples, loaded (a group stays packed, G4 for four; raw(group, i) is its sample i)
// and stored (from words, one per sample)

struct Bytes8 {
  static constexpr int B = 1;
  struct G4 { unsigned d[1]; };
  static __device__ __forceinline__ unsigned raw(const G4& g, int i) { return (g.d[0] >> (8 * i)) & 0xffu; }
  static __device__ __forceinline__ unsigned ld1(const unsigned char* p) { return ld_plain<unsigned char>(p); }
  static __device__ __forceinline__ unsigned ld2a(const unsigned char* p) { return ld_plain<unsigned short>(p); }   // p even
  static __device__ __forceinline__ unsigned ld2(const unsigned char* p) {
    return (reinterpret_cast<uintptr_t>(p) & 1) ? (ld1(p) | (ld1(p + 1) << 8)) : ld2a(p);
  }
  static __device__ __forceinline__ G4 ld4(const unsigned char* p) {
    const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
    if (m == 0) return G4{{*reinterpret_cast<const unsigned*>(p)}};
    if (m == 2) return G4{{ld2a(p) | (ld2a(p + 2) << 16)}};
    return G4{{ld1(p) | (ld2a(p + 1) << 8) | (ld1(p + 3) << 24)}};
  }
  static __device__ __forceinline__ void st1(unsigned char* p, unsigned v) { st_plain<unsigned char>(p, (unsigned char)v); }
  static __device__ __forceinline__ void st2a(unsigned char* p, unsigned v) { st_plain<unsigned short>(p, (unsigned short)v); }
  static __device__ __forceinline__ void st2(unsigned char* p, const unsigned s[2]) {
    const unsigned v = s[0] | (s[1] << 8);
    if (reinterpret_cast<uintptr_t>(p) & 1) {
      st1(p, v);
      st1(p + 1, v >> 8);
    } else {
      st2a(p, v);
    }
  }
  static __device__ __forceinline__ void st4(unsigned char* p, const unsigned s[4]) {
    const unsigned v = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
    const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
    if (m == 0) {
      *reinterpret_cast<unsigned*>(p) = v;
    } else if (m == 2) {
      st2a(p, v);
      st2a(p + 2, v >> 16);
    } else {
      st1(p, v);
      st2a(p + 1, v >> 8);
      st1(p + 3, v >> 24);
    }
  }
};

struct Words16 {
  static constexpr int B = 2;
  struct G4 { unsigned d[2]; };
  static __device__ __forceinline__ unsigned raw(const G4& g, int i) { return (g.d[i >> 1] >> (16 * (i & 1))) & 0xffffu; }
  static __device__ __forceinline__ unsigned ld1(const unsigned char* p) { return ld_plain<unsigned short>(p); }
  static __device__ __forceinline__ unsigned ld2a(const unsigned char* p) { return ld_plain<unsigned>(p); }   // p 4-aligned
  static __device__ __forceinline__ unsigned ld2(const unsigned char* p) {
    return (reinterpret_cast<uintptr_t>(p) & 2) ? (ld1(p) | (ld1(p + 2) << 16)) : ld2a(p);
  }
  static __device__ __forceinline__ G4 ld4(const unsigned char* p) {
    const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 7);
    unsigned lo, hi;
    if (m == 0) {
      const unsigned long long v = ld_plain<unsigned long long>(p);
      lo = (unsigned)v;
      hi = (unsigned)(v >> 32);
    } else if (m == 4) {
      lo = ld2a(p);
      hi = ld2a(p + 4);
    } else {
      const unsigned a = ld1(p), b = ld2a(p + 2), c = ld1(p + 6);
      lo = a | (b << 16);
      hi = (b >> 16) | (c << 16);
    }
    return G4{{lo, hi}};
  }
  static __device__ __forceinline__ void st1(unsigned char* p, unsigned v) { st_plain<unsigned short>(p, (unsigned short)v); }
  static __device__ __forceinline__ void st2a(unsigned char* p, unsigned v) { st_plain<unsigned>(p, v); }
  static __device__ __forceinline__ void st2(unsigned char* p, const unsigned s[2]) {
    const unsigned v = s[0] | (s[1] << 16);
    if (reinterpret_cast<uintptr_t>(p) & 2) {
      st1(p, v);
      st1(p + 2, v >> 16);
    } else {
      st2a(p, v);
    }
  }
  static __device__ __forceinline__ void st4(unsigned char* p, const unsigned s[4]) {
    const unsigned lo = s[0] | (s[1] << 16), hi = s[2] | (s[3] << 16);
    const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 7);
    if (m == 0) {
      st_plain<unsigned long long>(p, (unsigned long long)lo | ((unsigned long long)hi << 32));
    } else if (m == 4) {
      st2a(p, lo);
      st2a(p + 4, hi);
    } else {
      st1(p, lo);
      st2a(p + 2, (lo >> 16) | (hi << 16));
      st1(p + 6, hi >> 16);
    }
  }
};

// ---- interleaved 16-bit words: the 4 pixels of a lane are a group of NW = 12 (pixel stride 3 words) or 16 (4 words) words at an
// even address p, two words per dword of d.  Of 16 words the last -- the fourth word of the last pixel -- is not needed and is
// read only inside an aligned dword or qword that holds a needed word as well.  p & 7 = 0: qwords; 4: dwords; 2 or 6: a word,
// dwords, and (NW = 12) a word.

__device__ __forceinline__ unsigned word_of(const unsigned* d, int i) { return (d[i >> 1] >> (16 * (i & 1))) & 0xffffu; }

template <int NW>
__device__ __forceinline__ void ld_words(const unsigned char* p, unsigned d[NW / 2]) {
  static_assert(NW == 12 || NW == 16, "4 pixels of 3 or 4 words");
  const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 7);
  if (m == 0) {
#pragma unroll
    for (int k = 0; k < NW / 4; ++k) {
      const unsigned long long v = ld_plain<unsigned long long>(p + 8 * k);
      d[2 * k] = (unsigned)v;
      d[2 * k + 1] = (unsigned)(v >> 32);
    }
  } else if (m == 4) {
#pragma unroll
    for (int k = 0; k < NW / 2; ++k) d[k] = ld_plain<unsigned>(p + 4 * k);
  } else {
    constexpr int NM = NW / 2 - 1;                     // the aligned dwords between the first word and the last
    unsigned mid[NM];
    const unsigned first = ld_plain<unsigned short>(p);
#pragma unroll
    for (int k = 0; k < NM; ++k) mid[k] = ld_plain<unsigned>(p + 2 + 4 * k);
    const unsigned last = NW == 12 ? (unsigned)ld_plain<unsigned short>(p + 2 * NW - 2) : 0u;
    d[0] = first | (mid[0] << 16);
#pragma unroll
    for (int k = 1; k < NM; ++k) d[k] = (mid[k - 1] >> 16) | (mid[k] << 16);
    d[NM] = (mid[NM - 1] >> 16) | (last << 16);
  }
}

// 12 words (4 pixels of 3) from the 6 dwords of d to an even address p, in the same pieces
__device__ __forceinline__ void st_words12(unsigned char* p, const unsigned d[6]) {
  const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(p) & 7);
  if (m == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) st_plain<unsigned long long>(p + 8 * k, (unsigned long long)d[2 * k] | ((unsigned long long)d[2 * k + 1] << 32));
  } else if (m == 4) {
#pragma unroll
    for (int k = 0; k < 6; ++k) st_plain<unsigned>(p + 4 * k, d[k]);
  } else {
    st_plain<unsigned short>(p, (unsigned short)d[0]);
#pragma unroll
    for (int k = 0; k < 5; ++k) st_plain<unsigned>(p + 2 + 4 * k, (d[k] >> 16) | (d[k + 1] << 16));
    st_plain<unsigned short>(p + 22, (unsigned short)(d[5] >> 16));
  }
}

}  // namespace dvsr
