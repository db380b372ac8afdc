// fw_resample_limbs.h — the limb arithmetic of systematic resampling (fw_resample.hip) as plain
// functions on 32- and 64-bit words: the host compiles the same text
// (tests/resample_div_check.cpp), as it does for fw_overlap_bits.h.
//
//   fw_rsm_point(j, u, T, C) = floor(((j 2^32 + u) T) / (C 2^32))
//
// for j < C <= 2^20, u < 2^32 and T <= 2^50: point j of the C evenly spaced points, offset by the
// one draw u, on the line [0, T) of the cumulative weights.  The product is below 2^102, so it is
// carried in four 32-bit limbs; the lowest limb is dropped (the division by 2^32: floor(floor(N /
// 2^32) / C) = floor(N / (C 2^32))) and the other three are divided by C limb by limb, every
// partial dividend (rem 2^32 + limb) < C 2^32 <= 2^52.  No 128-bit type is used: its division does
// not link on the device.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FW_RSM_FN __host__ __device__ __forceinline__
#else
#define FW_RSM_FN static inline
#endif

#define FW_RSM_MAX_CHAINS (1 << 20)  // C <= 2^20: j 2^32 + u < 2^52
#define FW_RSM_ONE (1u << 30)        // the heaviest chain's weight

FW_RSM_FN uint64_t fw_rsm_point(uint32_t j, uint32_t u, uint64_t T, uint32_t C) {
  const uint64_t t0 = (uint32_t)T, t1 = T >> 32;  // T = t1 2^32 + t0
  // (j 2^32 + u) (t1 2^32 + t0) = j t1 2^64 + (j t0 + u t1) 2^32 + u t0, column by column
  const uint64_t c0 = (uint64_t)u * t0;
  const uint64_t m1 = (uint64_t)j * t0, m2 = (uint64_t)u * t1;  // each < 2^64: summed in halves
  const uint64_t c1 = (c0 >> 32) + (uint32_t)m1 + (uint32_t)m2;                 // limb 1 and its carry
  const uint64_t c2 = (c1 >> 32) + (m1 >> 32) + (m2 >> 32) + (uint32_t)((uint64_t)j * t1);
  const uint64_t c3 = (c2 >> 32) + (((uint64_t)j * t1) >> 32);
  // limbs 3, 2, 1 of the product = limbs 2, 1, 0 of floor(product / 2^32)
  const uint64_t l2 = (uint32_t)c3, l1 = (uint32_t)c2, l0 = (uint32_t)c1;
  uint64_t rem = l2 % C;  // l2 / C == 0 whenever the point is below T < 2^64
  const uint64_t d1 = (rem << 32) | l1;
  const uint64_t q1 = d1 / C;
  rem = d1 % C;
  const uint64_t d0 = (rem << 32) | l0;
  const uint64_t q0 = d0 / C;
  return (q1 << 32) + q0;
}
