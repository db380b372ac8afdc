// fw_overlap_bits.h — the field arithmetic of the plan-overlap kernel (fw_overlap.hip) on packed
// label words, as plain functions on 32-bit words: the host compiles the same text
// (tests/overlap_bits_check.cpp), as it does for fw_window_rows.h.
//
// A group is LB consecutive dwords w[0 .. LB) of a label record, LB one of 2, 3, 4, 5, 8: node
// j < 32 of the group sits in bits [j LB, j LB + LB) of the LB * 32-bit string, so 3- and 5-bit
// fields straddle dwords.  A node mask has bit j for node j.
//
//   fw_ovl_zero_mask<LB>(d)          nodes whose field of d is 0
//   fw_ovl_eq_mask<LB>(w, v)         nodes whose field equals v
//   fw_ovl_pair_mask<LB>(r, x, a, b) nodes whose field of r equals a and whose field of x equals b
//   fw_ovl_diff_mask<LB>(a, b)       nodes whose fields of a and b differ
//   fw_ovl_field<LB>(w, j)           the field of node j (constant indices only: no scratch)
//   fw_ovl_tail_mask(count)          the first count nodes of a group, 1 <= count <= 32
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FW_OVL_FN __host__ __device__ __forceinline__
#else
#define FW_OVL_FN static inline
#endif

// bit 0 of every LB-bit field of a 64-bit string
template <int LB>
FW_OVL_FN uint64_t fw_ovl_ones() {
  return LB == 2   ? 0x5555555555555555ull
         : LB == 3 ? 0x9249249249249249ull
         : LB == 4 ? 0x1111111111111111ull
         : LB == 5 ? 0x1084210842108421ull
                   : 0x0101010101010101ull;
}

// the low dword of {hi, lo} >> s, 0 <= s < 32 (v_alignbit_b32 on the device)
FW_OVL_FN uint32_t fw_ovl_shr(uint32_t hi, uint32_t lo, int s) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> s);
}

// d >>= s over the whole LB-dword string (zeros come in at the top)
template <int LB>
FW_OVL_FN void fw_ovl_or_shr(uint32_t d[LB], int s) {
#pragma unroll
  for (int i = 0; i < LB; ++i) d[i] |= fw_ovl_shr(i + 1 < LB ? d[i + 1] : 0u, d[i], s);
}

// bits 0, LB, 2 LB, ... of x -> bits 0, 1, 2, ... (the other bits of x are ignored)
template <int LB>
FW_OVL_FN uint32_t fw_ovl_compress(uint32_t x) {
  if (LB == 2) {
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0f0f0f0fu;
    x = (x | (x >> 4)) & 0x00ff00ffu;
    x = (x | (x >> 8)) & 0x0000ffffu;
  } else if (LB == 3) {
    x &= 0x49249249u;                  // 0, 3, .., 30
    x = (x | (x >> 2)) & 0xc30c30c3u;  // pairs at 0, 6, .., 30
    x = (x | (x >> 4)) & 0x0f00f00fu;  // fours at 0, 12, 24
    x = (x | (x >> 8)) & 0x0f0000ffu;  // eight at 0, four at 24
    x = (x | (x >> 16)) & 0x00000fffu;
  } else if (LB == 4) {
    x &= 0x11111111u;
    x = (x | (x >> 3)) & 0x03030303u;
    x = (x | (x >> 6)) & 0x000f000fu;
    x = (x | (x >> 12)) & 0x000000ffu;
  } else if (LB == 5) {
    x &= 0x42108421u;                  // 0, 5, .., 30
    x = (x | (x >> 4)) & 0xc0300c03u;  // pairs at 0, 10, 20, 30
    x = (x | (x >> 8)) & 0x00f0000fu;  // fours at 0, 20
    x = (x | (x >> 16)) & 0x000000ffu;
  } else {
    x &= 0x01010101u;
    x = (x | (x >> 7)) & 0x00030003u;
    x = (x | (x >> 14)) & 0x0000000fu;
  }
  return x;
}

// nodes whose field of d is not 0: every field is OR-folded onto its lowest bit (across dwords
// for the straddling widths), then dword i gives the nodes whose fields start in it: the first
// is node ceil(32 i / LB), at bit (LB - 32 i mod LB) mod LB.
template <int LB>
FW_OVL_FN uint32_t fw_ovl_nonzero_mask(const uint32_t d[LB]) {
  uint32_t f[LB];
#pragma unroll
  for (int i = 0; i < LB; ++i) f[i] = d[i];
  if (LB == 2 || LB == 4 || LB == 8) {  // no field crosses a dword
#pragma unroll
    for (int i = 0; i < LB; ++i) {
      f[i] |= f[i] >> 1;
      if (LB >= 4) f[i] |= f[i] >> 2;
      if (LB == 8) f[i] |= f[i] >> 4;
    }
  } else {
    fw_ovl_or_shr<LB>(f, 1);  // bit b: bits b .. b + 1
    if (LB == 5) fw_ovl_or_shr<LB>(f, 2);  // .. b + 3
    fw_ovl_or_shr<LB>(f, 1);  // .. b + LB - 1
  }
  uint32_t m = 0u;
#pragma unroll
  for (int i = 0; i < LB; ++i)
    m |= fw_ovl_compress<LB>(f[i] >> ((LB - (32 * i) % LB) % LB)) << ((32 * i + LB - 1) / LB);
  return m;
}

template <int LB>
FW_OVL_FN uint32_t fw_ovl_zero_mask(const uint32_t d[LB]) {
  return ~fw_ovl_nonzero_mask<LB>(d);
}

// dword i of the string whose every field is v (v < 2^LB): the 64-bit repetition, taken from
// the phase at which dword i starts
template <int LB>
FW_OVL_FN uint32_t fw_ovl_splat(uint64_t rep, int i) {
  return (uint32_t)(rep >> ((32 * i) % LB));
}

template <int LB>
FW_OVL_FN uint32_t fw_ovl_eq_mask(const uint32_t w[LB], uint32_t v) {
  const uint64_t rep = (uint64_t)v * fw_ovl_ones<LB>();
  uint32_t d[LB];
#pragma unroll
  for (int i = 0; i < LB; ++i) d[i] = w[i] ^ fw_ovl_splat<LB>(rep, i);
  return fw_ovl_zero_mask<LB>(d);
}

// one reduction for both records: a field of (r ^ a..) | (x ^ b..) is 0 iff both fields match
template <int LB>
FW_OVL_FN uint32_t fw_ovl_pair_mask(const uint32_t r[LB], const uint32_t x[LB], uint32_t a,
                                    uint32_t b) {
  const uint64_t ra = (uint64_t)a * fw_ovl_ones<LB>(), rb = (uint64_t)b * fw_ovl_ones<LB>();
  uint32_t d[LB];
#pragma unroll
  for (int i = 0; i < LB; ++i)
    d[i] = (r[i] ^ fw_ovl_splat<LB>(ra, i)) | (x[i] ^ fw_ovl_splat<LB>(rb, i));
  return fw_ovl_zero_mask<LB>(d);
}

template <int LB>
FW_OVL_FN uint32_t fw_ovl_diff_mask(const uint32_t a[LB], const uint32_t b[LB]) {
  uint32_t d[LB];
#pragma unroll
  for (int i = 0; i < LB; ++i) d[i] = a[i] ^ b[i];
  return fw_ovl_nonzero_mask<LB>(d);
}

// the field of node j < 32.  The dword pair is picked with compares against constants, so a
// register array is never indexed by a variable (that would put it in scratch).
template <int LB>
FW_OVL_FN uint32_t fw_ovl_field(const uint32_t w[LB], int j) {
  const int bit = j * LB, at = bit >> 5;
  uint32_t lo = w[0], hi = LB > 1 ? w[1] : 0u;
#pragma unroll
  for (int i = 1; i < LB; ++i)
    if (at == i) {
      lo = w[i];
      hi = i + 1 < LB ? w[i + 1] : 0u;
    }
  return fw_ovl_shr(hi, lo, bit & 31) & ((1u << LB) - 1u);
}

FW_OVL_FN uint32_t fw_ovl_tail_mask(int count) {
  return count >= 32 ? 0xffffffffu : (1u << count) - 1u;
}
