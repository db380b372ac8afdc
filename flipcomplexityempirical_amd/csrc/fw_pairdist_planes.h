// fw_pairdist_planes.h — the bit-plane arithmetic of the pairwise plan distance (fw_pairdist.hip),
// as plain functions on 32-bit words: the host compiles the same text
// (tests/pairdist_planes_check.cpp), as it does for fw_overlap_bits.h and fw_window_rows.h.
//
// A group is LB consecutive dwords w[0 .. LB) of a label record (fw_overlap_bits.h): node j < 32
// sits in bits [j LB, j LB + LB) of the LB * 32-bit string, so 3- and 5-bit fields straddle
// dwords.  The group's planes are LB dwords: plane p holds bit p of the 32 labels, node j at
// bit j.  Two groups' labels differ exactly at the nodes where some plane differs, so
//
//   fw_pwd_planes<LB>(w, tail, pl)   the planes of w, masked to the nodes of `tail`
//                                    (fw_ovl_tail_mask: the last group of a record ends at n)
//   fw_pwd_diff<LB>(a, b)            (a0 ^ b0) | (a1 ^ b1) | ..: the nodes at which two groups,
//                                    given as planes, differ
//   fw_pwd_count(x)                  their number
//
// and a pair costs LB XORs, LB - 1 ORs and one population count per 32 nodes; the transposition
// is paid once per chain and group, whatever the number of partners.
#pragma once

#include <stdint.h>

#include "fw_overlap_bits.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define FW_PWD_POPC(x) ((uint32_t)__popc(x))
#else
#define FW_PWD_POPC(x) ((uint32_t)__builtin_popcount(x))
#endif

// Bit p of node j is bit p + j LB of the string.  Of those, dword i holds the bits b with
// (32 i + b) mod LB = p: the first is b0 = (p - 32 i) mod LB, of node j0 = (32 i + b0 - p) / LB,
// and the others follow at LB-bit steps, which fw_ovl_compress<LB> gathers (zeros come in at the
// top of the shifted dword, and a dword's last node is below 32).
template <int LB>
FW_OVL_FN void fw_pwd_planes(const uint32_t w[LB], uint32_t tail, uint32_t pl[LB]) {
#pragma unroll
  for (int p = 0; p < LB; ++p) {
    uint32_t m = 0u;
#pragma unroll
    for (int i = 0; i < LB; ++i) {
      const int b0 = ((p - 32 * i) % LB + LB) % LB;
      const int j0 = (32 * i + b0 - p) / LB;
      m |= fw_ovl_compress<LB>(w[i] >> b0) << j0;
    }
    pl[p] = m & tail;
  }
}

template <int LB>
FW_OVL_FN uint32_t fw_pwd_diff(const uint32_t a[LB], const uint32_t b[LB]) {
  uint32_t x = a[0] ^ b[0];
#pragma unroll
  for (int p = 1; p < LB; ++p) x |= a[p] ^ b[p];
  return x;
}

FW_OVL_FN uint32_t fw_pwd_count(uint32_t x) { return FW_PWD_POPC(x); }
