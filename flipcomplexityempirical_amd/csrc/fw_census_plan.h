// fw_census_plan.h — the arithmetic of the ensemble census (fw_census.hip) that does not need a
// device: the field of a node cut from a window of label words, the node range a tile's rows
// reach, and the split of a group's chains into slices.  Plain functions on integers: the host
// compiles the same text (tests/census_plan_check.cpp), as it does for fw_overlap_bits.h.
//
//   fw_cen_field<LB>(win, bit)          the LB-bit field at bit offset `bit` of the dword string win
//   fw_cen_tile_reach(rowptr, col, ..)  smallest and largest node among a tile's nodes and their
//                                       neighbours
//   fw_cen_window(lo, hi, lb, ..)       the dwords of a record that hold the fields of nodes lo..hi
//   fw_cen_slices(count, len)           slices of `len` chains that cover `count` chains
//   fw_cen_slice_range(s, len, count..) the chains [i0, i1) of slice s (the last may be short)
#pragma once

#include <stdint.h>

#include "fw_overlap_bits.h"

// The field at bit offset `bit` of win (node x of a record whose window starts at dword wd0 sits
// at bit x LB - 32 wd0).  The dword after the field's first is read only when the field crosses
// into it (3 and 5 bits), so no dword past the last field of the window is touched.
template <int LB>
FW_OVL_FN uint32_t fw_cen_field(const uint32_t* win, uint32_t bit) {
  const uint32_t at = bit >> 5, sh = bit & 31u;
  const uint32_t lo = win[at];
  uint32_t hi = 0u;
  if ((LB == 3 || LB == 5) && sh + LB > 32u) hi = win[at + 1];
  return fw_ovl_shr(hi, lo, (int)sh) & ((1u << LB) - 1u);
}

// the smallest and largest node id among nodes [t0, t1) and the neighbours in their CSR rows
FW_OVL_FN void fw_cen_tile_reach(const int32_t* rowptr, const int32_t* col, int t0, int t1,
                                 int* lo, int* hi) {
  int a = t0, b = t1 - 1;
  for (int e = rowptr[t0]; e < rowptr[t1]; ++e) {
    if (col[e] < a) a = col[e];
    if (col[e] > b) b = col[e];
  }
  *lo = a;
  *hi = b;
}

// dwords [*wd0, *wd0 + *wdn) of a record hold every bit of the fields of nodes lo..hi
FW_OVL_FN void fw_cen_window(int lo, int hi, int lb, int* wd0, int* wdn) {
  const int64_t first = ((int64_t)lo * lb) >> 5, last = ((int64_t)(hi + 1) * lb + 31) >> 5;
  *wd0 = (int)first;
  *wdn = (int)(last - first);
}

FW_OVL_FN int fw_cen_slices(int count, int len) { return (count + len - 1) / len; }

FW_OVL_FN void fw_cen_slice_range(int s, int len, int count, int* i0, int* i1) {
  const int64_t a = (int64_t)s * len, b = a + len;
  *i0 = (int)(a < count ? a : count);
  *i1 = (int)(b < count ? b : count);
}
