// fw_window_rows.h — the 7x7 contiguity window of the grid kernel, one window row per lane.
//
// Row-lane q (0..6) of a chain's 16-lane row holds window row q (v's row is 3) as one byte:
// bit c is window column c (v's column is 3), bit 7 a zero guard column.  The flood fills of
// v's four possible sources (up, left, right, down: CSR order) sit side by side in the four
// bytes of one 32-bit register, and A4 is the row's a-mask replicated into the four bytes,
// so one dilation is two 32-bit shifts, the two neighbouring lanes' values and one AND for
// all four fills at once: a shift out of a byte lands in a guard bit, which & A4 clears.
// Lanes 7..15 carry zero, so nothing leaks between the chains of a wavefront.
//
// Plain functions on uint32_t without lane exchange or memory access: the kernel supplies
// the neighbouring lanes' values (DPP) and the label words (LDS), and
// tests/window_rows_check.cpp runs the same text on the host against the oracle's
// orc_window_verdict (oracle/flipchain_oracle.c).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FW_WR_FN __host__ __device__ inline
#else
#define FW_WR_FN inline
#endif

// "label == a" of the seven LB-bit labels that start at bit sh (0..31) of the dword pair
// hi:lo, as bits 0..6.  The compaction steps are eq_bits32's (fw_device.h), cut to 7 fields.
template <int LB>
FW_WR_FN uint32_t win_row_mask(uint32_t lo, uint32_t hi, uint32_t sh, uint32_t a) {
  static_assert(LB == 2 || LB == 3 || LB == 4, "window rows: 2-, 3- or 4-bit labels");
  const uint32_t x = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);  // one v_alignbit_b32
  uint32_t e;
  if (LB == 2) {
    const uint32_t y = x ^ (a * 0x1555u);
    e = ~(y | (y >> 1)) & 0x1555u;
    e = (e | (e >> 1)) & 0x3333u;
    e = (e | (e >> 2)) & 0x0F0Fu;
    e = e | (e >> 4);
  } else if (LB == 3) {
    const uint32_t y = x ^ (a * 0x49249u);
    e = ~(y | (y >> 1) | (y >> 2)) & 0x49249u;  // bits 0, 3, ..., 18
    e = (e | (e >> 2)) & 0xC30C3u;
    e = (e | (e >> 4)) & 0xF00Fu;
    e = e | (e >> 8);
  } else {
    const uint32_t y = x ^ (a * 0x1111111u);
    e = ~(y | (y >> 1) | (y >> 2) | (y >> 3)) & 0x1111111u;
    e = (e | (e >> 3)) & 0x03030303u;
    e = (e | (e >> 6)) & 0x000F000Fu;
    e = e | (e >> 12);
  }
  return e & 0x7Fu;
}

// Window columns c with 0 <= vc - 3 + c < W.
FW_WR_FN uint32_t win_col_mask(int vc, int W) {
  const int lo = 3 - vc, hi = vc + 4 - W;
  return (0x7Fu << (lo > 0 ? lo : 0)) & (0x7Fu >> (hi > 0 ? hi : 0)) & 0x7Fu;
}

// The source cells of lane q, fill d in byte d: up (row 2, column 3), left (3, 2), right
// (3, 4), down (4, 3); amb: bit d set when source d is an a-cell of the grid.
FW_WR_FN uint32_t win_seed(int q, uint32_t amb) {
  const uint32_t up = (amb & 1u) << 3, lf = ((amb >> 1) & 1u) << (8 + 2);
  const uint32_t rt = ((amb >> 2) & 1u) << (16 + 4), dn = ((amb >> 3) & 1u) << (24 + 3);
  return q == 2 ? up : q == 3 ? (lf | rt) : q == 4 ? dn : 0u;
}

// 0xFF in byte d for every source d of amb.
FW_WR_FN uint32_t win_exist4(uint32_t amb) {
  return (((amb & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu;
}

// One dilation of the four fills: this lane's x, the lanes' above and below (0 past the
// window's first and last row).
FW_WR_FN uint32_t win_dilate(uint32_t x, uint32_t above, uint32_t below, uint32_t A4) {
  return (x | (x << 1) | (x >> 1) | above | below) & A4;
}

// Nonzero when, in this lane's row, the fill of an existing source (E4 = win_exist4)
// differs from the union of the fills.  Fills of one window component are equal, so some
// fill holds every source exactly when no lane reports a miss.
FW_WR_FN uint32_t win_miss(uint32_t x, uint32_t E4) {
  const uint32_t u = (x | (x >> 8) | (x >> 16) | (x >> 24)) & 0x7Fu;
  return (x ^ (u * 0x01010101u)) & E4;
}

// 0x80 in byte d when fill d holds a border cell of this lane's row: rows 0 and 6
// entirely, columns 0 and 6 elsewhere.  ORed over the lanes it is the fills' border flags.
FW_WR_FN uint32_t win_touch(uint32_t x, int q) {
  const uint32_t b = (q == 0 || q == 6) ? 0x7F7F7F7Fu : 0x41414141u;
  return ((x & b) + 0x7F7F7F7Fu) & 0x80808080u;
}

// The order-free rule of the oracle's sequential verdict: 1 if some fill holds every source
// (no lane misses), else 0 if the (nonempty) fill of an existing source touches no border
// (touch: win_touch ORed over the lanes), else -1 (undecided).
FW_WR_FN int win_verdict(bool miss, uint32_t touch, uint32_t E4) {
  if (!miss) return 1;
  return (E4 & 0x80808080u & ~touch) ? 0 : -1;
}
