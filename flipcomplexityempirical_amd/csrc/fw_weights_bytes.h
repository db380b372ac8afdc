// fw_weights_bytes.h — level-2 proposal weights of the grid kernel from byte-aligned label
// reads, for 2-bit labels on grids whose width is a multiple of 4.
//
// Row-lane q of a chain's 16-lane row holds the four nodes x0 .. x0+3 of group gi
// (x0 = 64 gi + 4 q).  With W % 4 == 0 they are exactly byte 16 gi + q of the packed labels,
// they never straddle a grid row, the nodes above and below are the bytes W/4 before and
// after, and the left neighbour of x0 / the right neighbour of x0+3 sit in the neighbouring
// lanes' bytes: no bit offsets, word indices or 64-bit shifts.  Row-lanes 0 and 15 have no
// such neighbour lane and read one more byte, the one before / after the group.
//
// Plain functions on uint32_t without lane exchange or memory access: the kernel supplies
// the bytes (LDS) and the neighbouring lanes' one-hot words (DPP), and
// tests/weights_bytes_check.cpp runs the same text on the host against the per-node rule.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FW_WB_FN __host__ __device__ inline
#else
#define FW_WB_FN inline
#endif

// v_perm_b32 for selector bytes 0..7: byte i of the result is byte sel_i of the eight bytes
// hi:lo (0..3: lo).
FW_WB_FN uint32_t wb_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const uint64_t both = ((uint64_t)hi << 32) | lo;
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) r |= (uint32_t)((both >> (8 * ((sel >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);
  return r;
#endif
}

// Byte offsets, from the chain's label base, of the four bytes lane q of group gi reads:
// its own, the ones of the grid rows above and below (the own byte again where the row does
// not exist: r0 is the grid row of x0, and r0 >= H for a lane past the last node) and the
// edge byte of row-lanes 0 and 15 (the other lanes re-read their own).
//
// Bounds, for gi <= G = ceil(n / 64) (the derive loop walks whole u16 pairs of groups, so it
// may visit group G; level 2 stays below G): own <= 16 G + 15 and edge <= 16 G + 16, while a
// slot holds at least 16 G label bytes (the label region is n / 4 + 8 bytes rounded up to
// 16) followed by at least 64 bytes of group sums, so every read stays inside the lane's own
// slot; bytes at or past n / 4 belong to nodes >= n and are cleared by mN, and the edge byte
// after a row's last node by mR.  up >= 0 because r0 > 0 puts own at or past W / 4.
// edge = -1 only for lane 0 of group 0: the last byte of the 16-byte guard in front of slot
// 0, or of the previous slot; that node is in column 0, so mL clears it.
FW_WB_FN void wb_offsets(int gi, int q, int r0, int W, int H, int& own, int& up, int& dn,
                         int& edge) {
  own = gi * 16 + q;
  up = r0 > 0 ? own - (W >> 2) : own;
  dn = r0 < H - 1 ? own + (W >> 2) : own;
  edge = own + (q == 0 ? -1 : (q == 15 ? 1 : 0));
}

// Which of the lane's four nodes (one per byte) exist and have each neighbour; c0 is the grid
// column of x0 (a multiple of 4, c0 + 3 < W), and a group's tail past n is whole lanes.
FW_WB_FN void wb_masks(int x0, int r0, int c0, int W, int H, int n, uint32_t& mN, uint32_t& mU,
                       uint32_t& mD, uint32_t& mL, uint32_t& mR) {
  mN = x0 < n ? 0xFFFFFFFFu : 0u;
  mU = r0 > 0 ? 0xFFFFFFFFu : 0u;
  mD = r0 < H - 1 ? 0xFFFFFFFFu : 0u;
  mL = c0 == 0 ? 0xFFFFFF00u : 0xFFFFFFFFu;
  mR = c0 == W - 4 ? 0x00FFFFFFu : 0xFFFFFFFFu;
}

// The four 2-bit labels of byte b as one-hot bytes (1 << label), node t in byte t.
FW_WB_FN uint32_t wb_onehot(uint32_t b) {
  const uint32_t t = ((b << 12) | b) & 0x000F000Fu;
  const uint32_t s = ((t << 6) | t) & 0x03030303u;
  return wb_perm(0u, 0x08040201u, s);
}

// What row-lanes 0 and 15 take in place of a neighbour lane's one-hot word: the one-hot
// label of the edge byte's last node in byte 3 (lane 0: the node left of x0), of its first
// node in byte 0 (lane 15: the node right of x0+3).  Other lanes never use it.
FW_WB_FN uint32_t wb_edge(uint32_t be, int q) {
  const uint32_t oh = 1u << ((be >> (q == 0 ? 6 : 0)) & 3u);
  return oh | (oh << 24);
}

// per byte: 0x80 where the one-hot bytes a and b differ
FW_WB_FN uint32_t wb_ne_bytes(uint32_t a, uint32_t b) {
  return ~((a & b) + 0x7F7F7F7Fu) & 0x80808080u;
}
// per-byte popcount (bytes < 16)
FW_WB_FN uint32_t wb_byte_popc(uint32_t f) {
  const uint32_t t = f - ((f >> 1) & 0x55555555u);
  return (t & 0x33333333u) + ((t >> 2) & 0x33333333u);
}

// Proposal weights w4 (CUT: the cut-edge proposal's, else the pairs proposal's) and, when
// NEED_CD or CUT, cut degrees cd4 of the lane's four nodes, one per byte.  O, U, Dn: the
// one-hot words of the own, up and down bytes; Oprev / Onext: the one-hot words of row-lanes
// q-1 / q+1 (wb_edge for lanes 0 / 15).
template <bool CUT, bool NEED_CD>
FW_WB_FN void wb_weights(uint32_t O, uint32_t U, uint32_t Dn, uint32_t Oprev, uint32_t Onext,
                         uint32_t mN, uint32_t mU, uint32_t mD, uint32_t mL, uint32_t mR,
                         uint32_t& w4, uint32_t& cd4) {
  w4 = 0;
  cd4 = 0;
  const uint32_t L = (O << 8) | (Oprev >> 24);  // x-1: one v_alignbit_b32
  const uint32_t R = (O >> 8) | (Onext << 24);  // x+1
  if (!CUT) {
    const uint32_t bits = (U & mU) | (L & mL) | (R & mR) | (Dn & mD);
    w4 = wb_byte_popc(bits & ~O & mN);
  }
  if (NEED_CD || CUT) {
    const uint32_t ne = (wb_ne_bytes(U, O) & mU) >> 7, nl = (wb_ne_bytes(L, O) & mL) >> 7,
                   nr = (wb_ne_bytes(R, O) & mR) >> 7, nd = (wb_ne_bytes(Dn, O) & mD) >> 7;
    cd4 = (ne + nl + nr + nd) & mN;
    if (CUT) w4 = cd4;
  }
}
