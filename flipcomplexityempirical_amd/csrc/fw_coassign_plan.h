// fw_coassign_plan.h — the arithmetic and the blocking of the node co-assignment step
// (fw_coassign.hip) that do not need a device.  Plain functions on integers: the host compiles
// the same text (tests/coassign_plan_check.cpp), as it does for fw_census_plan.h and
// fw_pairdist_plan.h.
//
// Transpose.  Member position i of a group sits at bit i % 32 of member word i / 32; plane b of
// list entry j is the uint32 whose bits are bit b of the labels of node nodes[j] in those 32
// members, zero past the group's last member.  A wave owns 64 members (two words) and a tile of
// FW_COA_TT list entries; its lanes read the labels from the dword window the tile's nodes span
// in each record (ascending lists: one range), staged in LDS rows of an odd stride when
// 64 nw rows of it fit, nw = 4, 2 or 1 waves a workgroup.
//
//   fw_coa_tile_window(nodes, m, t, lb, ..)  the dwords of a record tile t's nodes lie in
//   fw_coa_stage(wd_max, allow, ..)          waves per workgroup and row stride, or not staged
//   fw_coa_bit(x, b, valid)                  what a member contributes to plane b
//   fw_coa_plane_word(lab, count, b)         the plane word of up to 32 members' labels
//   fw_coa_together<LB>(a, b, members)       members of one word that label two entries alike
//
// Product.  A workgroup of FW_COA_THREADS threads owns a tile x tile block of entry pairs of one
// group and walks the member words in chunks.  Per chunk it stages rows [word][plane] of 2 tile
// entries (the block's a-entries at 0 .. tile, its b-entries at tile .. 2 tile, rs = 2 tile + 4
// as in fw_pairdist_plan.h), twice: the image is double-buffered.  A thread carries
// FW_COA_CARRY dwords of the next chunk in registers, which bounds a chunk.
#pragma once

#include <stdint.h>

#include "fw_census_plan.h"
#include "fw_pairdist_planes.h"

#define FW_COA_THREADS 256
#define FW_COA_TILE 64             // entries a side by default; 16 and 32 can be forced
#define FW_COA_TT 64               // entries of a transpose tile: one per lane at the stores
#define FW_COA_CARRY 16            // dwords of the next chunk a thread holds
#define FW_COA_LDS_BYTES 65536     // the project's bound on a workgroup's LDS
#define FW_COA_MAX_ELEMS (1ll << 28)

struct FwCoaPlan {
  int32_t tile, shift, rs, chunk;  // shift = log2(2 tile)
  int32_t n_words, n_chunks, lds_bytes;
};

// force_tile: 16, 32 or 64 (anything else: the default); force_chunk >= 1 lowers the chunk
FW_OVL_FN FwCoaPlan fw_coa_plan(int per_group, int lb, int force_tile, int force_chunk) {
  FwCoaPlan q;
  q.tile = force_tile == 16 || force_tile == 32 || force_tile == 64 ? force_tile : FW_COA_TILE;
  q.shift = q.tile == 16 ? 5 : q.tile == 32 ? 6 : 7;
  q.rs = 2 * q.tile + 4;
  q.n_words = (per_group + 31) / 32;
  int w = FW_COA_THREADS * FW_COA_CARRY / (2 * q.tile * lb);
  const int fit = FW_COA_LDS_BYTES / (2 * lb * q.rs * 4);
  if (w > fit) w = fit;
  if (w > q.n_words) w = q.n_words;
  if (force_chunk >= 1 && force_chunk < w) w = force_chunk;
  if (w < 1) w = 1;
  q.chunk = w;
  q.n_chunks = (q.n_words + w - 1) / w;
  q.lds_bytes = 2 * w * lb * q.rs * 4;
  return q;
}

// chunk c covers the member words [*w0, *w0 + *wn)
FW_OVL_FN void fw_coa_chunk_range(const FwCoaPlan& q, int c, int* w0, int* wn) {
  const int a = c * q.chunk, rest = q.n_words - a;
  *w0 = a;
  *wn = rest < q.chunk ? (rest > 0 ? rest : 0) : q.chunk;
}

FW_OVL_FN int fw_coa_tiles(int m) { return (m + FW_COA_TT - 1) / FW_COA_TT; }

// transpose tile t holds the entries [*e0, *e0 + *en); dwords [*wd0, *wd0 + *wdn) of a record
// hold every bit of their nodes' fields (nodes ascending: the first and the last bound them)
FW_OVL_FN void fw_coa_tile_window(const int32_t* nodes, int m, int t, int lb, int* e0, int* en,
                                  int* wd0, int* wdn) {
  const int a = t * FW_COA_TT, b = a + FW_COA_TT < m ? a + FW_COA_TT : m;
  *e0 = a;
  *en = b - a;
  fw_cen_window(nodes[a], nodes[b - 1], lb, wd0, wdn);
}

// rows of wd_max dwords, padded to an odd stride so that lanes on different records fall on
// different banks; as many waves (64 rows each) a workgroup as FW_COA_LDS_BYTES holds beside the
// 64 nw chain ids.  Returns 1 when staged; otherwise the lanes read the records in HBM.
FW_OVL_FN int fw_coa_stage(int wd_max, int allow, int* nw, int* stride) {
  const int s = wd_max | 1;
  *stride = s;
  for (int w = 4; w >= 1; w >>= 1)
    if (allow && (int64_t)64 * w * (s + 1) * 4 <= FW_COA_LDS_BYTES) {
      *nw = w;
      return 1;
    }
  *nw = 4;
  *stride = 0;
  return 0;
}

// a member's contribution to plane b of its word: bit b of its label, nothing past the group
FW_OVL_FN bool fw_coa_bit(uint32_t x, int b, bool valid) { return valid && ((x >> b) & 1u); }

// plane b of the labels of members 0 .. count - 1 of one word (count <= 32): what the device
// takes from one half of a ballot over fw_coa_bit
FW_OVL_FN uint32_t fw_coa_plane_word(const uint32_t* lab, int count, int b) {
  uint32_t w = 0u;
  for (int i = 0; i < 32; ++i)
    if (fw_coa_bit(i < count ? lab[i] : 0u, b, i < count)) w |= 1u << i;
  return w;
}

// members of one word, `members` of them, whose labels of two entries are equal: pad bits are
// zero in every plane and so differ nowhere
template <int LB>
FW_OVL_FN uint32_t fw_coa_together(const uint32_t a[LB], const uint32_t b[LB], int members) {
  return (uint32_t)members - fw_pwd_count(fw_pwd_diff<LB>(a, b));
}
