// fw_pairdist_plan.h — the blocking of the pairwise plan distance (fw_pairdist.hip) that does not
// need a device: tile, chunk and LDS image.  Plain functions on integers: the host compiles the
// same text (tests/pairdist_planes_check.cpp), as it does for fw_census_plan.h.
//
// A workgroup of FW_PWD_THREADS threads owns a tile x tile block of pairs and walks the record in
// chunks of `chunk` 32-node groups.  Per chunk it stages the planes of 2 tile chains as
// uint32 [plane][group][rs] (chain-minor; the a-chains at 0 .. tile, the b-chains at tile .. 2
// tile, rs = 2 tile + 4: rows stay 16-byte aligned and consecutive groups of one chain fall on
// banks 4 apart), twice: the image is double-buffered.  A thread carries ipt = 16 / lb chain
// groups of the next chunk in registers, so a chunk has at most FW_PWD_THREADS ipt of them; the
// two buffers stay inside FW_PWD_LDS_BYTES.
#pragma once

#include <stdint.h>

#include "fw_overlap_bits.h"

#define FW_PWD_THREADS 256
#define FW_PWD_TILE 64            // chains a side by default; 16 and 32 can be forced
#define FW_PWD_LDS_BYTES 65536    // the project's bound on a workgroup's LDS
#define FW_PWD_MAX_PAIRS (1ll << 28)

struct FwPwdPlan {
  int32_t tile, chunk, rs, ipt;
  int32_t n_groups, n_chunks, lds_bytes;
};

FW_OVL_FN int fw_pwd_ipt(int lb) { return 16 / lb; }

// force_tile: 16, 32 or 64 (anything else: the default); force_chunk >= 1 lowers the chunk
FW_OVL_FN FwPwdPlan fw_pwd_plan(int n, int lb, int force_tile, int force_chunk) {
  FwPwdPlan q;
  q.tile = force_tile == 16 || force_tile == 32 || force_tile == 64 ? force_tile : FW_PWD_TILE;
  q.rs = 2 * q.tile + 4;
  q.ipt = fw_pwd_ipt(lb);
  q.n_groups = (n + 31) / 32;
  int g = FW_PWD_THREADS * q.ipt / (2 * q.tile);
  const int fit = FW_PWD_LDS_BYTES / (2 * lb * q.rs * 4);
  if (g > fit) g = fit;
  if (g > q.n_groups) g = q.n_groups;
  if (force_chunk >= 1 && force_chunk < g) g = force_chunk;
  if (g < 1) g = 1;
  q.chunk = g;
  q.n_chunks = (q.n_groups + g - 1) / g;
  q.lds_bytes = 2 * g * lb * q.rs * 4;
  return q;
}

// chunk c covers the groups [*g0, *g0 + *gn)
FW_OVL_FN void fw_pwd_chunk_range(const FwPwdPlan& q, int c, int* g0, int* gn) {
  const int a = c * q.chunk, rest = q.n_groups - a;
  *g0 = a;
  *gn = rest < q.chunk ? (rest > 0 ? rest : 0) : q.chunk;
}
