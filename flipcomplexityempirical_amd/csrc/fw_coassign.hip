// fw_coassign.hip — node-pair co-assignment across the chains of the handle: how many plans of a
// group put nodes u and v of a list in the same district (the coassign entry points of
// include/flipwalk.h; parameter struct in fw_internal.h, the blocking and the bit arithmetic in
// fw_coassign_plan.h).  Like the exchange, record, tally, geometry, overlap, census and pairdist
// steps this runs between launches on the handle's stream, from the label records the run
// kernels leave in HBM; no run kernel knows of it.  It is the pairwise plan distance transposed:
// fix two nodes and reduce over the chains.
//
// fw_coassign_transpose_kernel<LB, STAGED>: workgroup (transpose tile of FW_COA_TT list entries,
// group, 64 nw members), one member per thread, a wave owning 64 members: two member words.
// STAGED: the workgroup copies the dword window its tile's nodes span in each of its records
// into LDS (coalesced dword loads; rows of an odd stride, so lanes on different records fall on
// different banks) and lane l cuts member l's label of entry j from its row; otherwise (windows
// too long for LDS) the lanes read their records in HBM.  One ballot per plane yields both
// member words of the wave; lanes without a member vote 0, so bits past the group's last member
// are zero in every plane.  Lane j keeps the words of entry j, and after the tile the wave
// stores them entry-minor, planes[g][word][plane][entry]: consecutive lanes, consecutive dwords.
// Every wave reaches both barriers: they come before anything that depends on a member.
//
// fw_coassign_product_kernel<LB>: fw_pairdist_kernel's shape over those planes.  A workgroup of
// 256 threads owns a tile x tile block of entry pairs of one group (thread (ti, tj) the 4 x 4
// pairs of a-entries 4 ti .. and b-entries 4 tj ..) and walks the member words in chunks.  The
// rows [word][plane] of its 2 tile entries are contiguous in HBM and go to LDS as they are
// (entries past the list as zero), double-buffered: the loads of chunk c + 1 are issued before
// the count of chunk c and stored after it, so one barrier per chunk suffices.  Per pair and
// word the count is LB XORs, LB - 1 ORs and one v_bcnt_u32_b32 over the *differing* members
// (pad bits differ nowhere) into a 32-bit accumulator; at the end per_group - diff is added to
// the uint64 together[g][i][j].  Blocks below the diagonal do nothing, a block above it adds to
// [i][j] and [j][i], and a diagonal block, which computes both orders itself, to [i][j] alone:
// every accumulator element has one owning lane, and no atomics are used.
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include "fw_internal.h"
#include "fw_coassign_plan.h"

namespace {

template <int LB, bool STAGED>
__global__ __launch_bounds__(FW_COA_THREADS) void fw_coassign_transpose_kernel(FwCoassignParams p) {
  extern __shared__ __align__(16) uint32_t lds[];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int slots = (p.per_group + 63) >> 6, spw = (slots + p.nw - 1) / p.nw;
  const int t = (int)(blockIdx.x % (unsigned)p.n_ttiles), rest = (int)(blockIdx.x / (unsigned)p.n_ttiles);
  const int g = rest / spw, s = rest - g * spw;
  const int e0 = t * FW_COA_TT, en = p.m - e0 < FW_COA_TT ? p.m - e0 : FW_COA_TT;
  const int i0 = s * nt, i = i0 + tid;  // the workgroup's first member, the thread's member
  const bool valid = i < p.per_group;
  int32_t chain = 0;
  if (valid) chain = p.chain_of ? p.chain_of[(size_t)i * p.n_groups + g] : i;
  const uint32_t* win = reinterpret_cast<const uint32_t*>(p.labels + (int64_t)chain * p.lab_stride);
  if (STAGED) {
    int32_t* cid = reinterpret_cast<int32_t*>(lds);  // [nt]
    uint32_t* rows = lds + nt;                       // [nt][stride]
    cid[tid] = chain;
    __syncthreads();
    const int wd0 = p.twin[2 * t], wdn = p.twin[2 * t + 1];
    const int nrec = p.per_group - i0 < nt ? p.per_group - i0 : nt;
    for (int it = tid; it < nrec * wdn; it += nt) {
      const int r = it / wdn, w = it - r * wdn;
      const uint32_t* rec = reinterpret_cast<const uint32_t*>(p.labels + (int64_t)cid[r] * p.lab_stride);
      rows[r * p.stride + w] = wd0 + w < p.lab_words ? rec[wd0 + w] : 0u;
    }
    __syncthreads();
    win = rows + tid * p.stride;
  }
  uint32_t klo[LB], khi[LB];
#pragma unroll
  for (int b = 0; b < LB; ++b) klo[b] = khi[b] = 0u;
  for (int jj = 0; jj < en; ++jj) {
    const uint32_t bit = p.ebit[e0 + jj];
    const uint32_t x = valid ? fw_cen_field<LB>(win, bit) : 0u;
#pragma unroll
    for (int b = 0; b < LB; ++b) {
      const unsigned long long bal = __ballot(fw_coa_bit(x, b, valid));
      if (lane == jj) {
        klo[b] = (uint32_t)bal;
        khi[b] = (uint32_t)(bal >> 32);
      }
    }
  }
  const int w0 = 2 * (s * p.nw + wave);  // the member word of the wave's lanes 0 .. 31
  if (lane < en) {
#pragma unroll
    for (int b = 0; b < LB; ++b) {
      if (w0 < p.n_words)
        p.planes[(((size_t)g * p.n_words + w0) * LB + b) * p.ms + e0 + lane] = klo[b];
      if (w0 + 1 < p.n_words)
        p.planes[(((size_t)g * p.n_words + w0 + 1) * LB + b) * p.ms + e0 + lane] = khi[b];
    }
  }
}

// A chunk of wn member words is wn LB rows (row = word * LB + plane) of 2 tile slots; slots
// [0, tile) are the block's a-entries, [tile, 2 tile) its b-entries.  A thread keeps its slot and
// takes the rows r0, r0 + rstep, ..: pass k of the workgroup covers rows k rstep .. (k + 1) rstep.
struct CoaLane {
  const uint32_t* src;  // the thread's entry (entry 0 when past the list) in row 0 of the group's first word
  bool in_list;
  int r0, rstep, at;    // at: its dword in row r0 of a buffer
};

// the loads are unconditional (a row past the chunk reads row 0 and is dropped): sixteen
// predicated loads cost the kernel half its occupancy in registers
template <int LB>
__device__ __forceinline__ void coa_fetch(const FwCoassignParams& p, const CoaLane& l, int w0, int wn,
                                          uint32_t (&w)[FW_COA_CARRY]) {
  const int rows = wn * LB;
  const uint32_t* src = l.src + (size_t)w0 * LB * p.ms;
#pragma unroll
  for (int k = 0; k < FW_COA_CARRY; ++k) {
    const int r = l.r0 + k * l.rstep;
    const bool ok = l.in_list && r < rows;
    const uint32_t v = src[(size_t)(ok ? r : 0) * p.ms];
    w[k] = ok ? v : 0u;
  }
}

template <int LB>
__device__ __forceinline__ void coa_stage(const FwCoassignParams& p, const CoaLane& l, int wn,
                                          uint32_t* buf, const uint32_t (&w)[FW_COA_CARRY]) {
  const int rows = wn * LB;
#pragma unroll
  for (int k = 0; k < FW_COA_CARRY; ++k)
    if (l.r0 + k * l.rstep < rows) buf[l.at + k * l.rstep * p.rs] = w[k];
}

#define FW_COA_PAIR(i, j)                                                  \
  {                                                                        \
    uint32_t x = A[0][i] ^ B[0][j];                                        \
    _Pragma("unroll") for (int q = 1; q < LB; ++q) x |= A[q][i] ^ B[q][j]; \
    acc##i##j += fw_pwd_count(x);                                          \
  }

template <int LB>
__global__ __launch_bounds__(FW_COA_THREADS) void fw_coassign_product_kernel(FwCoassignParams p) {
  extern __shared__ __align__(16) uint32_t lds[];
  const int gx = (p.m + p.tile - 1) / p.tile;  // a flat grid: a grid's y extent stops at 65535
  const int g = (int)(blockIdx.x / (unsigned)(gx * gx)), rem = (int)(blockIdx.x - (unsigned)g * (unsigned)(gx * gx));
  const int by = rem / gx, bx = rem - by * gx;
  if (bx < by) return;  // the whole workgroup: no barrier is left waiting
  const int tile = p.tile, side = tile >> 2;  // threads a side
  const int tid = threadIdx.x, ti = tid / side, tj = tid - ti * side;
  const bool counts = ti < side;  // tile 16 and 32 leave threads that only stage
  const int a0 = by * tile, b0 = bx * tile;
  const int buf_words = p.chunk * LB * p.rs;
  const uint32_t* gp = p.planes + (size_t)g * p.n_words * LB * p.ms;
  if (rem == 0 && tid == 0) p.cnt[g] += (uint64_t)p.per_group;
  uint32_t acc00 = 0, acc01 = 0, acc02 = 0, acc03 = 0, acc10 = 0, acc11 = 0, acc12 = 0, acc13 = 0,
           acc20 = 0, acc21 = 0, acc22 = 0, acc23 = 0, acc30 = 0, acc31 = 0, acc32 = 0, acc33 = 0;
  uint32_t w[FW_COA_CARRY];
  CoaLane l;
  {
    const int slot = tid & ((1 << p.shift) - 1), e = slot < tile ? a0 + slot : b0 + slot - tile;
    l.r0 = tid >> p.shift;
    l.rstep = FW_COA_THREADS >> p.shift;
    l.at = l.r0 * p.rs + slot;
    l.in_list = e < p.m;
    l.src = gp + (l.in_list ? e : 0);
    const int wn = p.n_words < p.chunk ? p.n_words : p.chunk;
    coa_fetch<LB>(p, l, 0, wn, w);
    coa_stage<LB>(p, l, wn, lds, w);
  }
  __syncthreads();
  for (int c = 0; c < p.n_chunks; ++c) {
    const int w0 = c * p.chunk, wn = p.n_words - w0 < p.chunk ? p.n_words - w0 : p.chunk;
    const int w1 = w0 + p.chunk, wn1 = p.n_words - w1 < p.chunk ? p.n_words - w1 : p.chunk;
    const bool more = c + 1 < p.n_chunks;
    if (more) coa_fetch<LB>(p, l, w1, wn1, w);  // in flight during the count
    if (counts) {
      const uint32_t* cur = lds + (c & 1) * buf_words;
      // as in fw_pairdist_kernel: unrolled further, the wide widths spill
#pragma unroll(LB <= 3 ? 2 : 1)
      for (int wl = 0; wl < wn; ++wl) {
        uint32_t A[LB][4], B[LB][4];
#pragma unroll
        for (int q = 0; q < LB; ++q) {
          const uint32_t* row = cur + (wl * LB + q) * p.rs;
          const uint4 av = *reinterpret_cast<const uint4*>(row + 4 * ti);
          const uint4 bv = *reinterpret_cast<const uint4*>(row + tile + 4 * tj);
          A[q][0] = av.x, A[q][1] = av.y, A[q][2] = av.z, A[q][3] = av.w;
          B[q][0] = bv.x, B[q][1] = bv.y, B[q][2] = bv.z, B[q][3] = bv.w;
        }
        FW_COA_PAIR(0, 0) FW_COA_PAIR(0, 1) FW_COA_PAIR(0, 2) FW_COA_PAIR(0, 3)
        FW_COA_PAIR(1, 0) FW_COA_PAIR(1, 1) FW_COA_PAIR(1, 2) FW_COA_PAIR(1, 3)
        FW_COA_PAIR(2, 0) FW_COA_PAIR(2, 1) FW_COA_PAIR(2, 2) FW_COA_PAIR(2, 3)
        FW_COA_PAIR(3, 0) FW_COA_PAIR(3, 1) FW_COA_PAIR(3, 2) FW_COA_PAIR(3, 3)
      }
    }
    if (more) coa_stage<LB>(p, l, wn1, lds + ((c + 1) & 1) * buf_words, w);
    __syncthreads();  // chunk c + 1 is complete, and chunk c has been read by every wave
  }
  if (!counts) return;
  const bool mirror = bx != by;
  const uint32_t out[4][4] = {{acc00, acc01, acc02, acc03},
                              {acc10, acc11, acc12, acc13},
                              {acc20, acc21, acc22, acc23},
                              {acc30, acc31, acc32, acc33}};
  uint64_t* T = p.together + (size_t)g * (size_t)p.m * (size_t)p.m;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ia = a0 + 4 * ti + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int jb = b0 + 4 * tj + j;
      if (ia < p.m && jb < p.m) {
        const uint64_t same = (uint64_t)((uint32_t)p.per_group - out[i][j]);
        T[(size_t)ia * p.m + jb] += same;
        if (mirror) T[(size_t)jb * p.m + ia] += same;
      }
    }
  }
}

template <int LB>
void* transpose_fn(bool staged) {
  return staged ? reinterpret_cast<void*>(&fw_coassign_transpose_kernel<LB, true>)
                : reinterpret_cast<void*>(&fw_coassign_transpose_kernel<LB, false>);
}

}  // namespace

// FLIPWALK_COA_TILE (16, 32, 64: entries a side of a product block), FLIPWALK_COA_CHUNK (member
// words per staging step) and FLIPWALK_COA_STAGE (0: never stage label windows in LDS) override
// the plan (tests force every blocking and both ways to the labels on small shapes)
int fw_coassign_env(const char* name) {
  const char* e = getenv(name);
  return e && e[0] ? atoi(e) : -1;
}

int fw_launch_coassign_transpose(const FwCoassignParams& p, void* stream) {
  void* fn;
  switch (p.lb) {
    case 2: fn = transpose_fn<2>(p.staged); break;
    case 3: fn = transpose_fn<3>(p.staged); break;
    case 4: fn = transpose_fn<4>(p.staged); break;
    case 5: fn = transpose_fn<5>(p.staged); break;
    case 8: fn = transpose_fn<8>(p.staged); break;
    default: return (int)hipErrorInvalidValue;
  }
  void* args[] = {const_cast<FwCoassignParams*>(&p)};
  const int slots = (p.per_group + 63) / 64, spw = (slots + p.nw - 1) / p.nw;
  const unsigned blocks = (unsigned)p.n_ttiles * (unsigned)p.n_groups * (unsigned)spw;
  return (int)hipLaunchKernel(fn, dim3(blocks), dim3(64 * p.nw), args, (size_t)p.t_lds_bytes,
                              (hipStream_t)stream);
}

int fw_launch_coassign_product(const FwCoassignParams& p, void* stream) {
  void* fn;
  switch (p.lb) {
    case 2: fn = reinterpret_cast<void*>(&fw_coassign_product_kernel<2>); break;
    case 3: fn = reinterpret_cast<void*>(&fw_coassign_product_kernel<3>); break;
    case 4: fn = reinterpret_cast<void*>(&fw_coassign_product_kernel<4>); break;
    case 5: fn = reinterpret_cast<void*>(&fw_coassign_product_kernel<5>); break;
    case 8: fn = reinterpret_cast<void*>(&fw_coassign_product_kernel<8>); break;
    default: return (int)hipErrorInvalidValue;
  }
  void* args[] = {const_cast<FwCoassignParams*>(&p)};
  const unsigned gx = (unsigned)((p.m + p.tile - 1) / p.tile);
  return (int)hipLaunchKernel(fn, dim3(gx * gx * (unsigned)p.n_groups), dim3(FW_COA_THREADS), args,
                              (size_t)p.lds_bytes, (hipStream_t)stream);
}
