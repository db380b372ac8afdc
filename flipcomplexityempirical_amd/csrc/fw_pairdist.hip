// fw_pairdist.hip — Hamming distances between the current plans of two lists of chains, all
// pairs: D[i][j] = #{v : X_{a_i}(v) != X_{b_j}(v)}, then per row its sum, its nearest partner
// and the histogram of the values (the pairdist entry points of include/flipwalk.h; parameter
// structs in fw_internal.h).  Like the exchange, record, tally, geometry, overlap and census
// steps this runs between launches on the handle's stream, from the label records the run
// kernels leave in HBM; no run kernel knows of it.
//
// fw_pairdist_kernel<LB> has the shape of a GEMM with XOR / OR / popcount in place of the
// multiply-add.  A workgroup of 256 threads owns a tile x tile block of pairs (64 x 64: thread
// (ti, tj) the 4 x 4 pairs of a-chains 4 ti .. and b-chains 4 tj .., in sixteen 32-bit
// accumulators with constant indices) and walks the records in chunks of `chunk` 32-node groups
// (fw_pairdist_plan.h).  Per chunk every thread loads up to 16 / LB chain groups from HBM
// (consecutive lanes take consecutive groups of one record, as wide as a group's alignment
// allows: 16 B at 4 and 8 bits, 8 B at 2, dwords at 3 and 5), transposes each once into LB bit
// planes (fw_pairdist_planes.h; the last group masked to n, dwords past the label words read as
// zero since the group sums follow them in the record) and stores them as uint32
// [plane][group][chain] in LDS.  The image is double-buffered: the loads of chunk c + 1 are
// issued before the count of chunk c and their planes are stored after it, into the other
// buffer, so one barrier per chunk suffices.  In the count a thread reads, per group and plane,
// its four b-chains with one ds_read_b128 (consecutive lanes, consecutive 16 bytes) and its four
// a-chains with another (one address per 16 lanes: a broadcast), and per pair LB XORs, LB - 1
// ORs and one v_bcnt_u32_b32 that adds into the accumulator.  Positions past the end of a list
// are staged as zero planes and never stored.  Every element of D has one owning lane: in the
// symmetric case the blocks below the diagonal do nothing, a block above it stores D[i][j] and
// D[j][i], and a diagonal block, which computes both orders itself, stores D[i][j] alone.
//
// fw_pairdist_reduce_kernel: one wave per row of D (four rows a workgroup, rows strided over
// the grid).  Lanes stride over the row: the sum in 64 bits, the least (d, j) as one 64-bit key
// reduced by a fixed butterfly, so ties go to the lowest j, and the row's values counted into
// the workgroup's LDS bins (n + 1 <= 12288) and added to hist with one 64-bit integer atomic
// per non-empty bin at the end, or straight into hist with one atomic per value on longer
// records.  The adds are integer: the histogram does not depend on their order.
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include "fw_internal.h"
#include "fw_pairdist_plan.h"
#include "fw_pairdist_planes.h"

namespace {

// dwords [g LB, g LB + LB) of a record -> w (fw_overlap.hip's load_group)
template <int LB>
__device__ __forceinline__ void pwd_load_group(const uint32_t* rec, int g, int lab_words,
                                               uint32_t w[LB]) {
  const int at = g * LB;
  if (at + LB <= lab_words) {
    if (LB == 4 || LB == 8) {
      const uint4* q = reinterpret_cast<const uint4*>(rec + at);
#pragma unroll
      for (int i = 0; i < LB / 4; ++i) {
        const uint4 v = q[i];
        w[4 * i] = v.x;
        w[4 * i + 1] = v.y;
        w[4 * i + 2] = v.z;
        w[4 * i + 3] = v.w;
      }
    } else if (LB == 2) {
      const uint2 v = *reinterpret_cast<const uint2*>(rec + at);
      w[0] = v.x;
      w[1] = v.y;
    } else {
#pragma unroll
      for (int i = 0; i < LB; ++i) w[i] = rec[at + i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < LB; ++i) w[i] = at + i < lab_words ? rec[at + i] : 0u;
  }
}

// item `it` of a chunk of gn groups is group it % gn of chain slot it / gn; slots [0, tile) are
// the block's a-positions, [tile, 2 tile) its b-positions
template <int LB>
__device__ __forceinline__ void pwd_fetch(const FwPairdistParams& p, int a0, int b0, int g0, int gn,
                                          uint32_t (&w)[16 / LB][LB]) {
  const int items = 2 * p.tile * gn;
#pragma unroll
  for (int k = 0; k < 16 / LB; ++k) {
#pragma unroll
    for (int i = 0; i < LB; ++i) w[k][i] = 0u;
    const int it = k * FW_PWD_THREADS + (int)threadIdx.x;
    if (it < items) {
      const int slot = it / gn, gl = it - slot * gn;
      const bool is_a = slot < p.tile;
      const int pos = is_a ? a0 + slot : b0 + slot - p.tile;
      if (pos < (is_a ? p.ma : p.mb)) {
        const int32_t chain = is_a ? p.a[pos] : p.b[pos];
        pwd_load_group<LB>(reinterpret_cast<const uint32_t*>(p.labels + (int64_t)chain * p.lab_stride),
                           g0 + gl, p.lab_words, w[k]);
      }
    }
  }
}

template <int LB>
__device__ __forceinline__ void pwd_stage(const FwPairdistParams& p, int g0, int gn, uint32_t* buf,
                                          const uint32_t (&w)[16 / LB][LB]) {
  const int items = 2 * p.tile * gn;
#pragma unroll
  for (int k = 0; k < 16 / LB; ++k) {
    const int it = k * FW_PWD_THREADS + (int)threadIdx.x;
    if (it < items) {
      const int slot = it / gn, gl = it - slot * gn;
      uint32_t pl[LB];
      fw_pwd_planes<LB>(w[k], fw_ovl_tail_mask(p.n - 32 * (g0 + gl)), pl);
#pragma unroll
      for (int q = 0; q < LB; ++q) buf[(q * p.chunk + gl) * p.rs + slot] = pl[q];
    }
  }
}

#define FW_PWD_PAIR(i, j)                                            \
  {                                                                  \
    uint32_t x = A[0][i] ^ B[0][j];                                  \
    _Pragma("unroll") for (int q = 1; q < LB; ++q) x |= A[q][i] ^ B[q][j]; \
    acc##i##j += fw_pwd_count(x);                                    \
  }

template <int LB>
__global__ __launch_bounds__(FW_PWD_THREADS) void fw_pairdist_kernel(FwPairdistParams p) {
  extern __shared__ __align__(16) uint32_t lds[];
  const int gx = (p.mb + p.tile - 1) / p.tile;  // a flat grid: a grid's y extent stops at 65535
  const int by = (int)(blockIdx.x / (unsigned)gx), bx = (int)(blockIdx.x - (unsigned)by * (unsigned)gx);
  if (p.symmetric && bx < by) return;  // the whole workgroup: no barrier is left waiting
  const int tile = p.tile, side = tile >> 2;  // threads a side
  const int tid = threadIdx.x, ti = tid / side, tj = tid - ti * side;
  const bool counts = ti < side;  // tile 16 and 32 leave threads that only stage
  const int a0 = by * tile, b0 = bx * tile;
  const int buf_words = p.chunk * LB * p.rs;
  uint32_t acc00 = 0, acc01 = 0, acc02 = 0, acc03 = 0, acc10 = 0, acc11 = 0, acc12 = 0, acc13 = 0,
           acc20 = 0, acc21 = 0, acc22 = 0, acc23 = 0, acc30 = 0, acc31 = 0, acc32 = 0, acc33 = 0;
  uint32_t w[16 / LB][LB];
  const int groups = (p.n + 31) >> 5;
  {
    const int gn = groups < p.chunk ? groups : p.chunk;
    pwd_fetch<LB>(p, a0, b0, 0, gn, w);
    pwd_stage<LB>(p, 0, gn, lds, w);
  }
  __syncthreads();
  for (int c = 0; c < p.n_chunks; ++c) {
    const int g0 = c * p.chunk, gn = groups - g0 < p.chunk ? groups - g0 : p.chunk;
    const int g1 = g0 + p.chunk, gn1 = groups - g1 < p.chunk ? groups - g1 : p.chunk;
    const bool more = c + 1 < p.n_chunks;
    if (more) pwd_fetch<LB>(p, a0, b0, g1, gn1, w);  // in flight during the count
    if (counts) {
      const uint32_t* cur = lds + (c & 1) * buf_words;
      // two groups in flight at the narrow widths; left alone, the compiler unrolls this loop
      // far enough at 4 bits and above to spill
#pragma unroll(LB <= 3 ? 2 : 1)
      for (int gl = 0; gl < gn; ++gl) {
        uint32_t A[LB][4], B[LB][4];
#pragma unroll
        for (int q = 0; q < LB; ++q) {
          const uint32_t* row = cur + (q * p.chunk + gl) * p.rs;
          const uint4 av = *reinterpret_cast<const uint4*>(row + 4 * ti);
          const uint4 bv = *reinterpret_cast<const uint4*>(row + tile + 4 * tj);
          A[q][0] = av.x, A[q][1] = av.y, A[q][2] = av.z, A[q][3] = av.w;
          B[q][0] = bv.x, B[q][1] = bv.y, B[q][2] = bv.z, B[q][3] = bv.w;
        }
        FW_PWD_PAIR(0, 0) FW_PWD_PAIR(0, 1) FW_PWD_PAIR(0, 2) FW_PWD_PAIR(0, 3)
        FW_PWD_PAIR(1, 0) FW_PWD_PAIR(1, 1) FW_PWD_PAIR(1, 2) FW_PWD_PAIR(1, 3)
        FW_PWD_PAIR(2, 0) FW_PWD_PAIR(2, 1) FW_PWD_PAIR(2, 2) FW_PWD_PAIR(2, 3)
        FW_PWD_PAIR(3, 0) FW_PWD_PAIR(3, 1) FW_PWD_PAIR(3, 2) FW_PWD_PAIR(3, 3)
      }
    }
    if (more) pwd_stage<LB>(p, g1, gn1, lds + ((c + 1) & 1) * buf_words, w);
    __syncthreads();  // chunk c + 1 is complete, and chunk c has been read by every wave
  }
  if (!counts) return;
  const bool mirror = p.symmetric && bx != by;
  const uint32_t out[4][4] = {{acc00, acc01, acc02, acc03},
                              {acc10, acc11, acc12, acc13},
                              {acc20, acc21, acc22, acc23},
                              {acc30, acc31, acc32, acc33}};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ia = a0 + 4 * ti + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int jb = b0 + 4 * tj + j;
      if (ia < p.ma && jb < p.mb) {
        p.D[(int64_t)ia * p.mb + jb] = (int32_t)out[i][j];
        if (mirror) p.D[(int64_t)jb * p.mb + ia] = (int32_t)out[i][j];
      }
    }
  }
}

__global__ __launch_bounds__(256) void fw_pairdist_reduce_kernel(FwPairdistReduceParams r) {
  extern __shared__ __align__(16) uint32_t bins[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < r.lds_bins; i += 256) bins[i] = 0u;
  __syncthreads();
  for (int row = blockIdx.x * 4 + wave; row < r.ma; row += gridDim.x * 4) {
    const int32_t* d = r.D + (int64_t)row * r.mb;
    unsigned long long sum = 0ull, best = ~0ull;
    for (int j = lane; j < r.mb; j += 64) {
      const int32_t v = d[j];
      sum += (unsigned long long)(uint32_t)v;
      if (!(r.symmetric && j == row)) {
        const unsigned long long key = ((unsigned long long)(uint32_t)v << 32) | (uint32_t)j;
        best = key < best ? key : best;
      }
      if ((!r.symmetric || j > row) && v >= 0 && v <= r.n) {
        if (r.lds_bins)
          atomicAdd(&bins[v], 1u);
        else
          atomicAdd(&r.hist[v], 1ull);
      }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const uint32_t slo = (uint32_t)__shfl_xor((int)(uint32_t)sum, s, 64);
      const uint32_t shi = (uint32_t)__shfl_xor((int)(uint32_t)(sum >> 32), s, 64);
      const uint32_t blo = (uint32_t)__shfl_xor((int)(uint32_t)best, s, 64);
      const uint32_t bhi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), s, 64);
      sum += ((unsigned long long)shi << 32) | slo;
      const unsigned long long other = ((unsigned long long)bhi << 32) | blo;
      best = other < best ? other : best;
    }
    if (lane == 0) {
      r.rowsum[row] = (int64_t)sum;
      const bool none = best == ~0ull;  // the symmetric case with one member
      r.nearest[2 * (int64_t)row] = none ? -1 : (int32_t)(uint32_t)(best >> 32);
      r.nearest[2 * (int64_t)row + 1] = none ? -1 : (int32_t)(uint32_t)best;
    }
  }
  __syncthreads();  // every wave's rows are in the bins
  for (int i = threadIdx.x; i < r.lds_bins; i += 256)
    if (bins[i]) atomicAdd(&r.hist[i], (unsigned long long)bins[i]);
}

}  // namespace

int fw_pairdist_env(const char* name) {
  const char* e = getenv(name);
  return e && e[0] ? atoi(e) : -1;
}

int fw_launch_pairdist(const FwPairdistParams& p, void* stream) {
  void* fn;
  switch (p.lb) {
    case 2: fn = reinterpret_cast<void*>(&fw_pairdist_kernel<2>); break;
    case 3: fn = reinterpret_cast<void*>(&fw_pairdist_kernel<3>); break;
    case 4: fn = reinterpret_cast<void*>(&fw_pairdist_kernel<4>); break;
    case 5: fn = reinterpret_cast<void*>(&fw_pairdist_kernel<5>); break;
    case 8: fn = reinterpret_cast<void*>(&fw_pairdist_kernel<8>); break;
    default: return (int)hipErrorInvalidValue;
  }
  void* args[] = {const_cast<FwPairdistParams*>(&p)};
  const unsigned gx = (unsigned)((p.mb + p.tile - 1) / p.tile), gy = (unsigned)((p.ma + p.tile - 1) / p.tile);
  return (int)hipLaunchKernel(fn, dim3(gx * gy), dim3(FW_PWD_THREADS), args, (size_t)p.lds_bytes,
                              (hipStream_t)stream);
}

int fw_launch_pairdist_reduce(const FwPairdistReduceParams& r, void* stream) {
  void* args[] = {const_cast<FwPairdistReduceParams*>(&r)};
  int grid = (r.ma + 3) / 4;
  if (grid > 2048) grid = 2048;
  return (int)hipLaunchKernel(reinterpret_cast<void*>(&fw_pairdist_reduce_kernel), dim3(grid),
                              dim3(256), args, sizeof(uint32_t) * (size_t)r.lds_bins,
                              (hipStream_t)stream);
}
