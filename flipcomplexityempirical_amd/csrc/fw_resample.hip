// fw_resample.hip — resampling plans across chains: the gather that lets chain i continue from the
// plan of chain src[i], and the source map of one systematic resampling by cut (the resample entry
// points of include/flipwalk.h; parameter structs in fw_internal.h).  Like the exchange, record,
// tally, geometry and overlap steps this runs between launches on the handle's stream, on the
// records the run kernels leave in HBM; no run kernel knows of it.
//
// fw_clone_kernel: one wave per destination chain, FW_RSM_CLONE_NW waves a workgroup.  A wave whose
// chain is a fixed point (src[i] == i) exits on that one load.  The others copy the source's label
// record (labels and the group sums behind them, lab_stride bytes) with 16-byte loads and stores,
// lane l taking pieces l, l + 64, ...; lanes d < k copy the k populations (and the k flagged-node
// counts), and lane 0 the four plan fields of the stats record, the current state's sampled wait
// and the family.  Every source is a fixed point of the map (checked on the host, or true by
// construction of the map kernel), so no source is written in the launch and the order of the waves
// cannot matter; every word has one owner and is a plain vector store; no atomics.
//
// fw_resample_map_kernel: ONE workgroup of 1,024 threads walks the chains in tiles of 1,024, in
// six passes separated by workgroup barriers (a single-workgroup scan: at most 2^20 chains, and the
// step runs once per thousands of chain steps; DESIGN.md §6f has its measured cost):
//   1. cref = min (sign +1) or max (sign -1) of the cuts;
//   2. w[i] = q[sign (cut_i - cref)], cum[i] = the inclusive prefix sum (uint64), S2 = sum of
//      (w >> 10)^2, T = cum[C - 1];
//   3. the points pts[j] = fw_rsm_point(j, u, T, C) (fw_resample_limbs.h), u the x0 word of the
//      Philox block below;
//   4. lower[i] = #{j : pts[j] < cum[i]} by binary search (the points ascend), so that the
//      offspring count is n_i = lower[i] - lower[i - 1];
//   5. dead chains (n_i = 0) get their rank among the dead, survivors keep themselves, and
//      extra[i] = the inclusive prefix sum of max(n_i - 1, 0);
//   6. the dead chain of rank r takes the survivor s with extra[s - 1] <= r < extra[s], again by
//      binary search.
// Every quantity is an integer; the scans add in a fixed tree; nothing depends on thread order.
//
// The draw: Philox4x32-10, key = seed, counter = (lo32(round), 2^30 | 2^29, lo32(chain_id0),
// hi32(chain_id0)).  Counter word 1 tells the streams apart: a proposal draw has word 1 = hi32 of
// the attempt counter < 2^30 (bits 30 and 31 clear), a wait draw has bit 31 set, an exchange draw
// has bit 30 set, bit 31 clear and a rung < 64 below it (bit 29 clear); this one has bits 30 and 29
// set and bit 31 clear, which none of the three can produce.
#include <hip/hip_runtime.h>

#include "fw_device.h"
#include "fw_internal.h"
#include "fw_resample_limbs.h"

namespace {

__global__ __launch_bounds__(64 * FW_RSM_CLONE_NW) void fw_clone_kernel(FwCloneParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * FW_RSM_CLONE_NW + (threadIdx.x >> 6);
  if (i >= p.n_chains) return;
  const int64_t s = p.src[i];
  if (s == i || s < 0 || s >= p.n_chains) return;  // the host has checked the range
  const uint4* from = reinterpret_cast<const uint4*>(p.labels + s * p.lab_stride);
  uint4* to = reinterpret_cast<uint4*>(p.labels + i * p.lab_stride);
  const int pieces = (int)(p.lab_stride >> 4);
  for (int j = lane; j < pieces; j += 64) to[j] = from[j];
  if (lane < p.k) {
    p.pops[i * p.k + lane] = p.pops[s * p.k + lane];
    if (p.bcnt) p.bcnt[i * p.k + lane] = p.bcnt[s * p.k + lane];
  }
  if (lane == 0) {
    const fw_chain_stats* a = p.stats + s;
    fw_chain_stats* b = p.stats + i;
    b->cut = a->cut;
    b->bnodes = a->bnodes;
    b->npairs = a->npairs;
    b->stuck = a->stuck;
    if (p.wsamp) p.wsamp[2 * i + 1] = p.wsamp[2 * s + 1];
    p.family[i] = p.family[s];
  }
}

// Inclusive prefix sum of v over the workgroup's 1,024 threads in thread order; *total = the sum.
// Two barriers; part [16] is the workgroup's scratch.
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* part, uint64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t up = __shfl_up(v, d, 64);
    if (lane >= d) v += up;
  }
  __syncthreads();  // the last use of part is over
  if (lane == 63) part[wave] = v;
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (int wv = 0; wv < FW_RSM_THREADS / 64; ++wv) {
    const uint64_t t = part[wv];
    if (wv < wave) before += t;
    all += t;
  }
  *total = all;
  return v + before;
}

// max of v over the workgroup (v >= 0)
__device__ __forceinline__ int64_t block_max(int64_t v, int64_t* part) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int64_t o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  int64_t m = part[0];
#pragma unroll
  for (int wv = 1; wv < FW_RSM_THREADS / 64; ++wv) m = part[wv] > m ? part[wv] : m;
  return m;
}

__global__ __launch_bounds__(FW_RSM_THREADS) void fw_resample_map_kernel(FwResampleParams p) {
  __shared__ uint64_t part[FW_RSM_THREADS / 64];
  const int tid = threadIdx.x, C = p.n_chains;

  // 1. the reference cut, as a maximum of sign * (-cut) so that one reduction serves both signs
  int64_t best = INT64_MIN;
  for (int i = tid; i < C; i += FW_RSM_THREADS) {
    const int64_t v = -(int64_t)p.sign * (int64_t)p.stats[i].cut;
    best = v > best ? v : best;
  }
  const int64_t cref = -(int64_t)p.sign * block_max(best, reinterpret_cast<int64_t*>(part));

  // 2. weights, their prefix sums and the sum of squares
  uint64_t carry = 0, s2 = 0;
  for (int base = 0; base < C; base += FW_RSM_THREADS) {
    const int i = base + tid;
    uint32_t w = 0;
    if (i < C) {
      int64_t d = (int64_t)p.sign * ((int64_t)p.stats[i].cut - cref);
      d = d < 0 ? 0 : (d > p.n_edges ? p.n_edges : d);  // 0 <= d <= n_edges for any cut a run leaves
      w = p.q[d];
      p.w[i] = w;
      s2 += (uint64_t)(w >> 10) * (uint64_t)(w >> 10);
    }
    uint64_t tile;
    const uint64_t inc = block_scan(w, part, &tile);
    if (i < C) p.cum[i] = carry + inc;
    carry += tile;
  }
  const uint64_t T = carry;
  uint64_t S2;
  (void)block_scan(s2, part, &S2);

  // 3. the points
  const U4 y = philox(p.round, 0x60000000u, (uint32_t)p.chain_id0, (uint32_t)((uint64_t)p.chain_id0 >> 32),
                      (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
  const uint32_t u = y.x0;
  for (int j = tid; j < C; j += FW_RSM_THREADS) p.pts[j] = fw_rsm_point((uint32_t)j, u, T, (uint32_t)C);
  __threadfence();
  __syncthreads();  // cum and pts are complete

  // 4. lower[i] = the first j with pts[j] >= cum[i] (C when there is none)
  for (int i = tid; i < C; i += FW_RSM_THREADS) {
    const uint64_t x = p.cum[i];
    int lo = 0, hi = C;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (p.pts[mid] < x) lo = mid + 1; else hi = mid;
    }
    p.lower[i] = lo;
  }
  __threadfence();
  __syncthreads();

  // 5. offspring; the dead take their rank, the survivors themselves; the extra copies' scan
  uint64_t dead_carry = 0, extra_carry = 0, alive = 0;
  int64_t most = 0;
  for (int base = 0; base < C; base += FW_RSM_THREADS) {
    const int i = base + tid;
    int n_i = 1;  // past the end: neither dead nor with extras
    if (i < C) n_i = p.lower[i] - (i ? p.lower[i - 1] : 0);
    const uint64_t dead = n_i == 0 ? 1u : 0u, ext = n_i > 1 ? (uint64_t)(n_i - 1) : 0u;
    uint64_t dead_tile, ext_tile;
    const uint64_t dead_inc = block_scan(dead, part, &dead_tile);
    const uint64_t ext_inc = block_scan(ext, part, &ext_tile);
    if (i < C) {
      p.src[i] = dead ? -(int32_t)(dead_carry + dead_inc) : i;  // -(rank + 1)
      p.extra[i] = (int32_t)(extra_carry + ext_inc);
      alive += dead ? 0u : 1u;
      most = n_i > most ? n_i : most;
    }
    dead_carry += dead_tile;
    extra_carry += ext_tile;
  }
  uint64_t survivors;
  (void)block_scan(alive, part, &survivors);
  most = block_max(most, reinterpret_cast<int64_t*>(part));
  __threadfence();
  __syncthreads();  // extra is complete

  // 6. the dead chain of rank r takes the first survivor s with extra[s] > r
  for (int i = tid; i < C; i += FW_RSM_THREADS) {
    const int v = p.src[i];  // this thread's own store of pass 5
    if (v >= 0) continue;
    const int r = -v - 1;
    int lo = 0, hi = C - 1;  // the sums of the dead and of the extras are equal: extra[C - 1] > r
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (p.extra[mid] > r) hi = mid; else lo = mid + 1;
    }
    p.src[i] = lo;
  }
  if (tid == 0) {
    p.info[0] = (int64_t)T;
    p.info[1] = (int64_t)S2;
    p.info[2] = cref;
    p.info[3] = (int64_t)survivors;
    p.info[4] = most;
    p.info[5] += (int64_t)C - (int64_t)survivors;  // one owner: launches of a stream are ordered
    p.info[6] = (int64_t)u;
  }
}

}  // namespace

int fw_launch_clone(const FwCloneParams& p, void* stream) {
  void* args[] = {const_cast<FwCloneParams*>(&p)};
  return (int)hipLaunchKernel(reinterpret_cast<void*>(&fw_clone_kernel),
                              dim3((unsigned)((p.n_chains + FW_RSM_CLONE_NW - 1) / FW_RSM_CLONE_NW)),
                              dim3(64 * FW_RSM_CLONE_NW), args, 0, (hipStream_t)stream);
}

int fw_launch_resample_map(const FwResampleParams& p, void* stream) {
  void* args[] = {const_cast<FwResampleParams*>(&p)};
  return (int)hipLaunchKernel(reinterpret_cast<void*>(&fw_resample_map_kernel), dim3(1),
                              dim3(FW_RSM_THREADS), args, 0, (hipStream_t)stream);
}
