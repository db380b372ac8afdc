// fw_overlap.hip — overlap matrices and Hamming distances of every chain's current plan against
// a reference plan or a partner chain's plan, and the histogram of the distances (the overlap
// entry points of include/flipwalk.h; parameter structs in fw_internal.h).  Like the exchange,
// record, tally and geometry steps this runs between launches on the handle's stream, from the
// label records the run kernels leave in HBM; no run kernel knows of it.
//
// Both plans of a pair are packed alike: node x in bits [x lb, x lb + lb), so lb consecutive
// dwords hold exactly 32 nodes at every width and the same dwords of the two records hold the
// same nodes.  A workgroup is NW waves, one chain per wave; nothing is shared between waves, so
// the labels are not staged in LDS.  Lane l takes the 32-node groups l, l + 64, ...: lb dwords
// of X (the current plan) and lb of R, loaded from HBM as wide as the alignment of a group
// allows (16 B at 4 and 8 bits, 8 B at 2, dwords at 3 and 5).  Dwords past the label words of a
// record (its group sums follow them) read as zero, and the last group is masked to n.
//
// fw_overlap_kernel<LB>: per-wave LDS bins uint32 [k][k].  Per group a lane takes the lowest
// remaining node, cuts its pair (r, x) from the words, forms by SWAR (fw_overlap_bits.h) the
// mask of the group's nodes with that pair, adds its population count to bin r k + x with one
// LDS atomic and clears those nodes; neighbouring nodes mostly share a pair, so a group takes
// one to three rounds, and a random reference up to 32.  The XOR of the two word sets, reduced
// to one bit per differing field, gives the distance.  The adds are integer: their sum does not
// depend on the order.  After the workgroup's barrier the wave's lanes write the k^2 bins to
// O[c] as int64 and lane 0 writes dist[c]: plain vector stores, one owner each; no global
// atomics touch O or dist.  Every wave reaches every barrier; a wave without a chain computes
// nothing.
//
// fw_overlap_hist_kernel: one thread per chain adds hist[group][dist[c]] with an integer atomic
// in HBM (up to n + 1 bins a group: no LDS copy).
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include "fw_internal.h"
#include "fw_overlap_bits.h"

namespace {

// dwords [g LB, g LB + LB) of a record -> w; whole groups inside the label words with one wide
// load where LB allows (rec is 16-byte aligned), the others dword by dword, zero past the words
template <int LB>
__device__ __forceinline__ void load_group(const uint32_t* rec, int g, int lab_words,
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

template <int LB>
__global__ __launch_bounds__(64 * FW_OVL_MAX_NW) void fw_overlap_kernel(FwOverlapParams p) {
  extern __shared__ __align__(16) uint32_t lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int k = p.k, kk = p.k * p.k;
  uint32_t* bins = lds + wave * kk;  // this wave's [k][k]
  const int64_t c = (int64_t)blockIdx.x * nw + wave;
  const bool live = c < p.n_chains;
  for (int i = lane; i < kk; i += 64) bins[i] = 0u;
  __syncthreads();
  uint32_t differ = 0u;
  if (live) {
    const uint32_t* xr = reinterpret_cast<const uint32_t*>(p.labels + c * p.lab_stride);
    const uint32_t* rr =
        p.partner ? reinterpret_cast<const uint32_t*>(p.labels + (int64_t)p.partner[c] * p.lab_stride)
                  : p.ref + c * p.ref_stride;
    const int groups = (p.n + 31) >> 5;
    for (int g = lane; g < groups; g += 64) {
      uint32_t X[LB], R[LB];
      load_group<LB>(xr, g, p.lab_words, X);
      load_group<LB>(rr, g, p.lab_words, R);
      uint32_t rem = fw_ovl_tail_mask(p.n - 32 * g);
      differ += (uint32_t)__popc(fw_ovl_diff_mask<LB>(R, X) & rem);
      while (rem) {
        const int j = __ffs((int)rem) - 1;
        const uint32_t a = fw_ovl_field<LB>(R, j), b = fw_ovl_field<LB>(X, j);
        const uint32_t m = fw_ovl_pair_mask<LB>(R, X, a, b) & rem;  // holds node j
        // labels the run kernels leave are below k; a stray value is not counted
        if (a < (uint32_t)k && b < (uint32_t)k) atomicAdd(&bins[a * k + b], (uint32_t)__popc(m));
        rem &= ~m;
      }
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) differ += (uint32_t)__shfl_xor((int)differ, s, 64);
  __syncthreads();  // the wave's bins are complete
  if (live) {
    int64_t* out = p.O + c * kk;
    for (int i = lane; i < kk; i += 64) out[i] = (int64_t)bins[i];
    if (lane == 0) p.dist[c] = (int32_t)differ;
  }
}

__global__ __launch_bounds__(256) void fw_overlap_hist_kernel(FwOverlapHistParams h) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= h.n_chains) return;
  int g = h.rung ? h.rung[c] : 0;
  if (g < 0 || g >= h.n_groups) g = 0;  // the exchange kernel keeps rungs inside the ladder
  const int d = h.dist[c];
  if (d >= 0 && d <= h.n) atomicAdd(&h.hist[(size_t)g * (size_t)(h.n + 1) + (size_t)d], 1ull);
}

}  // namespace

// Waves (chains) per workgroup: the largest NW <= 16 whose [k][k] bins fit 64 KB of LDS (k = 64:
// 4).  FLIPWALK_OVL_NW lowers it (tests force 1 and a partly filled last workgroup).
void fw_overlap_plan(int k, int* nw, int* lds_bytes) {
  const int per_wave = 4 * k * k;
  int w = (64 * 1024) / per_wave;
  if (w > FW_OVL_MAX_NW) w = FW_OVL_MAX_NW;
  if (w < 1) w = 1;  // cannot happen: k <= FW_MAX_K
  const char* e = getenv("FLIPWALK_OVL_NW");
  if (e && e[0]) {
    const int f = atoi(e);
    if (f >= 1 && f < w) w = f;
  }
  *nw = w;
  *lds_bytes = w * per_wave;
}

int fw_launch_overlap(const FwOverlapParams& p, int nw, int lds_bytes, void* stream) {
  void* fn;
  switch (p.lb) {
    case 2: fn = reinterpret_cast<void*>(&fw_overlap_kernel<2>); break;
    case 3: fn = reinterpret_cast<void*>(&fw_overlap_kernel<3>); break;
    case 4: fn = reinterpret_cast<void*>(&fw_overlap_kernel<4>); break;
    case 5: fn = reinterpret_cast<void*>(&fw_overlap_kernel<5>); break;
    case 8: fn = reinterpret_cast<void*>(&fw_overlap_kernel<8>); break;
    default: return (int)hipErrorInvalidValue;
  }
  void* args[] = {const_cast<FwOverlapParams*>(&p)};
  return (int)hipLaunchKernel(fn, dim3((unsigned)((p.n_chains + nw - 1) / nw)), dim3(64 * nw),
                              args, (size_t)lds_bytes, (hipStream_t)stream);
}

int fw_launch_overlap_hist(const FwOverlapHistParams& h, void* stream) {
  void* args[] = {const_cast<FwOverlapHistParams*>(&h)};
  return (int)hipLaunchKernel(reinterpret_cast<void*>(&fw_overlap_hist_kernel),
                              dim3((h.n_chains + 255) / 256), dim3(256), args, 0,
                              (hipStream_t)stream);
}
