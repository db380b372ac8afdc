// fw_geometry.hip — per-district node counts, cut edges, interior and exterior perimeters and
// areas of every chain's current plan, and the histogram of the per-district cut (the geometry
// entry points of include/flipwalk.h; parameter structs in fw_internal.h).  Like the exchange,
// record and tally steps this runs between launches on the handle's stream, from the label
// records the run kernels leave in HBM; no run kernel knows of it.
//
// An edge joins two arbitrary nodes, so a tile of labels (fw_tally.hip) is not enough: a wave
// keeps its chain's whole label field in LDS (ceil(n lb / 32) + 1 words, copied once with
// coalesced dword loads; the group sums that follow it in the record are not copied) and the
// edge list is streamed through it.  A workgroup is NW waves, one chain per wave; it walks the
// edges in tiles and stages each tile's {u, w, weight} in LDS once for all its waves (with unit
// weights no weight array is staged or read).  Lane l takes edge tile + 64 s + l: its endpoints
// are consecutive LDS slots, its two labels are cut from the wave's copy with the tally's
// v_alignbit_b32 extraction (one piece of code for 2-, 3-, 4-, 5- and 8-bit fields), and count
// and weight go to both districts when the labels differ.  The node quantities (count,
// exterior, area) are a second walk over the same resident labels with the two node arrays
// staged by tile in the same way.  Every loop bound is uniform over the workgroup, so every
// wave reaches every barrier; a wave without a chain stages no labels and computes nothing.
//
//  - fw_geometry_kernel<KB, W>: register accumulators, a compare and select-adds per district,
//    folded over the wave at the end of a walk.  Districts are taken KB at a time (one round
//    for k <= KB; more rounds serve k > 8 when the LDS bins below do not fit).
//  - fw_geometry_bins_kernel: per-wave LDS bins [Q][k][64], a private copy per lane (lane l
//    only touches bank l mod 32: no conflicts, no atomics); Q quantities are taken per walk, as
//    many as the LDS plan allows, and lane d adds up row d from a lane-dependent start.
// Sums are unsigned 32-bit: the host checked that every array's total is below 2^31, and a
// district's interior perimeter is at most the total edge weight.  Every G[c][d][f] is written
// once, by one lane, as a plain int64 vector store; there are no global atomics and no floats.
//
// fw_geometry_hist_kernel: one thread per chain adds its k values of G[c][d][1] to
// hist[group] with integer atomics in HBM (up to n_edges + 1 bins a group: no LDS copy).
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include "fw_internal.h"

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
  return v;
}

// The label words of one chain -> lw[0 .. lab_words).  Words past the record read as zero (the
// label part of a record is longer than lab_words; the check costs nothing).
__device__ __forceinline__ void copy_labels(const FwGeomParams& p, const uint8_t* rec,
                                            uint32_t* lw, int lane) {
  const int rec_words = (int)(p.lab_stride >> 2);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(rec);
  for (int i = lane; i < p.lab_words; i += 64) lw[i] = i < rec_words ? src[i] : 0u;
}

// Label of node x from the resident words.
__device__ __forceinline__ uint32_t node_label(const uint32_t* lw, int lb, int x) {
  const int bit = x * lb;
  // v_alignbit_b32: the low dword of {hi, lo} >> (bit & 31)
  return __builtin_amdgcn_alignbit(lw[(bit >> 5) + 1], lw[bit >> 5], (uint32_t)(bit & 31)) &
         ((1u << lb) - 1u);
}

// Edges [t0, t0 + tile) -> tu, tw (and tv with weights); slots past the list are not read back.
template <bool W>
__device__ __forceinline__ void stage_edges(const FwGeomParams& p, int t0, uint32_t* tu,
                                            uint32_t* tw, uint32_t* tv) {
  for (int i = threadIdx.x; i < p.tile; i += blockDim.x) {
    const bool in = t0 + i < p.n_edges;
    tu[i] = in ? (uint32_t)p.eu[t0 + i] : 0u;
    tw[i] = in ? (uint32_t)p.ew[t0 + i] : 0u;
    if (W) tv[i] = in ? p.ewt[t0 + i] : 0u;
  }
}

// Nodes [t0, t0 + tile): exterior -> te (0 without the array), area -> ta (1 without it).
__device__ __forceinline__ void stage_nodes(const FwGeomParams& p, int t0, uint32_t* te,
                                            uint32_t* ta) {
  for (int i = threadIdx.x; i < p.tile; i += blockDim.x) {
    const bool in = t0 + i < p.n;
    te[i] = in && p.ext ? p.ext[t0 + i] : 0u;
    ta[i] = in ? (p.area ? p.area[t0 + i] : 1u) : 0u;
  }
}

template <int KB, bool W>
__global__ __launch_bounds__(64 * FW_GEOM_MAX_NW) void fw_geometry_kernel(FwGeomParams p) {
  extern __shared__ __align__(16) uint32_t lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint32_t* t0s = lds;               // [tile] edge u      | node exterior
  uint32_t* t1s = lds + p.tile;      // [tile] edge w      | node area
  uint32_t* t2s = lds + 2 * p.tile;  // [tile] edge weight (W only)
  uint32_t* lw = lds + (W ? 3 : 2) * p.tile + wave * p.lab_words;  // this wave's labels
  const int64_t c = (int64_t)blockIdx.x * nw + wave;
  const bool live = c < p.n_chains;
  if (live) copy_labels(p, p.labels + c * p.lab_stride, lw, lane);
  const int k = p.k, lb = p.lb;
  for (int d0 = 0; d0 < k; d0 += KB) {
    // ---- edges: cut count and interior perimeter
    uint32_t ac[KB], aw[KB];
#pragma unroll
    for (int d = 0; d < KB; ++d) ac[d] = aw[d] = 0u;
    for (int t = 0; t < p.n_edges; t += p.tile) {
      __syncthreads();  // the previous tile has been read (first round: the labels are in)
      stage_edges<W>(p, t, t0s, t1s, t2s);
      __syncthreads();
      if (live) {
        const int end = p.n_edges - t < p.tile ? p.n_edges - t : p.tile;
        for (int o = lane; o < end; o += 64) {
          const uint32_t lu = node_label(lw, lb, (int)t0s[o]) - (uint32_t)d0;
          const uint32_t lv = node_label(lw, lb, (int)t1s[o]) - (uint32_t)d0;
          const bool cut = lu != lv;
          const uint32_t c1 = cut ? 1u : 0u;
          const uint32_t cw = W ? (cut ? t2s[o] : 0u) : 0u;
#pragma unroll
          for (int d = 0; d < KB; ++d) {
            const bool m = lu == (uint32_t)d || lv == (uint32_t)d;
            ac[d] += m ? c1 : 0u;
            if (W) aw[d] += m ? cw : 0u;
          }
        }
      }
    }
    // every index into the accumulators is a constant after unrolling: no scratch
#pragma unroll
    for (int d = 0; d < KB; ++d) {
      const uint32_t s1 = wave_sum(ac[d]);
      const uint32_t s2 = W ? wave_sum(aw[d]) : s1;
      if (live && lane == d && d0 + d < k) {
        int64_t* out = p.out + ((size_t)c * k + d0 + d) * 5;
        out[1] = (int64_t)s1;
        out[2] = (int64_t)s2;
      }
    }
    // ---- nodes: count, exterior perimeter, area
    uint32_t an[KB], ae[KB], aa[KB];
#pragma unroll
    for (int d = 0; d < KB; ++d) an[d] = ae[d] = aa[d] = 0u;
    for (int t = 0; t < p.n; t += p.tile) {
      __syncthreads();
      stage_nodes(p, t, t0s, t1s);
      __syncthreads();
      if (live) {
        const int end = p.n - t < p.tile ? p.n - t : p.tile;
        for (int o = lane; o < end; o += 64) {
          const uint32_t lab = node_label(lw, lb, t + o) - (uint32_t)d0;
          const uint32_t ve = t0s[o], va = t1s[o];
#pragma unroll
          for (int d = 0; d < KB; ++d) {
            const bool m = lab == (uint32_t)d;
            an[d] += m ? 1u : 0u;
            ae[d] += m ? ve : 0u;
            aa[d] += m ? va : 0u;
          }
        }
      }
    }
#pragma unroll
    for (int d = 0; d < KB; ++d) {
      const uint32_t s0 = wave_sum(an[d]), s3 = wave_sum(ae[d]), s4 = wave_sum(aa[d]);
      if (live && lane == d && d0 + d < k) {
        int64_t* out = p.out + ((size_t)c * k + d0 + d) * 5;
        out[0] = (int64_t)s0;
        out[3] = (int64_t)s3;
        out[4] = (int64_t)s4;
      }
    }
  }
}

// Row sums of the wave's bins -> G[c][lane][column of quantity q0 + q], then the bins restart at
// zero.  Edge quantities 0, 1 are columns 1, 2; node quantities 0, 1, 2 are columns 0, 3, 4.
// Called by every wave (the barriers), with the same nq.
__device__ __forceinline__ void flush_bins(const FwGeomParams& p, uint32_t* bins, int64_t c,
                                           bool live, int lane, int nq, int q0, bool nodes) {
  const int k = p.k;
  __syncthreads();  // the wave's bins are complete
  if (live && lane < k)
    for (int q = 0; q < nq; ++q) {
      uint32_t s = 0u;
      for (int i = 0; i < 64; ++i) s += bins[(q * k + lane) * 64 + ((i + lane) & 63)];
      const int f = q0 + q;
      p.out[((size_t)c * k + lane) * 5 + (nodes ? (f == 0 ? 0 : f + 2) : f + 1)] = (int64_t)s;
    }
  __syncthreads();  // row sums taken before the bins restart
  for (int i = lane; i < p.bins * k * 64; i += 64) bins[i] = 0u;
}

template <bool W>
__global__ __launch_bounds__(64 * FW_GEOM_MAX_NW) void fw_geometry_bins_kernel(FwGeomParams p) {
  extern __shared__ __align__(16) uint32_t lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int k = p.k, lb = p.lb, Q = p.bins;
  uint32_t* t0s = lds;
  uint32_t* t1s = lds + p.tile;
  uint32_t* t2s = lds + 2 * p.tile;
  uint32_t* lw = lds + (W ? 3 : 2) * p.tile + wave * p.lab_words;
  uint32_t* bins = lds + (W ? 3 : 2) * p.tile + nw * p.lab_words + wave * Q * k * 64;  // [Q][k][64]
  const int64_t c = (int64_t)blockIdx.x * nw + wave;
  const bool live = c < p.n_chains;
  if (live) copy_labels(p, p.labels + c * p.lab_stride, lw, lane);
  for (int i = lane; i < Q * k * 64; i += 64) bins[i] = 0u;
  // ---- edges: quantity 0 = cut count (column 1), 1 = interior perimeter (column 2)
  const int nqe = W ? 2 : 1;
  for (int q0 = 0; q0 < nqe; q0 += Q) {
    const int nq = nqe - q0 < Q ? nqe - q0 : Q;
    for (int t = 0; t < p.n_edges; t += p.tile) {
      __syncthreads();
      stage_edges<W>(p, t, t0s, t1s, t2s);
      __syncthreads();
      if (live) {
        const int end = p.n_edges - t < p.tile ? p.n_edges - t : p.tile;
        for (int o = lane; o < end; o += 64) {
          const uint32_t lu = node_label(lw, lb, (int)t0s[o]);
          const uint32_t lv = node_label(lw, lb, (int)t1s[o]);
          if (lu != lv && lu < (uint32_t)k && lv < (uint32_t)k) {
            const uint32_t wt = W ? t2s[o] : 1u;
            for (int q = 0; q < nq; ++q) {
              const uint32_t v = q0 + q == 0 ? 1u : wt;
              bins[(q * k + lu) * 64 + lane] += v;  // the lane's own copies
              bins[(q * k + lv) * 64 + lane] += v;
            }
          }
        }
      }
    }
    flush_bins(p, bins, c, live, lane, nq, q0, false);
  }
  if (!W && live && lane < k) {  // unit weights: the interior perimeter is the cut count
    int64_t* out = p.out + ((size_t)c * k + lane) * 5;
    out[2] = out[1];  // this lane's own store, just above
  }
  // ---- nodes: quantity 0 = count (column 0), 1 = exterior (column 3), 2 = area (column 4)
  for (int q0 = 0; q0 < 3; q0 += Q) {
    const int nq = 3 - q0 < Q ? 3 - q0 : Q;
    for (int t = 0; t < p.n; t += p.tile) {
      __syncthreads();
      stage_nodes(p, t, t0s, t1s);
      __syncthreads();
      if (live) {
        const int end = p.n - t < p.tile ? p.n - t : p.tile;
        for (int o = lane; o < end; o += 64) {
          const uint32_t lab = node_label(lw, lb, t + o);
          if (lab < (uint32_t)k) {
            const uint32_t ve = t0s[o], va = t1s[o];
            for (int q = 0; q < nq; ++q) {
              const int f = q0 + q;
              bins[(q * k + lab) * 64 + lane] += f == 0 ? 1u : f == 1 ? ve : va;
            }
          }
        }
      }
    }
    flush_bins(p, bins, c, live, lane, nq, q0, true);
  }
}

__global__ __launch_bounds__(256) void fw_geometry_hist_kernel(FwGeomHistParams h) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= h.n_chains) return;
  int g = h.rung ? h.rung[c] : 0;
  if (g < 0 || g >= h.n_groups) g = 0;  // the exchange kernel keeps rungs inside the ladder
  unsigned long long* row = h.hist + (size_t)g * (size_t)(h.n_edges + 1);
  for (int d = 0; d < h.k; ++d) {
    const int64_t v = h.G[((size_t)c * h.k + d) * 5 + 1];
    if (v >= 0 && v <= h.n_edges) atomicAdd(&row[v], 1ull);
  }
}

int env_int(const char* name) {
  const char* e = getenv(name);
  return e && e[0] ? atoi(e) : -1;
}

}  // namespace

// The launch plan of a handle's geometry for (n, k, lb, weights or not): the edge / node tile,
// the quantities binned per walk (0: register accumulators) and the largest NW <= 16 whose
// label copies, shared tile and bins fit the LDS budget.  FLIPWALK_GEOM_TILE / _BINS / _NW
// override the three choices where they fit (tests reach every path on small graphs).
void fw_geometry_plan(int n, int k, int lb, bool has_w, FwGeomPlan* out) {
  const int budget = (160 * 1024 - 64) / 4;  // dwords
  const int tiles = has_w ? 3 : 2;
  FwGeomPlan pl{};
  pl.lab_words = (int)((((int64_t)n * lb + 31) / 32 + 1 + 3) & ~3ll);
  pl.tile = FW_GEOM_TILE;
  {
    const int t = env_int("FLIPWALK_GEOM_TILE");
    if (t >= 64 && t <= FW_GEOM_TILE && t % 64 == 0) pl.tile = t;
  }
  // a label field near the LDS limit leaves room for a short tile only
  while (pl.tile > 64 && tiles * pl.tile + pl.lab_words > budget) pl.tile /= 2;
  const int room = budget - tiles * pl.tile;
  auto waves = [&](int q) {
    const int w = room / (pl.lab_words + q * k * 64);
    return w > FW_GEOM_MAX_NW ? FW_GEOM_MAX_NW : w;
  };
  pl.bins = 0;
  if (k > 8) {
    // Q quantities a walk: 2 + 3 quantities take 2, 3 or 5 walks for Q = 3, 2, 1; the plan
    // with the most chains per walk wins (ties to the fewer walks)
    const int walks[4] = {0, has_w ? 5 : 4, has_w ? 3 : 3, 2};
    const int force = env_int("FLIPWALK_GEOM_BINS");
    int best = 0;
    for (int q = 3; q >= 1; --q) {
      if (force >= 0 && force != q) continue;
      const int w = waves(q);
      if (w >= 1 && (best == 0 || w * walks[best] > waves(best) * walks[q])) best = q;
    }
    pl.bins = best;  // 0: the bins do not fit (or FLIPWALK_GEOM_BINS=0): districts 8 at a time
  }
  pl.nw = waves(pl.bins);
  if (pl.nw < 1) pl.nw = 1;  // cannot happen: a chain's labels fit LDS (fw_chains_create)
  {
    const int w = env_int("FLIPWALK_GEOM_NW");
    if (w >= 1 && w < pl.nw) pl.nw = w;
  }
  pl.lds_bytes = 4 * (tiles * pl.tile + pl.nw * (pl.lab_words + pl.bins * k * 64));
  *out = pl;
}

int fw_launch_geometry(const FwGeomParams& p, int lds_bytes, void* stream) {
  const bool w = p.ewt != nullptr;
  void* fn;
  if (p.bins)
    fn = w ? reinterpret_cast<void*>(&fw_geometry_bins_kernel<true>)
           : reinterpret_cast<void*>(&fw_geometry_bins_kernel<false>);
  else if (p.k <= 4)
    fn = w ? reinterpret_cast<void*>(&fw_geometry_kernel<4, true>)
           : reinterpret_cast<void*>(&fw_geometry_kernel<4, false>);
  else
    fn = w ? reinterpret_cast<void*>(&fw_geometry_kernel<8, true>)
           : reinterpret_cast<void*>(&fw_geometry_kernel<8, false>);
  if (lds_bytes > 64 * 1024) {
    const hipError_t e =
        hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return (int)e;
  }
  void* args[] = {const_cast<FwGeomParams*>(&p)};
  return (int)hipLaunchKernel(fn, dim3((unsigned)((p.n_chains + p.nw - 1) / p.nw)),
                              dim3(64 * p.nw), args, (size_t)lds_bytes, (hipStream_t)stream);
}

int fw_launch_geometry_hist(const FwGeomHistParams& h, void* stream) {
  void* args[] = {const_cast<FwGeomHistParams*>(&h)};
  return (int)hipLaunchKernel(reinterpret_cast<void*>(&fw_geometry_hist_kernel),
                              dim3((h.n_chains + 255) / 256), dim3(256), args, 0,
                              (hipStream_t)stream);
}
