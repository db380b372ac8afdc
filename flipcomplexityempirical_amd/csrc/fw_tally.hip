// fw_tally.hip — per-district sums of node columns over every chain's current plan, and the
// seat counts of elections between two columns (the tally entry points of include/flipwalk.h;
// parameter structs in fw_internal.h).  Like the exchange and record steps this runs between
// launches on the handle's stream, from the label records the run kernels leave in HBM; no run
// kernel knows of it.
//
// fw_tally_kernel: a workgroup is NW waves, one chain per wave.  The traffic that matters is
// the columns (every chain reads all of them), not the labels (read once), so the workgroup
// walks the nodes in tiles of FW_TALLY_TILE and stages each tile of the columns in LDS once
// for all its waves; each wave stages its own chain's label words of the tile beside it with
// coalesced dword loads.  Lane l then takes node tile + 64 s + l of step s: its column read is
// one of 64 consecutive LDS slots and its label is cut from two adjacent LDS dwords, whatever
// the width (3- and 5-bit fields straddle dwords).  Every loop bound is uniform over the
// workgroup, so every wave reaches every barrier; a wave without a chain computes nothing.
//
//  - k <= 8 (template KB = 4 or 8): columns are taken two at a time (the device copy is stored
//    as pairs, so a lane's two values are one 8-byte LDS read); 2 KB accumulators in registers,
//    a compare and two select-adds per district, folded over the wave at the end of the pair.
//  - k > 8: one column at a time into per-wave LDS bins [k][64], a private copy per lane (lane
//    l only ever touches bank l mod 32: no conflicts, no atomics); at the end of the column
//    lane d adds up row d, walking it from a lane-dependent start so that the reads spread
//    over the banks.
// Sums are unsigned 32-bit: the host checked that every column's total is below 2^31.  Each
// T[c][j][d] is written once, by one lane, as int64.
//
// fw_seats_kernel: one thread per chain compares the two columns of every election district
// by district, writes {wins, ties} and counts the chain into seat_hist[group][election][wins]
// with integer atomics (an integer sum does not depend on the order): into a workgroup's LDS
// copy first when the histogram is small, so that a launch makes a few global atomics per
// workgroup instead of one per chain.
#include <hip/hip_runtime.h>

#include "fw_internal.h"

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
  return v;
}

// Label words of nodes [tile, tile + FW_TALLY_TILE) of one chain -> lw[0 .. lws): lws =
// FW_TALLY_TILE * lb / 32 + 1 (the extra word serves a field that straddles the last
// boundary).  Words past the record read as zero; the record is a multiple of 16 bytes.
__device__ __forceinline__ void stage_labels(const FwTallyParams& t, const uint8_t* rec,
                                             int tile, int lws, uint32_t* lw, int lane) {
  const int w0 = tile / 32 * t.lb;  // tile is a multiple of 32
  const int rec_words = (int)(t.lab_stride >> 2);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(rec);
  for (int i = lane; i < lws; i += 64) lw[i] = w0 + i < rec_words ? src[w0 + i] : 0u;
}

// Label of the node at offset o of the tile from its staged words.
__device__ __forceinline__ uint32_t tile_label(const uint32_t* lw, int lb, int o) {
  const int bit = o * lb;
  // v_alignbit_b32: the low dword of {hi, lo} >> (bit & 31)
  return __builtin_amdgcn_alignbit(lw[(bit >> 5) + 1], lw[bit >> 5], (uint32_t)(bit & 31)) &
         ((1u << lb) - 1u);
}

template <int KB>
__global__ __launch_bounds__(64 * FW_TALLY_NW_REG) void fw_tally_kernel(FwTallyParams t) {
  extern __shared__ __align__(16) uint32_t lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int lws = FW_TALLY_TILE / 32 * t.lb + 1;
  uint2* ctile = reinterpret_cast<uint2*>(lds);                   // [FW_TALLY_TILE] column pair
  uint32_t* lw = lds + 2 * FW_TALLY_TILE + wave * ((lws + 3) & ~3);  // this wave's label words
  const int64_t c = (int64_t)blockIdx.x * nw + wave;
  const bool live = c < t.n_chains;
  const uint8_t* rec = t.labels + (live ? c : 0) * t.lab_stride;
  const int n = t.n;
  for (int j = 0; j < t.n_cols; j += 2) {
    const uint2* cp = reinterpret_cast<const uint2*>(t.cols) + (size_t)(j >> 1) * (size_t)n;
    uint32_t a0[KB], a1[KB];
#pragma unroll
    for (int d = 0; d < KB; ++d) a0[d] = a1[d] = 0u;
    for (int tile = 0; tile < n; tile += FW_TALLY_TILE) {
      __syncthreads();  // the previous tile has been read
      for (int i = threadIdx.x; i < FW_TALLY_TILE; i += blockDim.x)
        ctile[i] = tile + i < n ? cp[tile + i] : make_uint2(0u, 0u);
      if (live) stage_labels(t, rec, tile, lws, lw, lane);
      __syncthreads();
      if (live) {
        const int end = n - tile < FW_TALLY_TILE ? n - tile : FW_TALLY_TILE;
        for (int o = lane; o < end; o += 64) {
          const uint32_t lab = tile_label(lw, t.lb, o);
          const uint2 v = ctile[o];
#pragma unroll
          for (int d = 0; d < KB; ++d) {
            const bool m = lab == (uint32_t)d;
            a0[d] += m ? v.x : 0u;
            a1[d] += m ? v.y : 0u;
          }
        }
      }
    }
    // every index into a0 / a1 is a constant after unrolling: no scratch
#pragma unroll
    for (int d = 0; d < KB; ++d) {
      const uint32_t s0 = wave_sum(a0[d]), s1 = wave_sum(a1[d]);
      if (live && lane == d && d < t.k) {
        int64_t* out = t.sums + ((size_t)c * t.n_cols + j) * t.k + d;
        out[0] = (int64_t)s0;
        if (j + 1 < t.n_cols) out[t.k] = (int64_t)s1;
      }
    }
  }
}

__global__ __launch_bounds__(64 * FW_TALLY_NW_BIN) void fw_tally_bins_kernel(FwTallyParams t) {
  extern __shared__ __align__(16) uint32_t lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int lws = FW_TALLY_TILE / 32 * t.lb + 1;
  uint32_t* ctile = lds;                                          // [FW_TALLY_TILE] one column
  uint32_t* lw = lds + FW_TALLY_TILE + wave * ((lws + 3) & ~3);
  uint32_t* bins = lds + FW_TALLY_TILE + nw * ((lws + 3) & ~3) + wave * t.k * 64;  // [k][64]
  const int64_t c = (int64_t)blockIdx.x * nw + wave;
  const bool live = c < t.n_chains;
  const uint8_t* rec = t.labels + (live ? c : 0) * t.lab_stride;
  const int n = t.n, k = t.k;
  for (int d = 0; d < k; ++d) bins[d * 64 + lane] = 0u;
  for (int j = 0; j < t.n_cols; ++j) {
    // column j is component j & 1 of pair j >> 1
    const uint32_t* cp = t.cols + (size_t)(j >> 1) * (size_t)n * 2 + (j & 1);
    for (int tile = 0; tile < n; tile += FW_TALLY_TILE) {
      __syncthreads();
      for (int i = threadIdx.x; i < FW_TALLY_TILE; i += blockDim.x)
        ctile[i] = tile + i < n ? cp[2 * (size_t)(tile + i)] : 0u;
      if (live) stage_labels(t, rec, tile, lws, lw, lane);
      __syncthreads();
      if (live) {
        const int end = n - tile < FW_TALLY_TILE ? n - tile : FW_TALLY_TILE;
        for (int o = lane; o < end; o += 64) {
          const uint32_t lab = tile_label(lw, t.lb, o);
          if (lab < (uint32_t)k) bins[lab * 64 + lane] += ctile[o];  // the lane's own copy
        }
      }
    }
    __syncthreads();  // the wave's bins are complete
    if (live && lane < k) {
      uint32_t s = 0u;
      for (int i = 0; i < 64; ++i) s += bins[lane * 64 + ((i + lane) & 63)];
      t.sums[((size_t)c * t.n_cols + j) * k + lane] = (int64_t)s;
    }
    __syncthreads();  // row sums taken before the bins restart
    for (int d = 0; d < k; ++d) bins[d * 64 + lane] = 0u;
  }
}

__global__ __launch_bounds__(256) void fw_seats_kernel(FwSeatsParams s) {
  __shared__ uint32_t lh[FW_SEATS_LDS_BINS];
  const int bins = s.n_groups * s.n_el * (s.k + 1);
  const bool local = bins <= FW_SEATS_LDS_BINS;  // uniform
  if (local) {
    for (int i = threadIdx.x; i < bins; i += 256) lh[i] = 0u;
    __syncthreads();
  }
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < s.n_chains) {
    int g = s.rung ? s.rung[c] : 0;
    if (g < 0 || g >= s.n_groups) g = 0;  // the exchange kernel keeps rungs inside the ladder
    const int64_t* T = s.sums + (size_t)c * s.n_cols * s.k;
    for (int e = 0; e < s.n_el; ++e) {
      const int64_t* A = T + s.ab[e][0] * s.k;
      const int64_t* B = T + s.ab[e][1] * s.k;
      int wins = 0, ties = 0;
      for (int d = 0; d < s.k; ++d) {
        wins += A[d] > B[d] ? 1 : 0;
        ties += A[d] == B[d] ? 1 : 0;
      }
      s.seats[((size_t)c * s.n_el + e) * 2] = wins;
      s.seats[((size_t)c * s.n_el + e) * 2 + 1] = ties;
      const int bin = (g * s.n_el + e) * (s.k + 1) + wins;
      if (local)
        atomicAdd(&lh[bin], 1u);
      else
        atomicAdd(&s.hist[bin], 1ull);
    }
  }
  if (local) {
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256)
      if (lh[i]) atomicAdd(&s.hist[i], (unsigned long long)lh[i]);
  }
}

int tally_lws(int lb) { return (FW_TALLY_TILE / 32 * lb + 1 + 3) & ~3; }

}  // namespace

// Waves per workgroup and dynamic LDS bytes of the tally launch for (k, lb).
void fw_tally_plan(int k, int lb, int* nw, int* lds_bytes) {
  if (k <= 8) {
    *nw = FW_TALLY_NW_REG;
    *lds_bytes = 4 * (2 * FW_TALLY_TILE + *nw * tally_lws(lb));
  } else {
    *nw = k <= 32 ? FW_TALLY_NW_BIN : FW_TALLY_NW_BIN / 2;
    *lds_bytes = 4 * (FW_TALLY_TILE + *nw * tally_lws(lb) + *nw * k * 64);
  }
}

int fw_launch_tally(const FwTallyParams& t, void* stream) {
  int nw = 0, lds = 0;
  fw_tally_plan(t.k, t.lb, &nw, &lds);
  void* fn = t.k <= 4   ? reinterpret_cast<void*>(&fw_tally_kernel<4>)
             : t.k <= 8 ? reinterpret_cast<void*>(&fw_tally_kernel<8>)
                        : reinterpret_cast<void*>(&fw_tally_bins_kernel);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
  }
  void* args[] = {const_cast<FwTallyParams*>(&t)};
  return (int)hipLaunchKernel(fn, dim3((unsigned)((t.n_chains + nw - 1) / nw)), dim3(64 * nw),
                              args, (size_t)lds, (hipStream_t)stream);
}

int fw_launch_seats(const FwSeatsParams& s, void* stream) {
  void* args[] = {const_cast<FwSeatsParams*>(&s)};
  return (int)hipLaunchKernel(reinterpret_cast<void*>(&fw_seats_kernel),
                              dim3((s.n_chains + 255) / 256), dim3(256), args, 0,
                              (hipStream_t)stream);
}
