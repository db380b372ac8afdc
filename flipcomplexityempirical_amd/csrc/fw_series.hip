// fw_series.hip — thinned observable series and their autocovariances (the series entry
// points of include/flipwalk.h; parameter structs in fw_internal.h).  None of this runs inside
// the flip kernels: a sample is taken between launches from the stats records, and the
// reductions run when the host asks for them.
//
// Layout: every series buffer is sample-major, int32 [samples][n_series].  All four kernels put
// the series index on the lane, so a wave reads or writes 64 adjacent series of one sample:
// one 256-B row segment per instruction.
#include <hip/hip_runtime.h>

#include "fw_internal.h"

// ---------------------------------------------------------------- recording
// One thread per chain.  The stats records are an array of structs (the run kernels' layout),
// so the two reads are strided; the three writes are coalesced along the chain index.
__global__ __launch_bounds__(256) void fw_record_kernel(FwRecordParams r) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= r.n_chains) return;
  const size_t at = (size_t)r.sample * (size_t)r.n_chains + (size_t)c;
  r.cut[at] = r.stats[c].cut;
  r.bnodes[at] = r.stats[c].bnodes;
  if (r.rung_out) r.rung_out[at] = r.rung ? r.rung[c] : -1;
}

int fw_launch_record(const FwRecordParams& r, void* stream) {
  void* args[] = {const_cast<FwRecordParams*>(&r)};
  return (int)hipLaunchKernel(reinterpret_cast<void*>(&fw_record_kernel),
                              dim3((r.n_chains + 255) / 256), dim3(256), args, 0,
                              (hipStream_t)stream);
}

// ---------------------------------------------------------------- by-rung view
// A permutation per sample (every (set, rung) holds one chain): each thread writes its own
// slot, no atomics.  Rung rows are validated on the host or come from the exchange kernel; a
// value outside the ladder is skipped all the same, so no write can leave the row.
__global__ __launch_bounds__(256) void fw_regroup_kernel(FwRegroupParams r) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= r.n_chains) return;
  const int64_t set0 = (int64_t)r.set_of[c] * r.n_rungs;
  for (int64_t t = blockIdx.y; t < r.n; t += gridDim.y) {
    const size_t row = (size_t)t * (size_t)r.n_chains;
    const int rg = r.rung[row + c];
    if (rg < 0 || rg >= r.n_rungs || set0 < 0 || set0 + rg >= r.n_chains) continue;
    r.out[row + (size_t)(set0 + rg)] = r.x[row + c];
  }
}

int fw_launch_regroup(const FwRegroupParams& r, void* stream) {
  void* args[] = {const_cast<FwRegroupParams*>(&r)};
  // samples beyond 1,024 are walked by the same workgroups
  const unsigned rows = (unsigned)(r.n < 1024 ? r.n : 1024);
  return (int)hipLaunchKernel(reinterpret_cast<void*>(&fw_regroup_kernel),
                              dim3((r.n_chains + 255) / 256, rows), dim3(256), args, 0,
                              (hipStream_t)stream);
}

// ---------------------------------------------------------------- exact lagged sums
// P[l] = sum_{s=l}^{n-1} x[s-l] * x[s],  A[l] = sum_{u=0}^{n-1-l} x[u],  B[l] = sum_{s=l}^{n-1} x[s]
// as 64-bit integers (exact: the host checked n * xmax^2 < 2^63; values are in [0, 2^31), so a
// product is one 32 x 32 -> 64 multiply-add).
//
// A workgroup is FW_ACF_WAVES waves on the same 64 series (lane = series); wave w of
// workgroup (x, y) owns the lags [L0, L0 + 32), L0 = 32 * (4 * y + w), with its 32 products'
// accumulators in registers (every index into them is a compile-time constant after
// unrolling: no scratch).  It walks s = L0 .. n-1 once, loading row s and row s - L0
// (both coalesced), and keeps the last 32 values x[s-L0-31 .. s-L0] of its lane's series in a
// ring in LDS, [32][64] with the lane as the fast index: a read or write is 64 consecutive
// dwords, free of bank conflicts.  The ring starts as zeros, which stand for x[u], u < 0, so
// the inner loop has no conditions.  A lane only ever reads the ring column it wrote, and
// waves share nothing: no barrier, no atomics, no dependence on thread order.
// A and B need no accumulators of their own: with H = sum of the values pushed into the ring
// and T = sum of the rows s >= L0,  A[L0+i] = H - (the newest i ring entries),
// B[L0+i] = T - (x[L0] + .. + x[L0+i-1]).
__global__ __launch_bounds__(64 * FW_ACF_WAVES) void fw_acf_kernel(FwAcfParams a) {
  __shared__ uint32_t ring_all[FW_ACF_WAVES][FW_ACF_CHUNK][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L0 = ((int)blockIdx.y * FW_ACF_WAVES + wave) * FW_ACF_CHUNK;
  if (L0 > a.max_lag) return;  // the same in every lane of the wave
  const int j = (int)blockIdx.x * 64 + lane;
  const bool live = j < a.n_series;
  // lanes past the last series re-read it and store nothing
  const uint32_t* col = reinterpret_cast<const uint32_t*>(a.x) + (live ? j : a.n_series - 1);
  const int64_t N = a.n_series, n = a.n;
  uint32_t(*ring)[64] = ring_all[wave];
#pragma unroll
  for (int i = 0; i < FW_ACF_CHUNK; ++i) ring[i][lane] = 0u;
  uint64_t acc[FW_ACF_CHUNK];
#pragma unroll
  for (int i = 0; i < FW_ACF_CHUNK; ++i) acc[i] = 0ull;
  uint64_t tot = 0ull, pushed = 0ull;
  for (int64_t s = L0; s < n; s += 4) {
    // four rows' loads in flight before the first is used
    uint32_t xa[4], xh[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t sq = s + q < n ? s + q : n - 1;
      xa[q] = col[sq * N];
      xh[q] = col[(sq - L0) * N];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (s + q < n) {
        const int d = (int)((s + q - L0) & (FW_ACF_CHUNK - 1));
        ring[d][lane] = xh[q];
        tot += xa[q];
        pushed += xh[q];
#pragma unroll
        for (int i = 0; i < FW_ACF_CHUNK; ++i)
          acc[i] += (uint64_t)ring[(d - i) & (FW_ACF_CHUNK - 1)][lane] * (uint64_t)xa[q];
      }
    }
  }
  const int dl = (int)((n - 1 - L0) & (FW_ACF_CHUNK - 1));  // ring slot of x[n-1-L0]
  const size_t L1 = (size_t)a.max_lag + 1;
  uint64_t ra = pushed, rb = tot;
#pragma unroll
  for (int i = 0; i < FW_ACF_CHUNK; ++i) {
    const int l = L0 + i;
    if (l > a.max_lag) break;  // l <= max_lag < n: row l exists
    if (live) {
      a.sums[((size_t)l) * (size_t)N + (size_t)j] = (int64_t)acc[i];
      a.sums[(L1 + (size_t)l) * (size_t)N + (size_t)j] = (int64_t)ra;
      a.sums[(2 * L1 + (size_t)l) * (size_t)N + (size_t)j] = (int64_t)rb;
    }
    ra -= ring[(dl - i) & (FW_ACF_CHUNK - 1)][lane];
    rb -= col[(int64_t)l * N];
  }
}

int fw_launch_acf(const FwAcfParams& a, void* stream) {
  const int chunks = a.max_lag / FW_ACF_CHUNK + 1;
  void* args[] = {const_cast<FwAcfParams*>(&a)};
  return (int)hipLaunchKernel(
      reinterpret_cast<void*>(&fw_acf_kernel),
      dim3((a.n_series + 63) / 64, (chunks + FW_ACF_WAVES - 1) / FW_ACF_WAVES),
      dim3(64 * FW_ACF_WAVES), args, 0, (hipStream_t)stream);
}

// ---------------------------------------------------------------- pooled autocovariances
// Workgroup (q, g): output q of group g.  Thread p sums, from +0.0 and in ascending position,
// the terms of the members at positions p, p + 256, ...; then the halving tree
// a[i] += a[i + 128], 64, .. 1.  Plain IEEE double operations in the order the header states
// (contraction off), so a host restatement agrees bit for bit.
__global__ __launch_bounds__(FW_POOL_WIDTH) void fw_pool_kernel(FwPoolParams p) {
#pragma clang fp contract(off)
  __shared__ double part[FW_POOL_WIDTH];
  const int q = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
  const int L1 = p.max_lag + 1;
  const size_t N = (size_t)p.n_series;
  const int l = q < L1 ? q : 0;
  const double dn = (double)p.n;
  double s = 0.0;
  for (int pos = t; pos < p.members; pos += FW_POOL_WIDTH) {
    const size_t j = (size_t)g + (size_t)pos * (size_t)p.stride;
    const double m = (double)p.sums[(size_t)L1 * N + j] / dn;  // A[j][0] = the series' sum
    double term;
    if (q < L1) {
      const int64_t P = p.sums[(size_t)l * N + j];
      const int64_t A = p.sums[((size_t)L1 + l) * N + j];
      const int64_t B = p.sums[(2 * (size_t)L1 + l) * N + j];
      term = (((double)P - m * (double)(A + B)) + (double)(p.n - l) * m * m) / dn;
    } else if (q == L1) {
      term = m;
    } else {
      term = m * m;
    }
    s = s + term;
  }
  part[t] = s;
  __syncthreads();
  for (int h = FW_POOL_WIDTH / 2; h >= 1; h >>= 1) {
    if (t < h) part[t] = part[t] + part[t + h];
    __syncthreads();
  }
  if (t == 0) p.out[(size_t)g * (size_t)(L1 + 2) + (size_t)q] = part[0];
}

int fw_launch_pool(const FwPoolParams& p, int n_groups, void* stream) {
  void* args[] = {const_cast<FwPoolParams*>(&p)};
  return (int)hipLaunchKernel(reinterpret_cast<void*>(&fw_pool_kernel),
                              dim3(p.max_lag + 3, n_groups), dim3(FW_POOL_WIDTH), args, 0,
                              (hipStream_t)stream);
}
