// fw_census.hip — maps over the graph summed across the chains of the handle: how many chains
// label node v with district d, cut edge e, have v on a district boundary (the census entry
// points of include/flipwalk.h; parameter structs in fw_internal.h, the integer arithmetic in
// fw_census_plan.h).  Like the exchange, record, tally, geometry and overlap steps this runs
// between launches on the handle's stream, from the label records the run kernels leave in HBM;
// no run kernel knows of it.  The other measurements reduce over the nodes of one chain; this
// one fixes a piece of the graph and reduces over the chains.
//
// fw_census_kernel<LB, STAGED>: workgroup (tile, slice), nt = tile nodes rounded up to a wave
// multiple threads.  A tile is a node range with its CSR rows and its canonical edges (those
// whose lower endpoint lies in it: one contiguous id range); a slice is a range of the members
// of one group (FwCensusParams).  Once per workgroup the tile's CSR entries go to LDS, each as
// the bit offset of the neighbour's label in the tile's window of a record and a flag for w > v.
// Then, a batch of chains at a time, the window dwords of those records are staged in LDS
// (STAGED; coalesced dword loads, zero past the label words; two barriers a batch, and the
// loads of one workgroup overlap the counting of the others on the CU), or left where they are
// (windows too long for LDS: the lanes read the record in HBM).  Lane l owns node node0 + l: it
// cuts its label x, adds 1 to occ[x][l], walks its row, adds [X(w) != x] to the counter of each
// upper edge and keeps the boundary count in a register.  Every counter has one owner, so the
// LDS adds race with nothing; they are integer and their sum cannot depend on the order.  All
// counters are 32 bits wide and a slice has fewer than 2^31 chains: nothing narrower exists
// whose overflow would bound a slice.  At the end the workgroup stores its counts, transposed
// to [node][district], into its slice's row of part: plain vector stores, one owner each (tile
// 0 also stores the slice's chain count).  Every wave reaches every barrier: loop bounds are
// the same for the whole workgroup, and lanes without a node only skip the counting.
//
// fw_census_add_kernel: thread (j, g) adds part[g spg + s][j] over s, in ascending s, to the
// uint64 accumulator acc[g][j]: one owner each, no atomics anywhere.
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include "fw_internal.h"
#include "fw_census_plan.h"

namespace {

template <int LB, bool STAGED>
__global__ __launch_bounds__(FW_CEN_MAX_TILE) void fw_census_kernel(FwCensusParams p) {
  extern __shared__ __align__(16) uint32_t lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int sl = blockIdx.x / p.n_tiles, tile = blockIdx.x - sl * p.n_tiles;
  const int g = sl / p.spg, s = sl - g * p.spg;
  const int32_t* td = p.tiles + (size_t)tile * FW_CEN_TILE_INTS;
  const int node0 = td[0], n_nodes = td[1], ent0 = td[2], n_ent = td[3], edge0 = td[4],
            n_edge = td[5], wd0 = td[6], wdn = td[7];
  const bool do_occ = p.what & FW_CENSUS_NODES, do_cut = p.what & FW_CENSUS_EDGES,
             do_bnd = p.what & FW_CENSUS_BOUNDARY, walk = do_cut || do_bnd;
  uint32_t* occ = lds;  // [k][nt] when counted
  uint32_t* ecut = lds + p.off_ecut_lds;
  uint32_t* ent = lds + p.off_ent_lds;
  uint32_t* stage = lds + p.off_stage_lds;  // [batch][wd_max]
  if (do_occ)
    for (int i = tid; i < p.k * nt; i += nt) occ[i] = 0u;
  if (do_cut)
    for (int i = tid; i < n_edge; i += nt) ecut[i] = 0u;
  if (walk)
    for (int i = tid; i < n_ent; i += nt) ent[i] = p.ent[(size_t)ent0 + i];
  const bool own = tid < n_nodes;
  int r0 = 0, r1 = 0, eb = 0;
  uint32_t mybit = 0u;
  if (own) {
    const int v = node0 + tid;
    mybit = (uint32_t)((int64_t)v * LB - (int64_t)wd0 * 32);
    if (walk) {
      r0 = p.rowptr[v] - ent0;
      r1 = p.rowptr[v + 1] - ent0;
      eb = p.ebase[v] - edge0;
    }
  }
  int i0, i1;
  fw_cen_slice_range(s, p.slice_len, p.per_group, &i0, &i1);
  uint32_t bnd = 0u;
  __syncthreads();
  for (int b0 = i0; b0 < i1; b0 += p.batch) {
    const int nb = i1 - b0 < p.batch ? i1 - b0 : p.batch;
    if (STAGED) {
      if (b0 > i0) __syncthreads();  // the previous batch has been counted
      for (int j = 0; j < nb; ++j) {
        const int64_t c = p.chain_of ? p.chain_of[(size_t)(b0 + j) * p.n_groups + g] : b0 + j;
        const uint32_t* rec = reinterpret_cast<const uint32_t*>(p.labels + c * p.lab_stride);
        for (int w = tid; w < wdn; w += nt)
          stage[j * p.wd_max + w] = wd0 + w < p.lab_words ? rec[wd0 + w] : 0u;
      }
      __syncthreads();
    }
    if (own)
      for (int j = 0; j < nb; ++j) {
        const uint32_t* win;
        if (STAGED) {
          win = stage + j * p.wd_max;
        } else {
          const int64_t c = p.chain_of ? p.chain_of[(size_t)(b0 + j) * p.n_groups + g] : b0 + j;
          win = reinterpret_cast<const uint32_t*>(p.labels + c * p.lab_stride);
        }
        const uint32_t x = fw_cen_field<LB>(win, mybit);
        // labels the run kernels leave are below k; a stray value is not counted
        if (do_occ && x < (uint32_t)p.k) atomicAdd(&occ[x * nt + tid], 1u);
        uint32_t any = 0u;
        int e = eb;
        for (int r = r0; r < r1; ++r) {
          const uint32_t en = ent[r];
          const uint32_t d = fw_cen_field<LB>(win, en >> 1) != x ? 1u : 0u;
          any |= d;
          if (en & 1u) {
            if (do_cut && d) atomicAdd(&ecut[e], 1u);
            ++e;
          }
        }
        bnd += any;
      }
  }
  __syncthreads();  // the counters are complete
  uint32_t* out = p.part + (size_t)sl * (size_t)p.size;
  if (tile == 0 && tid == 0) out[0] = (uint32_t)(i1 - i0);
  if (do_occ) {
    uint32_t* o = out + p.off_occ + (size_t)node0 * p.k;
    for (int i = tid; i < n_nodes * p.k; i += nt) {
      const int v = i / p.k, d = i - v * p.k;
      o[i] = occ[d * nt + v];
    }
  }
  if (do_cut) {
    uint32_t* o = out + p.off_ecut + edge0;
    for (int i = tid; i < n_edge; i += nt) o[i] = ecut[i];
  }
  if (do_bnd && own) out[p.off_bnd + node0 + tid] = bnd;
}

__global__ __launch_bounds__(256) void fw_census_add_kernel(FwCensusAddParams a) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.size) return;
  const int g = blockIdx.y;
  const uint32_t* src = a.part + (size_t)g * a.spg * (size_t)a.size + j;
  uint64_t sum = 0;
  for (int s = 0; s < a.spg; ++s) sum += src[(size_t)s * (size_t)a.size];
  a.acc[(size_t)g * (size_t)a.size + j] += sum;
}

template <int LB>
void* census_fn(bool staged) {
  return staged ? reinterpret_cast<void*>(&fw_census_kernel<LB, true>)
                : reinterpret_cast<void*>(&fw_census_kernel<LB, false>);
}

}  // namespace

// FLIPWALK_CENSUS_TILE (nodes per tile), FLIPWALK_CENSUS_SLICE (chains per slice) and
// FLIPWALK_CENSUS_STAGE (0: never stage windows in LDS) override the plan (tests force several
// tiles and slices, ragged last ones and both ways to the labels on small shapes)
int fw_census_env(const char* name) {
  const char* e = getenv(name);
  return e && e[0] ? atoi(e) : -1;
}

int fw_launch_census(const FwCensusParams& p, void* stream) {
  void* fn;
  switch (p.lb) {
    case 2: fn = census_fn<2>(p.staged); break;
    case 3: fn = census_fn<3>(p.staged); break;
    case 4: fn = census_fn<4>(p.staged); break;
    case 5: fn = census_fn<5>(p.staged); break;
    case 8: fn = census_fn<8>(p.staged); break;
    default: return (int)hipErrorInvalidValue;
  }
  void* args[] = {const_cast<FwCensusParams*>(&p)};
  const unsigned blocks = (unsigned)p.n_tiles * (unsigned)p.n_groups * (unsigned)p.spg;
  return (int)hipLaunchKernel(fn, dim3(blocks), dim3(p.nt), args, (size_t)p.lds_bytes,
                              (hipStream_t)stream);
}

int fw_launch_census_add(const FwCensusAddParams& a, void* stream) {
  void* args[] = {const_cast<FwCensusAddParams*>(&a)};
  return (int)hipLaunchKernel(reinterpret_cast<void*>(&fw_census_add_kernel),
                              dim3((unsigned)((a.size + 255) / 256), (unsigned)a.n_groups),
                              dim3(256), args, 0, (hipStream_t)stream);
}
