// fw_api.hip — host implementation of the C-ABI in include/flipwalk.h.
//
// Owns device memory behind fw_graph / fw_chains handles, validates inputs the
// way GerryChain does (initial-state check -> FW_ESTATE, like MarkovChain's
// ValueError), packs labels into the kernels' LB-bit layout and launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fw_internal.h"
#include "fw_census_plan.h"
#include "fw_coassign_plan.h"
#include "fw_math.h"
#include "fw_pairdist_plan.h"
#include "fw_resample_limbs.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(FW_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));             \
  } while (0)

int round16(int64_t x) { return (int)((x + 15) / 16 * 16); }

// Same rule as flipcomplexityempirical_amd.graph.detect_grid.
int detect_grid(const std::vector<int32_t>& rp, const std::vector<int32_t>& col, int n) {
  if (n < 4) return 0;
  if (rp[1] - rp[0] != 2 || col[0] != 1) return 0;
  const int w = col[1];
  if (w < 2 || n % w || n / w < 2) return 0;
  const int h = n / w;
  int e = 0;
  for (int i = 0; i < h; ++i)
    for (int j = 0; j < w; ++j) {
      const int x = i * w + j;
      int nb[4], d = 0;
      if (i > 0) nb[d++] = x - w;
      if (j > 0) nb[d++] = x - 1;
      if (j < w - 1) nb[d++] = x + 1;
      if (i < h - 1) nb[d++] = x + w;
      if (rp[x] != e || rp[x + 1] - rp[x] != d) return 0;
      for (int t = 0; t < d; ++t)
        if (col[e + t] != nb[t]) return 0;
      e += d;
    }
  return w;
}

// Entries of a contiguity search's visit list held in LDS before it spills to HBM.
// FLIPWALK_LIST_CAP overrides it (tests force the spill path with a tiny cap).
int list_cap(int dflt) {
  const char* e = getenv("FLIPWALK_LIST_CAP");
  if (!e || !e[0]) return dflt;
  const int v = atoi(e);
  return v >= 1 ? v : dflt;
}

// x / gw == (x * m) >> s for every x < 2^15 with m < 2^17 (so the grid kernel divides with
// one full-rate 24-bit multiply), verified exhaustively; m = 0 if no shift works
void grid_div24(int gw, uint32_t* m_out, uint32_t* s_out) {
  *m_out = 0;
  *s_out = 0;
  for (uint32_t sh = 0; gw > 0 && sh < 32; ++sh) {
    const uint64_t m = (((uint64_t)1 << sh) + (uint64_t)gw - 1) / (uint64_t)gw;
    if (m >= ((uint64_t)1 << 17)) break;
    bool ok = m > 0;
    for (uint64_t x = 0; x < ((uint64_t)1 << 15) && ok; ++x) ok = ((x * m) >> sh) == x / (uint64_t)gw;
    if (ok) {
      *m_out = (uint32_t)m;
      *s_out = sh;
      return;
    }
  }
}

}  // namespace

struct fw_graph {
  int device = 0;
  int32_t n = 0, nnz = 0, maxdeg = 0, gw = 0, gh = 0;
  uint32_t gm24 = 0, gs24 = 0;  // grid_div24
  std::vector<int32_t> rowptr, col;
  std::vector<int64_t> pop;  // empty: unit populations
  int32_t* d_rowptr = nullptr;
  int32_t* d_col = nullptr;
  int64_t* d_pop = nullptr;
  int32_t* d_eid = nullptr;  // [nnz] canonical edge id per CSR entry
  int32_t* d_eu = nullptr;   // [E] canonical edge endpoints (u < w)
  int32_t* d_ew = nullptr;
  uint64_t* d_nbadj = nullptr;  // [nnz] (general graphs): adjacency among v's neighbours
  int32_t* d_ell = nullptr;     // [n][16] (general graphs, max degree <= 16): padded rows
  int32_t* d_dbound = nullptr;  // with d_ell: FwGraphDev::dbound
  double* d_invb = nullptr;     // [n+1] 1.0 / max(b, 1) for the Σ1/|B| observable
  int64_t popof(int x) const { return pop.empty() ? 1 : pop[x]; }
  FwGraphDev dev() const {
    FwGraphDev g;
    g.rowptr = d_rowptr;
    g.col = d_col;
    g.eid = d_eid;
    g.nbadj = d_nbadj;
    g.ell = d_ell;
    g.dbound = d_dbound;
    g.pop = d_pop;
    g.invb = d_invb;
    g.n = n;
    g.nedges = nnz / 2;
    g.maxdeg = maxdeg;
    g.gw = gw;
    g.gh = gh;
    // exact x / gw for x < 2^21 (the grid path is only taken for n < 2^21)
    g.gmagic = gw ? (((uint64_t)1 << 42) + (uint64_t)gw - 1) / (uint64_t)gw : 0;
    g.gm32 = gw ? (uint32_t)((((uint64_t)1 << 32) + (uint64_t)gw - 1) / (uint64_t)gw) : 0;
    g.gm24 = gm24;
    g.gs24 = gs24;
    return g;
  }
};

struct fw_chains {
  fw_graph* g = nullptr;
  int32_t n_chains = 0, k = 0, mode = 0, lb = 4, grid = 1, D = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  FwRunParams p{};
  uint8_t* d_labels = nullptr;
  fw_chain_stats* d_stats = nullptr;
  int64_t* d_pops = nullptr;
  double* d_thr = nullptr;
  uint64_t* d_thr53 = nullptr;
  unsigned long long* d_hist_cut = nullptr;
  unsigned long long* d_hist_b = nullptr;
  uint32_t* d_spill = nullptr;
  int32_t* d_next = nullptr;
  uint32_t* d_gscr = nullptr;  // chain kernel, 5-bit labels: search marks
  int32_t* d_segdone = nullptr;  // finished slices per work unit (launch_slices)
  uint64_t max_yields = 0;  // upper bound on any chain's yield count (maps need < 2^32)
  bool gcache_ok = false;   // the label records' group sums and the stats' cut / bnodes /
                            // npairs match the labels (FwRunParams::gcache_ok)
  bool ran = false;
  // spatial observables (fw_chains_enable_maps)
  int64_t* d_acc = nullptr;
  uint32_t* d_nf = nullptr;
  uint32_t* d_lf = nullptr;
  int64_t* d_ps = nullptr;
  int32_t* d_pend = nullptr;
  int64_t* d_labval = nullptr;
  // FW_ACCEPT_BOUNDARY
  uint8_t* d_flags = nullptr;
  int32_t* d_bcnt = nullptr;
  // fw_chains_set_schedule
  double* d_sched = nullptr;
  uint64_t* d_sched53 = nullptr;
  // fw_chains_enable_ring
  int32_t ring_n = 0;
  std::vector<int32_t> ring_u, ring_w;
  double* d_wsamp = nullptr;  // fw_chains_enable_waits: [n_chains][2] {sum, current draw}
  double* d_wlp = nullptr;    // [n+1] log1p(-p_b)
  int32_t* d_ring = nullptr;              // [2][ring_n] endpoints
  uint8_t* d_ring_node = nullptr;         // [n]
  unsigned long long* d_hist_ring = nullptr;  // [ring_n^2 + 1]
  // fw_chains_set_ladder (n_rungs == 0: no ladder); FwExchangeParams names the arrays
  int32_t n_rungs = 0;
  double* d_lad_thr = nullptr;
  uint64_t* d_lad_thr53 = nullptr;
  double* d_logb = nullptr;
  int32_t* d_rung = nullptr;
  int32_t* d_chain_of = nullptr;
  int64_t* d_gmin = nullptr;
  FwRungSnap* d_snap = nullptr;
  fw_rung_stats* d_rstats = nullptr;
  std::vector<int32_t> lad_set;  // set_of_chain of the current ladder
  int64_t lad_epoch = 0;         // 0: no ladder; bumped by every fw_chains_set_ladder
  // fw_chains_enable_series (ser_cap == 0: off): sample-major int32 [ser_cap][n_chains]
  int64_t ser_cap = 0, ser_n = 0;
  int32_t* d_ser_cut = nullptr;
  int32_t* d_ser_bn = nullptr;
  int32_t* d_ser_rung = nullptr;       // allocated on the first rung row (all -1 before it)
  std::vector<int64_t> ser_epoch;      // [ser_cap] ladder epoch each sample's rung row belongs to
  // fw_chains_set_columns (tal_cols == 0: none); FwTallyParams / FwSeatsParams name the arrays
  int32_t tal_cols = 0, tal_el = 0;
  int32_t tal_ab[FW_TALLY_MAX_EL][2] = {};
  int64_t n_tallied = 0;
  bool tal_have_sums = false, tal_have_seats = false;  // a tally ran since the columns / elections
  uint32_t* d_tal_cols = nullptr;
  int64_t* d_tal_sums = nullptr;
  int32_t* d_tal_seats = nullptr;            // [n_chains][FW_TALLY_MAX_EL][2] (n_el rows in use)
  unsigned long long* d_tal_hist = nullptr;  // room for 64 groups x 4 elections x (k + 1) bins
  // fw_chains_set_geometry (geo_set false: none); FwGeomParams / FwGeomHistParams name the arrays
  bool geo_set = false, geo_have = false;  // geo_have: measured since the last set_geometry
  int64_t n_measured = 0;
  FwGeomPlan geo_plan{};
  uint32_t* d_geo_w = nullptr;     // [n_edges] or null (unit weights)
  uint32_t* d_geo_area = nullptr;  // [n] or null (unit areas)
  uint32_t* d_geo_ext = nullptr;   // [n] or null (no exterior perimeter)
  int64_t* d_geo_out = nullptr;    // [n_chains][k][5]
  unsigned long long* d_geo_hist = nullptr;  // [n_groups][n_edges + 1], the group count in force
  // fw_chains_set_reference / fw_chains_set_partners; FwOverlapParams names the arrays
  int32_t ovl_ref = 0;        // 0: no reference, 1: one shared row, 2: a row per chain
  bool ovl_partners = false;
  int32_t ovl_last = -1;      // what MATRIX and DIST hold: FW_OVERLAP_REFERENCE / _PARTNER, -1: nothing
  int64_t ovl_measured = 0;
  uint32_t* d_ovl_ref = nullptr;      // [n_chains][ovl_words4]
  int32_t* d_ovl_partner = nullptr;   // [n_chains]
  int64_t* d_ovl_O = nullptr;         // [n_chains][k][k]
  int32_t* d_ovl_dist = nullptr;      // [n_chains]
  unsigned long long* d_ovl_hist = nullptr;  // [n_groups][n + 1], the group count in force
  // fw_chains_clone_async / fw_chains_resample_async; FwCloneParams / FwResampleParams name the
  // arrays (allocated by the first call; d_rsm_family == nullptr: every family is its own chain)
  int64_t n_resampled = 0, rsm_round = -1, rsm_host_clones = 0;
  bool rsm_have_src = false, rsm_have_w = false;  // a map / a resample's weights exist
  int32_t* d_rsm_src = nullptr;
  int32_t* d_rsm_family = nullptr;
  uint32_t* d_rsm_q = nullptr;     // [n_edges + 1]
  uint32_t* d_rsm_w = nullptr;
  uint64_t* d_rsm_cum = nullptr;
  uint64_t* d_rsm_pts = nullptr;
  int32_t* d_rsm_lower = nullptr;
  int32_t* d_rsm_extra = nullptr;
  int64_t* d_rsm_info = nullptr;   // [8]
  // uploads without a host wait: two pinned staging slots, each with the event of its last copy
  void* rsm_stage[2] = {nullptr, nullptr};
  hipEvent_t rsm_ev[2] = {nullptr, nullptr};
  int rsm_slot = 0;
  std::vector<uint32_t> rsm_q;     // the table d_rsm_q holds (an equal table is not uploaded again)
  // fw_chains_enable_census (cen.what == 0: off): the plan and, in FwCensusParams' names, the
  // arrays derived from the graph; d_cen_acc uint64 [n_groups][cen.size], the group count in force
  FwCensusParams cen{};
  int64_t cen_measured = 0;
  void* d_cen_graph[3] = {nullptr, nullptr, nullptr};  // tiles, ent, ebase
  uint32_t* d_cen_part = nullptr;
  uint64_t* d_cen_acc = nullptr;
  // fw_chains_pairdist_async (pwd_have false: nothing measured yet); FwPairdistParams names the
  // arrays.  Buffers grow with the lists and are never shrunk; d_pwd_hist uint64 [n + 1]
  bool pwd_have = false, pwd_sym = false;
  int32_t pwd_ma = 0, pwd_mb = 0, pwd_tile = 0, pwd_chunk = 0;
  int64_t pwd_measured = 0;
  int32_t* d_pwd_list[2] = {nullptr, nullptr};
  size_t pwd_list_cap[2] = {0, 0};   // elements
  int32_t* d_pwd_D = nullptr;
  size_t pwd_D_cap = 0;              // elements
  int64_t* d_pwd_rowsum = nullptr;
  int32_t* d_pwd_near = nullptr;
  size_t pwd_row_cap = 0;            // rows
  unsigned long long* d_pwd_hist = nullptr;
  // the lists' uploads: two pinned slots, each with the event of its last copy (as rsm_stage)
  void* pwd_stage[2] = {nullptr, nullptr};
  size_t pwd_stage_cap[2] = {0, 0};  // bytes
  hipEvent_t pwd_ev[2] = {nullptr, nullptr};
  int pwd_slot = 0;
  // fw_chains_enable_coassign (coa.m == 0: off): the plan and, in FwCoassignParams' names, the
  // arrays; coa_nodes is the list in force, d_coa[] = {ebit, twin, planes, together, cnt}
  FwCoassignParams coa{};
  int64_t coa_measured = 0;
  std::vector<int32_t> coa_nodes;
  void* d_coa[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

namespace {

// integer form of a Metropolis bound: CPython's u = M * 2^-53 with integer M < 2^53,
// so u < thr <=> M < thr * 2^53 (exact scaling) <=> M < ceil(thr * 2^53)
uint64_t thr53_of(double thr) {
  const double t = thr * 9007199254740992.0;
  return !(t > 0.0) ? 0ull : (t >= 9007199254740992.0 ? (1ull << 53) : (uint64_t)std::ceil(t));
}

// Label bits per node for a (k, maxdeg): the search marks visited nodes with codes
// k..k+deg-1 and v with the all-ones value, so k + maxdeg must stay below it.
int pick_lb(int k, int maxdeg) {
  if (k + maxdeg <= 15 && maxdeg <= 15) return 4;
  if (k + maxdeg <= 255) return 8;
  return 0;
}

// LB-bit little-endian fields: node x in bits [x*LB, x*LB + LB) of the byte stream (a
// 3-bit field may straddle two bytes; the label region is padded past its last field).
void pack_labels(const int16_t* lab, int n, int lb, uint8_t* out, int bytes) {
  std::memset(out, 0, (size_t)bytes);
  for (int x = 0; x < n; ++x) {
    const int64_t bit = (int64_t)x * lb;
    const uint32_t v = (uint32_t)(lab[x] & ((1 << lb) - 1)) << (bit & 7);
    out[bit >> 3] |= (uint8_t)v;
    if ((bit & 7) + lb > 8) out[(bit >> 3) + 1] |= (uint8_t)(v >> 8);
  }
}

void unpack_labels(const uint8_t* in, int n, int lb, int16_t* lab) {
  for (int x = 0; x < n; ++x) {
    const int64_t bit = (int64_t)x * lb;
    uint32_t v = in[bit >> 3];
    if ((bit & 7) + lb > 8) v |= (uint32_t)in[(bit >> 3) + 1] << 8;
    lab[x] = (int16_t)((v >> (bit & 7)) & ((1u << lb) - 1));
  }
}

// MarkovChain's initial-state validity: every district non-empty, connected and
// inside the population bounds.  Fills pops[k].
bool plan_valid(const fw_graph* g, const int16_t* lab, int k, int64_t lo, int64_t hi,
                int64_t* pops, std::string* why) {
  const int n = g->n;
  std::vector<int> first(k, -1);
  for (int d = 0; d < k; ++d) pops[d] = 0;
  for (int x = 0; x < n; ++x) {
    if (lab[x] < 0 || lab[x] >= k) {
      *why = "label out of range at node " + std::to_string(x);
      return false;
    }
    pops[lab[x]] += g->popof(x);
    if (first[lab[x]] < 0) first[lab[x]] = x;
  }
  std::vector<uint8_t> seen(n, 0);
  std::vector<int> q(n);
  for (int d = 0; d < k; ++d) {
    if (first[d] < 0) {
      *why = "district " + std::to_string(d) + " is empty";
      return false;
    }
    if (pops[d] < lo || pops[d] > hi) {
      *why = "district " + std::to_string(d) + " population " + std::to_string(pops[d]) +
             " outside [" + std::to_string(lo) + ", " + std::to_string(hi) + "]";
      return false;
    }
    int h = 0, t = 0;
    q[t++] = first[d];
    seen[first[d]] = 1;
    while (h < t) {
      int x = q[h++];
      for (int e = g->rowptr[x]; e < g->rowptr[x + 1]; ++e) {
        int y = g->col[e];
        if (!seen[y] && lab[y] == d) {
          seen[y] = 1;
          q[t++] = y;
        }
      }
    }
  }
  for (int x = 0; x < n; ++x)
    if (!seen[x]) {
      *why = "district " + std::to_string(lab[x]) + " is not contiguous (node " +
             std::to_string(x) + ")";
      return false;
    }
  return true;
}

// the per-district cut histogram of a handle with n_groups groups
size_t geo_hist_bytes(const fw_chains* c, int n_groups) {
  return sizeof(unsigned long long) * (size_t)n_groups * (size_t)(c->g->nnz / 2 + 1);
}

// the plan-distance histogram of a handle with n_groups groups
size_t ovl_hist_bytes(const fw_chains* c, int n_groups) {
  return sizeof(unsigned long long) * (size_t)n_groups * (size_t)(c->g->n + 1);
}

size_t ring_bins(int r) { return (size_t)r * (size_t)r + 1; }

// the seat histogram's buffer: the largest [groups][elections][k + 1] a handle of k districts
// can ask for, so neither fw_chains_set_elections nor fw_chains_set_ladder reallocates it
size_t tally_hist_bytes(int k) {
  return sizeof(unsigned long long) * FW_TALLY_MAX_GROUPS * FW_TALLY_MAX_EL * (size_t)(k + 1);
}

// first two cut ring edges of a plan in ring order: out = {i, j} (-1, -1 if fewer than two)
void ring_pair_of(const fw_chains* c, const int16_t* lab, int32_t* out) {
  out[0] = out[1] = -1;
  int found = 0;
  for (int r = 0; r < c->ring_n && found < 2; ++r)
    if (lab[c->ring_u[r]] != lab[c->ring_w[r]]) out[found++] = r;
  if (found < 2) out[0] = out[1] = -1;
}

// the rung stats' snapshot := the stats records st [n_chains] (fw_chains_set_ladder)
int ladder_snapshot(fw_chains* c, const fw_chain_stats* st) {
  std::vector<FwRungSnap> sn((size_t)c->n_chains);
  for (int i = 0; i < c->n_chains; ++i)
    sn[i] = FwRungSnap{st[i].yields, st[i].steps, st[i].accepts,
                       st[i].sum_cut, st[i].sum_bnodes, st[i].sum_invb};
  HIPCHK(hipMemcpy(c->d_snap, sn.data(), sizeof(FwRungSnap) * sn.size(), hipMemcpyHostToDevice));
  return FW_OK;
}

// ---- the ensemble census (fw_chains_enable_census): plan and buffers of a handle with n_groups
// groups, built aside so that on failure the handle keeps what it had
struct CenBuild {
  FwCensusParams p{};
  void* graph[3] = {nullptr, nullptr, nullptr};
  uint32_t* part = nullptr;
  uint64_t* acc = nullptr;
};

void cen_free(CenBuild* b) {
  void* bufs[] = {b->graph[0], b->graph[1], b->graph[2], b->part, b->acc};
  for (void* x : bufs)
    if (x) (void)hipFree(x);
  *b = CenBuild{};
}

int cen_build(const fw_chains* c, int32_t what, int n_groups, CenBuild* out) {
  const fw_graph* g = c->g;
  const int n = g->n, lb = c->lb, k = c->k, E = g->nnz / 2;
  const bool do_occ = what & FW_CENSUS_NODES, do_cut = what & FW_CENSUS_EDGES,
             walk = what & (FW_CENSUS_EDGES | FW_CENSUS_BOUNDARY);
  const int32_t* rowptr = g->rowptr.data();
  const int32_t* col = g->col.data();
  FwCensusParams p{};
  p.n = n;
  p.k = k;
  p.lb = lb;
  p.what = what;
  p.lab_words = (int)(((int64_t)n * lb + 31) / 32);
  p.n_groups = n_groups;
  // the canonical id of a row's first upper edge: ids run over (u < w) in CSR row order
  std::vector<int32_t> ebase((size_t)n + 1);
  {
    int e = 0;
    for (int v = 0; v < n; ++v) {
      ebase[v] = e;
      for (int t = rowptr[v]; t < rowptr[v + 1]; ++t) e += col[t] > v;
    }
    ebase[n] = e;  // == E
  }
  // tiles: FW_CEN_TILE nodes; the longest tile when the rows of a short one already reach
  // across most of a record (hub graphs, unordered node ids: every tile stages about the whole
  // record, so fewer tiles read less); halved while the tile's counters and rows overflow LDS
  const int env_tile = fw_census_env("FLIPWALK_CENSUS_TILE");
  int T = env_tile >= 1 ? std::min(env_tile, FW_CEN_MAX_TILE) : FW_CEN_TILE;
  bool fixed_tile = env_tile >= 1;
  std::vector<int32_t> tiles;
  int n_tiles = 0, nt = 64, wd_max = 0, fixed = 0;
  for (;;) {
    n_tiles = (n + T - 1) / T;
    nt = (T + 63) / 64 * 64;
    tiles.assign((size_t)n_tiles * FW_CEN_TILE_INTS, 0);
    int max_ent = 0, max_edge = 0;
    wd_max = 0;
    for (int i = 0; i < n_tiles; ++i) {
      const int t0 = i * T, t1 = std::min(n, t0 + T);
      int lo, hi, wd0, wdn;
      fw_cen_tile_reach(rowptr, col, t0, t1, &lo, &hi);
      fw_cen_window(lo, hi, lb, &wd0, &wdn);
      int32_t* td = &tiles[(size_t)i * FW_CEN_TILE_INTS];
      td[0] = t0;
      td[1] = t1 - t0;
      td[2] = rowptr[t0];
      td[3] = rowptr[t1] - rowptr[t0];
      td[4] = ebase[t0];
      td[5] = ebase[t1] - ebase[t0];
      td[6] = wd0;
      td[7] = wdn;
      max_ent = std::max(max_ent, td[3]);
      max_edge = std::max(max_edge, td[5]);
      wd_max = std::max(wd_max, wdn);
    }
    p.off_ecut_lds = do_occ ? k * nt : 0;
    p.off_ent_lds = p.off_ecut_lds + (do_cut ? max_edge : 0);
    fixed = p.off_ent_lds + (walk ? max_ent : 0);
    if (!fixed_tile && T < FW_CEN_MAX_TILE && n > T && 2 * wd_max > p.lab_words) {
      T = FW_CEN_MAX_TILE;
      fixed_tile = true;
      continue;
    }
    if (fixed <= FW_CEN_LDS_WORDS || T == 1) break;  // one node: k 64 + 2 FW_MAX_DEG dwords
    T = (T + 1) / 2;
    fixed_tile = true;
  }
  // windows staged in LDS, as many chains at a time as the rest of 64 KB holds; none: the
  // lanes read the records in HBM, and a tile's window is the record from its first dword
  int batch = fw_census_env("FLIPWALK_CENSUS_STAGE") != 0 && wd_max > 0
                  ? std::min(FW_CEN_MAX_BATCH, (FW_CEN_LDS_WORDS - fixed) / wd_max)
                  : 0;
  p.staged = batch >= 1;
  if (!p.staged) {
    batch = FW_CEN_MAX_BATCH;
    wd_max = 0;
    for (int i = 0; i < n_tiles; ++i) {
      tiles[(size_t)i * FW_CEN_TILE_INTS + 6] = 0;
      tiles[(size_t)i * FW_CEN_TILE_INTS + 7] = p.lab_words;
    }
  }
  p.n_tiles = n_tiles;
  p.nt = nt;
  p.batch = batch;
  p.wd_max = wd_max;
  p.off_stage_lds = fixed;
  p.lds_bytes = 4 * (fixed + batch * wd_max);
  std::vector<uint32_t> ent((size_t)std::max(g->nnz, 1), 0u);
  for (int i = 0; i < n_tiles; ++i) {
    const int32_t* td = &tiles[(size_t)i * FW_CEN_TILE_INTS];
    for (int v = td[0]; v < td[0] + td[1]; ++v)
      for (int t = rowptr[v]; t < rowptr[v + 1]; ++t)
        ent[t] = (uint32_t)((int64_t)col[t] * lb - (int64_t)td[6] * 32) << 1 | (col[t] > v ? 1u : 0u);
  }
  // a row of the partial sums and of the accumulators
  int64_t off = 1;
  p.off_occ = p.off_ecut = p.off_bnd = -1;
  if (do_occ) p.off_occ = off, off += (int64_t)n * k;
  if (do_cut) p.off_ecut = off, off += E;
  if (what & FW_CENSUS_BOUNDARY) p.off_bnd = off, off += n;
  p.size = off;
  // slices: about 4096 workgroups, the partial sums within 64 MB (a group needs one slice at
  // least).  The counters are 32 bits wide and a slice has at most n_chains < 2^31 members,
  // so no counter bounds the slice length.
  p.per_group = c->n_chains / n_groups;
  const int env_slice = fw_census_env("FLIPWALK_CENSUS_SLICE");
  if (env_slice >= 1) {
    p.slice_len = std::min(env_slice, p.per_group);
  } else {
    int64_t spg = std::max<int64_t>(1, 4096 / ((int64_t)n_tiles * n_groups));
    const int64_t cap = std::max<int64_t>(1, ((64ll << 20) / 4 / p.size) / n_groups);
    spg = std::min(std::min(spg, cap), (int64_t)p.per_group);
    p.slice_len = (int)((p.per_group + spg - 1) / spg);
  }
  p.spg = fw_cen_slices(p.per_group, p.slice_len);
  if ((int64_t)n_tiles * n_groups * p.spg >= (1ll << 31))
    return fail(FW_EUNSUPPORTED, "census: %d tiles x %d groups x %d slices", n_tiles, n_groups, p.spg);
  CenBuild b;
  const size_t sz[5] = {sizeof(int32_t) * tiles.size(), sizeof(uint32_t) * ent.size(),
                        sizeof(int32_t) * ebase.size(),
                        sizeof(uint32_t) * (size_t)n_groups * p.spg * (size_t)p.size,
                        sizeof(uint64_t) * (size_t)n_groups * (size_t)p.size};
  void* nb[5] = {};
  bool ok = true;
  for (int i = 0; i < 5 && ok; ++i) ok = hipMalloc(&nb[i], sz[i]) == hipSuccess;
  b.graph[0] = nb[0];
  b.graph[1] = nb[1];
  b.graph[2] = nb[2];
  b.part = static_cast<uint32_t*>(nb[3]);
  b.acc = static_cast<uint64_t*>(nb[4]);
  const bool up = ok && hipMemcpy(nb[0], tiles.data(), sz[0], hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(nb[1], ent.data(), sz[1], hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(nb[2], ebase.data(), sz[2], hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemset(nb[4], 0, sz[4]) == hipSuccess;
  if (!up) {
    cen_free(&b);
    (void)hipGetLastError();
    return ok ? fail(FW_EHIP, "census upload failed")
              : fail(FW_ENOMEM, "census of %d chains in %d groups", c->n_chains, n_groups);
  }
  p.tiles = static_cast<const int32_t*>(nb[0]);
  p.ent = static_cast<const uint32_t*>(nb[1]);
  p.ebase = static_cast<const int32_t*>(nb[2]);
  p.part = b.part;
  b.p = p;
  *out = b;
  return FW_OK;
}

// the handle takes a finished build (its previous one is freed)
void cen_adopt(fw_chains* c, const CenBuild& b) {
  CenBuild old;
  for (int i = 0; i < 3; ++i) old.graph[i] = c->d_cen_graph[i];
  old.part = c->d_cen_part;
  old.acc = c->d_cen_acc;
  cen_free(&old);
  for (int i = 0; i < 3; ++i) c->d_cen_graph[i] = b.graph[i];
  c->d_cen_part = b.part;
  c->d_cen_acc = b.acc;
  c->cen = b.p;
  c->cen_measured = 0;
}

// offset (uint64s into a row of the accumulators) and length of one array of the census
int cen_array(const fw_chains* c, int32_t what, int64_t* off, int64_t* len) {
  const FwCensusParams& p = c->cen;
  switch (what) {
    case FW_CENSUS_OCC: *off = p.off_occ, *len = (int64_t)p.n * p.k; break;
    case FW_CENSUS_ECUT: *off = p.off_ecut, *len = c->g->nnz / 2; break;
    case FW_CENSUS_BND: *off = p.off_bnd, *len = p.n; break;
    case FW_CENSUS_CNT: *off = 0, *len = 1; break;
    default: return fail(FW_EINVAL, "unknown census array %d", what);
  }
  if (!p.what) return fail(FW_ESTATE, "no census is enabled");
  if (*off < 0) return fail(FW_ESTATE, "census array %d was not enabled (mask %d)", what, p.what);
  return FW_OK;
}

// ---- node co-assignment (fw_chains_enable_coassign): plan and buffers of a handle with n_groups
// groups for a validated node list, built aside so that on failure the handle keeps what it had
struct CoaBuild {
  FwCoassignParams p{};
  void* buf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // ebit, twin, planes, together, cnt
};

void coa_free(CoaBuild* b) {
  for (void* x : b->buf)
    if (x) (void)hipFree(x);
  *b = CoaBuild{};
}

size_t coa_together_bytes(const FwCoassignParams& p) {
  return sizeof(uint64_t) * (size_t)p.n_groups * (size_t)p.m * (size_t)p.m;
}

int coa_build(const fw_chains* c, const std::vector<int32_t>& nodes, int n_groups, CoaBuild* out) {
  const int m = (int)nodes.size(), lb = c->lb, n = c->g->n;
  if ((int64_t)n_groups * m * m > FW_COA_MAX_ELEMS)
    return fail(FW_EUNSUPPORTED, "coassign: %d groups x %d x %d nodes exceed 2^28 elements", n_groups, m, m);
  if ((int64_t)n * lb > 0xFFFFFFFFll)
    return fail(FW_EUNSUPPORTED, "coassign: records of %lld label bits", (long long)n * lb);
  FwCoassignParams p{};
  p.m = m;
  p.ms = (m + 3) / 4 * 4;
  p.lb = lb;
  p.lab_words = (int)(((int64_t)n * lb + 31) / 32);
  p.n_groups = n_groups;
  p.per_group = c->n_chains / n_groups;
  const FwCoaPlan q = fw_coa_plan(p.per_group, lb, fw_coassign_env("FLIPWALK_COA_TILE"),
                                  fw_coassign_env("FLIPWALK_COA_CHUNK"));
  p.n_words = q.n_words;
  p.tile = q.tile;
  p.shift = q.shift;
  p.chunk = q.chunk;
  p.rs = q.rs;
  p.n_chunks = q.n_chunks;
  p.lds_bytes = q.lds_bytes;
  // transpose tiles and the window of a record each one's nodes span
  p.n_ttiles = fw_coa_tiles(m);
  std::vector<int32_t> twin((size_t)p.n_ttiles * 2);
  int wd_max = 0;
  for (int t = 0; t < p.n_ttiles; ++t) {
    int e0, en, wd0, wdn;
    fw_coa_tile_window(nodes.data(), m, t, lb, &e0, &en, &wd0, &wdn);
    twin[2 * (size_t)t] = wd0;
    twin[2 * (size_t)t + 1] = wdn;
    wd_max = std::max(wd_max, wdn);
  }
  p.staged = fw_coa_stage(wd_max, fw_coassign_env("FLIPWALK_COA_STAGE") != 0, &p.nw, &p.stride);
  p.t_lds_bytes = p.staged ? 64 * p.nw * (p.stride + 1) * 4 : 0;
  std::vector<uint32_t> ebit((size_t)m);
  for (int j = 0; j < m; ++j)
    ebit[j] = (uint32_t)((int64_t)nodes[j] * lb -
                         (p.staged ? (int64_t)twin[2 * (size_t)(j / FW_COA_TT)] * 32 : 0));
  const int64_t slots = (p.per_group + 63) / 64, spw = (slots + p.nw - 1) / p.nw;
  if ((int64_t)p.n_ttiles * n_groups * spw >= (1ll << 31))
    return fail(FW_EUNSUPPORTED, "coassign: %d tiles x %d groups x %lld member blocks", p.n_ttiles,
                n_groups, (long long)spw);
  CoaBuild b;
  const size_t sz[5] = {sizeof(uint32_t) * ebit.size(), sizeof(int32_t) * twin.size(),
                        sizeof(uint32_t) * (size_t)n_groups * p.n_words * lb * (size_t)p.ms,
                        coa_together_bytes(p), sizeof(uint64_t) * (size_t)n_groups};
  bool ok = true;
  for (int i = 0; i < 5 && ok; ++i) ok = hipMalloc(&b.buf[i], sz[i]) == hipSuccess;
  const bool up = ok && hipMemcpy(b.buf[0], ebit.data(), sz[0], hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(b.buf[1], twin.data(), sz[1], hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemset(b.buf[3], 0, sz[3]) == hipSuccess &&
                  hipMemset(b.buf[4], 0, sz[4]) == hipSuccess;
  if (!up) {
    coa_free(&b);
    (void)hipGetLastError();
    return ok ? fail(FW_EHIP, "coassign upload failed")
              : fail(FW_ENOMEM, "coassign of %d nodes, %d chains in %d groups", m, c->n_chains, n_groups);
  }
  p.ebit = static_cast<const uint32_t*>(b.buf[0]);
  p.twin = static_cast<const int32_t*>(b.buf[1]);
  p.planes = static_cast<uint32_t*>(b.buf[2]);
  p.together = static_cast<uint64_t*>(b.buf[3]);
  p.cnt = static_cast<uint64_t*>(b.buf[4]);
  b.p = p;
  *out = b;
  return FW_OK;
}

// the step is switched off and its buffers freed
void coa_disable(fw_chains* c) {
  CoaBuild old;
  for (int i = 0; i < 5; ++i) old.buf[i] = c->d_coa[i], c->d_coa[i] = nullptr;
  coa_free(&old);
  c->coa = FwCoassignParams{};
  c->coa_nodes.clear();
  c->coa_measured = 0;
}

// the handle takes a finished build for the list `nodes` (its previous one is freed)
void coa_adopt(fw_chains* c, const CoaBuild& b, const std::vector<int32_t>& nodes) {
  std::vector<int32_t> keep(nodes);  // nodes may be the handle's own list
  coa_disable(c);
  for (int i = 0; i < 5; ++i) c->d_coa[i] = b.buf[i];
  c->coa = b.p;
  c->coa_nodes.swap(keep);
}

}  // namespace

extern "C" {

const char* fw_last_error(void) { return g_err.c_str(); }

int32_t fw_version(void) { return 0x000700; }

int32_t fw_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

int fw_graph_create(const int32_t* rowptr, const int32_t* col, const int64_t* pop, int32_t n,
                    int32_t nnz, int device, fw_graph** out) {
  if (!out || !rowptr || (nnz > 0 && !col) || n <= 0 || nnz < 0)
    return fail(FW_EINVAL, "fw_graph_create: bad arguments");
  *out = nullptr;
  if (rowptr[0] != 0 || rowptr[n] != nnz) return fail(FW_EINVAL, "rowptr[0]/rowptr[n] mismatch");
  auto g = new fw_graph();
  g->device = device;
  g->n = n;
  g->nnz = nnz;
  g->rowptr.assign(rowptr, rowptr + n + 1);
  g->col.assign(col, col + nnz);
  bool unit = true;
  if (pop) {
    for (int x = 0; x < n; ++x) unit &= pop[x] == 1;
    if (!unit) g->pop.assign(pop, pop + n);
  }
  for (int x = 0; x < n; ++x) {
    const int b = rowptr[x], e = rowptr[x + 1];
    if (e < b) {
      delete g;
      return fail(FW_EINVAL, "rowptr not monotone at %d", x);
    }
    g->maxdeg = std::max(g->maxdeg, e - b);
    for (int t = b; t < e; ++t) {
      const int y = col[t];
      if (y < 0 || y >= n || y == x || (t > b && col[t - 1] >= y)) {
        delete g;
        return fail(FW_EINVAL, "row %d: neighbours must be ascending, in range, no self loop", x);
      }
      // symmetry: x must appear in y's (sorted) row
      if (!std::binary_search(col + rowptr[y], col + rowptr[y + 1], x)) {
        delete g;
        return fail(FW_EINVAL, "adjacency not symmetric: %d->%d", x, y);
      }
    }
  }
  g->gw = n < (1 << 21) ? detect_grid(g->rowptr, g->col, n) : 0;
  g->gh = g->gw ? n / g->gw : 0;
  grid_div24(g->gw, &g->gm24, &g->gs24);
  if (hipSetDevice(device) != hipSuccess) {
    delete g;
    return fail(FW_EHIP, "hipSetDevice(%d) failed", device);
  }
  // canonical edge ids: undirected pairs (u < w) numbered in CSR row order
  std::vector<int32_t> eid(std::max(nnz, 1)), eu, ew;
  for (int x = 0; x < n; ++x)
    for (int t = rowptr[x]; t < rowptr[x + 1]; ++t) {
      const int y = col[t];
      if (y > x) {
        eid[t] = (int32_t)eu.size();
        eu.push_back(x);
        ew.push_back(y);
      } else {  // (y, x) was numbered in row y
        const int32_t* q = std::lower_bound(col + rowptr[y], col + rowptr[y + 1], x);
        eid[t] = eid[q - col];
      }
    }
  const size_t ne = std::max<size_t>(eu.size(), 1);
  // general graphs: for entry (v, i), the positions j of v's neighbours adjacent to the
  // i-th (the kernel's local contiguity test; degrees <= 63 were checked above)
  std::vector<uint64_t> nbadj;
  if (!g->gw && nnz > 0 && g->maxdeg <= 63) {
    nbadj.assign(nnz, 0);
    for (int v = 0; v < n; ++v)
      for (int i = rowptr[v]; i < rowptr[v + 1]; ++i)
        for (int j = rowptr[v]; j < rowptr[v + 1]; ++j)
          if (j != i && std::binary_search(col + rowptr[col[i]], col + rowptr[col[i] + 1], col[j]))
            nbadj[i] |= 1ull << (j - rowptr[v]);
  }
  hipError_t e1 = hipMalloc(&g->d_rowptr, sizeof(int32_t) * (n + 1));
  hipError_t e2 = hipMalloc(&g->d_col, sizeof(int32_t) * std::max(nnz, 1));
  hipError_t e3 = g->pop.empty() ? hipSuccess : hipMalloc(&g->d_pop, sizeof(int64_t) * n);
  if (e3 == hipSuccess) e3 = hipMalloc(&g->d_eid, sizeof(int32_t) * eid.size());
  if (e3 == hipSuccess) e3 = hipMalloc(&g->d_eu, sizeof(int32_t) * ne);
  if (e3 == hipSuccess) e3 = hipMalloc(&g->d_ew, sizeof(int32_t) * ne);
  std::vector<int32_t> ell, dbound;
  if (!g->gw && g->maxdeg <= 16) {
    // padded rows; the neighbour-adjacency masks move to the same [n][16] layout
    ell.assign((size_t)n * 16, -1);
    std::vector<uint64_t> nb16(nbadj.empty() ? 0 : (size_t)n * 16, 0);
    for (int x = 0; x < n; ++x)
      for (int t = rowptr[x]; t < rowptr[x + 1]; ++t) {
        ell[(size_t)x * 16 + (t - rowptr[x])] = col[t];
        if (!nbadj.empty()) nb16[(size_t)x * 16 + (t - rowptr[x])] = nbadj[t];
      }
    nbadj.swap(nb16);
    if (e3 == hipSuccess) e3 = hipMalloc(&g->d_ell, sizeof(int32_t) * ell.size());
    // loop bounds of the padded-row walks: the select's over the 64 nodes of a group, the
    // gather's over v and its neighbours (C4: 9.7 and ~10 instead of the graph's 14)
    const int ng = (n + 63) / 64;
    dbound.assign((size_t)n + ng, 0);
    for (int x = 0; x < n; ++x) {
      int md = rowptr[x + 1] - rowptr[x];
      for (int t = rowptr[x]; t < rowptr[x + 1]; ++t)
        md = std::max(md, rowptr[col[t] + 1] - rowptr[col[t]]);
      dbound[x] = md;
      dbound[(size_t)n + x / 64] = std::max(dbound[(size_t)n + x / 64], rowptr[x + 1] - rowptr[x]);
    }
    if (e3 == hipSuccess) e3 = hipMalloc(&g->d_dbound, sizeof(int32_t) * dbound.size());
  }
  if (e3 == hipSuccess && !nbadj.empty())
    e3 = hipMalloc(&g->d_nbadj, sizeof(uint64_t) * nbadj.size());
  // the kernels read 1/|B| here instead of dividing in fp64 on every accepted step
  std::vector<double> invb((size_t)n + 1);
  for (int b = 0; b <= n; ++b) invb[b] = 1.0 / (double)(b > 0 ? b : 1);
  if (e3 == hipSuccess) e3 = hipMalloc(&g->d_invb, sizeof(double) * invb.size());
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
    fw_graph_destroy(g);
    return fail(FW_EHIP, "hipMalloc failed for graph");
  }
  bool up = hipMemcpy(g->d_rowptr, rowptr, sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice) ==
            hipSuccess;
  if (nnz) up &= hipMemcpy(g->d_col, col, sizeof(int32_t) * nnz, hipMemcpyHostToDevice) == hipSuccess;
  if (g->d_pop)
    up &= hipMemcpy(g->d_pop, g->pop.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice) ==
          hipSuccess;
  up &= hipMemcpy(g->d_eid, eid.data(), sizeof(int32_t) * eid.size(), hipMemcpyHostToDevice) ==
        hipSuccess;
  if (!nbadj.empty())
    up &= hipMemcpy(g->d_nbadj, nbadj.data(), sizeof(uint64_t) * nbadj.size(),
                    hipMemcpyHostToDevice) == hipSuccess;
  up &= hipMemcpy(g->d_invb, invb.data(), sizeof(double) * invb.size(), hipMemcpyHostToDevice) ==
        hipSuccess;
  if (!ell.empty())
    up &= hipMemcpy(g->d_ell, ell.data(), sizeof(int32_t) * ell.size(), hipMemcpyHostToDevice) ==
          hipSuccess;
  if (!dbound.empty())
    up &= hipMemcpy(g->d_dbound, dbound.data(), sizeof(int32_t) * dbound.size(),
                    hipMemcpyHostToDevice) == hipSuccess;
  if (!eu.empty()) {
    up &= hipMemcpy(g->d_eu, eu.data(), sizeof(int32_t) * eu.size(), hipMemcpyHostToDevice) ==
          hipSuccess;
    up &= hipMemcpy(g->d_ew, ew.data(), sizeof(int32_t) * ew.size(), hipMemcpyHostToDevice) ==
          hipSuccess;
  }
  if (!up || hipDeviceSynchronize() != hipSuccess) {
    fw_graph_destroy(g);
    return fail(FW_EHIP, "graph upload failed");
  }
  *out = g;
  return FW_OK;
}

void fw_graph_destroy(fw_graph* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->d_rowptr) (void)hipFree(g->d_rowptr);
  if (g->d_col) (void)hipFree(g->d_col);
  if (g->d_pop) (void)hipFree(g->d_pop);
  if (g->d_eid) (void)hipFree(g->d_eid);
  if (g->d_eu) (void)hipFree(g->d_eu);
  if (g->d_ew) (void)hipFree(g->d_ew);
  if (g->d_nbadj) (void)hipFree(g->d_nbadj);
  if (g->d_ell) (void)hipFree(g->d_ell);
  if (g->d_dbound) (void)hipFree(g->d_dbound);
  if (g->d_invb) (void)hipFree(g->d_invb);
  delete g;
}

int fw_graph_info(const fw_graph* g, int64_t info[5]) {
  if (!g || !info) return fail(FW_EINVAL, "fw_graph_info: null");
  info[0] = g->n;
  info[1] = g->nnz / 2;
  info[2] = g->maxdeg;
  info[3] = g->gw;
  info[4] = g->gh;
  return FW_OK;
}

void fw_chains_destroy(fw_chains* c) {
  if (!c) return;
  (void)hipSetDevice(c->g->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  void* bufs[] = {c->d_labels, c->d_stats, c->d_pops, c->d_thr, c->d_thr53, c->d_hist_cut, c->d_hist_b,
                  c->d_spill,  c->d_next,  c->d_acc,  c->d_nf,   c->d_lf,       c->d_ps,
                  c->d_pend,   c->d_labval, c->d_flags, c->d_bcnt, c->d_sched, c->d_sched53,
                  c->d_ring,   c->d_ring_node, c->d_hist_ring, c->d_gscr, c->d_segdone,
                  c->d_wsamp,  c->d_wlp,   c->d_lad_thr, c->d_lad_thr53, c->d_logb, c->d_rung,
                  c->d_chain_of, c->d_gmin, c->d_snap, c->d_rstats,
                  c->d_ser_cut, c->d_ser_bn, c->d_ser_rung,
                  c->d_tal_cols, c->d_tal_sums, c->d_tal_seats, c->d_tal_hist,
                  c->d_geo_w, c->d_geo_area, c->d_geo_ext, c->d_geo_out, c->d_geo_hist,
                  c->d_ovl_ref, c->d_ovl_partner, c->d_ovl_O, c->d_ovl_dist, c->d_ovl_hist,
                  c->d_rsm_src, c->d_rsm_family, c->d_rsm_q, c->d_rsm_w, c->d_rsm_cum, c->d_rsm_pts,
                  c->d_rsm_lower, c->d_rsm_extra, c->d_rsm_info,
                  c->d_cen_graph[0], c->d_cen_graph[1], c->d_cen_graph[2], c->d_cen_part,
                  c->d_cen_acc, c->d_pwd_list[0], c->d_pwd_list[1], c->d_pwd_D, c->d_pwd_rowsum,
                  c->d_pwd_near, c->d_pwd_hist,
                  c->d_coa[0], c->d_coa[1], c->d_coa[2], c->d_coa[3], c->d_coa[4]};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  for (int i = 0; i < 2; ++i) {
    if (c->pwd_stage[i]) (void)hipHostFree(c->pwd_stage[i]);
    if (c->pwd_ev[i]) (void)hipEventDestroy(c->pwd_ev[i]);
  }
  for (int i = 0; i < 2; ++i) {
    if (c->rsm_stage[i]) (void)hipHostFree(c->rsm_stage[i]);
    if (c->rsm_ev[i]) (void)hipEventDestroy(c->rsm_ev[i]);
  }
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// work units per slice: the grid kernel's chains per wave (4 / rows per chain), else chains
static long long slice_units(const fw_chains* c) {
  if (!c->p.use16) return c->n_chains;
  const int cpw = 4 / fw_grid16_launch_rows(c->p);
  return (c->n_chains + cpw - 1) / cpw;
}

int fw_chains_create(fw_graph* g, int32_t n_chains, int32_t k, const int16_t* init_labels,
                     int32_t init_per_chain, int32_t proposal_mode, int64_t pop_lo, int64_t pop_hi,
                     const double* thr, int32_t thr_per_chain, uint64_t seed, int64_t chain_id0,
                     fw_chains** out) {
  if (!out || !g || !init_labels || !thr || n_chains <= 0)
    return fail(FW_EINVAL, "fw_chains_create: bad arguments");
  *out = nullptr;
  if (k < 2 || k > FW_MAX_K) return fail(FW_EUNSUPPORTED, "k=%d outside [2, %d]", k, FW_MAX_K);
  if (proposal_mode < FW_PROPOSE_BI || proposal_mode > FW_PROPOSE_CUTEDGE)
    return fail(FW_EINVAL, "unknown proposal mode %d", proposal_mode);
  if (proposal_mode == FW_PROPOSE_BI && k != 2)
    return fail(FW_EINVAL, "slow_reversible_propose_bi needs k == 2 (got %d)", k);
  if (g->maxdeg > FW_MAX_DEG)
    return fail(FW_EUNSUPPORTED, "max degree %d > %d", g->maxdeg, FW_MAX_DEG);
  const int n = g->n, D = g->maxdeg;
  const int G = (n + 63) / 64;
  // row-major grids: the four-chains-per-wave kernel, 2-bit labels when k <= 4
  // (FLIPWALK_NO_GRID16=1 forces the one-chain-per-wave kernel, for A/B parity tests)
  const char* no16 = getenv("FLIPWALK_NO_GRID16");
  int64_t total_pop = 0;
  for (int x = 0; x < n; ++x) total_pop += g->popof(x);
  const bool use16 = fw_grid16_candidate(g->gw, D, G, k, total_pop) && g->gm24 != 0 &&
                     !(no16 && no16[0] == '1');
  int lb = use16 ? fw_grid16_lb(G, k) : pick_lb(k, g->maxdeg);
  {  // the chain kernel on a large grid (k <= 8): 3-bit labels in LDS, search marks in HBM,
     // so more chains fit a CU (C5: 7 -> 9).  FLIPWALK_CSR_LB=3 / 4 forces / forbids it.
    const char* e = getenv("FLIPWALK_CSR_LB");
    const int want = e && e[0] ? atoi(e) : 0;
    if (!use16 && g->gw > 0 && k <= 8 && lb == 4 && (want == 3 || (want == 0 && G > 256)))
      lb = 3;
    // general graphs on padded rows whose k + maxdeg needs 8-bit in-place codes: 5-bit
    // labels with the list search's marks in HBM when that fits more chains per CU — the
    // 8-bit plan is held to 16 by the 4-waves-per-SIMD register budget, the 5-bit one to 20
    // by the 5-wave budget of the lean kernel (C4, 9,000 nodes, k = 18: 16 -> 20 chains per
    // CU, 0.576 -> 0.588 x 10^9; before the lean instantiation the 5-wave budget spilled,
    // 0.495 vs 0.523, profiles/r02/ab/csr_5bit_c4.jsonl).  FLIPWALK_CSR_LB=5 / 8 forces /
    // forbids (5 also for k <= 15).
    if (!use16 && g->gw == 0 && g->d_ell != nullptr && k <= 31 && lb == 8 && want == 0) {
      const long long gs = round16((int64_t)fw_run_gsum_slots(G) * 2), lds = 160 * 1024;
      const long long wbytes = proposal_mode != FW_PROPOSE_CUTEDGE ? round16(((int64_t)n * 2 + 7) / 8) : 0;
      // the 2-bit LDS proposal weights (p.wb) need 4- or 5-bit labels: only l5 carries them
      const long long l8 = round16(((int64_t)n * 8 + 7) / 8 + 8) + gs + 4 * 128;
      const long long l5 = round16(((int64_t)n * 5 + 7) / 8 + 8) + gs + 4 * 8 + wbytes;
      if (n > 16384 || std::min(20ll, lds / l5) > std::min(16ll, lds / l8)) lb = 5;
    }
    if (!use16 && g->gw == 0 && g->d_ell != nullptr && k <= 31 && want == 5) lb = 5;
  }
  if (!lb) return fail(FW_EUNSUPPORTED, "k + maxdeg = %d too large", k + g->maxdeg);

  auto c = new fw_chains();
  c->g = g;
  c->n_chains = n_chains;
  c->k = k;
  c->mode = proposal_mode == FW_PROPOSE_BI ? FW_PROPOSE_PAIRS : proposal_mode;
  c->lb = lb;
  c->D = D;

  // ---- LDS layout
  FwRunParams& p = c->p;
  p.qcap = list_cap(256);
  p.qcap16 = list_cap(384);
  {  // FLIPWALK_FOLD_AT=x: fold the attempt-driven 32-bit counters early (tests)
    const char* e = getenv("FLIPWALK_FOLD_AT");
    const long long v = e && e[0] ? atoll(e) : 0;
    p.fold_at = v >= 64 && v <= 0x80000000ll ? (uint32_t)v : 0x80000000u;
  }
  {  // FLIPWALK_NO_BITBOARD=1: the grid kernel runs every exact search as the list search
    const char* e = getenv("FLIPWALK_NO_BITBOARD");
    p.no_bb = e && e[0] == '1' ? 1 : 0;
    const char* e2 = getenv("FLIPWALK_NO_ROWBB");
    p.no_rowbb = e2 && e2[0] == '1' ? 1 : 0;
  }
  // +8: the grid kernels read label dwords one past the last node
  p.lab_bytes = round16(((int64_t)n * lb + 7) / 8 + 8);
  // chain kernel on padded rows with pairs proposals: 2-bit per-node weights in LDS, so the
  // select reads a group's weights instead of walking its 64 padded rows in L2
  // (FLIPWALK_NO_WB=1: recompute them from the rows, as before)
  {
    const char* e = getenv("FLIPWALK_NO_WB");
    p.wb = !use16 && g->gw == 0 && g->d_ell != nullptr && (lb == 4 || lb == 5) &&
                   c->mode != FW_PROPOSE_CUTEDGE && !(e && e[0] == '1')
               ? 2
               : 0;
  }
  p.off_w = p.lab_bytes;
  p.off_gsum = p.off_w + (p.wb ? round16(((int64_t)n * p.wb + 7) / 8) : 0);
  p.off_list = p.off_gsum + round16((int64_t)fw_run_gsum_slots(G) * 2);  // u16 slots
  p.lds_bytes = p.off_list + p.qcap * 4;
  if (G > 64 * 16) {
    delete c;
    return fail(FW_EUNSUPPORTED, "graph too large (%d weight groups > 1024)", G);
  }
  if (p.lds_bytes > 160 * 1024 - 64) {
    delete c;
    return fail(FW_EUNSUPPORTED, "graph too large for LDS-resident chains (%d B)", p.lds_bytes);
  }

  // ---- initial-state validation and populations
  const int ninit = init_per_chain ? n_chains : 1;
  std::vector<int64_t> pops0((size_t)ninit * k);
  for (int i = 0; i < ninit; ++i) {
    std::string why;
    if (!plan_valid(g, init_labels + (size_t)i * n, k, pop_lo, pop_hi, pops0.data() + (size_t)i * k,
                    &why)) {
      delete c;
      return fail(FW_ESTATE, "initial plan%s invalid: %s",
                  init_per_chain ? (" " + std::to_string(i)).c_str() : "", why.c_str());
    }
  }
  // a chain's HBM record also holds its group sums (derived-state cache, FwRunParams)
  const int lab_stride = p.off_gsum + (int)round16((int64_t)4 * (use16 ? (G + 1) / 2
                                                                      : (fw_run_gsum_slots(G) + 1) / 2));
  std::vector<uint8_t> packed((size_t)n_chains * lab_stride);
  std::vector<int64_t> pops((size_t)n_chains * k);
  {
    std::vector<uint8_t> one(lab_stride);
    for (int i = 0; i < ninit; ++i) {
      pack_labels(init_labels + (size_t)i * n, n, lb, packed.data() + (size_t)i * lab_stride,
                  lab_stride);
    }
    for (int i = ninit; i < n_chains; ++i)
      std::memcpy(packed.data() + (size_t)i * lab_stride, packed.data(), lab_stride);
    for (int i = 0; i < n_chains; ++i)
      std::memcpy(pops.data() + (size_t)i * k, pops0.data() + (size_t)(init_per_chain ? i : 0) * k,
                  sizeof(int64_t) * k);
  }

  if (hipSetDevice(g->device) != hipSuccess) {
    delete c;
    return fail(FW_EHIP, "hipSetDevice failed");
  }
  p.g = g->dev();
  p.n_chains = n_chains;
  p.k = k;
  p.mode = c->mode;
  p.G = G;
  p.pop_lo = pop_lo;
  p.pop_hi = pop_hi;
  p.seed = seed;
  p.chain_id0 = chain_id0;
  p.lab_stride = lab_stride;
  p.lab_copy16 = lab_stride / 16;
  p.gcache_ok = 0;
  p.thr_stride = thr_per_chain ? 2 * D + 1 : 0;
  p.lb = lb;
  p.use16 = use16 ? 1 : 0;
  p.spec = 1;
  if ((use16 ? fw_grid16_plan(p, g->device, &c->grid)
             : fw_run_grid_size(p, lb, g->device, &c->grid)) != 0) {
    delete c;
    return fail(FW_EHIP, "occupancy query failed (LDS %d B)", use16 ? p.lds16 : p.lds_bytes);
  }
  {  // FLIPWALK_GRID_CAP=x: at most x workgroups (tests: more work units than waves)
    const char* e = getenv("FLIPWALK_GRID_CAP");
    const int v = e && e[0] ? atoi(e) : 0;
    if (v >= 1 && v < c->grid) c->grid = v;
  }
  const size_t nthr = (size_t)(thr_per_chain ? n_chains : 1) * (2 * D + 1);
  std::vector<uint64_t> thr53(nthr);
  for (size_t i = 0; i < nthr; ++i) thr53[i] = thr53_of(thr[i]);
  bool ok = hipMalloc(&c->d_labels, packed.size()) == hipSuccess &&
            hipMalloc(&c->d_stats, sizeof(fw_chain_stats) * n_chains) == hipSuccess &&
            hipMalloc(&c->d_pops, sizeof(int64_t) * pops.size()) == hipSuccess &&
            hipMalloc(&c->d_thr, sizeof(double) * nthr) == hipSuccess &&
            hipMalloc(&c->d_thr53, sizeof(uint64_t) * nthr) == hipSuccess &&
            hipMalloc(&c->d_hist_cut, sizeof(unsigned long long) * (g->nnz / 2 + 1 + FW_HIST_PAD)) ==
                hipSuccess &&
            hipMalloc(&c->d_hist_b, sizeof(unsigned long long) * (n + 1 + FW_HIST_PAD)) ==
                hipSuccess &&
            hipMalloc(&c->d_spill, sizeof(uint32_t) * (size_t)c->grid * n) ==
                hipSuccess &&
            hipMalloc(&c->d_next, sizeof(int32_t)) == hipSuccess &&
            hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess;
  if (!ok) {
    fw_chains_destroy(c);
    return fail(FW_ENOMEM, "device allocation failed for %d chains", n_chains);
  }
  ok = hipMemcpy(c->d_labels, packed.data(), packed.size(), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(c->d_pops, pops.data(), sizeof(int64_t) * pops.size(), hipMemcpyHostToDevice) ==
           hipSuccess &&
       hipMemcpy(c->d_thr, thr, sizeof(double) * nthr, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(c->d_thr53, thr53.data(), sizeof(uint64_t) * nthr, hipMemcpyHostToDevice) ==
           hipSuccess &&
       hipMemset(c->d_stats, 0, sizeof(fw_chain_stats) * n_chains) == hipSuccess &&
       hipMemset(c->d_hist_cut, 0, sizeof(unsigned long long) * (g->nnz / 2 + 1 + FW_HIST_PAD)) ==
           hipSuccess &&
       hipMemset(c->d_hist_b, 0, sizeof(unsigned long long) * (n + 1 + FW_HIST_PAD)) == hipSuccess;
  if (!ok || hipDeviceSynchronize() != hipSuccess) {
    fw_chains_destroy(c);
    return fail(FW_EHIP, "chain upload failed");
  }
  p.labels = c->d_labels;
  p.stats = c->d_stats;
  p.pops = c->d_pops;
  p.thr = c->d_thr;
  p.thr53 = c->d_thr53;
  p.hist_cut = c->d_hist_cut;
  p.hist_b = c->d_hist_b;
  p.spill = c->d_spill;
  p.next_chain = c->d_next;
  p.slices = 1;
  p.prio_shift = 5;
  // one per chain: enough for every kernel's work units (quads, pairs or chains)
  if (hipMalloc(&c->d_segdone, sizeof(int32_t) * (size_t)n_chains) != hipSuccess) {
    fw_chains_destroy(c);
    return fail(FW_ENOMEM, "device allocation failed for %d chains", n_chains);
  }
  p.seg_done = c->d_segdone;
  // HBM visit marks of the chain kernel's list search (race_search_gscr: 5-bit labels only,
  // which run on padded rows; 3-bit labels run only on grids, whose race_search_b3 keeps its
  // marks in the labels).  Footprint: 4 B per node per resident workgroup (C4: 9,000 nodes
  // x 19 x 256 workgroups = 175 MB), beside the equally sized search-list spill buffer.
  if (!use16 && lb == 5) {
    p.gscr_words = n;  // one 32-bit mark per node (race_search_gscr)
    const size_t gb = sizeof(uint32_t) * (size_t)c->grid * (size_t)p.gscr_words;
    if (hipMalloc(&c->d_gscr, gb) != hipSuccess || hipMemset(c->d_gscr, 0, gb) != hipSuccess) {
      fw_chains_destroy(c);
      return fail(FW_ENOMEM, "device allocation failed for %d chains", n_chains);
    }
    p.gscr = c->d_gscr;
  }
  *out = c;
  return FW_OK;
}

// Slices per work unit (a quad of the grid kernel, a chain of the chain kernel) for a
// launch of `steps` steps (see fw_grid16_kernel / fw_run_kernel): with more units than
// resident waves W, the S in 1..8 that minimises a uniform-duration model of the launch,
// ceil(nu S / W) / S rounds of whole-unit time plus ~0.6% of a unit's time per extra slice
// start (measured on the grid kernel: three 333-step launches cost 1.2% more than one
// 1000-step launch net of their tails).  FLIPWALK_SLICES=x forces x (1: whole units).
static int launch_slices(const fw_chains* c, int64_t steps) {
  const char* e = getenv("FLIPWALK_SLICES");
  const int force = e && e[0] ? atoi(e) : 0;
  const long long nq = slice_units(c), W = (long long)c->grid * (c->p.use16 ? fw_grid16_launch_nw(c->p) : 1);
  // the kernels number units in int32: nq * S stays below 2^31
  const long long s_max = std::max<long long>(1, std::min<long long>(8, 0x7FFFFFFFll / std::max(nq, 1ll)));
  if (force >= 1) return (int)std::min<long long>({(long long)force, std::max<int64_t>(steps, 1), s_max});
  if (nq <= W || steps < 64) return 1;
  // chains of a small state (C2's 40x40 grid: 400 B of labels) restart a slice for almost
  // nothing, and more, shorter units even out the units' unequal durations at the end of the
  // launch: the most slices (C2 at S = 3 / 6 / 8: 1.314 / 1.340 / 1.347 x 10^9; C3 at 6 and
  // C4 at 8 lose 0.2% / 2.8%: profiles/r05/slices/)
  if (c->p.lab_bytes <= 1024) return (int)std::min<long long>(s_max, steps / 64);
  int best = 1;
  double best_t = 1e300;
  for (int S = 1; S <= s_max; ++S) {
    const double rounds = (double)((nq * S + W - 1) / W) / S;
    const double t = rounds + 0.006 * (S - 1) * (double)nq / (double)W;
    if (t < best_t - 1e-9) {
      best_t = t;
      best = S;
    }
  }
  return best;
}

// The kernels' wave-priority levels (fw_grid16_kernel, fw_run_kernel): eighths of a unit's
// steps when every unit has a wave slot of its own (the 8,192-chain shard: +1.4% over 32nds),
// quarters when waves take several units (C2 +1.2%, C3 +0.3%, C4 / C5 / Frankengraph
// +0.4-0.6%; 16ths and 128ths lose 0.5% / 1.6% on C3: profiles/r05/prio_levels/)
static int launch_prio_shift(const fw_chains* c) {
  const long long nu = slice_units(c) * (long long)c->p.slices;
  const long long W = (long long)c->grid * (c->p.use16 ? fw_grid16_launch_nw(c->p) : 1);
  return nu <= W ? 3 : 2;
}

int fw_chains_run_async(fw_chains* c, int64_t steps, int32_t max_retries) {
  if (!c || steps < 0 || max_retries <= 0) return fail(FW_EINVAL, "fw_chains_run: bad arguments");
  HIPCHK(hipSetDevice(c->g->device));
  if (steps == 0) return FW_OK;
  if (c->d_acc && c->max_yields + (uint64_t)steps + 1 >= 0xFFFFFFFFull)
    return fail(FW_EUNSUPPORTED, "spatial maps hold yield indices below 2^32");
  if (c->p.trace && steps > FW_MAX_LAUNCH_STEPS)
    return fail(FW_EUNSUPPORTED, "a traced run takes at most %lld steps", (long long)FW_MAX_LAUNCH_STEPS);
  c->max_yields += (uint64_t)steps + (c->ran ? 0 : 1);
  c->ran = true;
  c->p.max_retries = max_retries;
  HIPCHK(hipEventRecord(c->ev0, c->stream));
  // the kernels count a launch's steps (and the per-step sums of degrees and boundary
  // changes) in 32 bits: a longer run is a sequence of launches of at most
  // FW_MAX_LAUNCH_STEPS counted steps (the trajectory does not depend on the split)
  int64_t cap = FW_MAX_LAUNCH_STEPS;
  {  // FLIPWALK_LAUNCH_STEPS=x: a smaller cap (tests of the split)
    const char* e = getenv("FLIPWALK_LAUNCH_STEPS");
    const long long v = e && e[0] ? atoll(e) : 0;
    if (v >= 1 && v < cap) cap = v;
  }
  for (int64_t left = steps; left > 0;) {
    const int64_t s = left < cap ? left : cap;
    c->p.steps = s;
    c->p.gcache_ok = c->gcache_ok ? 1 : 0;
    c->p.slices = !c->p.trace ? launch_slices(c, s) : 1;
    c->p.prio_shift = launch_prio_shift(c);
    if (c->p.slices > 1)
      HIPCHK(hipMemsetAsync(c->d_segdone, 0, sizeof(int32_t) * (size_t)slice_units(c), c->stream));
    HIPCHK(hipMemsetAsync(c->d_next, 0, sizeof(int32_t), c->stream));
    const int le = fw_launch_run(c->p, c->lb, c->grid, c->stream);
    if (le != 0) {
      c->gcache_ok = false;
      return fail(FW_EHIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)le));
    }
    c->gcache_ok = true;  // this launch writes every chain's record back
    left -= s;
  }
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  c->timed = true;
  return FW_OK;
}

int fw_chains_sync(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  return FW_OK;
}

int fw_chains_run(fw_chains* c, int64_t steps, int32_t max_retries) {
  int rc = fw_chains_run_async(c, steps, max_retries);
  if (rc) return rc;
  return fw_chains_sync(c);
}

int fw_chains_run_traced(fw_chains* c, int64_t steps, int32_t max_retries, int32_t* host_trace,
                         size_t bytes) {
  if (!c || !host_trace || steps <= 0) return fail(FW_EINVAL, "fw_chains_run_traced: bad arguments");
  const size_t need = sizeof(int32_t) * (size_t)c->n_chains * (size_t)steps;
  if (bytes < need) return fail(FW_EINVAL, "trace needs %zu bytes", need);
  HIPCHK(hipSetDevice(c->g->device));
  int32_t* d_trace = nullptr;
  HIPCHK(hipMalloc(&d_trace, need));
  int rc = FW_OK;
  if (hipMemsetAsync(d_trace, 0xFE, need, c->stream) != hipSuccess) {
    rc = fail(FW_EHIP, "trace memset failed");
  } else {
    c->p.trace = d_trace;
    rc = fw_chains_run(c, steps, max_retries);
    c->p.trace = nullptr;
    if (rc == FW_OK && hipMemcpy(host_trace, d_trace, need, hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(FW_EHIP, "trace download failed");
  }
  (void)hipFree(d_trace);
  return rc;
}

double fw_chains_last_kernel_ms(const fw_chains* c) {
  if (!c || !c->timed) return -1.0;
  float ms = -1.f;
  if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) return -1.0;
  return ms;
}

int fw_chains_launch_info(const fw_chains* c, int64_t info[8]) {
  if (!c || !info) return fail(FW_EINVAL, "fw_chains_launch_info: null");
  HIPCHK(hipSetDevice(c->g->device));
  const FwRunParams& p = c->p;
  void* fn = p.use16 ? fw_grid16_fn(p) : fw_run_fn(p, c->lb);
  if (!fn) return fail(FW_EHIP, "no kernel for this plan");
  hipFuncAttributes at;
  HIPCHK(hipFuncGetAttributes(&at, fn));
  const int nw = p.use16 ? fw_grid16_launch_nw(p) : 1;
  const int lds = p.use16 ? p.lds16 : p.lds_bytes;
  int per_cu = 0;
  HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64 * nw, (size_t)lds));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, c->g->device));
  info[0] = c->grid;
  info[1] = nw;
  info[2] = p.use16 ? 4 / fw_grid16_launch_rows(p) : 1;
  info[3] = lds;
  info[4] = at.numRegs;
  info[5] = (int64_t)at.localSizeBytes;
  info[6] = prop.multiProcessorCount;
  info[7] = per_cu;
  return FW_OK;
}

int fw_chains_read(fw_chains* c, int32_t what, void* host_dst, size_t bytes) {
  if (!c || !host_dst) return fail(FW_EINVAL, "fw_chains_read: null");
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const int n = c->g->n;
  size_t need = 0;
  switch (what) {
    case FW_READ_LABELS: {
      need = sizeof(int16_t) * (size_t)c->n_chains * n;
      if (bytes < need) return fail(FW_EINVAL, "labels need %zu bytes", need);
      std::vector<uint8_t> packed((size_t)c->n_chains * c->p.lab_stride);
      HIPCHK(hipMemcpy(packed.data(), c->d_labels, packed.size(), hipMemcpyDeviceToHost));
      for (int i = 0; i < c->n_chains; ++i)
        unpack_labels(packed.data() + (size_t)i * c->p.lab_stride, n, c->lb,
                      static_cast<int16_t*>(host_dst) + (size_t)i * n);
      return FW_OK;
    }
    case FW_READ_STATS:
      need = sizeof(fw_chain_stats) * c->n_chains;
      if (bytes < need) return fail(FW_EINVAL, "stats need %zu bytes", need);
      HIPCHK(hipMemcpy(host_dst, c->d_stats, need, hipMemcpyDeviceToHost));
      return FW_OK;
    case FW_READ_HIST_CUT:
      need = sizeof(uint64_t) * (c->g->nnz / 2 + 1);
      if (bytes < need) return fail(FW_EINVAL, "hist_cut needs %zu bytes", need);
      HIPCHK(hipMemcpy(host_dst, c->d_hist_cut, need, hipMemcpyDeviceToHost));
      return FW_OK;
    case FW_READ_HIST_B:
      need = sizeof(uint64_t) * (n + 1);
      if (bytes < need) return fail(FW_EINVAL, "hist_b needs %zu bytes", need);
      HIPCHK(hipMemcpy(host_dst, c->d_hist_b, need, hipMemcpyDeviceToHost));
      return FW_OK;
    case FW_READ_POPS:
      need = sizeof(int64_t) * (size_t)c->n_chains * c->k;
      if (bytes < need) return fail(FW_EINVAL, "pops need %zu bytes", need);
      HIPCHK(hipMemcpy(host_dst, c->d_pops, need, hipMemcpyDeviceToHost));
      return FW_OK;
    case FW_READ_HIST_RING:
      if (!c->ring_n) return fail(FW_ESTATE, "the ring observable is not enabled");
      need = sizeof(uint64_t) * ring_bins(c->ring_n);
      if (bytes < need) return fail(FW_EINVAL, "hist_ring needs %zu bytes", need);
      HIPCHK(hipMemcpy(host_dst, c->d_hist_ring, need, hipMemcpyDeviceToHost));
      return FW_OK;
    case FW_READ_RING_PAIR: {
      if (!c->ring_n) return fail(FW_ESTATE, "the ring observable is not enabled");
      need = sizeof(int32_t) * 2 * (size_t)c->n_chains;
      if (bytes < need) return fail(FW_EINVAL, "ring pairs need %zu bytes", need);
      std::vector<uint8_t> packed((size_t)c->n_chains * c->p.lab_stride);
      HIPCHK(hipMemcpy(packed.data(), c->d_labels, packed.size(), hipMemcpyDeviceToHost));
      std::vector<int16_t> lab(n);
      int32_t* out = static_cast<int32_t*>(host_dst);
      for (int i = 0; i < c->n_chains; ++i) {
        unpack_labels(packed.data() + (size_t)i * c->p.lab_stride, n, c->lb, lab.data());
        ring_pair_of(c, lab.data(), out + 2 * (size_t)i);
      }
      return FW_OK;
    }
    case FW_READ_WAITS:
      if (!c->d_wsamp) return fail(FW_ESTATE, "sampled waits are not enabled");
      need = sizeof(double) * 2 * (size_t)c->n_chains;
      if (bytes < need) return fail(FW_EINVAL, "waits need %zu bytes", need);
      HIPCHK(hipMemcpy(host_dst, c->d_wsamp, need, hipMemcpyDeviceToHost));
      return FW_OK;
    case FW_READ_RUNG:
      if (!c->n_rungs) return fail(FW_ESTATE, "no ladder is set");
      need = sizeof(int32_t) * (size_t)c->n_chains;
      if (bytes < need) return fail(FW_EINVAL, "rungs need %zu bytes", need);
      HIPCHK(hipMemcpy(host_dst, c->d_rung, need, hipMemcpyDeviceToHost));
      return FW_OK;
    case FW_READ_RUNG_STATS:
      if (!c->n_rungs) return fail(FW_ESTATE, "no ladder is set");
      need = sizeof(fw_rung_stats) * (size_t)c->n_chains;  // n_sets * n_rungs
      if (bytes < need) return fail(FW_EINVAL, "rung stats need %zu bytes", need);
      HIPCHK(hipMemcpy(host_dst, c->d_rstats, need, hipMemcpyDeviceToHost));
      return FW_OK;
    default:
      return fail(FW_EINVAL, "unknown read kind %d", what);
  }
}

int fw_chains_write(fw_chains* c, int32_t what, const void* host_src, size_t bytes) {
  if (!c || !host_src) return fail(FW_EINVAL, "fw_chains_write: null");
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const int n = c->g->n;
  size_t need = 0;
  switch (what) {
    case FW_READ_LABELS: {
      need = sizeof(int16_t) * (size_t)c->n_chains * n;
      if (bytes < need) return fail(FW_EINVAL, "labels need %zu bytes", need);
      const int16_t* lab = static_cast<const int16_t*>(host_src);
      std::vector<uint8_t> packed((size_t)c->n_chains * c->p.lab_stride);
      std::vector<int64_t> pops((size_t)c->n_chains * c->k);
      for (int i = 0; i < c->n_chains; ++i) {
        std::string why;
        if (!plan_valid(c->g, lab + (size_t)i * n, c->k, c->p.pop_lo, c->p.pop_hi,
                        pops.data() + (size_t)i * c->k, &why))
          return fail(FW_ESTATE, "plan %d invalid: %s", i, why.c_str());
        pack_labels(lab + (size_t)i * n, n, c->lb, packed.data() + (size_t)i * c->p.lab_stride,
                    c->p.lab_stride);
      }
      // the spatial maps carry per-node run state of the current plans (not part of a
      // checkpoint): a new plan under them would resume with wrong maps, so refuse
      if (c->d_acc)
        return fail(FW_ESTATE, "plans cannot be written while the spatial maps are enabled");
      c->gcache_ok = false;  // group sums and counts are re-derived from the new plans
      HIPCHK(hipMemcpy(c->d_labels, packed.data(), packed.size(), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(c->d_pops, pops.data(), sizeof(int64_t) * pops.size(),
                       hipMemcpyHostToDevice));
      if (c->p.bcnt) {  // FW_ACCEPT_BOUNDARY's flagged-node counts follow the new plans
        HIPCHK(hipMemset(c->d_bcnt, 0, sizeof(int32_t) * (size_t)c->n_chains * c->k));
        if (fw_launch_bcnt_init(c->p, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
          return fail(FW_EHIP, "flag count re-init failed");
      }
      return FW_OK;
    }
    case FW_READ_STATS:
      need = sizeof(fw_chain_stats) * c->n_chains;
      if (bytes < need) return fail(FW_EINVAL, "stats need %zu bytes", need);
      c->gcache_ok = false;  // cut / bnodes / npairs come from the caller's records
      HIPCHK(hipMemcpy(c->d_stats, host_src, need, hipMemcpyHostToDevice));
      c->ran = true;  // the initial state was yielded in the run being resumed
      {  // the maps' 2^32 yield-index guard counts the yields already made
        const fw_chain_stats* st = static_cast<const fw_chain_stats*>(host_src);
        uint64_t ymax = 0;
        for (int i = 0; i < c->n_chains; ++i) ymax = std::max<uint64_t>(ymax, st[i].yields);
        c->max_yields = ymax;
      }
      // a ladder's rung stats count from the written records on
      if (c->n_rungs) return ladder_snapshot(c, static_cast<const fw_chain_stats*>(host_src));
      return FW_OK;
    case FW_READ_HIST_CUT:
      need = sizeof(uint64_t) * (c->g->nnz / 2 + 1);
      if (bytes < need) return fail(FW_EINVAL, "hist_cut needs %zu bytes", need);
      HIPCHK(hipMemcpy(c->d_hist_cut, host_src, need, hipMemcpyHostToDevice));
      return FW_OK;
    case FW_READ_HIST_B:
      need = sizeof(uint64_t) * (n + 1);
      if (bytes < need) return fail(FW_EINVAL, "hist_b needs %zu bytes", need);
      HIPCHK(hipMemcpy(c->d_hist_b, host_src, need, hipMemcpyHostToDevice));
      return FW_OK;
    case FW_READ_HIST_RING:
      if (!c->ring_n) return fail(FW_ESTATE, "the ring observable is not enabled");
      need = sizeof(uint64_t) * ring_bins(c->ring_n);
      if (bytes < need) return fail(FW_EINVAL, "hist_ring needs %zu bytes", need);
      HIPCHK(hipMemcpy(c->d_hist_ring, host_src, need, hipMemcpyHostToDevice));
      return FW_OK;
    case FW_READ_WAITS:
      if (!c->d_wsamp) return fail(FW_ESTATE, "sampled waits are not enabled");
      need = sizeof(double) * 2 * (size_t)c->n_chains;
      if (bytes < need) return fail(FW_EINVAL, "waits need %zu bytes", need);
      HIPCHK(hipMemcpy(c->d_wsamp, host_src, need, hipMemcpyHostToDevice));
      return FW_OK;
    case FW_READ_RUNG_STATS:
      if (!c->n_rungs) return fail(FW_ESTATE, "no ladder is set");
      need = sizeof(fw_rung_stats) * (size_t)c->n_chains;
      if (bytes < need) return fail(FW_EINVAL, "rung stats need %zu bytes", need);
      HIPCHK(hipMemcpy(c->d_rstats, host_src, need, hipMemcpyHostToDevice));
      return FW_OK;
    default:
      return fail(FW_EINVAL, "fw_chains_write: unsupported kind %d", what);
  }
}

int fw_chains_reset_observables(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  std::vector<fw_chain_stats> st(c->n_chains);
  HIPCHK(hipMemcpy(st.data(), c->d_stats, sizeof(fw_chain_stats) * st.size(),
                   hipMemcpyDeviceToHost));
  for (auto& s : st) {
    s.yields = 0;
    s.sum_cut = 0;
    s.sum_bnodes = 0;
    s.sum_invb = 0.0;
  }
  HIPCHK(hipMemcpy(c->d_stats, st.data(), sizeof(fw_chain_stats) * st.size(),
                   hipMemcpyHostToDevice));
  if (c->n_rungs) {  // the rung stats restart with the sums
    HIPCHK(hipMemset(c->d_rstats, 0, sizeof(fw_rung_stats) * (size_t)c->n_chains));
    if (const int rc = ladder_snapshot(c, st.data())) return rc;
  }
  HIPCHK(hipMemset(c->d_hist_cut, 0,
                   sizeof(unsigned long long) * (c->g->nnz / 2 + 1 + FW_HIST_PAD)));
  HIPCHK(hipMemset(c->d_hist_b, 0, sizeof(unsigned long long) * (c->g->n + 1 + FW_HIST_PAD)));
  if (c->d_hist_ring)
    HIPCHK(hipMemset(c->d_hist_ring, 0, sizeof(unsigned long long) * ring_bins(c->ring_n)));
  if (c->d_acc) {  // maps restart from the current plans (yield indices restart at 0)
    const size_t C = (size_t)c->n_chains, n = (size_t)c->g->n, E = (size_t)c->g->nnz / 2;
    HIPCHK(hipMemset(c->d_acc, 0, sizeof(int64_t) * std::max<size_t>(C * E, 1)));
    HIPCHK(hipMemset(c->d_nf, 0, sizeof(uint32_t) * C * n));
    HIPCHK(hipMemset(c->d_lf, 0, sizeof(uint32_t) * C * n));
    if (fw_launch_map_init(c->p, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return fail(FW_EHIP, "map re-init failed");
    c->max_yields = 0;
  }
  return FW_OK;
}

int fw_chains_set_accept(fw_chains* c, int32_t rule, const uint8_t* node_flags) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (rule < FW_ACCEPT_CUT || rule > FW_ACCEPT_BOUNDARY)
    return fail(FW_EINVAL, "unknown accept rule %d", rule);
  if (c->n_rungs && rule != FW_ACCEPT_CUT)
    return fail(FW_EUNSUPPORTED, "a base ladder exchanges under FW_ACCEPT_CUT only");
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (rule == FW_ACCEPT_BOUNDARY) {
    if (!node_flags) return fail(FW_EINVAL, "FW_ACCEPT_BOUNDARY needs node flags");
    const int n = c->g->n;
    int nflag = 0;
    for (int x = 0; x < n; ++x) nflag += node_flags[x] ? 1 : 0;
    if (nflag == 0)  // boundary_condition reads blist[0] (grid_chain_sec11.py:46)
      return fail(FW_EINVAL, "boundary_condition needs at least one boundary_node");
    const size_t nb = sizeof(int32_t) * (size_t)c->n_chains * c->k;
    if (!c->d_flags) {
      if (hipMalloc(&c->d_flags, n) != hipSuccess || hipMalloc(&c->d_bcnt, nb) != hipSuccess)
        return fail(FW_ENOMEM, "flag buffers");
    }
    HIPCHK(hipMemcpy(c->d_flags, node_flags, n, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(c->d_bcnt, 0, nb));
    c->p.flags = c->d_flags;
    c->p.bcnt = c->d_bcnt;
    if (fw_launch_bcnt_init(c->p, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return fail(FW_EHIP, "flag count init failed");
  }
  c->p.accept = rule;
  return FW_OK;
}

int fw_chains_set_schedule(fw_chains* c, const double* rows, int32_t n_rows, int64_t t0) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (n_rows < 0 || (n_rows > 0 && !rows)) return fail(FW_EINVAL, "bad schedule rows");
  if (c->n_rungs && n_rows > 0)
    return fail(FW_EUNSUPPORTED, "a base ladder exchanges without a bound schedule only");
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->d_sched) (void)hipFree(c->d_sched);
  if (c->d_sched53) (void)hipFree(c->d_sched53);
  c->d_sched = nullptr;
  c->d_sched53 = nullptr;
  c->p.sched = nullptr;
  c->p.sched53 = nullptr;
  c->p.sched_rows = 0;
  c->p.sched_t0 = 0;
  if (n_rows == 0) return FW_OK;
  const size_t m = (size_t)n_rows * (2 * c->g->maxdeg + 1);
  std::vector<uint64_t> r53(m);
  for (size_t i = 0; i < m; ++i) r53[i] = thr53_of(rows[i]);
  if (hipMalloc(&c->d_sched, sizeof(double) * m) != hipSuccess ||
      hipMalloc(&c->d_sched53, sizeof(uint64_t) * m) != hipSuccess)
    return fail(FW_ENOMEM, "schedule of %d rows", n_rows);
  HIPCHK(hipMemcpy(c->d_sched, rows, sizeof(double) * m, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->d_sched53, r53.data(), sizeof(uint64_t) * m, hipMemcpyHostToDevice));
  c->p.sched = c->d_sched;
  c->p.sched53 = c->d_sched53;
  c->p.sched_rows = n_rows;
  c->p.sched_t0 = t0;
  return FW_OK;
}

int fw_chains_enable_maps(fw_chains* c, const int64_t* label_values) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (c->ran) return fail(FW_ESTATE, "enable the spatial maps before the first run");
  if (c->d_acc) return FW_OK;
  HIPCHK(hipSetDevice(c->g->device));
  const size_t C = (size_t)c->n_chains, n = (size_t)c->g->n, E = (size_t)c->g->nnz / 2;
  std::vector<int64_t> lv(c->k);
  for (int d = 0; d < c->k; ++d) lv[d] = label_values ? label_values[d] : d;
  bool ok = hipMalloc(&c->d_acc, sizeof(int64_t) * std::max<size_t>(C * E, 1)) == hipSuccess &&
            hipMalloc(&c->d_nf, sizeof(uint32_t) * C * n) == hipSuccess &&
            hipMalloc(&c->d_lf, sizeof(uint32_t) * C * n) == hipSuccess &&
            hipMalloc(&c->d_ps, sizeof(int64_t) * C * n) == hipSuccess &&
            hipMalloc(&c->d_pend, sizeof(int32_t) * 4 * C) == hipSuccess &&
            hipMalloc(&c->d_labval, sizeof(int64_t) * lv.size()) == hipSuccess;
  if (!ok) {
    void* bufs[] = {c->d_acc, c->d_nf, c->d_lf, c->d_ps, c->d_pend, c->d_labval};
    for (void* b : bufs)
      if (b) (void)hipFree(b);
    c->d_acc = nullptr;
    c->d_nf = c->d_lf = nullptr;
    c->d_ps = nullptr;
    c->d_pend = nullptr;
    c->d_labval = nullptr;
    return fail(FW_ENOMEM, "spatial maps need %zu MB of device memory",
                (C * (8 * E + 16 * n)) >> 20);
  }
  HIPCHK(hipMemcpy(c->d_labval, lv.data(), sizeof(int64_t) * lv.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(c->d_acc, 0, sizeof(int64_t) * std::max<size_t>(C * E, 1), c->stream));
  HIPCHK(hipMemsetAsync(c->d_nf, 0, sizeof(uint32_t) * C * n, c->stream));
  HIPCHK(hipMemsetAsync(c->d_lf, 0, sizeof(uint32_t) * C * n, c->stream));
  FwRunParams& p = c->p;
  p.m_acc = c->d_acc;
  p.m_nf = c->d_nf;
  p.m_lf = c->d_lf;
  p.m_ps = c->d_ps;
  p.m_pend = c->d_pend;
  p.m_labval = c->d_labval;
  const int le = fw_launch_map_init(p, c->stream);
  if (le != 0) return fail(FW_EHIP, "map init launch failed: %s", hipGetErrorString((hipError_t)le));
  HIPCHK(hipStreamSynchronize(c->stream));
  return FW_OK;
}

int fw_chains_enable_waits(fw_chains* c, const double* p_table) {
  if (!c || !p_table) return fail(FW_EINVAL, "fw_chains_enable_waits: null");
  if (c->ran) return fail(FW_ESTATE, "enable the sampled waits before the first run");
  const int n = c->g->n;
  std::vector<double> lp((size_t)n + 1);
  for (int b = 0; b <= n; ++b) {
    if (!(p_table[b] >= 0.0 && p_table[b] < 1.0))
      return fail(FW_EINVAL, "p_table[%d] = %g outside [0, 1)", b, p_table[b]);
    lp[b] = fw_log1p(-p_table[b]);
  }
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (!c->d_wsamp) {
    if (hipMalloc(&c->d_wsamp, sizeof(double) * 2 * (size_t)c->n_chains) != hipSuccess ||
        hipMalloc(&c->d_wlp, sizeof(double) * lp.size()) != hipSuccess) {
      if (c->d_wsamp) (void)hipFree(c->d_wsamp);
      c->d_wsamp = nullptr;
      return fail(FW_ENOMEM, "sampled-wait buffers");
    }
  }
  HIPCHK(hipMemcpy(c->d_wlp, lp.data(), sizeof(double) * lp.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(c->d_wsamp, 0, sizeof(double) * 2 * (size_t)c->n_chains));
  c->p.wsamp = c->d_wsamp;
  c->p.wlp = c->d_wlp;
  return FW_OK;
}

int fw_chains_set_ladder(fw_chains* c, const double* thr_rows, const double* log_base,
                         int32_t n_rungs, const int32_t* set_of_chain,
                         const int32_t* rung_of_chain) {
  if (!c || !thr_rows || !log_base || !set_of_chain || !rung_of_chain)
    return fail(FW_EINVAL, "fw_chains_set_ladder: null");
  if (n_rungs < 2 || n_rungs > 64) return fail(FW_EINVAL, "n_rungs = %d outside [2, 64]", n_rungs);
  const int C = c->n_chains;
  if (C % n_rungs)
    return fail(FW_EINVAL, "%d chains are not a multiple of %d rungs", C, n_rungs);
  const int n_sets = C / n_rungs;
  // C chains over C (set, rung) slots, none twice: every slot exactly once
  std::vector<int32_t> chain_of((size_t)C, -1);
  std::vector<int64_t> gmin((size_t)n_sets, -1);
  for (int i = 0; i < C; ++i) {
    const int s = set_of_chain[i], r = rung_of_chain[i];
    if (s < 0 || s >= n_sets || r < 0 || r >= n_rungs)
      return fail(FW_EINVAL, "chain %d: (set %d, rung %d) outside [0, %d) x [0, %d)", i, s, r,
                  n_sets, n_rungs);
    int32_t& slot = chain_of[(size_t)s * n_rungs + r];
    if (slot >= 0)
      return fail(FW_EINVAL, "chains %d and %d both sit on rung %d of set %d", slot, i, r, s);
    slot = i;
    if (gmin[s] < 0) gmin[s] = c->p.chain_id0 + i;  // ascending i: the set's smallest id
  }
  if (c->p.accept != FW_ACCEPT_CUT || c->p.sched != nullptr)
    return fail(FW_EUNSUPPORTED,
                "a base ladder exchanges under FW_ACCEPT_CUT without a bound schedule only");
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const size_t L = (size_t)(2 * c->D + 1);
  std::vector<uint64_t> lad53((size_t)n_rungs * L);
  for (size_t i = 0; i < lad53.size(); ++i) lad53[i] = thr53_of(thr_rows[i]);
  std::vector<double> thr((size_t)C * L);
  std::vector<uint64_t> thr53((size_t)C * L);
  for (int i = 0; i < C; ++i) {
    std::memcpy(&thr[(size_t)i * L], thr_rows + (size_t)rung_of_chain[i] * L, sizeof(double) * L);
    std::memcpy(&thr53[(size_t)i * L], &lad53[(size_t)rung_of_chain[i] * L], sizeof(uint64_t) * L);
  }
  std::vector<fw_chain_stats> st((size_t)C);
  HIPCHK(hipMemcpy(st.data(), c->d_stats, sizeof(fw_chain_stats) * st.size(),
                   hipMemcpyDeviceToHost));
  // the new buffers first: on failure the handle keeps what it had.  A handle created with
  // one shared table gets per-chain tables (slots 8, 9).
  const bool shared = c->p.thr_stride == 0;
  void* nb[10] = {};
  const size_t sz[10] = {sizeof(double) * n_rungs * L,    sizeof(uint64_t) * n_rungs * L,
                         sizeof(double) * n_rungs,        sizeof(int32_t) * C,
                         sizeof(int32_t) * C,             sizeof(int64_t) * n_sets,
                         sizeof(FwRungSnap) * C,          sizeof(fw_rung_stats) * C,
                         shared ? sizeof(double) * C * L : 0, shared ? sizeof(uint64_t) * C * L : 0};
  bool ok = true;
  for (int i = 0; i < 10 && ok; ++i) ok = sz[i] == 0 || hipMalloc(&nb[i], sz[i]) == hipSuccess;
  // the per-district cut histogram is kept by rung: a new one for the new group count
  unsigned long long* geo_hist = nullptr;
  if (c->geo_set && ok) ok = hipMalloc(&geo_hist, geo_hist_bytes(c, n_rungs)) == hipSuccess;
  // so is the plan-distance histogram
  unsigned long long* ovl_hist = nullptr;
  if (c->d_ovl_hist && ok) ok = hipMalloc(&ovl_hist, ovl_hist_bytes(c, n_rungs)) == hipSuccess;
  // and the census arrays, whose slices are planned per group
  CenBuild cen;
  if (c->cen.what && ok && cen_build(c, c->cen.what, n_rungs, &cen) != FW_OK) ok = false;
  // and the co-assignment matrices; a group count that takes them past 2^28 elements switches
  // the step off
  CoaBuild coa;
  bool coa_drop = false;
  if (c->coa.m && ok) {
    const int rc = coa_build(c, c->coa_nodes, n_rungs, &coa);
    coa_drop = rc == FW_EUNSUPPORTED;
    if (rc != FW_OK && !coa_drop) ok = false;
  }
  void* d_thr = shared ? nb[8] : (void*)c->d_thr;
  void* d_thr53 = shared ? nb[9] : (void*)c->d_thr53;
  const bool up =
      ok && hipMemcpy(nb[0], thr_rows, sz[0], hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(nb[1], lad53.data(), sz[1], hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(nb[2], log_base, sz[2], hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(nb[3], rung_of_chain, sz[3], hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(nb[4], chain_of.data(), sz[4], hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(nb[5], gmin.data(), sz[5], hipMemcpyHostToDevice) == hipSuccess &&
      hipMemset(nb[7], 0, sz[7]) == hipSuccess &&
      hipMemcpy(d_thr, thr.data(), sizeof(double) * C * L, hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(d_thr53, thr53.data(), sizeof(uint64_t) * C * L, hipMemcpyHostToDevice) ==
          hipSuccess &&
      (!geo_hist || hipMemset(geo_hist, 0, geo_hist_bytes(c, n_rungs)) == hipSuccess) &&
      (!ovl_hist || hipMemset(ovl_hist, 0, ovl_hist_bytes(c, n_rungs)) == hipSuccess);
  if (!up) {
    for (void* b : nb)
      if (b) (void)hipFree(b);
    if (geo_hist) (void)hipFree(geo_hist);
    if (ovl_hist) (void)hipFree(ovl_hist);
    cen_free(&cen);
    coa_free(&coa);
    return ok ? fail(FW_EHIP, "ladder upload failed")
              : fail(FW_ENOMEM, "ladder of %d rungs for %d chains", n_rungs, C);
  }
  void* old[] = {c->d_lad_thr, c->d_lad_thr53, c->d_logb, c->d_rung,
                 c->d_chain_of, c->d_gmin,     c->d_snap, c->d_rstats,
                 shared ? (void*)c->d_thr : nullptr, shared ? (void*)c->d_thr53 : nullptr};
  for (void* b : old)
    if (b) (void)hipFree(b);
  c->d_lad_thr = static_cast<double*>(nb[0]);
  c->d_lad_thr53 = static_cast<uint64_t*>(nb[1]);
  c->d_logb = static_cast<double*>(nb[2]);
  c->d_rung = static_cast<int32_t*>(nb[3]);
  c->d_chain_of = static_cast<int32_t*>(nb[4]);
  c->d_gmin = static_cast<int64_t*>(nb[5]);
  c->d_snap = static_cast<FwRungSnap*>(nb[6]);
  c->d_rstats = static_cast<fw_rung_stats*>(nb[7]);
  if (geo_hist) {
    (void)hipFree(c->d_geo_hist);
    c->d_geo_hist = geo_hist;
  }
  if (ovl_hist) {
    (void)hipFree(c->d_ovl_hist);
    c->d_ovl_hist = ovl_hist;
  }
  if (cen.acc) cen_adopt(c, cen);
  if (coa.p.m)
    coa_adopt(c, coa, c->coa_nodes);
  else if (coa_drop)
    coa_disable(c);
  c->d_thr = static_cast<double*>(d_thr);
  c->d_thr53 = static_cast<uint64_t*>(d_thr53);
  c->p.thr = c->d_thr;
  c->p.thr53 = c->d_thr53;
  c->p.thr_stride = (int32_t)L;
  c->n_rungs = n_rungs;
  c->lad_set.assign(set_of_chain, set_of_chain + C);
  c->lad_epoch += 1;  // series samples recorded so far belong to the previous ladder
  if (c->d_tal_hist)  // the seat histogram is kept by rung: its group count has changed
    HIPCHK(hipMemset(c->d_tal_hist, 0, tally_hist_bytes(c->k)));
  return ladder_snapshot(c, st.data());
}

int fw_chains_exchange_async(fw_chains* c, int64_t round) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (!c->n_rungs) return fail(FW_EINVAL, "fw_chains_exchange_async: no ladder is set");
  if (round < 0 || round > 0xFFFFFFFFll)
    return fail(FW_EINVAL, "round %lld outside [0, 2^32)", (long long)round);
  HIPCHK(hipSetDevice(c->g->device));
  FwExchangeParams e{};
  e.stats = c->d_stats;
  e.snap = c->d_snap;
  e.rstats = c->d_rstats;
  e.thr = c->d_thr;
  e.thr53 = c->d_thr53;
  e.lad_thr = c->d_lad_thr;
  e.lad_thr53 = c->d_lad_thr53;
  e.log_base = c->d_logb;
  e.rung = c->d_rung;
  e.chain_of = c->d_chain_of;
  e.gmin = c->d_gmin;
  e.n_sets = c->n_chains / c->n_rungs;
  e.n_rungs = c->n_rungs;
  e.row_len = 2 * c->D + 1;
  e.round = (uint32_t)round;
  e.seed = c->p.seed;
  // plans, cut, bnodes and npairs stay with their chains: the derived-state cache and the
  // run timing events are left alone
  const int le = fw_launch_exchange(e, c->stream);
  if (le != 0)
    return fail(FW_EHIP, "exchange launch failed: %s", hipGetErrorString((hipError_t)le));
  return FW_OK;
}

// ---------------------------------------------------------------- observable series
namespace {

struct SeriesWhat {
  int kind;
  bool by_rung;
};

int series_what(int32_t what, SeriesWhat* w) {
  if (what < 0 || (what & ~7) || (what & 3) == 3)
    return fail(FW_EINVAL, "unknown series kind %d", what);
  w->kind = what & 3;
  w->by_rung = (what & FW_SERIES_BY_RUNG) != 0;
  if (w->by_rung && w->kind == FW_SERIES_RUNG)
    return fail(FW_EINVAL, "FW_SERIES_BY_RUNG applies to FW_SERIES_CUT and FW_SERIES_BNODES only");
  return FW_OK;
}

int32_t* series_buf(fw_chains* c, int kind) {
  return kind == FW_SERIES_CUT      ? c->d_ser_cut
         : kind == FW_SERIES_BNODES ? c->d_ser_bn
                                    : c->d_ser_rung;
}

// the rung rows, all -1 until something writes them (ordered on the handle's stream)
int series_rung_alloc(fw_chains* c) {
  if (c->d_ser_rung) return FW_OK;
  const size_t bytes = sizeof(int32_t) * (size_t)c->ser_cap * (size_t)c->n_chains;
  if (hipMalloc(&c->d_ser_rung, bytes) != hipSuccess) {
    c->d_ser_rung = nullptr;
    (void)hipGetLastError();
    return fail(FW_ENOMEM, "rung series of %lld samples x %d chains", (long long)c->ser_cap,
                c->n_chains);
  }
  HIPCHK(hipMemsetAsync(c->d_ser_rung, 0xFF, bytes, c->stream));
  return FW_OK;
}

int series_window_ok(const fw_chains* c, int64_t t0, int64_t n, int64_t limit, const char* who) {
  if (!c->ser_cap) return fail(FW_ESTATE, "%s: the series are not enabled", who);
  if (t0 < 0 || n < 1 || t0 > limit || n > limit - t0)
    return fail(FW_EINVAL, "%s: window [%lld, %lld + %lld) outside the %lld samples", who,
                (long long)t0, (long long)t0, (long long)n, (long long)limit);
  return FW_OK;
}

// Device pointer to the window [n][n_chains] of a view.  The plain view is the buffer itself;
// the by-rung view is a regrouped copy (*tmp, to be freed by the caller).
int series_view(fw_chains* c, SeriesWhat w, int64_t t0, int64_t n, const int32_t** x,
                int32_t** tmp) {
  const size_t C = (size_t)c->n_chains;
  *tmp = nullptr;
  if (!w.by_rung) {
    *x = series_buf(c, w.kind) + (size_t)t0 * C;
    return FW_OK;
  }
  if (!c->n_rungs) return fail(FW_ESTATE, "the by-rung view needs a ladder");
  for (int64_t t = t0; t < t0 + n; ++t)
    if (c->ser_epoch[(size_t)t] != c->lad_epoch)
      return fail(FW_ESTATE, "sample %lld was not recorded under the current ladder",
                  (long long)t);
  int32_t* d_set = nullptr;
  if (hipMalloc(tmp, sizeof(int32_t) * (size_t)n * C) != hipSuccess ||
      hipMalloc(&d_set, sizeof(int32_t) * C) != hipSuccess) {
    if (*tmp) (void)hipFree(*tmp);
    *tmp = nullptr;
    (void)hipGetLastError();
    return fail(FW_ENOMEM, "by-rung view of %lld samples x %zu chains", (long long)n, C);
  }
  FwRegroupParams r{};
  r.x = series_buf(c, w.kind) + (size_t)t0 * C;
  r.rung = c->d_ser_rung + (size_t)t0 * C;
  r.set_of = d_set;
  r.out = *tmp;
  r.n_chains = c->n_chains;
  r.n_rungs = c->n_rungs;
  r.n = n;
  hipError_t e = hipMemcpyAsync(d_set, c->lad_set.data(), sizeof(int32_t) * C,
                                hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = (hipError_t)fw_launch_regroup(r, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d_set);
  if (e != hipSuccess) {
    (void)hipFree(*tmp);
    *tmp = nullptr;
    return fail(FW_EHIP, "by-rung regroup failed: %s", hipGetErrorString(e));
  }
  *x = *tmp;
  return FW_OK;
}

}  // namespace

int fw_chains_enable_series(fw_chains* c, int64_t capacity) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (capacity < 1) return fail(FW_EINVAL, "series capacity %lld < 1", (long long)capacity);
  if (c->ser_cap) return fail(FW_ESTATE, "the series are already enabled");
  HIPCHK(hipSetDevice(c->g->device));
  const size_t C = (size_t)c->n_chains;
  if ((size_t)capacity > SIZE_MAX / sizeof(int32_t) / C)
    return fail(FW_ENOMEM, "series of %lld samples x %zu chains", (long long)capacity, C);
  const size_t bytes = sizeof(int32_t) * (size_t)capacity * C;
  int32_t *a = nullptr, *b = nullptr;
  if (hipMalloc(&a, bytes) != hipSuccess || hipMalloc(&b, bytes) != hipSuccess) {
    if (a) (void)hipFree(a);
    (void)hipGetLastError();
    return fail(FW_ENOMEM, "series of %lld samples x %zu chains", (long long)capacity, C);
  }
  if (hipMemset(a, 0, bytes) != hipSuccess || hipMemset(b, 0, bytes) != hipSuccess) {
    (void)hipFree(a);
    (void)hipFree(b);
    return fail(FW_EHIP, "series clear failed");
  }
  c->d_ser_cut = a;
  c->d_ser_bn = b;
  c->ser_epoch.assign((size_t)capacity, 0);
  c->ser_cap = capacity;
  c->ser_n = 0;
  return FW_OK;
}

int fw_chains_record_async(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (!c->ser_cap) return fail(FW_ESTATE, "fw_chains_record_async: the series are not enabled");
  if (c->ser_n >= c->ser_cap)
    return fail(FW_ESTATE, "fw_chains_record_async: all %lld samples are taken",
                (long long)c->ser_cap);
  HIPCHK(hipSetDevice(c->g->device));
  if (c->n_rungs)
    if (const int rc = series_rung_alloc(c)) return rc;
  FwRecordParams r{};
  r.stats = c->d_stats;
  r.rung = c->n_rungs ? c->d_rung : nullptr;
  r.cut = c->d_ser_cut;
  r.bnodes = c->d_ser_bn;
  r.rung_out = c->d_ser_rung;
  r.n_chains = c->n_chains;
  r.sample = c->ser_n;
  // like the exchange step: the run timing events are left alone
  const int le = fw_launch_record(r, c->stream);
  if (le != 0) return fail(FW_EHIP, "record launch failed: %s", hipGetErrorString((hipError_t)le));
  c->ser_epoch[(size_t)c->ser_n] = c->lad_epoch;
  c->ser_n += 1;
  return FW_OK;
}

int fw_chains_series_info(const fw_chains* c, int64_t info[4]) {
  if (!c || !info) return fail(FW_EINVAL, "fw_chains_series_info: null");
  info[0] = c->ser_cap;
  info[1] = c->ser_n;
  info[2] = c->lad_epoch;
  info[3] = c->n_rungs;
  return FW_OK;
}

int fw_chains_series_reset(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (!c->ser_cap) return fail(FW_ESTATE, "fw_chains_series_reset: the series are not enabled");
  c->ser_n = 0;
  return FW_OK;
}

int fw_chains_read_series(fw_chains* c, int32_t what, int64_t t0, int64_t n, int32_t* dst,
                          size_t bytes) {
  if (!c || !dst) return fail(FW_EINVAL, "fw_chains_read_series: null");
  SeriesWhat w;
  if (const int rc = series_what(what, &w)) return rc;
  if (const int rc = series_window_ok(c, t0, n, c->ser_n, "fw_chains_read_series")) return rc;
  const size_t C = (size_t)c->n_chains, need = sizeof(int32_t) * (size_t)n * C;
  if (bytes < need) return fail(FW_EINVAL, "the window needs %zu bytes", need);
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (w.kind == FW_SERIES_RUNG && !c->d_ser_rung) {  // no rung row was ever kept
    std::fill(dst, dst + (size_t)n * C, -1);
    return FW_OK;
  }
  const int32_t* x = nullptr;
  int32_t* tmp = nullptr;
  if (const int rc = series_view(c, w, t0, n, &x, &tmp)) return rc;
  const hipError_t e = hipMemcpy(dst, x, need, hipMemcpyDeviceToHost);
  if (tmp) (void)hipFree(tmp);
  if (e != hipSuccess) return fail(FW_EHIP, "series download failed: %s", hipGetErrorString(e));
  return FW_OK;
}

int fw_chains_write_series(fw_chains* c, int32_t what, int64_t t0, int64_t n, const int32_t* src,
                           size_t bytes) {
  if (!c || !src) return fail(FW_EINVAL, "fw_chains_write_series: null");
  SeriesWhat w;
  if (const int rc = series_what(what, &w)) return rc;
  if (w.by_rung) return fail(FW_EINVAL, "series are written by chain, not by rung");
  if (const int rc = series_window_ok(c, t0, n, c->ser_cap, "fw_chains_write_series")) return rc;
  if (t0 > c->ser_n)
    return fail(FW_EINVAL, "a write at sample %lld would leave a gap after the %lld recorded",
                (long long)t0, (long long)c->ser_n);
  const size_t C = (size_t)c->n_chains, need = sizeof(int32_t) * (size_t)n * C;
  if (bytes < need) return fail(FW_EINVAL, "the window needs %zu bytes", need);
  if (w.kind != FW_SERIES_RUNG) {  // what the exact sums' overflow bound rests on
    const int64_t xmax = std::max<int64_t>(c->g->nnz / 2, c->g->n);
    for (size_t i = 0; i < (size_t)n * C; ++i)
      if (src[i] < 0 || src[i] > xmax)
        return fail(FW_EINVAL, "sample %lld, chain %zu: value %d outside [0, %lld]",
                    (long long)(t0 + (int64_t)(i / C)), i % C, src[i], (long long)xmax);
  } else if (c->n_rungs) {  // every (set, rung) exactly once per sample
    const int R = c->n_rungs;
    std::vector<int64_t> seen(C, -1);
    for (int64_t t = 0; t < n; ++t)
      for (size_t i = 0; i < C; ++i) {
        const int r = src[(size_t)t * C + i];
        if (r < 0 || r >= R)
          return fail(FW_EINVAL, "sample %lld, chain %zu: rung %d outside [0, %d)",
                      (long long)(t0 + t), i, r, R);
        int64_t& s = seen[(size_t)c->lad_set[i] * R + r];
        if (s == t)
          return fail(FW_EINVAL, "sample %lld: rung %d of set %d is held twice",
                      (long long)(t0 + t), r, c->lad_set[i]);
        s = t;
      }
  }
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (w.kind == FW_SERIES_RUNG)
    if (const int rc = series_rung_alloc(c)) return rc;
  const int64_t end = t0 + n;
  if (w.kind != FW_SERIES_RUNG && c->d_ser_rung && end > c->ser_n)
    // samples a value write creates carry no rung row
    HIPCHK(hipMemsetAsync(c->d_ser_rung + (size_t)c->ser_n * C, 0xFF,
                          sizeof(int32_t) * (size_t)(end - c->ser_n) * C, c->stream));
  HIPCHK(hipMemcpyAsync(series_buf(c, w.kind) + (size_t)t0 * C, src, need, hipMemcpyHostToDevice,
                        c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int64_t t = t0; t < end; ++t)
    if (w.kind == FW_SERIES_RUNG)
      c->ser_epoch[(size_t)t] = c->lad_epoch;
    else if (t >= c->ser_n)
      c->ser_epoch[(size_t)t] = 0;
  c->ser_n = std::max(c->ser_n, end);
  return FW_OK;
}

int fw_chains_series_acf(fw_chains* c, int32_t what, int64_t t0, int64_t n, int32_t max_lag,
                         int64_t* per_series, double* pooled) {
  if (!c) return fail(FW_EINVAL, "null handle");
  SeriesWhat w;
  if (const int rc = series_what(what, &w)) return rc;
  if (w.kind == FW_SERIES_RUNG)
    return fail(FW_EINVAL, "autocovariances are taken of FW_SERIES_CUT or FW_SERIES_BNODES");
  if (const int rc = series_window_ok(c, t0, n, c->ser_n, "fw_chains_series_acf")) return rc;
  if (max_lag < 0 || max_lag >= n)
    return fail(FW_EINVAL, "max_lag %d outside [0, n = %lld)", max_lag, (long long)n);
  if (max_lag > FW_SERIES_MAX_LAG)
    return fail(FW_EINVAL, "max_lag %d above %d", max_lag, FW_SERIES_MAX_LAG);
  const int64_t xmax = std::max<int64_t>(c->g->nnz / 2, c->g->n);
  if ((unsigned __int128)n * (unsigned __int128)xmax * (unsigned __int128)xmax >=
      ((unsigned __int128)1 << 63))
    return fail(FW_EINVAL, "n * xmax^2 = %lld * %lld^2 does not fit 63 bits", (long long)n,
                (long long)xmax);
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const int32_t* x = nullptr;
  int32_t* tmp = nullptr;
  if (const int rc = series_view(c, w, t0, n, &x, &tmp)) return rc;
  const size_t C = (size_t)c->n_chains, L1 = (size_t)max_lag + 1;
  const int n_groups = w.by_rung ? c->n_rungs : 1;
  int64_t* d_sums = nullptr;
  double* d_pool = nullptr;
  int rc = FW_OK;
  if (hipMalloc(&d_sums, sizeof(int64_t) * 3 * L1 * C) != hipSuccess ||
      hipMalloc(&d_pool, sizeof(double) * (size_t)n_groups * (L1 + 2)) != hipSuccess) {
    (void)hipGetLastError();
    rc = fail(FW_ENOMEM, "lagged sums of %zu series x %zu lags", C, L1);
  }
  if (rc == FW_OK) {
    FwAcfParams a{};
    a.x = x;
    a.sums = d_sums;
    a.n_series = c->n_chains;
    a.max_lag = max_lag;
    a.n = n;
    FwPoolParams p{};
    p.sums = d_sums;
    p.out = d_pool;
    p.n_series = c->n_chains;
    p.max_lag = max_lag;
    p.members = w.by_rung ? c->n_chains / c->n_rungs : c->n_chains;
    p.stride = w.by_rung ? c->n_rungs : 1;
    p.n = n;
    hipError_t e = (hipError_t)fw_launch_acf(a, c->stream);
    if (e == hipSuccess && pooled) e = (hipError_t)fw_launch_pool(p, n_groups, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && pooled)
      e = hipMemcpy(pooled, d_pool, sizeof(double) * (size_t)n_groups * (L1 + 2),
                    hipMemcpyDeviceToHost);
    if (e == hipSuccess && per_series) {
      // device layout [3][L1][series] (coalesced along the series) -> [series][3][L1]
      std::vector<int64_t> h(3 * L1 * C);
      e = hipMemcpy(h.data(), d_sums, sizeof(int64_t) * h.size(), hipMemcpyDeviceToHost);
      if (e == hipSuccess)
        for (size_t kl = 0; kl < 3 * L1; ++kl)
          for (size_t j = 0; j < C; ++j) per_series[j * 3 * L1 + kl] = h[kl * C + j];
    }
    if (e != hipSuccess) rc = fail(FW_EHIP, "series_acf failed: %s", hipGetErrorString(e));
  }
  if (d_sums) (void)hipFree(d_sums);
  if (d_pool) (void)hipFree(d_pool);
  if (tmp) (void)hipFree(tmp);
  return rc;
}

// ---------------------------------------------------------------- district tallies
int fw_chains_set_columns(fw_chains* c, const int64_t* cols, int32_t n_cols) {
  if (!c || !cols) return fail(FW_EINVAL, "fw_chains_set_columns: null");
  if (n_cols < 1 || n_cols > FW_TALLY_MAX_COLS)
    return fail(FW_EINVAL, "n_cols = %d outside [1, %d]", n_cols, FW_TALLY_MAX_COLS);
  const size_t n = (size_t)c->g->n, C = (size_t)c->n_chains;
  const int n_pairs = (n_cols + 1) / 2;
  // device form: columns 2p and 2p + 1 side by side, [n_pairs][n][2] (fw_tally.hip)
  std::vector<uint32_t> packed((size_t)n_pairs * n * 2, 0u);
  for (int j = 0; j < n_cols; ++j) {
    int64_t total = 0;
    for (size_t x = 0; x < n; ++x) {
      const int64_t v = cols[(size_t)j * n + x];
      if (v < 0) return fail(FW_EINVAL, "column %d: value %lld at node %zu is negative", j,
                             (long long)v, x);
      // v >= 2^31 alone is already too much; below it the running total cannot overflow
      if (v >= (1ll << 31) || (total += v) >= (1ll << 31))
        return fail(FW_EINVAL, "column %d: the total over the nodes must stay below 2^31", j);
      packed[((size_t)(j >> 1) * n + x) * 2 + (j & 1)] = (uint32_t)v;
    }
  }
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));  // a tally in flight reads the old columns
  // the new buffers first: on failure the handle keeps what it had
  uint32_t* d_cols = nullptr;
  int64_t* d_sums = nullptr;
  int32_t* d_seats = c->d_tal_seats;
  unsigned long long* d_hist = c->d_tal_hist;
  bool ok = hipMalloc(&d_cols, sizeof(uint32_t) * packed.size()) == hipSuccess &&
            hipMalloc(&d_sums, sizeof(int64_t) * C * n_cols * c->k) == hipSuccess &&
            (d_seats || hipMalloc(&d_seats, sizeof(int32_t) * C * FW_TALLY_MAX_EL * 2) == hipSuccess) &&
            (d_hist || hipMalloc(&d_hist, tally_hist_bytes(c->k)) == hipSuccess);
  const bool up = ok &&
                  hipMemcpy(d_cols, packed.data(), sizeof(uint32_t) * packed.size(),
                            hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemset(d_hist, 0, tally_hist_bytes(c->k)) == hipSuccess;
  if (!up) {
    if (d_cols) (void)hipFree(d_cols);
    if (d_sums) (void)hipFree(d_sums);
    if (d_seats && !c->d_tal_seats) (void)hipFree(d_seats);
    if (d_hist && !c->d_tal_hist) (void)hipFree(d_hist);
    (void)hipGetLastError();
    return ok ? fail(FW_EHIP, "column upload failed")
              : fail(FW_ENOMEM, "%d columns for %d chains", n_cols, c->n_chains);
  }
  if (c->d_tal_cols) (void)hipFree(c->d_tal_cols);
  if (c->d_tal_sums) (void)hipFree(c->d_tal_sums);
  c->d_tal_cols = d_cols;
  c->d_tal_sums = d_sums;
  c->d_tal_seats = d_seats;
  c->d_tal_hist = d_hist;
  c->tal_cols = n_cols;
  c->tal_el = 0;
  c->tal_have_sums = c->tal_have_seats = false;
  return FW_OK;
}

int fw_chains_set_elections(fw_chains* c, const int32_t* ab, int32_t n_el) {
  if (!c || (!ab && n_el != 0)) return fail(FW_EINVAL, "fw_chains_set_elections: null");
  if (n_el < 0 || n_el > FW_TALLY_MAX_EL)
    return fail(FW_EINVAL, "n_el = %d outside [0, %d]", n_el, FW_TALLY_MAX_EL);
  if (!c->tal_cols) return fail(FW_ESTATE, "fw_chains_set_elections: no columns are set");
  for (int e = 0; e < n_el; ++e) {
    const int a = ab[2 * e], b = ab[2 * e + 1];
    if (a < 0 || a >= c->tal_cols || b < 0 || b >= c->tal_cols)
      return fail(FW_EINVAL, "election %d: columns (%d, %d) outside [0, %d)", e, a, b, c->tal_cols);
    if (a == b) return fail(FW_EINVAL, "election %d: both parties are column %d", e, a);
  }
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemset(c->d_tal_hist, 0, tally_hist_bytes(c->k)));
  for (int e = 0; e < n_el; ++e) {
    c->tal_ab[e][0] = ab[2 * e];
    c->tal_ab[e][1] = ab[2 * e + 1];
  }
  c->tal_el = n_el;
  c->tal_have_seats = false;
  return FW_OK;
}

int fw_chains_tally_async(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (!c->tal_cols) return fail(FW_ESTATE, "fw_chains_tally_async: no columns are set");
  HIPCHK(hipSetDevice(c->g->device));
  FwTallyParams t{};
  t.labels = c->d_labels;
  t.lab_stride = c->p.lab_stride;
  t.cols = c->d_tal_cols;
  t.sums = c->d_tal_sums;
  t.n_chains = c->n_chains;
  t.n = c->g->n;
  t.k = c->k;
  t.lb = c->lb;
  t.n_cols = c->tal_cols;
  // like the exchange and record steps: the run timing events are left alone
  int le = fw_launch_tally(t, c->stream);
  if (le != 0) return fail(FW_EHIP, "tally launch failed: %s", hipGetErrorString((hipError_t)le));
  c->tal_have_sums = true;
  if (c->tal_el) {
    FwSeatsParams s{};
    s.sums = c->d_tal_sums;
    s.rung = c->n_rungs ? c->d_rung : nullptr;
    s.seats = c->d_tal_seats;
    s.hist = c->d_tal_hist;
    std::memcpy(s.ab, c->tal_ab, sizeof s.ab);
    s.n_chains = c->n_chains;
    s.k = c->k;
    s.n_cols = c->tal_cols;
    s.n_el = c->tal_el;
    s.n_groups = c->n_rungs ? c->n_rungs : 1;
    le = fw_launch_seats(s, c->stream);
    if (le != 0) return fail(FW_EHIP, "seat launch failed: %s", hipGetErrorString((hipError_t)le));
  }
  c->tal_have_seats = true;
  c->n_tallied += 1;
  return FW_OK;
}

namespace {

// bytes of a FW_TALLY_* array of the handle as it is configured now
int tally_bytes(const fw_chains* c, int32_t what, size_t* need) {
  const size_t C = (size_t)c->n_chains;
  switch (what) {
    case FW_TALLY_SUMS:
      *need = sizeof(int64_t) * C * c->tal_cols * c->k;
      return FW_OK;
    case FW_TALLY_SEATS:
      *need = sizeof(int32_t) * C * c->tal_el * 2;
      return FW_OK;
    case FW_TALLY_HIST:
      *need = sizeof(uint64_t) * (size_t)(c->n_rungs ? c->n_rungs : 1) * c->tal_el * (c->k + 1);
      return FW_OK;
    default:
      return fail(FW_EINVAL, "unknown tally kind %d", what);
  }
}

}  // namespace

int fw_chains_read_tally(fw_chains* c, int32_t what, void* dst, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_read_tally: null");
  size_t need = 0;
  if (const int rc = tally_bytes(c, what, &need)) return rc;
  if (!c->tal_cols) return fail(FW_ESTATE, "fw_chains_read_tally: no columns are set");
  if ((what == FW_TALLY_SUMS && !c->tal_have_sums) || (what == FW_TALLY_SEATS && !c->tal_have_seats))
    return fail(FW_ESTATE, "fw_chains_read_tally: nothing has been tallied yet");
  if (bytes < need || (!dst && need)) return fail(FW_EINVAL, "the tally needs %zu bytes", need);
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (!need) return FW_OK;
  const void* src = what == FW_TALLY_SUMS    ? (const void*)c->d_tal_sums
                    : what == FW_TALLY_SEATS ? (const void*)c->d_tal_seats
                                             : (const void*)c->d_tal_hist;
  HIPCHK(hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
  return FW_OK;
}

int fw_chains_write_tally(fw_chains* c, int32_t what, const void* src, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_write_tally: null");
  if (what != FW_TALLY_HIST)
    return fail(FW_EINVAL, "fw_chains_write_tally: only FW_TALLY_HIST can be written (got %d)", what);
  if (!c->tal_cols) return fail(FW_ESTATE, "fw_chains_write_tally: no columns are set");
  size_t need = 0;
  if (const int rc = tally_bytes(c, what, &need)) return rc;
  if (bytes < need || (!src && need)) return fail(FW_EINVAL, "the seat histogram needs %zu bytes", need);
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (need) HIPCHK(hipMemcpy(c->d_tal_hist, src, need, hipMemcpyHostToDevice));
  return FW_OK;
}

int fw_chains_tally_reset(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (c->d_tal_hist) {
    HIPCHK(hipSetDevice(c->g->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemset(c->d_tal_hist, 0, tally_hist_bytes(c->k)));
  }
  c->n_tallied = 0;
  return FW_OK;
}

int fw_chains_tally_info(const fw_chains* c, int64_t info[5]) {
  if (!c || !info) return fail(FW_EINVAL, "fw_chains_tally_info: null");
  info[0] = c->tal_cols;
  info[1] = c->tal_el;
  info[2] = c->lb;
  info[3] = c->n_rungs ? c->n_rungs : 1;
  info[4] = c->n_tallied;
  return FW_OK;
}

// ---------------------------------------------------------------- per-district geometry
namespace {

// a geometry array as the device keeps it: every value >= 0, the total below 2^31
int geo_pack(const char* name, const int64_t* src, size_t len, std::vector<uint32_t>* out) {
  out->clear();
  if (!src) return FW_OK;
  out->resize(len);
  int64_t total = 0;
  for (size_t i = 0; i < len; ++i) {
    const int64_t v = src[i];
    if (v < 0) return fail(FW_EINVAL, "%s: value %lld at index %zu is negative", name, (long long)v, i);
    // v >= 2^31 alone is already too much; below it the running total cannot overflow
    if (v >= (1ll << 31) || (total += v) >= (1ll << 31))
      return fail(FW_EINVAL, "%s: the total must stay below 2^31", name);
    (*out)[i] = (uint32_t)v;
  }
  return FW_OK;
}

int geo_bytes(const fw_chains* c, int32_t what, size_t* need) {
  switch (what) {
    case FW_GEOM_DISTRICTS:
      *need = sizeof(int64_t) * (size_t)c->n_chains * c->k * 5;
      return FW_OK;
    case FW_GEOM_HIST:
      *need = geo_hist_bytes(c, c->n_rungs ? c->n_rungs : 1);
      return FW_OK;
    default:
      return fail(FW_EINVAL, "unknown geometry kind %d", what);
  }
}

}  // namespace

int fw_chains_set_geometry(fw_chains* c, const int64_t* edge_w, const int64_t* area,
                           const int64_t* ext) {
  if (!c) return fail(FW_EINVAL, "fw_chains_set_geometry: null");
  const size_t n = (size_t)c->g->n, E = (size_t)(c->g->nnz / 2);
  std::vector<uint32_t> hw, ha, he;
  if (const int rc = geo_pack("edge weights", edge_w, E, &hw)) return rc;
  if (const int rc = geo_pack("area", area, n, &ha)) return rc;
  if (const int rc = geo_pack("exterior", ext, n, &he)) return rc;
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));  // a measurement in flight reads the old arrays
  // the new buffers first: on failure the handle keeps what it had
  const int n_groups = c->n_rungs ? c->n_rungs : 1;
  const std::vector<uint32_t>* host[3] = {&hw, &ha, &he};
  uint32_t* dev[3] = {nullptr, nullptr, nullptr};
  int64_t* d_out = c->d_geo_out;
  unsigned long long* d_hist = c->d_geo_hist;
  bool ok = true;
  for (int i = 0; i < 3 && ok; ++i)
    ok = host[i]->empty() || hipMalloc(&dev[i], sizeof(uint32_t) * host[i]->size()) == hipSuccess;
  ok = ok &&
       (d_out || hipMalloc(&d_out, sizeof(int64_t) * (size_t)c->n_chains * c->k * 5) == hipSuccess) &&
       (d_hist || hipMalloc(&d_hist, geo_hist_bytes(c, n_groups)) == hipSuccess);
  bool up = ok;
  for (int i = 0; i < 3 && up; ++i)
    up = host[i]->empty() || hipMemcpy(dev[i], host[i]->data(), sizeof(uint32_t) * host[i]->size(),
                                       hipMemcpyHostToDevice) == hipSuccess;
  up = up && hipMemset(d_hist, 0, geo_hist_bytes(c, n_groups)) == hipSuccess;
  if (!up) {
    for (uint32_t* d : dev)
      if (d) (void)hipFree(d);
    if (d_out && !c->d_geo_out) (void)hipFree(d_out);
    if (d_hist && !c->d_geo_hist) (void)hipFree(d_hist);
    (void)hipGetLastError();
    return ok ? fail(FW_EHIP, "geometry upload failed")
              : fail(FW_ENOMEM, "geometry of %d chains", c->n_chains);
  }
  uint32_t* old[] = {c->d_geo_w, c->d_geo_area, c->d_geo_ext};
  for (uint32_t* b : old)
    if (b) (void)hipFree(b);
  c->d_geo_w = dev[0];
  c->d_geo_area = dev[1];
  c->d_geo_ext = dev[2];
  c->d_geo_out = d_out;
  c->d_geo_hist = d_hist;
  fw_geometry_plan(c->g->n, c->k, c->lb, dev[0] != nullptr, &c->geo_plan);
  c->geo_set = true;
  c->geo_have = false;
  c->n_measured = 0;
  return FW_OK;
}

int fw_chains_geometry_async(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (!c->geo_set) return fail(FW_ESTATE, "fw_chains_geometry_async: no geometry is set");
  HIPCHK(hipSetDevice(c->g->device));
  FwGeomParams p{};
  p.labels = c->d_labels;
  p.lab_stride = c->p.lab_stride;
  p.eu = c->g->d_eu;
  p.ew = c->g->d_ew;
  p.ewt = c->d_geo_w;
  p.area = c->d_geo_area;
  p.ext = c->d_geo_ext;
  p.out = c->d_geo_out;
  p.n_chains = c->n_chains;
  p.n = c->g->n;
  p.n_edges = c->g->nnz / 2;
  p.k = c->k;
  p.lb = c->lb;
  p.lab_words = c->geo_plan.lab_words;
  p.tile = c->geo_plan.tile;
  p.bins = c->geo_plan.bins;
  p.nw = c->geo_plan.nw;
  // like the exchange, record and tally steps: the run timing events are left alone
  int le = fw_launch_geometry(p, c->geo_plan.lds_bytes, c->stream);
  if (le != 0)
    return fail(FW_EHIP, "geometry launch failed: %s", hipGetErrorString((hipError_t)le));
  FwGeomHistParams h{};
  h.G = c->d_geo_out;
  h.rung = c->n_rungs ? c->d_rung : nullptr;
  h.hist = c->d_geo_hist;
  h.n_chains = c->n_chains;
  h.k = c->k;
  h.n_groups = c->n_rungs ? c->n_rungs : 1;
  h.n_edges = p.n_edges;
  le = fw_launch_geometry_hist(h, c->stream);
  if (le != 0)
    return fail(FW_EHIP, "geometry histogram launch failed: %s", hipGetErrorString((hipError_t)le));
  c->geo_have = true;
  c->n_measured += 1;
  return FW_OK;
}

int fw_chains_read_geometry(fw_chains* c, int32_t what, void* dst, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_read_geometry: null");
  size_t need = 0;
  if (const int rc = geo_bytes(c, what, &need)) return rc;
  if (!c->geo_set) return fail(FW_ESTATE, "fw_chains_read_geometry: no geometry is set");
  if (what == FW_GEOM_DISTRICTS && !c->geo_have)
    return fail(FW_ESTATE, "fw_chains_read_geometry: nothing has been measured yet");
  if (bytes < need || !dst) return fail(FW_EINVAL, "the geometry needs %zu bytes", need);
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const void* src = what == FW_GEOM_DISTRICTS ? (const void*)c->d_geo_out : (const void*)c->d_geo_hist;
  HIPCHK(hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
  return FW_OK;
}

int fw_chains_write_geometry(fw_chains* c, int32_t what, const void* src, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_write_geometry: null");
  if (what != FW_GEOM_HIST)
    return fail(FW_EINVAL, "fw_chains_write_geometry: only FW_GEOM_HIST can be written (got %d)", what);
  if (!c->geo_set) return fail(FW_ESTATE, "fw_chains_write_geometry: no geometry is set");
  size_t need = 0;
  if (const int rc = geo_bytes(c, what, &need)) return rc;
  if (bytes < need || !src) return fail(FW_EINVAL, "the geometry histogram needs %zu bytes", need);
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(c->d_geo_hist, src, need, hipMemcpyHostToDevice));
  return FW_OK;
}

int fw_chains_geometry_reset(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (c->d_geo_hist) {
    HIPCHK(hipSetDevice(c->g->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemset(c->d_geo_hist, 0, geo_hist_bytes(c, c->n_rungs ? c->n_rungs : 1)));
  }
  c->n_measured = 0;
  return FW_OK;
}

int fw_chains_geometry_info(const fw_chains* c, int64_t info[5]) {
  if (!c || !info) return fail(FW_EINVAL, "fw_chains_geometry_info: null");
  info[0] = c->d_geo_w ? 1 : 0;
  info[1] = c->lb;
  info[2] = c->n_rungs ? c->n_rungs : 1;
  info[3] = c->g->nnz / 2;
  info[4] = c->n_measured;
  return FW_OK;
}

// ---------------------------------------------------------------- plan overlap and distance
namespace {

// dwords of a record that hold labels, and a reference row's length (16-byte rows)
int ovl_words(const fw_chains* c) { return (int)(((int64_t)c->g->n * c->lb + 31) / 32); }
int ovl_row_words(const fw_chains* c) { return (ovl_words(c) + 3) & ~3; }

// the buffers every overlap entry point shares, allocated by the first set_reference or
// set_partners; on failure the handle keeps what it had
int ovl_ensure(fw_chains* c) {
  if (c->d_ovl_hist) return FW_OK;
  const size_t C = (size_t)c->n_chains, kk = (size_t)c->k * c->k;
  const size_t hist = ovl_hist_bytes(c, c->n_rungs ? c->n_rungs : 1);
  void* nb[4] = {};
  const size_t sz[4] = {sizeof(uint32_t) * C * ovl_row_words(c), sizeof(int64_t) * C * kk,
                        sizeof(int32_t) * C, hist};
  bool ok = true;
  for (int i = 0; i < 4 && ok; ++i) ok = hipMalloc(&nb[i], sz[i]) == hipSuccess;
  const bool up = ok && hipMemset(nb[3], 0, hist) == hipSuccess;
  if (!up) {
    for (void* b : nb)
      if (b) (void)hipFree(b);
    (void)hipGetLastError();
    return ok ? fail(FW_EHIP, "overlap buffers could not be zeroed")
              : fail(FW_ENOMEM, "overlap buffers of %d chains", c->n_chains);
  }
  c->d_ovl_ref = static_cast<uint32_t*>(nb[0]);
  c->d_ovl_O = static_cast<int64_t*>(nb[1]);
  c->d_ovl_dist = static_cast<int32_t*>(nb[2]);
  c->d_ovl_hist = static_cast<unsigned long long*>(nb[3]);
  return FW_OK;
}

int ovl_bytes(const fw_chains* c, int32_t what, size_t* need) {
  switch (what) {
    case FW_OVERLAP_MATRIX:
      *need = sizeof(int64_t) * (size_t)c->n_chains * c->k * c->k;
      return FW_OK;
    case FW_OVERLAP_DIST:
      *need = sizeof(int32_t) * (size_t)c->n_chains;
      return FW_OK;
    case FW_OVERLAP_HIST:
      *need = ovl_hist_bytes(c, c->n_rungs ? c->n_rungs : 1);
      return FW_OK;
    case FW_OVERLAP_REF:
      *need = sizeof(int16_t) * (size_t)(c->ovl_ref == 2 ? c->n_chains : 1) * c->g->n;
      return FW_OK;
    default:
      return fail(FW_EINVAL, "unknown overlap kind %d", what);
  }
}

}  // namespace

int fw_chains_set_reference(fw_chains* c, const int16_t* labels, int32_t per_chain) {
  if (!c) return fail(FW_EINVAL, "fw_chains_set_reference: null");
  const int n = c->g->n, rows = labels && !per_chain ? 1 : c->n_chains;
  const int row_words = ovl_row_words(c);
  std::vector<uint8_t> packed;
  if (labels) {
    if (per_chain != 0 && per_chain != 1)
      return fail(FW_EINVAL, "per_chain = %d is neither 0 nor 1", per_chain);
    for (size_t i = 0; i < (size_t)rows * n; ++i)
      if (labels[i] < 0 || labels[i] >= c->k)
        return fail(FW_EINVAL, "reference label %d of node %zu (row %zu) outside [0, %d)",
                    (int)labels[i], i % n, i / n, c->k);
    packed.resize((size_t)rows * row_words * 4);
    for (int i = 0; i < rows; ++i)
      pack_labels(labels + (size_t)i * n, n, c->lb, packed.data() + (size_t)i * row_words * 4,
                  row_words * 4);
  }
  HIPCHK(hipSetDevice(c->g->device));
  if (const int rc = ovl_ensure(c)) return rc;
  const size_t hist = ovl_hist_bytes(c, c->n_rungs ? c->n_rungs : 1);
  if (labels) {
    HIPCHK(hipStreamSynchronize(c->stream));  // a measurement in flight reads the old reference
    HIPCHK(hipMemcpy(c->d_ovl_ref, packed.data(), packed.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(c->d_ovl_hist, 0, hist));
  } else {
    // a snapshot at this point of the stream: the label words of every record, not the group
    // sums behind them; no host synchronisation
    HIPCHK(hipMemcpy2DAsync(c->d_ovl_ref, (size_t)row_words * 4, c->d_labels,
                            (size_t)c->p.lab_stride, (size_t)ovl_words(c) * 4,
                            (size_t)c->n_chains, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemsetAsync(c->d_ovl_hist, 0, hist, c->stream));
  }
  c->ovl_ref = labels && !per_chain ? 1 : 2;
  c->ovl_last = -1;
  c->ovl_measured = 0;
  return FW_OK;
}

int fw_chains_set_partners(fw_chains* c, const int32_t* partner) {
  if (!c || !partner) return fail(FW_EINVAL, "fw_chains_set_partners: null");
  for (int i = 0; i < c->n_chains; ++i)
    if (partner[i] < 0 || partner[i] >= c->n_chains)
      return fail(FW_EINVAL, "partner %d of chain %d outside [0, %d)", partner[i], i, c->n_chains);
  HIPCHK(hipSetDevice(c->g->device));
  if (const int rc = ovl_ensure(c)) return rc;
  if (!c->d_ovl_partner)
    if (hipMalloc(&c->d_ovl_partner, sizeof(int32_t) * (size_t)c->n_chains) != hipSuccess) {
      (void)hipGetLastError();
      c->d_ovl_partner = nullptr;
      return fail(FW_ENOMEM, "partners of %d chains", c->n_chains);
    }
  HIPCHK(hipStreamSynchronize(c->stream));  // a measurement in flight reads the old partners
  HIPCHK(hipMemcpy(c->d_ovl_partner, partner, sizeof(int32_t) * (size_t)c->n_chains,
                   hipMemcpyHostToDevice));
  c->ovl_partners = true;
  if (c->ovl_last == FW_OVERLAP_PARTNER) c->ovl_last = -1;
  return FW_OK;
}

int fw_chains_overlap_async(fw_chains* c, int32_t against) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (against != FW_OVERLAP_REFERENCE && against != FW_OVERLAP_PARTNER)
    return fail(FW_EINVAL, "fw_chains_overlap_async: unknown kind %d", against);
  if (against == FW_OVERLAP_REFERENCE && !c->ovl_ref)
    return fail(FW_ESTATE, "fw_chains_overlap_async: no reference is set");
  if (against == FW_OVERLAP_PARTNER && !c->ovl_partners)
    return fail(FW_ESTATE, "fw_chains_overlap_async: no partners are set");
  HIPCHK(hipSetDevice(c->g->device));
  FwOverlapParams p{};
  p.labels = c->d_labels;
  p.lab_stride = c->p.lab_stride;
  p.ref = c->d_ovl_ref;
  p.ref_stride = c->ovl_ref == 2 ? ovl_row_words(c) : 0;
  p.partner = against == FW_OVERLAP_PARTNER ? c->d_ovl_partner : nullptr;
  p.O = c->d_ovl_O;
  p.dist = c->d_ovl_dist;
  p.n_chains = c->n_chains;
  p.n = c->g->n;
  p.k = c->k;
  p.lb = c->lb;
  p.lab_words = ovl_words(c);
  int nw = 1, lds_bytes = 0;
  fw_overlap_plan(c->k, &nw, &lds_bytes);
  // like the exchange, record, tally and geometry steps: the run timing events are left alone
  int le = fw_launch_overlap(p, nw, lds_bytes, c->stream);
  if (le != 0)
    return fail(FW_EHIP, "overlap launch failed: %s", hipGetErrorString((hipError_t)le));
  FwOverlapHistParams h{};
  h.dist = c->d_ovl_dist;
  h.rung = c->n_rungs ? c->d_rung : nullptr;
  h.hist = c->d_ovl_hist;
  h.n_chains = c->n_chains;
  h.n_groups = c->n_rungs ? c->n_rungs : 1;
  h.n = p.n;
  le = fw_launch_overlap_hist(h, c->stream);
  if (le != 0)
    return fail(FW_EHIP, "overlap histogram launch failed: %s", hipGetErrorString((hipError_t)le));
  c->ovl_last = against;
  c->ovl_measured += 1;
  return FW_OK;
}

int fw_chains_read_overlap(fw_chains* c, int32_t what, void* dst, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_read_overlap: null");
  size_t need = 0;
  if (const int rc = ovl_bytes(c, what, &need)) return rc;
  if (!c->d_ovl_hist)
    return fail(FW_ESTATE, "fw_chains_read_overlap: neither a reference nor partners are set");
  if ((what == FW_OVERLAP_MATRIX || what == FW_OVERLAP_DIST) && c->ovl_last < 0)
    return fail(FW_ESTATE, "fw_chains_read_overlap: nothing has been measured yet");
  if (what == FW_OVERLAP_REF && !c->ovl_ref)
    return fail(FW_ESTATE, "fw_chains_read_overlap: no reference is set");
  if (bytes < need || !dst) return fail(FW_EINVAL, "the overlap needs %zu bytes", need);
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (what == FW_OVERLAP_REF) {
    const int rows = c->ovl_ref == 2 ? c->n_chains : 1, row_bytes = ovl_row_words(c) * 4;
    std::vector<uint8_t> packed((size_t)rows * row_bytes);
    HIPCHK(hipMemcpy(packed.data(), c->d_ovl_ref, packed.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < rows; ++i)
      unpack_labels(packed.data() + (size_t)i * row_bytes, c->g->n, c->lb,
                    static_cast<int16_t*>(dst) + (size_t)i * c->g->n);
    return FW_OK;
  }
  const void* src = what == FW_OVERLAP_MATRIX ? (const void*)c->d_ovl_O
                    : what == FW_OVERLAP_DIST ? (const void*)c->d_ovl_dist
                                              : (const void*)c->d_ovl_hist;
  HIPCHK(hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
  return FW_OK;
}

int fw_chains_write_overlap(fw_chains* c, int32_t what, const void* src, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_write_overlap: null");
  if (what != FW_OVERLAP_HIST)
    return fail(FW_EINVAL, "fw_chains_write_overlap: only FW_OVERLAP_HIST can be written (got %d)", what);
  if (!c->d_ovl_hist)
    return fail(FW_ESTATE, "fw_chains_write_overlap: neither a reference nor partners are set");
  size_t need = 0;
  if (const int rc = ovl_bytes(c, what, &need)) return rc;
  if (bytes < need || !src) return fail(FW_EINVAL, "the distance histogram needs %zu bytes", need);
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(c->d_ovl_hist, src, need, hipMemcpyHostToDevice));
  return FW_OK;
}

int fw_chains_overlap_reset(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (c->d_ovl_hist) {
    HIPCHK(hipSetDevice(c->g->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemset(c->d_ovl_hist, 0, ovl_hist_bytes(c, c->n_rungs ? c->n_rungs : 1)));
  }
  c->ovl_measured = 0;
  return FW_OK;
}

int fw_chains_overlap_info(const fw_chains* c, int64_t info[5]) {
  if (!c || !info) return fail(FW_EINVAL, "fw_chains_overlap_info: null");
  info[0] = c->ovl_ref;
  info[1] = c->lb;
  info[2] = c->n_rungs ? c->n_rungs : 1;
  info[3] = c->ovl_partners ? 1 : 0;
  info[4] = c->ovl_measured;
  return FW_OK;
}

// ---------------------------------------------------------------- resampling across chains
namespace {

size_t rsm_stage_bytes(const fw_chains* c) {
  return sizeof(uint32_t) * std::max((size_t)c->n_chains, (size_t)(c->g->nnz / 2 + 1));
}

// the buffers every resample entry point shares, allocated by the first clone or resample (the
// families start as the identity); on failure the handle keeps what it had
int rsm_ensure(fw_chains* c) {
  if (c->d_rsm_family) return FW_OK;
  const size_t C = (size_t)c->n_chains;
  void* nb[9] = {};
  const size_t sz[9] = {sizeof(int32_t) * C,  sizeof(int32_t) * C,  sizeof(uint32_t) * (size_t)(c->g->nnz / 2 + 1),
                        sizeof(uint32_t) * C, sizeof(uint64_t) * C, sizeof(uint64_t) * C,
                        sizeof(int32_t) * C,  sizeof(int32_t) * C,  sizeof(int64_t) * 8};
  void* st[2] = {};
  hipEvent_t ev[2] = {};
  bool ok = true;
  for (int i = 0; i < 9 && ok; ++i) ok = hipMalloc(&nb[i], sz[i]) == hipSuccess;
  for (int i = 0; i < 2 && ok; ++i)
    ok = hipHostMalloc(&st[i], rsm_stage_bytes(c), hipHostMallocDefault) == hipSuccess &&
         hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
  std::vector<int32_t> iota(C);
  for (size_t i = 0; i < C; ++i) iota[i] = (int32_t)i;
  const bool up = ok && hipMemcpy(nb[1], iota.data(), sz[1], hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemset(nb[8], 0, sz[8]) == hipSuccess;
  if (!up) {
    for (void* b : nb)
      if (b) (void)hipFree(b);
    for (int i = 0; i < 2; ++i) {
      if (st[i]) (void)hipHostFree(st[i]);
      if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
    (void)hipGetLastError();
    return ok ? fail(FW_EHIP, "resample buffers could not be initialised")
              : fail(FW_ENOMEM, "resample buffers of %d chains", c->n_chains);
  }
  c->d_rsm_src = static_cast<int32_t*>(nb[0]);
  c->d_rsm_family = static_cast<int32_t*>(nb[1]);
  c->d_rsm_q = static_cast<uint32_t*>(nb[2]);
  c->d_rsm_w = static_cast<uint32_t*>(nb[3]);
  c->d_rsm_cum = static_cast<uint64_t*>(nb[4]);
  c->d_rsm_pts = static_cast<uint64_t*>(nb[5]);
  c->d_rsm_lower = static_cast<int32_t*>(nb[6]);
  c->d_rsm_extra = static_cast<int32_t*>(nb[7]);
  c->d_rsm_info = static_cast<int64_t*>(nb[8]);
  for (int i = 0; i < 2; ++i) {
    c->rsm_stage[i] = st[i];
    c->rsm_ev[i] = ev[i];
  }
  return FW_OK;
}

// host array -> device array on the handle's stream through a pinned slot: the host waits only
// for the copy that used the slot two uploads ago, never for the stream
int rsm_upload(fw_chains* c, void* dst, const void* src, size_t bytes) {
  const int s = c->rsm_slot;
  c->rsm_slot ^= 1;
  HIPCHK(hipEventSynchronize(c->rsm_ev[s]));
  std::memcpy(c->rsm_stage[s], src, bytes);
  HIPCHK(hipMemcpyAsync(dst, c->rsm_stage[s], bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipEventRecord(c->rsm_ev[s], c->stream));
  return FW_OK;
}

// what both entry points refuse (include/flipwalk.h)
int rsm_refuse(const fw_chains* c, const char* who) {
  if (c->d_acc)
    return fail(FW_ESTATE, "%s: plans cannot be moved while the spatial maps are enabled", who);
  if (c->n_rungs)
    return fail(FW_EUNSUPPORTED, "%s: a laddered handle's chains are not resampled", who);
  return FW_OK;
}

int rsm_launch_clone(fw_chains* c) {
  FwCloneParams p{};
  p.labels = c->d_labels;
  p.lab_stride = c->p.lab_stride;
  p.stats = c->d_stats;
  p.pops = c->d_pops;
  p.bcnt = c->p.bcnt;
  p.wsamp = c->d_wsamp;
  p.src = c->d_rsm_src;
  p.family = c->d_rsm_family;
  p.n_chains = c->n_chains;
  p.k = c->k;
  // the copied record, its group sums and the three copied counts stay consistent with each
  // other, so the derived-state cache stays as it was; the run timing events are left alone
  const int le = fw_launch_clone(p, c->stream);
  if (le != 0) return fail(FW_EHIP, "clone launch failed: %s", hipGetErrorString((hipError_t)le));
  c->rsm_have_src = true;
  return FW_OK;
}

}  // namespace

int fw_chains_clone_async(fw_chains* c, const int32_t* src) {
  if (!c || !src) return fail(FW_EINVAL, "fw_chains_clone_async: null");
  const int C = c->n_chains;
  int64_t moved = 0;
  for (int i = 0; i < C; ++i) {
    if (src[i] < 0 || src[i] >= C)
      return fail(FW_EINVAL, "source %d of chain %d outside [0, %d)", src[i], i, C);
    if (src[src[i]] != src[i])
      return fail(FW_EINVAL, "source %d of chain %d is not a fixed point (its own source is %d)",
                  src[i], i, src[src[i]]);
    moved += src[i] != i;
  }
  if (const int rc = rsm_refuse(c, "fw_chains_clone_async")) return rc;
  HIPCHK(hipSetDevice(c->g->device));
  if (const int rc = rsm_ensure(c)) return rc;
  if (const int rc = rsm_upload(c, c->d_rsm_src, src, sizeof(int32_t) * (size_t)C)) return rc;
  if (const int rc = rsm_launch_clone(c)) return rc;
  c->rsm_host_clones += moved;
  return FW_OK;
}

int fw_chains_resample_async(fw_chains* c, const uint32_t* q, int32_t sign, int64_t round) {
  if (!c || !q) return fail(FW_EINVAL, "fw_chains_resample_async: null");
  const int E = c->g->nnz / 2;
  if (sign != 1 && sign != -1) return fail(FW_EINVAL, "sign = %d is neither +1 nor -1", sign);
  if (round < 0 || round > 0xFFFFFFFFll)
    return fail(FW_EINVAL, "round %lld outside [0, 2^32)", (long long)round);
  if (q[0] != FW_RSM_ONE) return fail(FW_EINVAL, "q[0] = %u is not 2^30", q[0]);
  for (int d = 1; d <= E; ++d)
    if (q[d] > q[d - 1]) return fail(FW_EINVAL, "q[%d] = %u > q[%d] = %u: the table must not increase", d, q[d], d - 1, q[d - 1]);
  if (c->n_chains > FW_RSM_MAX_CHAINS)
    return fail(FW_EUNSUPPORTED, "%d chains > 2^20: the points' limb arithmetic stops there", c->n_chains);
  if (const int rc = rsm_refuse(c, "fw_chains_resample_async")) return rc;
  HIPCHK(hipSetDevice(c->g->device));
  if (const int rc = rsm_ensure(c)) return rc;
  if (c->rsm_q.size() != (size_t)E + 1 || std::memcmp(c->rsm_q.data(), q, sizeof(uint32_t) * ((size_t)E + 1))) {
    c->rsm_q.clear();  // nothing is cached should the upload fail
    if (const int rc = rsm_upload(c, c->d_rsm_q, q, sizeof(uint32_t) * ((size_t)E + 1))) return rc;
    c->rsm_q.assign(q, q + E + 1);
  }
  FwResampleParams r{};
  r.stats = c->d_stats;
  r.q = c->d_rsm_q;
  r.w = c->d_rsm_w;
  r.cum = c->d_rsm_cum;
  r.pts = c->d_rsm_pts;
  r.lower = c->d_rsm_lower;
  r.extra = c->d_rsm_extra;
  r.src = c->d_rsm_src;
  r.info = c->d_rsm_info;
  r.n_chains = c->n_chains;
  r.n_edges = E;
  r.sign = sign;
  r.round = (uint32_t)round;
  r.seed = c->p.seed;
  r.chain_id0 = c->p.chain_id0;
  const int le = fw_launch_resample_map(r, c->stream);
  if (le != 0) return fail(FW_EHIP, "resample launch failed: %s", hipGetErrorString((hipError_t)le));
  c->rsm_have_w = true;
  if (const int rc = rsm_launch_clone(c)) return rc;
  c->n_resampled += 1;
  c->rsm_round = round;
  return FW_OK;
}

int fw_chains_resample_info(fw_chains* c, int64_t info[8]) {
  if (!c || !info) return fail(FW_EINVAL, "fw_chains_resample_info: null");
  int64_t dev[8] = {};
  if (c->d_rsm_info) {
    HIPCHK(hipSetDevice(c->g->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(dev, c->d_rsm_info, sizeof dev, hipMemcpyDeviceToHost));
  }
  info[0] = c->n_resampled;
  info[1] = c->rsm_round;
  for (int i = 0; i < 5; ++i) info[2 + i] = dev[i];
  info[7] = dev[5] + c->rsm_host_clones;
  return FW_OK;
}

int fw_chains_read_resample(fw_chains* c, int32_t what, void* dst, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_read_resample: null");
  if (what != FW_RESAMPLE_SRC && what != FW_RESAMPLE_FAMILY && what != FW_RESAMPLE_WEIGHTS)
    return fail(FW_EINVAL, "unknown resample kind %d", what);
  if (what == FW_RESAMPLE_SRC && !c->rsm_have_src)
    return fail(FW_ESTATE, "fw_chains_read_resample: nothing has been cloned or resampled yet");
  if (what == FW_RESAMPLE_WEIGHTS && !c->rsm_have_w)
    return fail(FW_ESTATE, "fw_chains_read_resample: nothing has been resampled yet");
  const size_t need = 4 * (size_t)c->n_chains;
  if (bytes < need || !dst) return fail(FW_EINVAL, "the resample array needs %zu bytes", need);
  if (!c->d_rsm_family) {  // FAMILY of a handle that never cloned
    for (int i = 0; i < c->n_chains; ++i) static_cast<int32_t*>(dst)[i] = i;
    return FW_OK;
  }
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const void* src = what == FW_RESAMPLE_SRC      ? (const void*)c->d_rsm_src
                    : what == FW_RESAMPLE_FAMILY ? (const void*)c->d_rsm_family
                                                 : (const void*)c->d_rsm_w;
  HIPCHK(hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
  return FW_OK;
}

int fw_chains_write_resample(fw_chains* c, int32_t what, const void* src, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_write_resample: null");
  if (what != FW_RESAMPLE_FAMILY)
    return fail(FW_EINVAL, "fw_chains_write_resample: only FW_RESAMPLE_FAMILY can be written (got %d)", what);
  const size_t need = sizeof(int32_t) * (size_t)c->n_chains;
  if (bytes < need || !src) return fail(FW_EINVAL, "the families need %zu bytes", need);
  const int32_t* f = static_cast<const int32_t*>(src);
  for (int i = 0; i < c->n_chains; ++i)
    if (f[i] < 0 || f[i] >= c->n_chains)
      return fail(FW_EINVAL, "family %d of chain %d outside [0, %d)", f[i], i, c->n_chains);
  HIPCHK(hipSetDevice(c->g->device));
  if (const int rc = rsm_ensure(c)) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(c->d_rsm_family, src, need, hipMemcpyHostToDevice));
  return FW_OK;
}

// ---------------------------------------------------------------- ensemble census
int fw_chains_enable_census(fw_chains* c, int32_t what) {
  const int32_t all = FW_CENSUS_NODES | FW_CENSUS_EDGES | FW_CENSUS_BOUNDARY;
  if (what <= 0 || (what & ~all))
    return fail(FW_EINVAL, "fw_chains_enable_census: mask %d is not a non-zero subset of %d", what, all);
  if (!c) return fail(FW_EINVAL, "fw_chains_enable_census: null");
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  CenBuild b;
  if (const int rc = cen_build(c, what, c->n_rungs ? c->n_rungs : 1, &b)) return rc;
  cen_adopt(c, b);
  return FW_OK;
}

int fw_chains_census_async(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (!c->cen.what) return fail(FW_ESTATE, "fw_chains_census_async: no census is enabled");
  HIPCHK(hipSetDevice(c->g->device));
  FwCensusParams p = c->cen;
  p.labels = c->d_labels;
  p.lab_stride = c->p.lab_stride;
  p.rowptr = c->g->d_rowptr;
  p.chain_of = c->n_rungs ? c->d_chain_of : nullptr;
  // like the exchange, record and tally steps: the run timing events are left alone
  int le = fw_launch_census(p, c->stream);
  if (le != 0)
    return fail(FW_EHIP, "census launch failed: %s", hipGetErrorString((hipError_t)le));
  FwCensusAddParams a{};
  a.part = c->d_cen_part;
  a.acc = c->d_cen_acc;
  a.size = p.size;
  a.n_groups = p.n_groups;
  a.spg = p.spg;
  le = fw_launch_census_add(a, c->stream);
  if (le != 0)
    return fail(FW_EHIP, "census sum launch failed: %s", hipGetErrorString((hipError_t)le));
  c->cen_measured += 1;
  return FW_OK;
}

int fw_chains_read_census(fw_chains* c, int32_t what, void* dst, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_read_census: null");
  int64_t off = 0, len = 0;
  if (const int rc = cen_array(c, what, &off, &len)) return rc;
  const size_t row = sizeof(uint64_t) * (size_t)len, need = row * (size_t)c->cen.n_groups;
  if (bytes < need || !dst) return fail(FW_EINVAL, "the census array needs %zu bytes", need);
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (row)
    HIPCHK(hipMemcpy2D(dst, row, c->d_cen_acc + off, sizeof(uint64_t) * (size_t)c->cen.size, row,
                       (size_t)c->cen.n_groups, hipMemcpyDeviceToHost));
  return FW_OK;
}

int fw_chains_write_census(fw_chains* c, int32_t what, const void* src, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_write_census: null");
  int64_t off = 0, len = 0;
  if (const int rc = cen_array(c, what, &off, &len)) return rc;
  const size_t row = sizeof(uint64_t) * (size_t)len, need = row * (size_t)c->cen.n_groups;
  if (bytes < need || !src) return fail(FW_EINVAL, "the census array needs %zu bytes", need);
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (row)
    HIPCHK(hipMemcpy2D(c->d_cen_acc + off, sizeof(uint64_t) * (size_t)c->cen.size, src, row, row,
                       (size_t)c->cen.n_groups, hipMemcpyHostToDevice));
  return FW_OK;
}

int fw_chains_census_reset(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (c->d_cen_acc) {
    HIPCHK(hipSetDevice(c->g->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemset(c->d_cen_acc, 0,
                     sizeof(uint64_t) * (size_t)c->cen.n_groups * (size_t)c->cen.size));
  }
  c->cen_measured = 0;
  return FW_OK;
}

int fw_chains_census_info(const fw_chains* c, int64_t info[5]) {
  if (!c || !info) return fail(FW_EINVAL, "fw_chains_census_info: null");
  info[0] = c->cen.what;
  info[1] = c->lb;
  info[2] = c->n_rungs ? c->n_rungs : 1;
  info[3] = c->g->nnz / 2;
  info[4] = c->cen_measured;
  return FW_OK;
}

// ---------------------------------------------------------------- node co-assignment
int fw_chains_enable_coassign(fw_chains* c, const int32_t* nodes, int32_t m) {
  if (!c) return fail(FW_EINVAL, "fw_chains_enable_coassign: null handle");
  const int n = c->g->n;
  std::vector<int32_t> list;
  if (!nodes) {
    list.resize((size_t)n);
    for (int v = 0; v < n; ++v) list[v] = v;
  } else {
    if (m < 1) return fail(FW_EINVAL, "fw_chains_enable_coassign: m = %d < 1", m);
    for (int j = 0; j < m; ++j) {
      if (nodes[j] < 0 || nodes[j] >= n)
        return fail(FW_EINVAL, "fw_chains_enable_coassign: node %d at %d outside [0, %d)", nodes[j], j, n);
      if (j && nodes[j] <= nodes[j - 1])
        return fail(FW_EINVAL, "fw_chains_enable_coassign: the list is not strictly ascending at %d", j);
    }
    list.assign(nodes, nodes + m);
  }
  const int n_groups = c->n_rungs ? c->n_rungs : 1;
  if ((int64_t)n_groups * (int64_t)list.size() * (int64_t)list.size() > FW_COA_MAX_ELEMS)
    return fail(FW_EUNSUPPORTED, "fw_chains_enable_coassign: %d groups x %zu x %zu nodes exceed 2^28 elements",
                n_groups, list.size(), list.size());
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  CoaBuild b;
  if (const int rc = coa_build(c, list, n_groups, &b)) return rc;
  coa_adopt(c, b, list);
  return FW_OK;
}

int fw_chains_coassign_async(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (!c->coa.m) return fail(FW_ESTATE, "fw_chains_coassign_async: co-assignment is not enabled");
  HIPCHK(hipSetDevice(c->g->device));
  FwCoassignParams p = c->coa;
  p.labels = c->d_labels;
  p.lab_stride = c->p.lab_stride;
  p.chain_of = c->n_rungs ? c->d_chain_of : nullptr;
  // like the exchange, record, tally and census steps: the run timing events are left alone
  int le = fw_launch_coassign_transpose(p, c->stream);
  if (le != 0)
    return fail(FW_EHIP, "coassign transpose launch failed: %s", hipGetErrorString((hipError_t)le));
  le = fw_launch_coassign_product(p, c->stream);
  if (le != 0)
    return fail(FW_EHIP, "coassign product launch failed: %s", hipGetErrorString((hipError_t)le));
  c->coa_measured += 1;
  return FW_OK;
}

int fw_chains_read_coassign(fw_chains* c, int32_t what, void* dst, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_read_coassign: null");
  if (!c->coa.m) return fail(FW_ESTATE, "fw_chains_read_coassign: co-assignment is not enabled");
  const FwCoassignParams& p = c->coa;
  size_t need = 0;
  switch (what) {
    case FW_COASSIGN_TOGETHER: need = coa_together_bytes(p); break;
    case FW_COASSIGN_CNT: need = sizeof(uint64_t) * (size_t)p.n_groups; break;
    case FW_COASSIGN_NODES: need = sizeof(int32_t) * (size_t)p.m; break;
    default: return fail(FW_EINVAL, "unknown coassign array %d", what);
  }
  if (bytes < need || !dst) return fail(FW_EINVAL, "the coassign array needs %zu bytes", need);
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (what == FW_COASSIGN_NODES)
    std::memcpy(dst, c->coa_nodes.data(), need);
  else
    HIPCHK(hipMemcpy(dst, what == FW_COASSIGN_TOGETHER ? (const void*)p.together : (const void*)p.cnt,
                     need, hipMemcpyDeviceToHost));
  return FW_OK;
}

int fw_chains_write_coassign(fw_chains* c, int32_t what, const void* src, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_write_coassign: null");
  if (!c->coa.m) return fail(FW_ESTATE, "fw_chains_write_coassign: co-assignment is not enabled");
  const FwCoassignParams& p = c->coa;
  size_t need = 0;
  switch (what) {
    case FW_COASSIGN_TOGETHER: need = coa_together_bytes(p); break;
    case FW_COASSIGN_CNT: need = sizeof(uint64_t) * (size_t)p.n_groups; break;
    case FW_COASSIGN_NODES:
      return fail(FW_EINVAL, "fw_chains_write_coassign: the node list is set by fw_chains_enable_coassign");
    default: return fail(FW_EINVAL, "unknown coassign array %d", what);
  }
  if (bytes < need || !src) return fail(FW_EINVAL, "the coassign array needs %zu bytes", need);
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(what == FW_COASSIGN_TOGETHER ? (void*)p.together : (void*)p.cnt, src, need,
                   hipMemcpyHostToDevice));
  return FW_OK;
}

int fw_chains_coassign_reset(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (c->coa.m) {
    HIPCHK(hipSetDevice(c->g->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemset(c->coa.together, 0, coa_together_bytes(c->coa)));
    HIPCHK(hipMemset(c->coa.cnt, 0, sizeof(uint64_t) * (size_t)c->coa.n_groups));
  }
  c->coa_measured = 0;
  return FW_OK;
}

int fw_chains_coassign_info(const fw_chains* c, int64_t info[7]) {
  if (!c || !info) return fail(FW_EINVAL, "fw_chains_coassign_info: null");
  info[0] = c->coa.m;
  info[1] = c->lb;
  info[2] = c->n_rungs ? c->n_rungs : 1;
  info[3] = c->coa_measured;
  info[4] = c->coa.tile;
  info[5] = c->coa.chunk;
  info[6] = c->coa.staged;
  return FW_OK;
}

// ---------------------------------------------------------------- pairwise plan distances
namespace {

size_t pwd_hist_bytes(const fw_chains* c) {
  return sizeof(unsigned long long) * ((size_t)c->g->n + 1);
}

int pwd_ensure_hist(fw_chains* c) {
  if (c->d_pwd_hist) return FW_OK;
  void* h = nullptr;
  if (hipMalloc(&h, pwd_hist_bytes(c)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FW_ENOMEM, "pair-distance histogram of %d bins", c->g->n + 1);
  }
  if (hipMemset(h, 0, pwd_hist_bytes(c)) != hipSuccess) {
    (void)hipFree(h);
    return fail(FW_EHIP, "the pair-distance histogram could not be zeroed");
  }
  c->d_pwd_hist = static_cast<unsigned long long*>(h);
  return FW_OK;
}

// *buf holds at least `want` bytes afterwards.  The new buffer is allocated before the old one
// is let go, so on failure the handle keeps what it had; a kernel in flight may still use the
// old one, so the stream is waited for before it is freed (only when a buffer grows).
int pwd_grow(fw_chains* c, void** buf, size_t* cap, size_t want, size_t unit, const char* what) {
  if (*cap >= want) return FW_OK;
  void* nb = nullptr;
  if (hipMalloc(&nb, want * unit) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FW_ENOMEM, "pair distances: %s of %zu elements", what, want);
  }
  if (*buf) {
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
      (void)hipFree(nb);
      return fail(FW_EHIP, "pair distances: the stream could not be waited for");
    }
    (void)hipFree(*buf);
  }
  *buf = nb;
  *cap = want;
  return FW_OK;
}

// a list -> the device on the handle's stream through a pinned slot: the host waits only for
// the copy that last used the slot, never for the stream
int pwd_upload(fw_chains* c, int32_t* dst, const int32_t* src, int32_t m) {
  const int s = c->pwd_slot;
  const size_t bytes = sizeof(int32_t) * (size_t)m;
  if (!c->pwd_ev[s] &&
      hipEventCreateWithFlags(&c->pwd_ev[s], hipEventDisableTiming) != hipSuccess) {
    c->pwd_ev[s] = nullptr;
    (void)hipGetLastError();
    return fail(FW_ENOMEM, "pair distances: no event for a staging slot");
  }
  HIPCHK(hipEventSynchronize(c->pwd_ev[s]));
  if (c->pwd_stage_cap[s] < bytes) {
    void* ns = nullptr;
    if (hipHostMalloc(&ns, bytes, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(FW_ENOMEM, "pair distances: a pinned slot of %zu bytes", bytes);
    }
    if (c->pwd_stage[s]) (void)hipHostFree(c->pwd_stage[s]);
    c->pwd_stage[s] = ns;
    c->pwd_stage_cap[s] = bytes;
  }
  c->pwd_slot ^= 1;
  std::memcpy(c->pwd_stage[s], src, bytes);
  HIPCHK(hipMemcpyAsync(dst, c->pwd_stage[s], bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipEventRecord(c->pwd_ev[s], c->stream));
  return FW_OK;
}

int pwd_bytes(const fw_chains* c, int32_t what, size_t* need) {
  switch (what) {
    case FW_PAIRDIST_MATRIX: *need = sizeof(int32_t) * (size_t)c->pwd_ma * (size_t)c->pwd_mb; return FW_OK;
    case FW_PAIRDIST_ROWSUM: *need = sizeof(int64_t) * (size_t)c->pwd_ma; return FW_OK;
    case FW_PAIRDIST_NEAREST: *need = sizeof(int32_t) * 2 * (size_t)c->pwd_ma; return FW_OK;
    case FW_PAIRDIST_HIST: *need = pwd_hist_bytes(c); return FW_OK;
    default: return fail(FW_EINVAL, "unknown pair-distance kind %d", what);
  }
}

}  // namespace

int fw_chains_pairdist_async(fw_chains* c, const int32_t* a, int32_t ma, const int32_t* b,
                             int32_t mb) {
  if (!c) return fail(FW_EINVAL, "fw_chains_pairdist_async: null handle");
  if (!a) return fail(FW_EINVAL, "fw_chains_pairdist_async: null list a");
  if (ma < 1) return fail(FW_EINVAL, "fw_chains_pairdist_async: ma = %d < 1", ma);
  if (b && mb < 1) return fail(FW_EINVAL, "fw_chains_pairdist_async: mb = %d < 1", mb);
  const bool sym = !b;
  if (sym) mb = ma;
  for (int i = 0; i < ma; ++i)
    if (a[i] < 0 || a[i] >= c->n_chains)
      return fail(FW_EINVAL, "a[%d] = %d outside [0, %d)", i, a[i], c->n_chains);
  for (int j = 0; b && j < mb; ++j)
    if (b[j] < 0 || b[j] >= c->n_chains)
      return fail(FW_EINVAL, "b[%d] = %d outside [0, %d)", j, b[j], c->n_chains);
  if ((int64_t)ma * mb > FW_PWD_MAX_PAIRS)
    return fail(FW_EUNSUPPORTED, "%d x %d pairs > 2^28", ma, mb);
  HIPCHK(hipSetDevice(c->g->device));
  if (const int rc = pwd_ensure_hist(c)) return rc;
  if (const int rc = pwd_grow(c, (void**)&c->d_pwd_list[0], &c->pwd_list_cap[0], (size_t)ma,
                              sizeof(int32_t), "list a"))
    return rc;
  if (!sym)
    if (const int rc = pwd_grow(c, (void**)&c->d_pwd_list[1], &c->pwd_list_cap[1], (size_t)mb,
                                sizeof(int32_t), "list b"))
      return rc;
  if (const int rc = pwd_grow(c, (void**)&c->d_pwd_D, &c->pwd_D_cap, (size_t)ma * (size_t)mb,
                              sizeof(int32_t), "matrix"))
    return rc;
  if (c->pwd_row_cap < (size_t)ma) {
    // both row arrays or neither: the second is grown first under its own count
    size_t cap_near = c->pwd_row_cap, cap_sum = c->pwd_row_cap;
    if (const int rc = pwd_grow(c, (void**)&c->d_pwd_near, &cap_near, (size_t)ma,
                                2 * sizeof(int32_t), "nearest"))
      return rc;
    if (const int rc = pwd_grow(c, (void**)&c->d_pwd_rowsum, &cap_sum, (size_t)ma,
                                sizeof(int64_t), "row sums")) {
      // nearest is larger than recorded, which is harmless
      return rc;
    }
    c->pwd_row_cap = (size_t)ma;
  }
  if (const int rc = pwd_upload(c, c->d_pwd_list[0], a, ma)) return rc;
  if (!sym)
    if (const int rc = pwd_upload(c, c->d_pwd_list[1], b, mb)) return rc;
  const FwPwdPlan q = fw_pwd_plan(c->g->n, c->lb, fw_pairdist_env("FLIPWALK_PWD_TILE"),
                                  fw_pairdist_env("FLIPWALK_PWD_CHUNK"));
  FwPairdistParams p{};
  p.labels = c->d_labels;
  p.lab_stride = c->p.lab_stride;
  p.a = c->d_pwd_list[0];
  p.b = sym ? c->d_pwd_list[0] : c->d_pwd_list[1];
  p.D = c->d_pwd_D;
  p.ma = ma;
  p.mb = mb;
  p.symmetric = sym ? 1 : 0;
  p.n = c->g->n;
  p.lb = c->lb;
  p.lab_words = (int)(((int64_t)c->g->n * c->lb + 31) / 32);
  p.tile = q.tile;
  p.chunk = q.chunk;
  p.rs = q.rs;
  p.n_chunks = q.n_chunks;
  p.lds_bytes = q.lds_bytes;
  // like the exchange, record, tally and census steps: the run timing events are left alone
  int le = fw_launch_pairdist(p, c->stream);
  if (le != 0)
    return fail(FW_EHIP, "pair-distance launch failed: %s", hipGetErrorString((hipError_t)le));
  FwPairdistReduceParams r{};
  r.D = c->d_pwd_D;
  r.rowsum = c->d_pwd_rowsum;
  r.nearest = c->d_pwd_near;
  r.hist = c->d_pwd_hist;
  r.ma = ma;
  r.mb = mb;
  r.symmetric = p.symmetric;
  r.n = p.n;
  r.lds_bins = p.n + 1 <= 12288 ? p.n + 1 : 0;
  le = fw_launch_pairdist_reduce(r, c->stream);
  if (le != 0)
    return fail(FW_EHIP, "pair-distance reduction launch failed: %s",
                hipGetErrorString((hipError_t)le));
  c->pwd_have = true;
  c->pwd_sym = sym;
  c->pwd_ma = ma;
  c->pwd_mb = mb;
  c->pwd_tile = q.tile;
  c->pwd_chunk = q.chunk;
  c->pwd_measured += 1;
  return FW_OK;
}

int fw_chains_read_pairdist(fw_chains* c, int32_t what, void* dst, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_read_pairdist: null");
  size_t need = 0;
  if (const int rc = pwd_bytes(c, what, &need)) return rc;
  if (what != FW_PAIRDIST_HIST && !c->pwd_have)
    return fail(FW_ESTATE, "fw_chains_read_pairdist: nothing has been measured yet");
  if (bytes < need || !dst) return fail(FW_EINVAL, "the pair distances need %zu bytes", need);
  if (what == FW_PAIRDIST_HIST && !c->d_pwd_hist) {  // never measured, never written: all zero
    std::memset(dst, 0, need);
    return FW_OK;
  }
  HIPCHK(hipSetDevice(c->g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const void* src = what == FW_PAIRDIST_MATRIX   ? (const void*)c->d_pwd_D
                    : what == FW_PAIRDIST_ROWSUM ? (const void*)c->d_pwd_rowsum
                    : what == FW_PAIRDIST_NEAREST ? (const void*)c->d_pwd_near
                                                  : (const void*)c->d_pwd_hist;
  HIPCHK(hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
  return FW_OK;
}

int fw_chains_write_pairdist(fw_chains* c, int32_t what, const void* src, size_t bytes) {
  if (!c) return fail(FW_EINVAL, "fw_chains_write_pairdist: null");
  if (what != FW_PAIRDIST_HIST)
    return fail(FW_EINVAL, "fw_chains_write_pairdist: only FW_PAIRDIST_HIST can be written (got %d)", what);
  const size_t need = pwd_hist_bytes(c);
  if (bytes < need || !src) return fail(FW_EINVAL, "the pair-distance histogram needs %zu bytes", need);
  HIPCHK(hipSetDevice(c->g->device));
  if (const int rc = pwd_ensure_hist(c)) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(c->d_pwd_hist, src, need, hipMemcpyHostToDevice));
  return FW_OK;
}

int fw_chains_pairdist_reset(fw_chains* c) {
  if (!c) return fail(FW_EINVAL, "null handle");
  if (c->d_pwd_hist) {
    HIPCHK(hipSetDevice(c->g->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemset(c->d_pwd_hist, 0, pwd_hist_bytes(c)));
  }
  c->pwd_measured = 0;
  return FW_OK;
}

int fw_chains_pairdist_info(const fw_chains* c, int64_t info[7]) {
  if (!c || !info) return fail(FW_EINVAL, "fw_chains_pairdist_info: null");
  const FwPwdPlan q = fw_pwd_plan(c->g->n, c->lb, fw_pairdist_env("FLIPWALK_PWD_TILE"),
                                  fw_pairdist_env("FLIPWALK_PWD_CHUNK"));
  info[0] = c->pwd_ma;
  info[1] = c->pwd_mb;
  info[2] = c->pwd_sym ? 1 : 0;
  info[3] = c->lb;
  info[4] = c->pwd_measured;
  info[5] = c->pwd_have ? c->pwd_tile : q.tile;
  info[6] = c->pwd_have ? c->pwd_chunk : q.chunk;
  return FW_OK;
}

int fw_chains_enable_ring(fw_chains* c, const int32_t* ring_u, const int32_t* ring_w,
                          int32_t n_ring) {
  if (!c || !ring_u || !ring_w) return fail(FW_EINVAL, "fw_chains_enable_ring: null");
  if (n_ring < 2 || n_ring > 1024) return fail(FW_EINVAL, "n_ring = %d outside [2, 1024]", n_ring);
  const fw_graph* g = c->g;
  std::vector<uint8_t> node((size_t)g->n, 0);
  for (int r = 0; r < n_ring; ++r) {
    const int u = ring_u[r], w = ring_w[r];
    if (u < 0 || u >= g->n || w < 0 || w >= g->n ||
        !std::binary_search(g->col.begin() + g->rowptr[u], g->col.begin() + g->rowptr[u + 1], w))
      return fail(FW_EINVAL, "ring edge %d (%d, %d) is not an edge of the graph", r, u, w);
    node[u] = node[w] = 1;
  }
  HIPCHK(hipSetDevice(g->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (!c->d_ring_node && hipMalloc(&c->d_ring_node, (size_t)g->n) != hipSuccess)
    return fail(FW_ENOMEM, "ring node flags");
  // the new buffers first: on failure the handle keeps its previous ring intact
  int32_t* d_ring = nullptr;
  unsigned long long* d_hist = nullptr;
  if (hipMalloc(&d_ring, sizeof(int32_t) * 2 * (size_t)n_ring) != hipSuccess ||
      hipMalloc(&d_hist, sizeof(unsigned long long) * ring_bins(n_ring)) != hipSuccess) {
    if (d_ring) (void)hipFree(d_ring);
    return fail(FW_ENOMEM, "ring histogram of %d edges", n_ring);
  }
  if (c->d_ring) (void)hipFree(c->d_ring);
  if (c->d_hist_ring) (void)hipFree(c->d_hist_ring);
  c->d_ring = d_ring;
  c->d_hist_ring = d_hist;
  c->ring_u.assign(ring_u, ring_u + n_ring);
  c->ring_w.assign(ring_w, ring_w + n_ring);
  c->ring_n = n_ring;
  HIPCHK(hipMemcpy(c->d_ring, ring_u, sizeof(int32_t) * n_ring, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->d_ring + n_ring, ring_w, sizeof(int32_t) * n_ring, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->d_ring_node, node.data(), node.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(c->d_hist_ring, 0, sizeof(unsigned long long) * ring_bins(n_ring)));
  c->p.ring_n = n_ring;
  c->p.ring_u = c->d_ring;
  c->p.ring_w = c->d_ring + n_ring;
  c->p.ring_node = c->d_ring_node;
  c->p.hist_ring = c->d_hist_ring;
  return FW_OK;
}

int fw_chains_read_map(fw_chains* c, int32_t what, int32_t chain0, int32_t n_chains, int32_t flags,
                       int64_t* dst, size_t bytes) {
  if (!c || !dst) return fail(FW_EINVAL, "fw_chains_read_map: null");
  if (!c->d_acc) return fail(FW_ESTATE, "spatial maps are not enabled");
  if (what < FW_MAP_CUT_TIMES || what > FW_MAP_LAST_FLIPPED)
    return fail(FW_EINVAL, "unknown map %d", what);
  if (chain0 < 0 || n_chains <= 0 || (int64_t)chain0 + n_chains > c->n_chains)
    return fail(FW_EINVAL, "chain range [%d, %d) outside [0, %d)", chain0, chain0 + n_chains,
                c->n_chains);
  const int E = c->g->nnz / 2, n = c->g->n;
  const size_t M = what == FW_MAP_CUT_TIMES ? (size_t)E : (size_t)n;
  const bool sum = (flags & FW_MAP_SUM) != 0;
  const size_t need = sizeof(int64_t) * M * (sum ? 1 : (size_t)n_chains);
  if (bytes < need) return fail(FW_EINVAL, "map needs %zu bytes", need);
  if (M == 0) return FW_OK;
  HIPCHK(hipSetDevice(c->g->device));
  int64_t* d_out = nullptr;
  HIPCHK(hipMalloc(&d_out, need));
  FwMapRead m{};
  m.acc = c->d_acc;
  m.nf = c->d_nf;
  m.lf = c->d_lf;
  m.ps = c->d_ps;
  m.pend = c->d_pend;
  m.labval = c->d_labval;
  m.labels = c->d_labels;
  m.lab_stride = c->p.lab_stride;
  m.stats = c->d_stats;
  m.eu = c->g->d_eu;
  m.ew = c->g->d_ew;
  m.n = n;
  m.E = E;
  m.lb = c->lb;
  m.what = what;
  m.sum = sum ? 1 : 0;
  m.finalize = (flags & FW_MAP_FINALIZE) ? 1 : 0;
  m.chain0 = chain0;
  m.n_chains = n_chains;
  m.out = d_out;
  int rc = FW_OK;
  const int le = fw_launch_map_read(m, c->stream);
  if (le != 0)
    rc = fail(FW_EHIP, "map read launch failed: %s", hipGetErrorString((hipError_t)le));
  else if (hipMemcpyAsync(dst, d_out, need, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
           hipStreamSynchronize(c->stream) != hipSuccess)
    rc = fail(FW_EHIP, "map download failed");
  (void)hipFree(d_out);
  return rc;
}

int fw_eval_flips(fw_graph* g, const int16_t* labels, int32_t k, const int32_t* v,
                  const int16_t* target, int32_t m, int64_t pop_lo, int64_t pop_hi, int32_t* dcut,
                  uint8_t* contig, uint8_t* pop_ok, int32_t* dboundary) {
  if (!g || !labels || (m > 0 && (!v || !target || !dcut || !contig || !pop_ok || !dboundary)) ||
      m < 0)
    return fail(FW_EINVAL, "fw_eval_flips: bad arguments");
  if (m == 0) return FW_OK;
  if (k < 2 || k > FW_MAX_K) return fail(FW_EUNSUPPORTED, "k=%d outside [2, %d]", k, FW_MAX_K);
  if (g->maxdeg > FW_MAX_DEG) return fail(FW_EUNSUPPORTED, "max degree %d", g->maxdeg);
  const int lb = pick_lb(k, g->maxdeg);
  if (!lb) return fail(FW_EUNSUPPORTED, "k + maxdeg too large");
  const int n = g->n;
  std::vector<int64_t> pops(k, 0);
  for (int x = 0; x < n; ++x) {
    if (labels[x] < 0 || labels[x] >= k) return fail(FW_EINVAL, "label out of range at %d", x);
    pops[labels[x]] += g->popof(x);
  }
  for (int i = 0; i < m; ++i) {
    if (v[i] < 0 || v[i] >= n || target[i] < 0 || target[i] >= k || target[i] == labels[v[i]])
      return fail(FW_EINVAL, "flip %d (v=%d, target=%d) is not a relabelling", i, v[i], target[i]);
  }
  FwEvalParams p{};
  p.qcap = list_cap(256);
  p.lab_bytes = round16(((int64_t)n * lb + 7) / 8);
  p.off_list = p.lab_bytes;
  p.lds_bytes = p.off_list + p.qcap * 4;
  if (p.lds_bytes > 160 * 1024 - 64) return fail(FW_EUNSUPPORTED, "graph too large for LDS");
  std::vector<uint8_t> packed(p.lab_bytes);
  pack_labels(labels, n, lb, packed.data(), p.lab_bytes);
  HIPCHK(hipSetDevice(g->device));
  const int grid = std::min(m, 2048);
  uint8_t* d_lab = nullptr;
  int64_t* d_pops = nullptr;
  int32_t *d_v = nullptr, *d_dcut = nullptr, *d_db = nullptr;
  int16_t* d_t = nullptr;
  uint8_t *d_contig = nullptr, *d_pok = nullptr;
  uint32_t* d_spill = nullptr;
  bool ok = hipMalloc(&d_lab, p.lab_bytes) == hipSuccess &&
            hipMalloc(&d_pops, sizeof(int64_t) * k) == hipSuccess &&
            hipMalloc(&d_v, sizeof(int32_t) * m) == hipSuccess &&
            hipMalloc(&d_t, sizeof(int16_t) * m) == hipSuccess &&
            hipMalloc(&d_dcut, sizeof(int32_t) * m) == hipSuccess &&
            hipMalloc(&d_db, sizeof(int32_t) * m) == hipSuccess &&
            hipMalloc(&d_contig, m) == hipSuccess && hipMalloc(&d_pok, m) == hipSuccess &&
            hipMalloc(&d_spill, sizeof(uint32_t) * (size_t)grid * n) == hipSuccess;
  int rc = FW_OK;
  if (!ok) {
    rc = fail(FW_ENOMEM, "device allocation failed in fw_eval_flips");
  } else {
    ok = hipMemcpy(d_lab, packed.data(), p.lab_bytes, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_pops, pops.data(), sizeof(int64_t) * k, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_v, v, sizeof(int32_t) * m, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_t, target, sizeof(int16_t) * m, hipMemcpyHostToDevice) == hipSuccess;
    p.g = g->dev();
    p.labels = d_lab;
    p.pops = d_pops;
    p.k = k;
    p.m = m;
    p.v = d_v;
    p.target = d_t;
    p.pop_lo = pop_lo;
    p.pop_hi = pop_hi;
    p.dcut = d_dcut;
    p.contig = d_contig;
    p.pop_ok = d_pok;
    p.dboundary = d_db;
    p.spill = d_spill;
    if (!ok) {
      rc = fail(FW_EHIP, "upload failed in fw_eval_flips");
    } else if (const int le = fw_launch_eval(p, lb, grid, nullptr)) {
      rc = fail(FW_EHIP, "eval launch failed: %s", hipGetErrorString((hipError_t)le));
    } else if (hipDeviceSynchronize() != hipSuccess) {
      rc = fail(FW_EHIP, "eval kernel failed: %s", hipGetErrorString(hipGetLastError()));
    } else {
      ok = hipMemcpy(dcut, d_dcut, sizeof(int32_t) * m, hipMemcpyDeviceToHost) == hipSuccess &&
           hipMemcpy(dboundary, d_db, sizeof(int32_t) * m, hipMemcpyDeviceToHost) == hipSuccess &&
           hipMemcpy(contig, d_contig, m, hipMemcpyDeviceToHost) == hipSuccess &&
           hipMemcpy(pop_ok, d_pok, m, hipMemcpyDeviceToHost) == hipSuccess;
      if (!ok) rc = fail(FW_EHIP, "download failed in fw_eval_flips");
    }
  }
  void* bufs[] = {d_lab, d_pops, d_v, d_t, d_dcut, d_db, d_contig, d_pok, d_spill};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  return rc;
}

}  // extern "C"
