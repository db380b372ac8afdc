// fw_internal.h — structs shared by the host API (fw_api.hip) and the kernels
// (fw_kernels.hip).  Not part of the public ABI.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/flipwalk.h"

// Kernel-variant limits (checked on the host before any launch).
#define FW_MAX_DEG 63   // lanes 1..deg of one wave hold v's neighbours during commit
#define FW_MAX_K 64     // foreign-label sets are 64-bit masks
#define FW_HIST_PAD 64  // histogram window slack past the last bin
// counted steps per kernel launch: per-launch step counters and the per-step sums of
// degrees (<= 63) and boundary changes (<= 64) stay below 2^31 in 32 bits
#define FW_MAX_LAUNCH_STEPS (1ll << 25)

struct FwGraphDev {
  const int32_t* rowptr;  // [n+1]
  const int32_t* col;     // [nnz]
  const int32_t* eid;     // [nnz] canonical edge id of each CSR entry
  const uint64_t* nbadj;  // [nnz] entry (v, i): bit j set iff neighbours i and j of v are adjacent
  const int32_t* ell;     // [n][16] neighbours padded with -1 (general graphs, max degree <= 16)
  const int32_t* dbound;  // with ell: [n] max degree over x and its neighbours, then
                          // [ceil(n/64)] max degree in each 64-node group (row loop bounds)
  const int64_t* pop;     // [n] or nullptr (unit populations)
  const double* invb;     // [n+1] 1.0 / max(b, 1), correctly rounded (no fp64 divide per step)
  int32_t n, nedges, maxdeg;
  int32_t gw, gh;         // grid width/height (gw == 0: general CSR)
  uint64_t gmagic;        // ceil(2^42 / gw): x / gw == (x * gmagic) >> 42 for x < 2^21
  uint32_t gm32;          // ceil(2^32 / gw): x / gw == mulhi(x, gm32) for x * gw < 2^32
  uint32_t gm24, gs24;    // x / gw == umul24(x, gm24) >> gs24 for x < 2^15 (0: none found)
};

struct FwRunParams {
  FwGraphDev g;
  uint8_t* labels;             // packed LB-bit labels, chain c at labels + c*lab_stride
  int64_t lab_stride;          // bytes per chain (multiple of 16)
  fw_chain_stats* stats;       // [n_chains]
  int64_t* pops;               // [n_chains][k]
  const double* thr;           // [n_chains or 1][2*maxdeg+1]
  const uint64_t* thr53;       // same shape: ceil(thr * 2^53) clamped to 2^53 (u < thr <=>
                               // u * 2^53 < thr53 for CPython's 53-bit u)
  int32_t thr_stride;          // 0 (shared table) or 2*maxdeg+1
  // threshold schedule (fw_chains_set_schedule): when set, a proposal whose step_num
  // (accepted flips so far + 1) is t uses row clamp(t - sched_t0, 0, sched_rows - 1)
  const double* sched;         // [sched_rows][2*maxdeg+1] or null
  const uint64_t* sched53;     // the same rows in the integer form of thr53
  int64_t sched_t0;
  int32_t sched_rows;
  unsigned long long* hist_cut;  // [nedges+1+FW_HIST_PAD]
  unsigned long long* hist_b;    // [n+1+FW_HIST_PAD]
  uint32_t* spill;             // [grid][n] search-list spill
  uint32_t* gscr;              // race_search_gscr (5-bit labels, padded rows): [grid][n] 32-bit visit marks (zero)
  int32_t gscr_words;
  int32_t* next_chain;         // dynamic chain counter (zeroed before launch)
  int32_t* trace;              // optional [n_chains][steps]: v*64+target if accepted, -1 if not
  int32_t n_chains, k, mode, G;  // G = ceil(n/64) weight groups
  int64_t pop_lo, pop_hi;
  uint64_t seed;
  int64_t chain_id0;
  int64_t steps;
  int32_t max_retries;
  uint32_t fold_at;             // n_sdeg at which attempt-driven 32-bit counters fold (2^31)
  int32_t qcap;                // search-list entries held in LDS
  // LDS layout (bytes from the dynamic shared base)
  int32_t lab_bytes;           // packed label bytes (multiple of 16)
  int32_t off_gsum, off_list, lds_bytes;
  // chain kernel on padded rows, pairs proposals: 2-bit per-node proposal weights at off_w
  // (between the labels and the group sums), saturated at 3 (wb = 2; 0: none)
  int32_t off_w, wb;
  int32_t off_ssum;            // grid kernel, large grids: supergroup sums in the slot
  int32_t lb;                  // label bits per node (2, 4 or 8)
  int32_t use16;               // 1: launch the four-chains-per-wave grid kernel
  // grid kernel LDS plan (fw_grid16_plan): 4*nw chain slots, shared scratch and list
  int32_t slot_stride;         // bytes between chain slots
  int32_t nw;                  // waves per workgroup (of the plan's lean kernel)
  int32_t spec;                // rows per chain of the lean kernel (speculative attempts: 1, 2, 4)
  int32_t w2;                  // 1: the lean R = 1 kernel under a 2-waves-per-SIMD register budget
                               // (launches with at most 2 waves of work per SIMD: fw_grid16_plan)
  int32_t off_scr, scr_bytes;  // 4-bit search scratch
  int32_t off_list16, qcap16;  // shared visit list
  int32_t no_bb;               // 1: exact searches skip the bitboard form (tests)
  int32_t no_rowbb;            // 1: large grids skip the row-parallel bitboard form (A/B)
  int32_t wpe5;                // 1: the 5-waves-per-SIMD chain-kernel instantiation
  int32_t lds16;               // dynamic LDS bytes per workgroup
  // derived-state cache.  A chain's HBM label record (lab_stride bytes) mirrors the start
  // of its LDS slot: labels, then the group sums (grid kernel: u16 pairs; chain kernel:
  // the padded u32 layout of gsum_slot).  Each launch writes the first
  // lab_copy16 16-B pieces back; when gcache_ok the next launch loads them all and takes
  // cut / bnodes / npairs from the stats record instead of re-deriving them from every
  // node's neighbourhood (host writes of labels or stats clear gcache_ok)
  int32_t lab_copy16;
  int32_t gcache_ok;
  // grid kernel work units: quads x slices (fw_grid16_kernel); seg_done [quads] counts a
  // quad's finished slices (zeroed before a launch with slices > 1)
  int32_t slices;
  int32_t* seg_done;
  // both kernels: a wave's priority level counts 2^-prio_shift of its unit's steps
  int32_t prio_shift;
  // spatial observables (nullptr: off).  Per chain c: acc [E] (int64: sum of -t when an
  // edge becomes cut and +t when it becomes uncut, so cut_times = acc + [cut now] * Y),
  // nf / lf [n] (num_flips, last_flipped of finished runs), ps [n] (part_sum), and the
  // pending run {node, district, first yield, -} of the current state's creating flip.
  int64_t* m_acc;
  uint32_t* m_nf;
  uint32_t* m_lf;
  int64_t* m_ps;
  int32_t* m_pend;
  const int64_t* m_labval;     // [k] GerryChain label values
  // accept rule (FW_ACCEPT_*); FW_ACCEPT_BOUNDARY: node flags and, per chain, the count
  // of flagged nodes in each district [n_chains][k]
  int32_t accept;
  const uint8_t* flags;
  int32_t* bcnt;
  // district-shape observable (fw_chains_enable_ring; ring_n == 0: off): ring edge r joins
  // ring_u[r] and ring_w[r]; ring_node[x] = 1 iff x is an endpoint of a ring edge; yields
  // counted per pair of first two cut ring edges, index i*ring_n + j (ring_n^2: < 2 cut)
  int32_t ring_n;
  const int32_t* ring_u;
  const int32_t* ring_w;
  const uint8_t* ring_node;
  unsigned long long* hist_ring;  // [ring_n^2 + 1]
  // sampled geometric waits (fw_chains_enable_waits; nullptr: off): per chain {sum over
  // yields, the current state's draw}; wlp [n+1] = log1p(-b / (N^k - 1)) (fw_math.h)
  double* wsamp;
  const double* wlp;
};

// fw_chains_read_map: finalise maps of a chain range (see include/flipwalk.h)
struct FwMapRead {
  const int64_t* acc;
  const uint32_t* nf;
  const uint32_t* lf;
  const int64_t* ps;
  const int32_t* pend;
  const int64_t* labval;
  const uint8_t* labels;
  int64_t lab_stride;
  const fw_chain_stats* stats;
  const int32_t* eu;  // [E] edge endpoints, canonical order
  const int32_t* ew;
  int32_t n, E, lb, what, sum, finalize;
  int32_t chain0, n_chains;
  int64_t* out;
};

struct FwEvalParams {
  FwGraphDev g;
  const uint8_t* labels;  // packed LB-bit labels of the one state
  int32_t lab_bytes;
  const int64_t* pops;    // [k] populations of the state
  int32_t k, m;
  const int32_t* v;
  const int16_t* target;
  int64_t pop_lo, pop_hi;
  int32_t* dcut;
  uint8_t* contig;
  uint8_t* pop_ok;
  int32_t* dboundary;
  uint32_t* spill;        // [grid][n]
  int32_t qcap;
  int32_t off_list, lds_bytes;
};

// fw_chains_exchange_async: the fields of a stats record the rung stats accumulate, as of
// the last exchange (or set_ladder / reset / stats write)
struct FwRungSnap {
  uint64_t yields, steps, accepts;
  int64_t sum_cut, sum_bnodes;
  double sum_invb;
};

// One replica-exchange step (see include/flipwalk.h); set s holds chains chain_of[s][0..n_rungs)
struct FwExchangeParams {
  const fw_chain_stats* stats;  // [n_chains]
  FwRungSnap* snap;             // [n_chains]
  fw_rung_stats* rstats;        // [n_sets][n_rungs]
  double* thr;                  // [n_chains][row_len]: the run kernels' per-chain tables
  uint64_t* thr53;
  const double* lad_thr;        // [n_rungs][row_len]
  const uint64_t* lad_thr53;
  const double* log_base;       // [n_rungs]
  int32_t* rung;                // [n_chains]
  int32_t* chain_of;            // [n_sets][n_rungs]
  const int64_t* gmin;          // [n_sets] smallest global chain id of the set
  int32_t n_sets, n_rungs, row_len;
  uint32_t round;
  uint64_t seed;
};

// ---- thinned observable series (fw_chains_enable_series, fw_series.hip) ----------------
// Series buffers are sample-major int32 [capacity][n_chains]: a wave's 64 lanes touch 64
// adjacent chains of one sample (256 B).
#define FW_SERIES_MAX_LAG 1023
#define FW_ACF_CHUNK 32   // lags per wave of the autocovariance kernel
#define FW_ACF_WAVES 4    // waves (lag chunks) per workgroup, all on the same 64 series
#define FW_POOL_WIDTH 256 // sequential partials of the pooled sums

// fw_chains_record_async: sample `sample` of every chain
struct FwRecordParams {
  const fw_chain_stats* stats;  // [n_chains]
  const int32_t* rung;          // [n_chains] or null (no ladder: -1 is recorded)
  int32_t* cut;                 // [capacity][n_chains]
  int32_t* bnodes;
  int32_t* rung_out;            // null when no rung row is kept
  int32_t n_chains;
  int64_t sample;
};

// by-rung view of a window: out[t][set_of[c] * n_rungs + rung[t][c]] = x[t][c]
struct FwRegroupParams {
  const int32_t* x;       // window start, [n][n_chains]
  const int32_t* rung;    // window start, [n][n_chains]
  const int32_t* set_of;  // [n_chains]
  int32_t* out;           // [n][n_chains]
  int32_t n_chains, n_rungs;
  int64_t n;
};

// exact lagged sums of a window: sums[(k * (max_lag + 1) + l) * n_series + j], k = 0 (P),
// 1 (A), 2 (B) of include/flipwalk.h; lag-major on the device so that stores and the pooling
// loads are coalesced along the series index (the host transposes for per_series)
struct FwAcfParams {
  const int32_t* x;  // window start, [n][n_series]
  int64_t* sums;
  int32_t n_series, max_lag;
  int64_t n;
};

// pooled autocovariances: out[g][0..max_lag] = sum of c_j[l], out[g][max_lag+1] = sum of m_j,
// out[g][max_lag+2] = sum of m_j^2 over the members j = first + pos * stride, pos < members,
// of group g (first = g), in the order include/flipwalk.h states
struct FwPoolParams {
  const int64_t* sums;
  double* out;  // [n_groups][max_lag + 3]
  int32_t n_series, max_lag, members, stride;
  int64_t n;
};

// ---- district tallies of node columns (fw_chains_set_columns, fw_tally.hip) --------------
#define FW_TALLY_MAX_COLS 8
#define FW_TALLY_MAX_EL 4
#define FW_TALLY_MAX_GROUPS 64  // rungs of a ladder (fw_chains_set_ladder)
#define FW_TALLY_TILE 1024      // nodes of the columns staged in LDS at a time (a multiple of 64)
#define FW_TALLY_NW_REG 16      // waves (chains) per workgroup, register accumulators (k <= 8)
#define FW_TALLY_NW_BIN 8       // waves per workgroup with LDS bins (k <= 32; half of it above)
#define FW_SEATS_LDS_BINS 2048  // seat histograms up to this many bins are summed in LDS first

// fw_chains_tally_async: sums[c][j][d] = sum of column j over the nodes chain c labels d
struct FwTallyParams {
  const uint8_t* labels;  // packed lb-bit label records, chain c at labels + c * lab_stride
  int64_t lab_stride;     // bytes, a multiple of 16
  const uint32_t* cols;   // [ceil(n_cols / 2)][n][2]: columns 2p and 2p + 1 (zeros when absent)
  int64_t* sums;          // [n_chains][n_cols][k]
  int32_t n_chains, n, k, lb, n_cols;
};

// the seat step: seats[c][e] = {wins, ties} of election e = (ab[e][0], ab[e][1]) and
// hist[g][e][wins] += 1, g = rung[c] (0 without a ladder)
struct FwSeatsParams {
  const int64_t* sums;       // [n_chains][n_cols][k]
  const int32_t* rung;       // [n_chains] or null
  int32_t* seats;            // [n_chains][n_el][2]
  unsigned long long* hist;  // [n_groups][n_el][k + 1]
  int32_t ab[FW_TALLY_MAX_EL][2];
  int32_t n_chains, k, n_cols, n_el, n_groups;
};

// ---- per-district geometry (fw_chains_set_geometry, fw_geometry.hip) ---------------------
#define FW_GEOM_TILE 1024   // edges / nodes staged in LDS at a time (a multiple of 64)
#define FW_GEOM_MAX_NW 16   // waves (chains) per workgroup at the most

// the launch plan (fw_geometry_plan): dwords of a wave's resident label copy, the tile, the
// quantities binned per walk (0: register accumulators) and the waves per workgroup
struct FwGeomPlan {
  int32_t lab_words, tile, bins, nw, lds_bytes;
};

// fw_chains_geometry_async: out[c][d] = {nodes, cut edges, interior perimeter, exterior
// perimeter, area} of district d of chain c
struct FwGeomParams {
  const uint8_t* labels;  // packed lb-bit label records, chain c at labels + c * lab_stride
  int64_t lab_stride;     // bytes, a multiple of 16
  const int32_t* eu;      // [n_edges] canonical edge endpoints (u < w)
  const int32_t* ew;
  const uint32_t* ewt;    // [n_edges] edge weights, or null (unit weights: nothing is read)
  const uint32_t* area;   // [n] or null (1 each)
  const uint32_t* ext;    // [n] or null (0 each)
  int64_t* out;           // [n_chains][k][5]
  int32_t n_chains, n, n_edges, k, lb;
  int32_t lab_words, tile, bins, nw;  // FwGeomPlan
};

// hist[g][out[c][d][1]] += 1 for every district, g = rung[c] (0 without a ladder)
struct FwGeomHistParams {
  const int64_t* G;          // [n_chains][k][5]
  const int32_t* rung;       // [n_chains] or null
  unsigned long long* hist;  // [n_groups][n_edges + 1]
  int32_t n_chains, k, n_groups, n_edges;
};

// ---- plan overlap and Hamming distance (fw_chains_set_reference, fw_overlap.hip) ---------
#define FW_OVL_MAX_NW 16  // waves (chains) per workgroup at the most

// fw_chains_overlap_async: O[c][d][e] = #{v : R_c(v) = d and X_c(v) = e}, dist[c] = #{v : R_c(v)
// != X_c(v)}; X_c is the record of chain c, R_c the record of chain partner[c] when partner is
// set, else the reference row ref + c * ref_stride
struct FwOverlapParams {
  const uint8_t* labels;   // packed lb-bit label records, chain c at labels + c * lab_stride
  int64_t lab_stride;      // bytes, a multiple of 16
  const uint32_t* ref;     // [1 or n_chains][ref_stride] packed like the records
  int64_t ref_stride;      // dwords between reference rows, a multiple of 4 (0: one shared row)
  const int32_t* partner;  // [n_chains] or null (against ref)
  int64_t* O;              // [n_chains][k][k]
  int32_t* dist;           // [n_chains]
  int32_t n_chains, n, k, lb;
  int32_t lab_words;       // ceil(n lb / 32): the dwords of a record that hold labels
};

// hist[g][dist[c]] += 1, g = rung[c] (0 without a ladder)
struct FwOverlapHistParams {
  const int32_t* dist;       // [n_chains]
  const int32_t* rung;       // [n_chains] or null
  unsigned long long* hist;  // [n_groups][n + 1]
  int32_t n_chains, n_groups, n;
};

// ---- resampling plans across chains (fw_chains_clone_async, fw_resample.hip) ---------------
#define FW_RSM_THREADS 1024  // the one workgroup of the map kernel
#define FW_RSM_CLONE_NW 4    // waves (destination chains) per workgroup of the gather

// fw_chains_clone_async: chain i takes the plan of chain src[i] (a fixed point of src); what
// describes the plan moves, what describes the chain stays (include/flipwalk.h)
struct FwCloneParams {
  uint8_t* labels;        // label records, chain c at labels + c * lab_stride
  int64_t lab_stride;     // bytes, a multiple of 16
  fw_chain_stats* stats;  // [n_chains]: cut, bnodes, npairs, stuck move
  int64_t* pops;          // [n_chains][k]
  int32_t* bcnt;          // [n_chains][k] or null (FW_ACCEPT_BOUNDARY's flagged-node counts)
  double* wsamp;          // [n_chains][2] or null: the current state's draw [1] moves
  const int32_t* src;     // [n_chains]
  int32_t* family;        // [n_chains]
  int32_t n_chains, k;
};

// fw_chains_resample_async: the source map of one systematic resampling by cut.  info =
// {T, S2, cref, survivors, max offspring, clones (accumulated over the handle's resamples), u, -}
struct FwResampleParams {
  const fw_chain_stats* stats;  // [n_chains]
  const uint32_t* q;            // [n_edges + 1]
  uint32_t* w;                  // [n_chains] weights
  uint64_t* cum;                // [n_chains] inclusive prefix sums of w
  uint64_t* pts;                // [n_chains] the points p_j
  int32_t* lower;               // [n_chains] #{j : p_j < cum[i]}
  int32_t* extra;               // [n_chains] inclusive prefix sums of max(offspring - 1, 0)
  int32_t* src;                 // [n_chains] the map
  int64_t* info;                // [8]
  int32_t n_chains, n_edges, sign;
  uint32_t round;
  uint64_t seed;
  int64_t chain_id0;
};

// ---- ensemble census: maps over the graph, summed across chains (fw_census.hip) -------------
#define FW_CEN_TILE 256          // nodes of a tile by default (one lane each)
#define FW_CEN_MAX_TILE 1024     // and at the most: a workgroup's threads
#define FW_CEN_MAX_BATCH 16      // chains staged in LDS between two barriers at the most
#define FW_CEN_LDS_WORDS 16384   // dwords of LDS a workgroup may plan with (64 KB)
#define FW_CEN_TILE_INTS 8       // int32 per tile record

// fw_chains_census_async, first stage.  Workgroup (tile, slice) counts, over the chains of its
// slice, the nodes, upper edges and boundary flags of its tile and stores them as uint32 into
// row `slice` of part.  A tile record is {node0, nodes, entry0 (rowptr[node0]), entries, edge0
// (first canonical edge id with its lower endpoint in the tile), edges, wd0, wdn (the dwords
// [wd0, wd0 + wdn) of a record its nodes and their neighbours lie in; staged == 0: 0 and the
// record's label words)}.  ent[t] of CSR entry t = (v, w): (w lb - 32 wd0(tile of v)) << 1 |
// (w > v).  Slice sl = g spg + s holds the members [s slice_len, ..) of group g; member i of
// group g is chain chain_of[i n_groups + g] under a ladder, else chain i.
struct FwCensusParams {
  const uint8_t* labels;    // packed lb-bit label records, chain c at labels + c * lab_stride
  int64_t lab_stride;       // bytes, a multiple of 16
  const int32_t* rowptr;    // [n + 1]
  const int32_t* tiles;     // [n_tiles][FW_CEN_TILE_INTS]
  const uint32_t* ent;      // [nnz]
  const int32_t* ebase;     // [n] canonical id of the first edge (v, w > v) of row v
  const int32_t* chain_of;  // [per_group][n_groups] or null (no ladder)
  uint32_t* part;           // [n_groups * spg][size]
  int32_t n, k, lb, what, lab_words;
  int32_t n_tiles, n_groups, spg, slice_len, per_group;
  int32_t nt, staged, batch, wd_max;        // threads; the LDS staging of label windows
  int32_t off_ecut_lds, off_ent_lds, off_stage_lds, lds_bytes;  // dwords, dwords, dwords, bytes
  // a row of part and of the accumulators: cnt at 0, then the enabled parts (-1: absent)
  int64_t size, off_occ, off_ecut, off_bnd;
};

// second stage: acc[g][j] += sum over the slices s of group g of part[g spg + s][j]
struct FwCensusAddParams {
  const uint32_t* part;
  uint64_t* acc;  // [n_groups][size]
  int64_t size;
  int32_t n_groups, spg;
};

// Host-side launchers implemented in fw_census.hip.
int fw_census_env(const char* name);  // a test knob's value, -1 when unset
int fw_launch_census(const FwCensusParams& p, void* stream);
int fw_launch_census_add(const FwCensusAddParams& a, void* stream);

// ---- pairwise plan distances between two lists of chains (fw_pairdist.hip) ------------------
// fw_chains_pairdist_async, first kernel.  Workgroup (bx, by) owns the pairs of a-positions
// [by tile, ..) and b-positions [bx tile, ..); in the symmetric case (b is a) only bx >= by
// works, and an off-diagonal block also stores its transpose.  tile, chunk, rs: fw_pairdist_plan.h.
struct FwPairdistParams {
  const uint8_t* labels;   // packed lb-bit label records, chain c at labels + c * lab_stride
  int64_t lab_stride;      // bytes, a multiple of 16
  const int32_t* a;        // [ma] chain ids
  const int32_t* b;        // [mb] chain ids (== a when symmetric)
  int32_t* D;              // [ma][mb]
  int32_t ma, mb, symmetric;
  int32_t n, lb, lab_words;
  int32_t tile, chunk, rs, n_chunks, lds_bytes;
};

// second kernel: one wave per row of D.  lds_bins: n + 1 when the workgroup counts its rows'
// values in LDS before adding them to hist, 0 when it adds them to hist directly.
struct FwPairdistReduceParams {
  const int32_t* D;
  int64_t* rowsum;              // [ma]
  int32_t* nearest;             // [ma][2]
  unsigned long long* hist;     // [n + 1]
  int32_t ma, mb, symmetric, n, lds_bins;
};

// Host-side launchers implemented in fw_pairdist.hip.
int fw_pairdist_env(const char* name);  // a test knob's value, -1 when unset
int fw_launch_pairdist(const FwPairdistParams& p, void* stream);
int fw_launch_pairdist_reduce(const FwPairdistReduceParams& r, void* stream);

// ---- node co-assignment across the chains (fw_coassign.hip) ---------------------------------
// fw_chains_coassign_async.  First kernel: the labels of the listed nodes, transposed into bit
// planes across the members of each group, planes[g][word][plane][entry] (rows of ms dwords);
// workgroup (transpose tile, group, 64 nw members).  Second kernel: workgroup (bx, by, g) owns
// the entry pairs [by tile, ..) x [bx tile, ..) of group g; only bx >= by works, and an
// off-diagonal block also adds to the transposed element.  Member i of group g is chain
// chain_of[i n_groups + g] under a ladder, else chain i.  Blocking: fw_coassign_plan.h.
struct FwCoassignParams {
  const uint8_t* labels;    // packed lb-bit label records, chain c at labels + c * lab_stride
  int64_t lab_stride;       // bytes, a multiple of 16
  const int32_t* chain_of;  // [per_group][n_groups] or null (no ladder)
  const uint32_t* ebit;     // [m] bit offset of entry j's field in its tile's window
  const int32_t* twin;      // [n_ttiles][2] {wd0, wdn} of a transpose tile (not staged: unused)
  uint32_t* planes;         // [n_groups][n_words][lb][ms]
  uint64_t* together;       // [n_groups][m][m]
  uint64_t* cnt;            // [n_groups]
  int32_t m, ms, lb, lab_words, n_groups, per_group, n_words;
  int32_t n_ttiles, staged, nw, stride, t_lds_bytes;     // transpose
  int32_t tile, shift, chunk, rs, n_chunks, lds_bytes;   // product (FwCoaPlan)
};

// Host-side launchers implemented in fw_coassign.hip.
int fw_coassign_env(const char* name);  // a test knob's value, -1 when unset
int fw_launch_coassign_transpose(const FwCoassignParams& p, void* stream);
int fw_launch_coassign_product(const FwCoassignParams& p, void* stream);

// Host-side launchers implemented in fw_resample.hip.
int fw_launch_clone(const FwCloneParams& p, void* stream);
int fw_launch_resample_map(const FwResampleParams& p, void* stream);

// Host-side launchers implemented in fw_overlap.hip.
void fw_overlap_plan(int k, int* nw, int* lds_bytes);
int fw_launch_overlap(const FwOverlapParams& p, int nw, int lds_bytes, void* stream);
int fw_launch_overlap_hist(const FwOverlapHistParams& h, void* stream);

// Host-side launchers implemented in fw_geometry.hip.
void fw_geometry_plan(int n, int k, int lb, bool has_w, FwGeomPlan* out);
int fw_launch_geometry(const FwGeomParams& p, int lds_bytes, void* stream);
int fw_launch_geometry_hist(const FwGeomHistParams& h, void* stream);

// Host-side launchers implemented in fw_tally.hip.
void fw_tally_plan(int k, int lb, int* nw, int* lds_bytes);
int fw_launch_tally(const FwTallyParams& t, void* stream);
int fw_launch_seats(const FwSeatsParams& s, void* stream);

// Host-side launchers implemented in fw_series.hip.
int fw_launch_record(const FwRecordParams& r, void* stream);
int fw_launch_regroup(const FwRegroupParams& r, void* stream);
int fw_launch_acf(const FwAcfParams& a, void* stream);
int fw_launch_pool(const FwPoolParams& p, int n_groups, void* stream);

// Host-side launchers implemented in fw_kernels.hip.
int fw_launch_exchange(const FwExchangeParams& e, void* stream);
int fw_launch_map_init(const FwRunParams& p, void* stream);
int fw_launch_map_read(const FwMapRead& m, void* stream);
int fw_launch_bcnt_init(const FwRunParams& p, void* stream);
int fw_launch_run(const FwRunParams& p, int lb, int grid, void* stream);
int fw_launch_eval(const FwEvalParams& p, int lb, int grid, void* stream);
int fw_run_grid_size(FwRunParams& p, int lb, int device, int* grid);
int fw_run_gsum_slots(int G);  // u16 group-sum slots of the chain kernel
// fw_grid16.hip
bool fw_grid16_candidate(int gw, int maxdeg, int G, int k, int64_t total_pop);
int fw_grid16_lb(int G, int k);
void* fw_grid16_fn(const FwRunParams& p);
void* fw_run_fn(const FwRunParams& p, int lb);  // the chain-kernel instantiation fw_launch_run takes
int fw_grid16_launch_nw(const FwRunParams& p);
int fw_grid16_launch_rows(const FwRunParams& p);
int fw_grid16_plan(FwRunParams& p, int device, int* grid);
int fw_grid16_launch(const FwRunParams& p, int grid, void* stream);
int fw_grid16_launch_rows(const FwRunParams& p);  // rows per chain of the kernel launched
int fw_grid16_launch_nw(const FwRunParams& p);    // waves per workgroup of that kernel
