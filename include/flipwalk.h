/*
 * flipwalk.h — C-ABI of the MI355X-native batched single-node flip walk.
 *
 * This is the drop-in boundary for the one hot path of
 * drdeford/FlipComplexityEmpirical: GerryChain's
 *
 *   MarkovChain(proposal, Validator([single_flip_contiguous, popbound]),
 *               accept=cut_accept, initial_state, total_steps)
 *
 * as constructed at grid_chain_sec11.py:340-342 (also All_States_Chain.py:300-302,
 * Frankenstein_chain.py:370-372) and iterated at grid_chain_sec11.py:366.
 * The reference has no FFI of its own (it is pure Python over GerryChain); the
 * entry points below are what a ctypes binding of that loop binds.  Each one
 * names the reference interface it replaces.
 *
 * Conventions
 *  - Return 0 on success, a negative FW_E* code on error; fw_last_error() gives
 *    a thread-local message.
 *  - Host buffers are owned by the caller and copied in/out.  Device memory is
 *    owned by the library behind the opaque handles.
 *  - One handle is bound to one HIP device; calls on one handle must be
 *    serialised; different handles may be driven from different host threads.
 *  - Graphs are CSR with strictly ascending neighbour lists, no self loops, and
 *    symmetric adjacency (checked by fw_graph_create).  Node ids 0..n-1.
 *  - District labels are 0..k-1 (the façade maps GerryChain labels such as
 *    ±1 onto them in sorted order).
 *
 * Randomness (a deterministic restatement of the reference's unseeded
 * `random.choice` / `random.random`, grid_chain_sec11.py:143,179): proposal
 * attempt t of global chain g draws ONE Philox4x32-10 block
 *     key = (lo32(seed), hi32(seed)),  ctr = (lo32(t), hi32(t), lo32(g), hi32(g))
 * giving words x0..x3.  The proposal takes the r-th element, r =
 * floor(((x1<<32)|x0) * P / 2^64), of the proposal set in canonical order (P =
 * its size); the Metropolis draw is CPython's random() construction
 * u = ((x2>>5)*2^26 + (x3>>6)) * 2^-53.
 */
#ifndef FLIPWALK_H
#define FLIPWALK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ---------------------------------------------------------- */
#define FW_OK 0
#define FW_EINVAL (-1)      /* bad argument / malformed graph                */
#define FW_EHIP (-2)        /* HIP runtime error                             */
#define FW_ESTATE (-3)      /* invalid initial state (GerryChain ValueError) */
#define FW_EUNSUPPORTED (-4)/* configuration outside what the kernels handle */
#define FW_ENOMEM (-5)

/* ---- proposal modes -------------------------------------------------------
 * FW_PROPOSE_BI     slow_reversible_propose_bi  grid_chain_sec11.py:132-145
 *                   uniform boundary node, flipped to the other label (k==2).
 * FW_PROPOSE_PAIRS  slow_reversible_propose     grid_chain_sec11.py:117-130 with
 *                   the pair updater b_nodes :151-153 — uniform over distinct
 *                   (node, foreign-neighbour-label) pairs, ordered (node, label).
 * FW_PROPOSE_CUTEDGE gerrychain.proposals.propose_random_flip (imported
 *                   grid_chain_sec11.py:24): uniform cut edge, uniform
 *                   endpoint == uniform directed cut edge (v,u) ordered (v,u);
 *                   v takes u's label.                                        */
#define FW_PROPOSE_BI 0
#define FW_PROPOSE_PAIRS 1
#define FW_PROPOSE_CUTEDGE 2

/* ---- accept rules (fw_chains_set_accept) --------------------------------------
 * FW_ACCEPT_CUT      cut_accept grid_chain_sec11.py:171-179 (the default):
 *                    accept iff u < thr[Δcut + maxdeg]  (thr[d] = base**(-d))
 * FW_ACCEPT_BRATIO   annealing_cut_accept_backwards grid_chain_sec11.py:81-110:
 *                    accept iff u < thr[Δcut + maxdeg] * (|B'| / |B|), |B| = boundary
 *                    nodes (b_nodes_bi) before / after the flip; the host tabulates
 *                    thr[d] = base**(beta*(-d)) (the reference: base .1, beta 5)
 * FW_ACCEPT_BOUNDARY uniform_accept + boundary_condition :43-52,159-165: accept iff
 *                    the nodes flagged boundary_node span >= 2 districts after the flip
 * (u = the CPython random() draw of the attempt, include/flipwalk.h header.)        */
#define FW_ACCEPT_CUT 0
#define FW_ACCEPT_BRATIO 1
#define FW_ACCEPT_BOUNDARY 2

/* ---- what fw_chains_read can return -------------------------------------- */
#define FW_READ_LABELS 0   /* int16  [n_chains][n]                            */
#define FW_READ_STATS 1    /* fw_chain_stats [n_chains]                       */
#define FW_READ_HIST_CUT 2 /* uint64 [n_edges+1]  yields with |cut edges| = i */
#define FW_READ_HIST_B 3   /* uint64 [n+1]        yields with |B| = i         */
#define FW_READ_POPS 4     /* int64  [n_chains][k] district populations       */
#define FW_READ_HIST_RING 5 /* uint64 [n_ring*n_ring+1] yields per ring pair (below) */
#define FW_READ_RING_PAIR 6 /* int32  [n_chains][2] current ring pair (i, j), -1 = none */
#define FW_READ_WAITS 7    /* double [n_chains][2] {sum of sampled waits over yields, the
                              current state's draw} (fw_chains_enable_waits)             */
#define FW_READ_RUNG 8        /* int32 [n_chains] current rung of each chain (read only)   */
#define FW_READ_RUNG_STATS 9  /* fw_rung_stats [n_sets][n_rungs] (read and fw_chains_write) */

/* ---- district-shape observable (fw_chains_enable_ring) ----------------------
 * boundary_slope (grid_chain_sec11.py:55-78; Frankenstein_chain.py:57-80) collects the
 * cut edges that lie on the outer ring of the grid (both endpoints in its first/last row
 * or column, plus the four corner diagonals of the sec11 graph); the driver (:371-394)
 * takes the first two, temp[0] and temp[1], and records the slope of the line through
 * their midpoints and the angle they subtend at the grid centre, once per yield.  The
 * kernels keep, per yield, the pair (i, j), i < j, of the first two CUT ring edges in the
 * caller's ring order and count yields per pair: FW_READ_HIST_RING index i*n_ring + j,
 * index n_ring*n_ring for yields with fewer than two cut ring edges (the reference would
 * raise IndexError there).  The host turns pairs into slopes and angles with the
 * reference's own float formula.  With exactly two cut ring edges (a two-district plan
 * whose boundary crosses the ring twice) the result does not depend on the order;
 * with more, the reference picks by CPython set-iteration order, which depends on the
 * interpreter's tuple hash, and the build picks the first two in ring order.            */

/* ---- spatial observables (fw_chains_enable_maps / fw_chains_read_map) ------
 * The reference driver's per-edge and per-node maps, updated once per yield
 * (grid_chain_sec11.py:383-384 cut_times, :396-400 part_sum / last_flipped /
 * num_flips, finalised at :416-419; the same code in Frankenstein_chain.py and
 * All_States_Chain.py).  Edges are indexed canonically: undirected (u < w) pairs
 * in CSR row order.  Values are int64.                                           */
#define FW_MAP_CUT_TIMES 0    /* [n_edges] yields in which the edge was cut          */
#define FW_MAP_NUM_FLIPS 1    /* [n] yields whose state was created by flipping node */
#define FW_MAP_PART_SUM 2     /* [n] part_sum (starts at the initial label value)    */
#define FW_MAP_LAST_FLIPPED 3 /* [n] last such yield index (0: never)                */
#define FW_MAP_SUM 1          /* flag: sum over the chain range into one row          */
#define FW_MAP_FINALIZE 2     /* flag: PART_SUM of never-flipped nodes := yields*label */

/* Per-chain counters and running observables (the per-yield block of
 * grid_chain_sec11.py:366-402, reduced to sums; one struct per chain). */
typedef struct fw_chain_stats {
  uint64_t attempts;    /* proposals drawn, including invalid (retried) ones   */
  uint64_t steps;       /* valid proposals = MarkovChain counter increments    */
  uint64_t accepts;     /* Metropolis-accepted flips                           */
  uint64_t pop_fail;    /* proposals rejected by the population bound          */
  uint64_t contig_fail; /* proposals (pop-valid) rejected by contiguity        */
  uint64_t bfs_runs;    /* contiguity checks that needed a graph search        */
  uint64_t bfs_nodes;   /* nodes dequeued by those searches                    */
  uint64_t bfs_deg;     /* sum of degrees of dequeued nodes                    */
  uint64_t sum_deg;     /* sum over proposals of deg(v)                        */
  uint64_t acc_deg;     /* sum over accepts of deg(v)                          */
  uint64_t n_bchg;      /* nodes entering/leaving the boundary, over accepts   */
  uint64_t yields;      /* yielded states counted (initial state included)     */
  int64_t sum_cut;      /* sum over yields of len(cut_edges)   (rce, :367)     */
  int64_t sum_bnodes;   /* sum over yields of len(b_nodes)     (rbn, :369)     */
  double sum_invb;      /* sum over yields of 1/len(b_nodes); the expected
                           geom wait (:147-148) is (N^k-1)*sum_invb - yields   */
  int32_t cut;          /* current len(cut_edges)                              */
  int32_t bnodes;       /* current number of boundary nodes                    */
  int32_t npairs;       /* current size of the proposal set                    */
  int32_t stuck;        /* 1 once max_retries consecutive proposals failed     */
} fw_chain_stats;

/* Per-rung observables of one replica set (fw_chains_set_ladder): what the chains did
 * while they sat on the rung, whichever chain that was. */
typedef struct fw_rung_stats {          /* 64 bytes */
  uint64_t yields, steps, accepts;      /* summed over the launches a chain spent on the rung */
  int64_t sum_cut, sum_bnodes;
  double sum_invb;
  uint64_t swap_tried, swap_done;       /* pair (r, r+1), kept at rung r */
} fw_rung_stats;

typedef struct fw_graph fw_graph;
typedef struct fw_chains fw_chains;

/* Thread-local description of the last error on this thread. */
const char* fw_last_error(void);

/* Library/ABI version, e.g. 0x000600 for 0.6.0 (0.2: spatial maps; 0.3: bound
 * schedules; 0.4: ring observable, checkpoint/resume; 0.5: sampled geometric waits;
 * 0.6: fw_chains_launch_info; 0.7: fw_build_info; the ladder entry points
 * fw_chains_set_ladder / fw_chains_exchange_async, the observable-series entry points and
 * the tally entry points and the geometry entry points arrived in 0.7 without a bump). */
int32_t fw_version(void);

/* Provenance of this build (static string, never NULL): "src=<sha256 of the flip
 * kernels, headers and ABI source> flags=<compiler flags, including any -D>
 * series=<sha256 of fw_series.hip> tally=<sha256 of fw_tally.hip> geom=<sha256 of
 * fw_geometry.hip> win=<sha256 of fw_window_rows.h> ovl=<sha256 of the overlap sources>
 * rsm=<sha256 of the resample sources> wb=<sha256 of fw_weights_bytes.h>".  Bench lines and PMC
 * profiles carry it, so a measurement names the code it measured. */
const char* fw_build_info(void);

/* Number of visible HIP devices (0 when none; never fails). */
int32_t fw_device_count(void);

/* Upload a CSR graph (replaces gerrychain.Graph / networkx adjacency,
 * grid_chain_sec11.py:191-260, All_States_Chain.py:221).  pop may be NULL
 * (every node population 1, grid_chain_sec11.py:218).  Row-major W×H grids
 * are detected and get an implicit-neighbour kernel. */
int fw_graph_create(const int32_t* rowptr, const int32_t* col, const int64_t* pop,
                    int32_t n, int32_t nnz, int device, fw_graph** out);
void fw_graph_destroy(fw_graph* g);
/* info[0]=n, info[1]=n_edges, info[2]=maxdeg, info[3]=grid width (0 = not a grid),
 * info[4]=grid height */
int fw_graph_info(const fw_graph* g, int64_t info[5]);

/* Create n_chains chains (replaces Partition(graph, assignment, updaters) +
 * within_percent_of_ideal_population + MarkovChain.__init__'s validity check,
 * grid_chain_sec11.py:316-342).
 *  init_labels  int16 [1 or n_chains][n], values 0..k-1 (init_per_chain 0/1)
 *  pop_lo/hi    integer population bounds ceil(lo), floor(hi) of Bounds
 *  thr          float64 [1 or n_chains][2*maxdeg+1]; thr[d+maxdeg] is the
 *               Metropolis bound base**(-d) for Δcut = d (cut_accept,
 *               grid_chain_sec11.py:171-179), thr_per_chain 0/1
 *  seed         Philox key; chain_id0 = global id of the first local chain
 * Fails with FW_ESTATE when an initial plan is not contiguous or violates the
 * bounds (GerryChain raises ValueError). */
int fw_chains_create(fw_graph* g, int32_t n_chains, int32_t k, const int16_t* init_labels,
                     int32_t init_per_chain, int32_t proposal_mode, int64_t pop_lo,
                     int64_t pop_hi, const double* thr, int32_t thr_per_chain, uint64_t seed,
                     int64_t chain_id0, fw_chains** out);
void fw_chains_destroy(fw_chains* c);

/* Advance every chain by `steps` counted steps (MarkovChain.__next__ called
 * `steps` times; the initial state is yielded once, on the first call).  A
 * chain that draws max_retries consecutive invalid proposals is marked stuck
 * instead of looping forever (the reference would hang).  Blocking. */
int fw_chains_run(fw_chains* c, int64_t steps, int32_t max_retries);

/* Same, asynchronous on the handle's stream; fw_chains_sync waits.  The last
 * kernel's device time (ms, HIP events on that stream) is returned by
 * fw_chains_last_kernel_ms. */
int fw_chains_run_async(fw_chains* c, int64_t steps, int32_t max_retries);
int fw_chains_sync(fw_chains* c);
double fw_chains_last_kernel_ms(const fw_chains* c);

/* The launch plan of the handle's next fw_chains_run (no reference counterpart: the
 * occupancy figures SURVEY.md §8d asks the measurement to report).
 *  info[0] workgroups of the persistent grid     info[1] waves per workgroup
 *  info[2] chains per wave                       info[3] LDS bytes per workgroup
 *  info[4] VGPRs per lane of the kernel           info[5] scratch (spill) bytes per lane
 *  info[6] compute units of the device           info[7] workgroups resident per CU */
int fw_chains_launch_info(const fw_chains* c, int64_t info[8]);

/* fw_chains_run plus a per-step trace: host_trace [n_chains][steps] receives, for
 * each counted step, v*64 + target when the flip was accepted, -1 when the
 * Metropolis draw kept the old state, and a value < -1 for steps a stuck chain
 * never took.  Used by the façade's GerryChain-style iterator to rebuild every
 * yielded Partition on the host. */
int fw_chains_run_traced(fw_chains* c, int64_t steps, int32_t max_retries, int32_t* host_trace,
                         size_t bytes);

/* Copy a state array back to the host (see FW_READ_*). */
int fw_chains_read(fw_chains* c, int32_t what, void* host_dst, size_t bytes);

/* Overwrite a state array from the host: the inverse of fw_chains_read, for exact
 * checkpoint / resume (the chain states plus the Philox attempt counter in
 * the stats record are a complete checkpoint of the counter-based RNG).  what is
 * FW_READ_LABELS (every plan is validated like an initial state, FW_ESTATE otherwise, and
 * the district populations are recomputed from it), FW_READ_STATS (counters, sums and
 * the attempt counter; the stuck flag included), FW_READ_HIST_CUT, FW_READ_HIST_B or
 * FW_READ_HIST_RING.  A chain resumed from {labels, stats} continues exactly as the
 * uninterrupted chain (same proposals, same Metropolis draws).  The FW_ACCEPT_BOUNDARY
 * flagged-node counts are recomputed from written plans; the spatial maps are not part of a
 * checkpoint, and a plan write on a handle with maps enabled fails with FW_ESTATE.  A stats
 * write also restores the yield count the maps' 2^32 index guard starts from. */
int fw_chains_write(fw_chains* c, int32_t what, const void* host_src, size_t bytes);

/* Zero the per-chain sums and the yield histograms (not the chain states, and not the
 * observable series: fw_chains_series_reset). */
int fw_chains_reset_observables(fw_chains* c);

/* Select the accept rule (FW_ACCEPT_*) for every chain; node_flags [n] (1 =
 * boundary_node) is required by FW_ACCEPT_BOUNDARY and ignored otherwise.  May be
 * called between runs. */
int fw_chains_set_accept(fw_chains* c, int32_t rule, const uint8_t* node_flags);

/* Step-dependent Metropolis bounds for FW_ACCEPT_CUT / FW_ACCEPT_BRATIO, shared by
 * every chain: the commented beta schedule of annealing_cut_accept_backwards
 * (grid_chain_sec11.py:85-93, t = partition["step_num"], the step_num updater
 * :282-289 = flips accepted since the initial plan, + 1 for the proposal).  A
 * proposal with step_num t uses row clamp(t - t0, 0, n_rows - 1) of rows
 * [n_rows][2*maxdeg+1] in place of the chain's thr table (Δcut + maxdeg indexes
 * a row, as for thr).  n_rows == 0 removes the schedule.  May be called between
 * runs; the accepted-flip count is the FW_READ_STATS accepts field. */
int fw_chains_set_schedule(fw_chains* c, const double* rows, int32_t n_rows, int64_t t0);

/* Turn on the spatial observables for every chain (before the first run).
 * label_values [k] are the GerryChain assignment values of districts 0..k-1
 * (e.g. {-1, 1} for the reference's k=2 plans); NULL means 0..k-1.  Costs
 * 8*n_edges + 16*n bytes of HBM per chain.  Yields per chain must stay below 2^32. */
int fw_chains_enable_maps(fw_chains* c, const int64_t* label_values);

/* Turn on the district-shape observable for every chain: ring edge r joins nodes
 * ring_u[r] and ring_w[r] (an edge of the graph; 2 <= n_ring <= 1024), in the order that
 * picks "the first two".  Zeroes the ring histogram; may be called between runs. */
int fw_chains_enable_ring(fw_chains* c, const int32_t* ring_u, const int32_t* ring_w,
                          int32_t n_ring);

/* Turn on sampled geometric waits for every chain (before the first run): geom_wait
 * (grid_chain_sec11.py:147-148) = int(np.random.geometric(len(b_nodes)/(N**k - 1))) - 1,
 * drawn once per state object and re-used when a Metropolis rejection re-yields it
 * (:368; the Partition caches it), summed over yields (:410-411).  p_table [n+1] holds
 * b/(N^k - 1) for every boundary size b, divided as the reference divides (Python int /
 * int).  The state created by proposal attempt t of global chain g (the initial state:
 * t = 2^63 - 1) draws the Philox block key = seed, ctr = (lo32(t), hi32(t) | 2^31,
 * lo32(g), hi32(g)), takes u = CPython random() of its words (x0, x1) and waits
 * floor(log1p(-u) / log1p(-p)) (inversion; log1p evaluated in plain IEEE double
 * operations, so every implementation agrees bit for bit).  Read / write with
 * FW_READ_WAITS.  The Rao-Blackwellised expectation (stats sum_invb) stays available. */
int fw_chains_enable_waits(fw_chains* c, const double* p_table);

/* Replica exchange (parallel tempering) across a ladder of Metropolis bases.  No reference
 * counterpart: the reference sweeps its bases one run at a time; this joins
 * the rungs of such a sweep into one sampler.  A replica set is n_rungs chains of the
 * handle, one per rung; rung r runs under thr_rows[r] (thr[d + maxdeg] = base_r ** (-d))
 * and log_base[r] = log(base_r).  set_of_chain / rung_of_chain [n_chains] place every chain.
 *  - FW_EINVAL unless 2 <= n_rungs <= 64, n_chains % n_rungs == 0, set ids lie in
 *    [0, n_chains / n_rungs) and every (set, rung) occurs exactly once (checked on the
 *    host before the device is touched).
 *  - FW_EUNSUPPORTED unless the accept rule is FW_ACCEPT_CUT and no schedule is set: only
 *    then is the jump chain's stationary law f(x) * base ** (-cut(x)) with f free of the
 *    base, so that the swap ratio below is exact for all three proposal modes.  On a
 *    laddered handle fw_chains_set_accept with another rule and fw_chains_set_schedule
 *    with rows fail with FW_EUNSUPPORTED.
 * The call gives every chain the thr row of its rung (a handle created with one shared
 * table gets per-chain tables), zeroes the rung stats and snapshots the stats records.
 * It may be called again; that, followed by a FW_READ_RUNG_STATS write, restores a
 * checkpoint.  fw_chains_reset_observables also zeroes the rung stats and re-snapshots;
 * a FW_READ_STATS write re-snapshots.
 *
 * fw_chains_exchange_async (0 <= round < 2^32; FW_EINVAL without a ladder) enqueues one
 * exchange step on the handle's stream, with no host synchronisation; it does not touch
 * fw_chains_last_kernel_ms.  One wave per replica set, lane r owning the chain now on
 * rung r; no atomics, no dependence on thread order:
 *  1. Accumulate.  rung_stats[set][r] += (stats - snapshot) of the chain's yields, steps,
 *     accepts, sum_cut and sum_bnodes; sum_invb = sum_invb + (cur - snap) in plain IEEE
 *     double operations; then snapshot = stats.
 *  2. Swap.  For each pair (r, r+1) with r = round (mod 2), r+1 < n_rungs and neither chain
 *     stuck: d = cut(chain on r) - cut(chain on r+1) from the stats records,
 *     x = (double)d * (log_base[r] - log_base[r+1]) (one subtraction, one multiplication);
 *     the Philox4x32-10 block key = seed, ctr = (lo32(round), 2^30 | r, lo32(g), hi32(g)),
 *     g = the smallest global chain id (chain_id0 + local index) in the set, gives
 *     u = ((x2>>5)*2^26 + (x3>>6)) * 2^-53; the pair swaps iff log1p(-u) <= x (log1p as
 *     for the sampled waits: plain IEEE double operations), i.e. with probability
 *     min(1, (base_r / base_{r+1}) ** d).  swap_tried / swap_done count at rung r.  On a
 *     swap the two chains trade rungs: FW_READ_RUNG and each chain's thr row change;
 *     plans, counters and sums stay with the chain.
 * Counter word 1 has bit 30 set and bit 31 clear: disjoint from the proposal draws (word 1
 * = hi32(t) < 2^30) and from the wait draws (bit 31 set).  The run kernels are unchanged:
 * they read a chain's thr row at the start of every launch.
 * (These entry points arrived in 0.7 without a version bump.) */
int fw_chains_set_ladder(fw_chains* c, const double* thr_rows /*[n_rungs][2*maxdeg+1]*/,
                         const double* log_base /*[n_rungs]*/, int32_t n_rungs,
                         const int32_t* set_of_chain, const int32_t* rung_of_chain);
int fw_chains_exchange_async(fw_chains* c, int64_t round);

/* ---- thinned observable series ------------------------------------------------------
 * The reference keeps rce, rbn and waits as per-yield lists (grid_chain_sec11.py:350-369) and
 * plots them as traces; the sums and histograms above drop the order in time.  A series keeps
 * it, thinned: one sample of every chain's current len(cut_edges) and len(b_nodes) wherever
 * the caller asks for one between launches, as the exchange step is placed.
 *
 * fw_chains_enable_series (once per handle: FW_ESTATE the second time; capacity >= 1;
 * FW_ENOMEM) allocates sample-major device buffers int32 [capacity][n_chains] for cut and
 * bnodes; the rung buffer of the same shape is allocated on the first rung row (a recorded
 * sample of a laddered handle, or a FW_SERIES_RUNG write) and reads as -1 before it.
 *
 * fw_chains_record_async enqueues one small kernel on the handle's stream (no host
 * synchronisation; fw_chains_last_kernel_ms is not touched) that writes sample n_samples of
 * every chain: cut and bnodes from the stats records, rung from the ladder (-1 without one);
 * n_samples is incremented at enqueue.  FW_ESTATE when the series are not enabled or full.
 * The host stamps each sample with the ladder epoch it was recorded under: 0 without a ladder,
 * and every fw_chains_set_ladder starts the next epoch.
 *
 * fw_chains_series_info: info[0] = capacity (0: not enabled), info[1] = n_samples,
 * info[2] = the current ladder epoch, info[3] = n_rungs.
 *
 * fw_chains_read_series / fw_chains_write_series move the window [t0, t0 + n), n >= 1, of
 * `what` = FW_SERIES_CUT, FW_SERIES_BNODES or FW_SERIES_RUNG.  The plain view is int32
 * [n][n_chains], by chain.  A read of CUT or BNODES or'ed with FW_SERIES_BY_RUNG is
 * [n][n_sets * n_rungs]: slot set * n_rungs + r of sample t holds the value of the chain that
 * sat on rung r of that set when sample t was taken; it needs a ladder and every sample of the
 * window stamped with the current epoch (FW_ESTATE otherwise).  A read window must lie inside
 * [0, n_samples), a write window inside [0, capacity) with t0 <= n_samples (no gaps), else
 * FW_EINVAL; a write sets n_samples = max(n_samples, t0 + n).  Writes exist for checkpoints
 * and tests: CUT / BNODES values must lie in [0, xmax], xmax = max(n_edges, n nodes) (what
 * any recorded value satisfies), else FW_EINVAL; a sample such a write creates has no rung row
 * (-1, epoch 0).  A RUNG write on a laddered handle must hold every (set, rung) exactly once
 * per sample (FW_EINVAL) and stamps its samples with the current epoch; without a ladder the
 * values are taken as they are, under epoch 0.
 *
 * fw_chains_series_reset sets n_samples = 0.  fw_chains_reset_observables does NOT touch the
 * series.
 *
 * fw_chains_series_acf (`what` = CUT or BNODES, optionally | FW_SERIES_BY_RUNG) synchronises
 * the stream and reduces the window's n_series = n_chains series x_j[0..n):
 *  1. per_series, int64 [n_series][3][max_lag + 1] = {P, A, B}, exact:
 *       P[j][l] = sum_{t=0}^{n-1-l} x_t * x_{t+l}
 *       A[j][l] = sum_{t=0}^{n-1-l} x_t          B[j][l] = sum_{t=l}^{n-1} x_t
 *     FW_EINVAL unless 0 <= max_lag < n, max_lag <= 1023 and n * xmax^2 < 2^63.
 *  2. pooled, double [n_groups][max_lag + 3] = {sum_j c_j[0..max_lag], sum_j m_j, sum_j m_j^2}
 *     in plain IEEE double operations (no contraction), evaluated exactly in this order:
 *       m_j    = (double)A[j][0] / (double)n
 *       c_j[l] = (((double)P - m_j * (double)(A + B)) + (double)(n - l) * m_j * m_j) / (double)n
 *     ((double)(n - l) * m_j first, then * m_j; A + B added as integers), summed over the
 *     members of a group in a fixed order: partial p, p = 0..255, is the sequential sum,
 *     from +0.0 and in ascending position, of the members whose position = p (mod 256); then
 *     the halving tree a[i] += a[i + 128], then 64, .., 1, and a[0] is the sum.
 *     Plain view: one group, every chain in ascending index.  By-rung view: n_rungs groups,
 *     group r = slots set * n_rungs + r in ascending set.
 * Either output may be NULL.  The kernels use no atomics and do not depend on thread order:
 * a host restatement of the above agrees bit for bit.
 * (These entry points arrived in 0.7 without a version bump.) */
#define FW_SERIES_CUT 0
#define FW_SERIES_BNODES 1
#define FW_SERIES_RUNG 2
#define FW_SERIES_BY_RUNG 4
int fw_chains_enable_series(fw_chains* c, int64_t capacity);
int fw_chains_record_async(fw_chains* c);
int fw_chains_series_info(const fw_chains* c, int64_t info[4]);
int fw_chains_series_reset(fw_chains* c);
int fw_chains_read_series(fw_chains* c, int32_t what, int64_t t0, int64_t n, int32_t* dst,
                          size_t bytes);
int fw_chains_write_series(fw_chains* c, int32_t what, int64_t t0, int64_t n, const int32_t* src,
                           size_t bytes);
int fw_chains_series_acf(fw_chains* c, int32_t what, int64_t t0, int64_t n, int32_t max_lag,
                         int64_t* per_series, double* pooled);

/* ---- district tallies of node columns and seat counts ---------------------------------
 * The reference gives every node vote columns (pink / purple, grid_chain_sec11.py:223) and
 * imports Election, mean_median and efficiency_gap; its census graphs carry many columns
 * besides TOTPOP.  A tally sums node columns per district over every chain's current plan, on
 * the device and between launches, as the exchange and record steps are placed; no run kernel
 * changes.  Every result is an exact integer.
 *
 * fw_chains_set_columns: cols int64 [n_cols][n], 1 <= n_cols <= 8, every value >= 0 and every
 * column's total over the nodes < 2^31 (so a district sum fits 32 bits; the device keeps the
 * columns as 32-bit values), else FW_EINVAL, checked on the host before the device is touched.
 * May be repeated: it replaces the columns, drops the elections and zeroes the seat histogram.
 *
 * fw_chains_set_elections: ab int32 [n_el][2], 0 <= n_el <= 4 (ab may be NULL when n_el is 0),
 * each entry a pair (a, b) of distinct column indices (FW_EINVAL); FW_ESTATE without columns.
 * Zeroes the seat histogram.
 *
 * fw_chains_tally_async (FW_ESTATE without columns) enqueues on the handle's stream, with no
 * host synchronisation and without touching fw_chains_last_kernel_ms, the tally of every
 * chain's current plan (stuck chains like any other):
 *   T[c][j][d]  = sum of column j over the nodes that chain c labels d
 *   wins[c][e]  = #{d : T[c][a][d] > T[c][b][d]} (strict),  ties[c][e] = #{d : T[c][a][d] ==
 *                 T[c][b][d]}   for election e = (a, b)
 *   seat_hist[g][e][wins[c][e]] += 1, g = the chain's current rung under a ladder, else 0.
 * The host counter n_tallied is incremented at enqueue.  T and {wins, ties} are plain vector
 * stores from one owner each (no atomics, no dependence on thread order); the seat histogram
 * is accumulated with integer atomics, whose sum does not depend on the order.
 *
 * fw_chains_read_tally synchronises, then copies
 *   FW_TALLY_SUMS   int64  [n_chains][n_cols][k]       of the last tally
 *   FW_TALLY_SEATS  int32  [n_chains][n_el][2]         {wins, ties} of the last tally
 *   FW_TALLY_HIST   uint64 [n_groups][n_el][k + 1]     accumulated over all tallies;
 *                                                      n_groups = n_rungs, or 1 without a ladder
 * FW_ESTATE without columns, and for SUMS / SEATS when nothing was tallied since the columns
 * (SEATS: the elections) were set.  fw_chains_write_tally restores FW_TALLY_HIST (checkpoints;
 * n_tallied is not changed); fw_chains_tally_reset zeroes the histogram and n_tallied.
 * fw_chains_tally_info: info = {n_cols, n_el, label bits per node of the handle's plans,
 * n_groups, n_tallied}.  fw_chains_reset_observables leaves all of this alone, as it leaves
 * the series alone; fw_chains_set_ladder zeroes the histogram, because its group count changes.
 * (These entry points arrived in 0.7 without a version bump.) */
#define FW_TALLY_SUMS 0
#define FW_TALLY_SEATS 1
#define FW_TALLY_HIST 2
int fw_chains_set_columns(fw_chains* c, const int64_t* cols /*[n_cols][n]*/, int32_t n_cols);
int fw_chains_set_elections(fw_chains* c, const int32_t* ab /*[n_el][2]*/, int32_t n_el);
int fw_chains_tally_async(fw_chains* c);
int fw_chains_read_tally(fw_chains* c, int32_t what, void* dst, size_t bytes);
int fw_chains_write_tally(fw_chains* c, int32_t what, const void* src, size_t bytes);
int fw_chains_tally_reset(fw_chains* c);
int fw_chains_tally_info(const fw_chains* c, int64_t info[5]);

/* ---- per-district geometry: cut edges, perimeters, areas -------------------------------
 * GerryChain's cut_edges_by_part, interior_boundaries, exterior_boundaries, perimeter, area and
 * polsby_popper (the reference imports GeographicPartition; its census graphs carry
 * shared_perim on the edges, boundary_perim and area on the nodes), measured for every chain's
 * current plan on the device and between launches, as the exchange, record and tally steps are
 * placed; no run kernel changes.  Every result is an exact integer; the scores are formed on
 * the host (compactness.py).
 *
 * fw_chains_set_geometry: edge_w int64 [n_edges] indexed by the canonical edge id (pairs u < w
 * in CSR row order) or NULL (every weight 1: no weight array is kept or read); area int64 [n]
 * or NULL (every node has area 1); ext int64 [n], a node's exterior perimeter, or NULL (0).
 * Every value >= 0 and the total of each array < 2^31 (so any district sum fits 32 bits, a
 * district's interior perimeter being at most the total edge weight; the device keeps the
 * values as 32-bit), else FW_EINVAL, checked on the host before the device is touched.  May be
 * repeated: it replaces the arrays and zeroes the histogram and n_measured.
 *
 * fw_chains_geometry_async (FW_ESTATE before fw_chains_set_geometry) enqueues on the handle's
 * stream, with no host synchronisation and without touching fw_chains_last_kernel_ms, for
 * every chain c (stuck chains like any other) with lab its current plan:
 *   G[c][d][0] = number of nodes labelled d
 *   G[c][d][1] = number of edges (u, w) with lab[u] != lab[w] and d in {lab[u], lab[w]}
 *   G[c][d][2] = sum of edge_w over those edges           (interior perimeter)
 *   G[c][d][3] = sum of ext over the nodes labelled d     (exterior perimeter)
 *   G[c][d][4] = sum of area over the nodes labelled d
 *   hist[g][G[c][d][1]] += 1 for every district d, g = the chain's current rung under a
 *                ladder, else 0.
 * The host counter n_measured is incremented at enqueue.  Every G value is a plain vector
 * store from one owner (no atomics, no dependence on thread order); the histogram is
 * accumulated with integer atomics, whose sum does not depend on the order.
 *
 * fw_chains_read_geometry synchronises, then copies
 *   FW_GEOM_DISTRICTS  int64  [n_chains][k][5]          of the last measurement
 *   FW_GEOM_HIST       uint64 [n_groups][n_edges + 1]   accumulated over all measurements;
 *                                                       n_groups = n_rungs, or 1 without a ladder
 * FW_ESTATE before fw_chains_set_geometry, and for DISTRICTS when nothing was measured since
 * it; FW_EINVAL for a buffer that is too small.  fw_chains_write_geometry restores FW_GEOM_HIST
 * (checkpoints; n_measured is not changed); fw_chains_geometry_reset zeroes the histogram and
 * n_measured.  fw_chains_geometry_info: info = {has edge weights (0 / 1), label bits per node
 * of the handle's plans, n_groups, n_edges, n_measured}.  fw_chains_reset_observables leaves
 * all of this alone; fw_chains_set_ladder on a handle with geometry set re-sizes the histogram
 * for the new group count and zeroes it.  (These entry points arrived in 0.7 without a version
 * bump.) */
#define FW_GEOM_DISTRICTS 0
#define FW_GEOM_HIST 1
int fw_chains_set_geometry(fw_chains* c, const int64_t* edge_w /*[n_edges] or NULL*/,
                           const int64_t* area /*[n] or NULL*/, const int64_t* ext /*[n] or NULL*/);
int fw_chains_geometry_async(fw_chains* c);
int fw_chains_read_geometry(fw_chains* c, int32_t what, void* dst, size_t bytes);
int fw_chains_write_geometry(fw_chains* c, int32_t what, const void* src, size_t bytes);
int fw_chains_geometry_reset(fw_chains* c);
int fw_chains_geometry_info(const fw_chains* c, int64_t info[5]);

/* ---- plan overlap and Hamming distance against snapshots and partner chains ------------
 * How long a flip chain takes to forget its plan (the question of the reference's paper) is not
 * visible in the cut count: a chain whose cut has long decorrelated can still hold every
 * district where the seed put it.  An overlap compares every chain's current plan X_c with a
 * reference plan R_c, node by node, on the device and between launches, as the exchange, record,
 * tally and geometry steps are placed; no run kernel changes.  Every result is an exact integer
 * count of nodes; the scores are formed on the host (plandist.py).
 *
 * fw_chains_set_reference, labels == NULL: a snapshot.  Enqueues on the handle's stream, with no
 * host synchronisation, a device-to-device copy of the label words of every chain's record into
 * a reference buffer the handle owns; the reference becomes per-chain and is the plans at that
 * point of the stream.  labels != NULL: int16 [1][n] (per_chain 0, one plan shared by every
 * chain) or [n_chains][n] (per_chain 1), every value in [0, k), else FW_EINVAL, checked on the
 * host before the device is touched; a reference may be any labelling (it need not be
 * contiguous or balanced).  Either form replaces the reference, zeroes the histogram and
 * n_measured and invalidates MATRIX and DIST.
 *
 * fw_chains_set_partners: partner int32 [n_chains], every value in [0, n_chains), else
 * FW_EINVAL, checked on the host first; partner[c] == c is allowed (distance 0).  The array is
 * kept on the device; the histogram is not touched.
 *
 * fw_chains_overlap_async (FW_ESTATE for FW_OVERLAP_REFERENCE without a reference and for
 * FW_OVERLAP_PARTNER without partners, FW_EINVAL for another value) enqueues on the handle's
 * stream, with no host synchronisation and without touching fw_chains_last_kernel_ms, for every
 * chain c (stuck chains like any other), with R_c the stored reference (REFERENCE) or the
 * current plan of chain partner[c] (PARTNER; the kernel only reads the plans, so the order of
 * the chains cannot matter):
 *   O[c][d][e] = #{v : R_c(v) = d and X_c(v) = e}    (row sums: the reference's district sizes,
 *                column sums: the current ones, total n)
 *   dist[c]    = #{v : R_c(v) != X_c(v)} = n - trace(O[c])
 *   hist[g][dist[c]] += 1, g = the chain's current rung under a ladder, else 0.
 * The host counter n_measured is incremented at enqueue.  O and dist are plain vector stores
 * from one owner each (no global atomics, no dependence on thread order); the histogram is
 * accumulated with integer atomics, whose sum does not depend on the order.
 *
 * fw_chains_read_overlap synchronises, then copies
 *   FW_OVERLAP_MATRIX  int64  [n_chains][k][k]      of the last measurement
 *   FW_OVERLAP_DIST    int32  [n_chains]            of the last measurement
 *   FW_OVERLAP_HIST    uint64 [n_groups][n + 1]     accumulated over all measurements;
 *                                                   n_groups = n_rungs, or 1 without a ladder
 *   FW_OVERLAP_REF     int16  [1 or n_chains][n]    the stored reference, unpacked (checkpoints)
 * FW_ESTATE before any reference or partners were set, for REF without a reference, and for
 * MATRIX / DIST when the last measurement does not stand: nothing was measured since the
 * reference was set, or the last measurement was against partners that have been replaced
 * since.  FW_EINVAL for a buffer that is too small.  fw_chains_write_overlap restores
 * FW_OVERLAP_HIST only (checkpoints; n_measured is not changed); fw_chains_overlap_reset zeroes
 * the histogram and n_measured.  fw_chains_overlap_info: info = {reference kind (0 none,
 * 1 shared, 2 per chain), label bits per node of the handle's plans, n_groups, partners set
 * (0 / 1), n_measured}.  fw_chains_reset_observables leaves all of this alone;
 * fw_chains_set_ladder re-sizes the histogram for the new group count and zeroes it.  (These
 * entry points arrived in 0.7 without a version bump.) */
#define FW_OVERLAP_REFERENCE 0   /* against the stored reference          */
#define FW_OVERLAP_PARTNER   1   /* against the current plan of partner[c] */
#define FW_OVERLAP_MATRIX 0      /* int64  [n_chains][k][k]  last measurement */
#define FW_OVERLAP_DIST   1      /* int32  [n_chains]        last measurement */
#define FW_OVERLAP_HIST   2      /* uint64 [n_groups][n + 1] accumulated      */
#define FW_OVERLAP_REF    3      /* int16  [1 or n_chains][n] the stored reference */
int fw_chains_set_reference(fw_chains* c, const int16_t* labels, int32_t per_chain);
int fw_chains_set_partners(fw_chains* c, const int32_t* partner /*[n_chains]*/);
int fw_chains_overlap_async(fw_chains* c, int32_t against);
int fw_chains_read_overlap(fw_chains* c, int32_t what, void* dst, size_t bytes);
int fw_chains_write_overlap(fw_chains* c, int32_t what, const void* src, size_t bytes);
int fw_chains_overlap_reset(fw_chains* c);
int fw_chains_overlap_info(const fw_chains* c, int64_t info[5]);

/* ---- resampling plans across chains: clone, systematic resampling by cut ------------------
 * The exchange step trades rungs, never plans; these two let a chain continue from another
 * chain's plan, on the device and between launches, as the exchange, record, tally, geometry and
 * overlap steps are placed; no run kernel changes.  They serve population annealing (a population
 * at base 1, re-weighted and resampled while the base is stepped to the target), short bursts
 * (restart every chain from the best plan) and seeding an ensemble from a few chains.  No
 * reference counterpart: the reference runs one chain.
 *
 * fw_chains_clone_async: src int32 [n_chains]; chain i continues from the current plan of chain
 * src[i].  Checked on the host before the device is touched, FW_EINVAL otherwise: every value in
 * [0, n_chains), and every source a fixed point, src[src[i]] == src[i] (sources are then never
 * written, so the gather works in place).  Enqueues on the handle's stream with no host
 * synchronisation and without touching fw_chains_last_kernel_ms; src is copied to a device array
 * the handle owns through a pinned staging slot (the host waits at most for the upload two calls
 * back, never for the stream).
 *   What moves from src[i] to i, the plan: the whole label record (the labels and the group sums
 *   behind them), the k int64 populations, the stats fields cut, bnodes, npairs and stuck, under
 *   FW_ACCEPT_BOUNDARY the k flagged-node counts, with sampled waits the current state's draw
 *   (FW_READ_WAITS [i][1]), and family[i] (below).
 *   What stays with i, the chain: attempts (its Philox counter), steps, accepts, every sum and
 *   failure counter, yields, the wait sum, its thr row, its series, tallies, partners and
 *   reference.  Clones diverge at once: chain i draws with its own global id and attempt counter.
 * The result: after one or more runs a clone equals, bit for bit in everything a later run
 * produces, the host route {read labels, stats (and waits); labels[i] = labels[src[i]], the four
 * stats fields and the draw likewise; fw_chains_write}; before the first run it equals a handle
 * created with the per-chain initial plans init[src[i]] (every chain yields its new initial plan
 * once).  FW_ESTATE when the spatial maps are enabled (as fw_chains_write refuses plans under
 * them), FW_EUNSUPPORTED on a laddered handle (fw_chains_set_ladder on a handle that has cloned
 * is allowed).  One wave per destination chain with src[i] != i, 16-byte copies of the record,
 * plain vector stores from one owner each, no atomics.
 *
 * fw_chains_resample_async: the map is drawn on the device, with no host synchronisation, by
 * systematic resampling from integer weights of the cut, and applied as a clone.  q uint32
 * [n_edges + 1] is non-increasing with q[0] == 2^30, sign is +1 or -1, 0 <= round < 2^32
 * (FW_EINVAL otherwise); for a change of base b -> b', r = b'/b, the host passes q[d] =
 * round(2^30 rho^d), rho = min(r, 1/r), sign = +1 if r > 1 else -1 (population.weight_table).
 * C = n_chains <= 2^20 (FW_EUNSUPPORTED above); the refusals of clone apply.  Every quantity is
 * an integer and no step depends on thread order:
 *  1. cref = min (sign +1) or max (sign -1) of stats[i].cut over all chains (stuck chains like any
 *     other); W_i = q[sign (cut_i - cref)]: the heaviest chain weighs 2^30, nothing underflows.
 *  2. cum[i] = W_0 + .. + W_i (uint64), T = cum[C-1] <= 2^50, S2 = sum of (W_i >> 10)^2; the
 *     effective sample size is (T >> 10)^2 / S2.
 *  3. One Philox4x32-10 block, key = seed, ctr = (lo32(round), 2^30 | 2^29, lo32(chain_id0),
 *     hi32(chain_id0)); u = x0.  Counter word 1 has bits 30 and 29 set and bit 31 clear: disjoint
 *     from the proposal draws (word 1 < 2^30), the wait draws (bit 31 set) and the exchange
 *     draws (2^30 | rung, rung < 64: bit 29 clear).
 *  4. p_j = floor(((j 2^32 + u) T) / (C 2^32)), j = 0..C-1 (32-bit limbs: fw_resample_limbs.h).
 *  5. The offspring count n_i = #{j : cum[i-1] <= p_j < cum[i]} (cum[-1] = 0); sum n_i = C and
 *     floor(C W_i / T) <= n_i <= ceil(C W_i / T).
 *  6. src[i] = i when n_i >= 1; the dead chains (n_i = 0) in ascending index receive the extra
 *     copies (n_i - 1 per survivor) in ascending survivor index.  Every source is a fixed point.
 *  7. The clone above with that map, read from the device array.
 * The host counter n_resampled is incremented at enqueue.  Reads synchronise first:
 * fw_chains_resample_info: info = {n_resampled, the last round (-1: none), T, S2, cref, survivors,
 * max offspring (of the last resample), chains replaced by clones since creation (src[i] != i,
 * over both entry points)}.  fw_chains_read_resample copies FW_RESAMPLE_SRC int32 [C] (the last
 * map, from either entry point; FW_ESTATE before any), FW_RESAMPLE_FAMILY int32 [C] (the chain
 * whose initial plan this plan descends from; family[i] = i at creation) or FW_RESAMPLE_WEIGHTS
 * uint32 [C] (the last W; FW_ESTATE before a resample); FW_EINVAL for another kind or a buffer
 * that is too small.  fw_chains_write_resample restores FW_RESAMPLE_FAMILY (checkpoints; every
 * value in [0, C), else FW_EINVAL).  Left out: resampling across ranks, within the rungs of a
 * ladder, under the spatial maps, weights from anything but the cut (the host can score between
 * launches and call clone), adaptive bases, multinomial or residual schemes.  (These entry points
 * arrived in 0.7 without a version bump; fw_build_info gained rsm=<sha256 of fw_resample.hip and
 * fw_resample_limbs.h>.) */
#define FW_RESAMPLE_SRC 0      /* int32  [n_chains] the last source map          */
#define FW_RESAMPLE_FAMILY 1   /* int32  [n_chains] the ancestor chain of each plan */
#define FW_RESAMPLE_WEIGHTS 2  /* uint32 [n_chains] the last resample's weights  */
int fw_chains_clone_async(fw_chains* c, const int32_t* src /*[n_chains]*/);
int fw_chains_resample_async(fw_chains* c, const uint32_t* q /*[n_edges+1]*/, int32_t sign,
                             int64_t round);
int fw_chains_resample_info(fw_chains* c, int64_t info[8]);
int fw_chains_read_resample(fw_chains* c, int32_t what, void* dst, size_t bytes);
int fw_chains_write_resample(fw_chains* c, int32_t what, const void* src, size_t bytes);

/* ---- ensemble census: node occupancy, edge cut and boundary counts across the chains -------
 * The reference's heat maps (cut_times per edge, part_sum per node, the boundary frequencies)
 * are sums over the steps of one chain; fw_chains_enable_maps reproduces them per chain, inside
 * the run kernels.  With many chains the map a user wants is the one across the ensemble at a
 * sampled instant: how often node v lies in district d, how often edge e is cut, how often v
 * lies on a boundary; under a ladder, per rung.  Every other measurement reduces over the nodes
 * of one chain; a census fixes a node or an edge and sums over the chains.  It runs on the
 * device and between launches, as the exchange, record, tally, geometry and overlap steps are
 * placed, from the label records; no run kernel changes, and it only reads plans: it works on
 * every label width, on both run kernels' records, with the spatial maps enabled and on cloned
 * or resampled populations.
 *
 * fw_chains_enable_census: what is a non-zero mask of FW_CENSUS_NODES, FW_CENSUS_EDGES and
 * FW_CENSUS_BOUNDARY (FW_EINVAL for any other value, checked before the handle is looked at).
 * Allocates and zeroes the accumulators and zeroes n_measured; repeated, it replaces the
 * previous set (FW_ENOMEM when the arrays cannot be allocated: the handle keeps what it had).
 * What the passes need from the graph is derived here, once: node tiles with their CSR rows and
 * canonical edge ranges, the range of label words each tile's rows reach, and the slices.
 *
 * fw_chains_census_async (FW_ESTATE before fw_chains_enable_census) enqueues on the handle's
 * stream, with no host synchronisation and without touching fw_chains_last_kernel_ms.  With X_c
 * the current plan of chain c (stuck chains like any other), g(c) the chain's current rung under
 * a ladder, else 0 (read on the device from the exchange step's own arrays: the host does not
 * wait for them), and e = (u, w) the canonical edge id (pairs u < w in CSR row order, as the
 * geometry uses), it adds
 *   cnt[g]       += #{c : g(c) = g}
 *   occ[g][v][d] += #{c : g(c) = g and X_c(v) = d}                                  (NODES)
 *   ecut[g][e]   += #{c : g(c) = g and X_c(u) != X_c(w)}                            (EDGES)
 *   bnd[g][v]    += #{c : g(c) = g and some neighbour w of v has X_c(w) != X_c(v)}  (BOUNDARY)
 * The host counter n_measured is incremented at enqueue.  All sums are integers.  A first
 * kernel counts, per node tile and per slice of a group's chains, into 32-bit counters with one
 * owner each and leaves them with plain vector stores in a [slice][..] buffer; a second adds
 * the slices, in ascending order, into the uint64 accumulators, one owner each: no atomics in
 * HBM, and no dependence on thread order, tile sizes or slice sizes.  A slice has fewer than
 * 2^31 chains (n_chains is an int32), so the 32-bit counters bound no slice length.
 *
 * fw_chains_read_census synchronises, then copies one array, accumulated over all measurements
 * (n_groups = n_rungs, or 1 without a ladder):
 *   FW_CENSUS_OCC   uint64 [n_groups][n][k]
 *   FW_CENSUS_ECUT  uint64 [n_groups][n_edges]
 *   FW_CENSUS_BND   uint64 [n_groups][n]
 *   FW_CENSUS_CNT   uint64 [n_groups]
 * FW_ESTATE when the part was not enabled (CNT comes with any part), FW_EINVAL for another kind
 * or a buffer that is too small.  fw_chains_write_census restores any of the four (checkpoints;
 * n_measured is not changed); fw_chains_census_reset zeroes the arrays and n_measured.
 * fw_chains_census_info: info = {the enabled mask (0: none), label bits per node of the
 * handle's plans, n_groups, n_edges, n_measured}.  fw_chains_reset_observables leaves all of
 * this alone; fw_chains_set_ladder re-sizes the arrays for the new group count and zeroes them
 * and n_measured.  Left out: merging across ranks (the arrays are plain sums a caller can
 * all-reduce), weights per node or per chain, node-pair co-assignment.  (These entry points
 * arrived in 0.7 without a version bump; fw_build_info gained cen=<sha256 of fw_census.hip and
 * fw_census_plan.h>.) */
#define FW_CENSUS_NODES    1   /* enable mask: occupancy per node and district */
#define FW_CENSUS_EDGES    2   /* enable mask: cut count per edge              */
#define FW_CENSUS_BOUNDARY 4   /* enable mask: boundary count per node         */
#define FW_CENSUS_OCC  1       /* uint64 [n_groups][n][k]     */
#define FW_CENSUS_ECUT 2       /* uint64 [n_groups][n_edges]  */
#define FW_CENSUS_BND  4       /* uint64 [n_groups][n]        */
#define FW_CENSUS_CNT  8       /* uint64 [n_groups]           */
int fw_chains_enable_census(fw_chains* c, int32_t what);
int fw_chains_census_async(fw_chains* c);
int fw_chains_read_census(fw_chains* c, int32_t what, void* dst, size_t bytes);
int fw_chains_write_census(fw_chains* c, int32_t what, const void* src, size_t bytes);
int fw_chains_census_reset(fw_chains* c);
int fw_chains_census_info(const fw_chains* c, int64_t info[5]);

/* ---- pairwise plan distances between two lists of chains: matrix, row sums, nearest, histogram
 * The tally, geometry and census steps reduce one plan each, and the overlap step compares a
 * chain with its own reference or with one partner.  This step answers how far the plans of an
 * ensemble are from each other: the matrix that embedding, clustering, medoids, two-sample
 * tests between groups of chains and the count of distinct plans after a resample start from.
 * It runs on the device and between launches, as those steps are placed, from the label records;
 * no run kernel changes, and it only reads plans: it works on every label width, on both run
 * kernels' records, under a ladder (by chain id; grouping by rung is the caller's, through
 * fw_chains_rungs) and on cloned or resampled populations.
 *
 * fw_chains_pairdist_async: a is int32 [ma], b is int32 [mb], values chain ids in [0, n_chains),
 * duplicates allowed; b == NULL means b = a (the symmetric case; mb is ignored).  The lists are
 * validated on the host before the device is touched: FW_EINVAL for a NULL handle or a NULL a,
 * ma < 1, mb < 1 with b given, or a value out of range; FW_EUNSUPPORTED for ma * mb > 2^28;
 * FW_ENOMEM when a buffer cannot be grown (the handle keeps what it had).  The lists reach the
 * device through two pinned staging slots with events (the host waits only for the copy that
 * last used a slot); the call enqueues on the handle's stream with no stream wait and no host
 * synchronisation, except that a call whose lists are longer than any before waits for the
 * stream once before it lets the smaller buffers go.  fw_chains_last_kernel_ms is not touched.
 * With X_c the current plan of chain c (stuck chains like any other):
 *   D[i][j]     = #{v < n : X_{a_i}(v) != X_{b_j}(v)}                   int32 [ma][mb]
 *                 districts are compared by name, as FW_OVERLAP_DIST compares them (the
 *                 label-permutation-minimal distance stays on the host: plandist)
 *   rowsum[i]   = sum over j of D[i][j]                                  int64 [ma]
 *   nearest[i]  = (min over j of D[i][j], the lowest j attaining it)     int32 [ma][2]
 *                 in the symmetric case position j = i is left out, by position and not by
 *                 chain id, and with ma = 1 the entry is (-1, -1)
 *   hist[d]    += #{(i, j) : D[i][j] = d}                                uint64 [n + 1]
 *                 over the positions i < j in the symmetric case, over all (i, j) otherwise;
 *                 accumulated over measurements until fw_chains_pairdist_reset
 * and the host counter n_measured is incremented at enqueue.  A first kernel computes D in
 * tile x tile blocks of pairs from bit planes of the label words staged in LDS (only the blocks
 * on or above the diagonal in the symmetric case, stored to both D[i][j] and D[j][i]; the
 * diagonal is the computed value, which is 0); a second reads D with one wave per row.  Every
 * element of D, rowsum and nearest has one owning lane, ties in nearest go to the lowest j by a
 * fixed reduction, and hist is summed with 64-bit integer atomics: no result depends on the
 * tile, the chunk or the order of threads.  FLIPWALK_PWD_TILE (16, 32, 64) and
 * FLIPWALK_PWD_CHUNK (32-node groups per staging step) force the blocking, for tests.
 *
 * fw_chains_read_pairdist synchronises, then copies what the last measurement left
 * (FW_PAIRDIST_MATRIX, _ROWSUM, _NEAREST; FW_ESTATE before any measurement) or the accumulated
 * FW_PAIRDIST_HIST (all zero before any); FW_EINVAL for another kind or a buffer that is too
 * small.  fw_chains_write_pairdist restores FW_PAIRDIST_HIST (checkpoints; n_measured is not
 * changed; FW_EINVAL for any other kind); fw_chains_pairdist_reset zeroes hist and n_measured.
 * fw_chains_pairdist_info: info = {the last ma, the last mb, 1 if the last measurement was
 * symmetric, label bits per node of the handle's plans, n_measured, the tile, the chunk (of the
 * last measurement, or of the plan in force before any)}.  fw_chains_reset_observables and
 * fw_chains_set_ladder leave all of this alone.  Left out: matched distances and the k x k table
 * per pair on the device, distances to stored snapshots or across handles, weighted distances,
 * grouping by rung on the device, merging across ranks.  (These entry points arrived in 0.7
 * without a version bump; fw_build_info gained pwd=<sha256 of fw_pairdist.hip,
 * fw_pairdist_planes.h and fw_pairdist_plan.h>.) */
#define FW_PAIRDIST_MATRIX  0   /* int32 [ma][mb]  */
#define FW_PAIRDIST_ROWSUM  1   /* int64 [ma]      */
#define FW_PAIRDIST_NEAREST 2   /* int32 [ma][2]   */
#define FW_PAIRDIST_HIST    3   /* uint64 [n + 1]  */
int fw_chains_pairdist_async(fw_chains* c, const int32_t* a, int32_t ma, const int32_t* b,
                             int32_t mb);
int fw_chains_read_pairdist(fw_chains* c, int32_t what, void* dst, size_t bytes);
int fw_chains_write_pairdist(fw_chains* c, int32_t what, const void* src, size_t bytes);
int fw_chains_pairdist_reset(fw_chains* c);
int fw_chains_pairdist_info(const fw_chains* c, int64_t info[7]);

/* ---- node co-assignment across the chains: the pair matrix of a node list, by rung -----------
 * The census gives the one-point maps over the graph and fw_chains_pairdist_async the two-point
 * function over plans.  This step gives the two-point function over nodes: how many plans of
 * the ensemble put nodes u and v in the same district.  It is what cores (sets of nodes whose
 * fate is tied) and consensus maps are read from, it shows which regions of a flip walk are
 * frozen, and it is defined without reference to district names, so it keeps its meaning for
 * k > 2, where occupancy is blurred by label symmetry.  It runs on the device and between
 * launches, as the exchange, record, tally, geometry, overlap, census and pairdist steps are
 * placed, from the label records; no run kernel changes, and it only reads plans: it works on
 * every label width, on both run kernels' records, with the spatial maps enabled and on cloned
 * or resampled populations.
 *
 * fw_chains_enable_coassign: nodes is int32 [m], strictly ascending, values in [0, n);
 * nodes == NULL means all n nodes (m is ignored).  Everything is checked on the host before the
 * device is touched: FW_EINVAL for a NULL handle, m < 1, a value out of range or a list that is
 * not strictly ascending; FW_EUNSUPPORTED when n_groups * m * m > 2^28 (n_groups = n_rungs, or 1
 * without a ladder); FW_ENOMEM when a buffer cannot be allocated (the handle keeps what it had).
 * Allocates and zeroes the accumulators and zeroes n_measured; repeated, it replaces the node
 * list.  The plan is derived here, once: tiles of 64 list entries with the window of label
 * words each one's nodes span in a record, the member words of a group (32 members each), the
 * tile of the pair blocks and the chunk of member words staged at a time.
 *
 * fw_chains_coassign_async (FW_ESTATE before fw_chains_enable_coassign) enqueues on the
 * handle's stream, with no host synchronisation and without touching fw_chains_last_kernel_ms.
 * Groups are the census's: member i of group g is chain chain_of[i * n_groups + g] under a
 * ladder (the chain on rung g of set i, read on the device from the exchange step's own arrays:
 * the host does not wait for them), else chain i; per_group = n_chains / n_groups.  With X_c the
 * current plan of chain c (stuck chains like any other) it adds
 *   cnt[g]            += per_group
 *   together[g][i][j] += #{members c of g : X_c(nodes[i]) == X_c(nodes[j])}
 * so the matrix is symmetric and its diagonal equals cnt[g].  The host counter n_measured is
 * incremented at enqueue.  A first kernel transposes the labels of the listed nodes into bit
 * planes across the members (member i at bit i % 32 of member word i / 32; bits past per_group
 * zero), from label windows staged in LDS, or from the records in HBM where a tile's window is
 * too long; a second takes tile x tile blocks of node pairs on or above the diagonal, walks the
 * member words in chunks staged in LDS, counts per pair the differing members (XOR / OR /
 * popcount over the planes, as the pairwise distance does over nodes) and adds per_group - diff
 * to the uint64 accumulators, an off-diagonal block to both [i][j] and [j][i].  Every element
 * has one owning lane and there are no atomics: no result depends on the tile, the chunk, the
 * staging or the order of threads.  Counts of one measurement are 32 bits wide (per_group <
 * 2^31).  FLIPWALK_COA_TILE (16, 32, 64), FLIPWALK_COA_CHUNK (member words per staging step) and
 * FLIPWALK_COA_STAGE=0 (labels from HBM) force the plan, for tests; they are read at enable.
 *
 * fw_chains_read_coassign synchronises, then copies one array, accumulated over all
 * measurements:
 *   FW_COASSIGN_TOGETHER  uint64 [n_groups][m][m]
 *   FW_COASSIGN_CNT       uint64 [n_groups]
 *   FW_COASSIGN_NODES     int32 [m], the list in force (read only)
 * FW_ESTATE before enable; FW_EINVAL for another kind or a buffer that is too small.
 * fw_chains_write_coassign restores TOGETHER or CNT (checkpoints; n_measured is not changed;
 * FW_EINVAL for NODES); fw_chains_coassign_reset zeroes the arrays and n_measured.
 * fw_chains_coassign_info: info = {m (0: not enabled), label bits per node of the handle's
 * plans, n_groups, n_measured, the node tile of a pair block, the member-word chunk, 1 if the
 * label windows are staged in LDS}.  fw_chains_reset_observables leaves all of this alone;
 * fw_chains_set_ladder on an enabled handle re-sizes the arrays for the new group count and
 * zeroes them and n_measured, and switches the step off (as before enable) when the new size
 * exceeds the 2^28 bound.  Left out: subsets or weights of chains, merging across ranks (the
 * arrays are plain sums a caller can all-reduce), the k x k joint label table per node pair,
 * clustering on the device (coassign.py reads cores from the matrix on the host).  (These entry
 * points arrived in 0.7 without a version bump; fw_build_info gained coa=<sha256 of
 * fw_coassign.hip and fw_coassign_plan.h>.) */
#define FW_COASSIGN_TOGETHER 0  /* uint64 [n_groups][m][m] */
#define FW_COASSIGN_CNT      1  /* uint64 [n_groups]       */
#define FW_COASSIGN_NODES    2  /* int32 [m], read only    */
int fw_chains_enable_coassign(fw_chains* c, const int32_t* nodes, int32_t m);
int fw_chains_coassign_async(fw_chains* c);
int fw_chains_read_coassign(fw_chains* c, int32_t what, void* dst, size_t bytes);
int fw_chains_write_coassign(fw_chains* c, int32_t what, const void* src, size_t bytes);
int fw_chains_coassign_reset(fw_chains* c);
int fw_chains_coassign_info(const fw_chains* c, int64_t info[7]);

/* Read a map (FW_MAP_*) of chains [chain0, chain0 + n_chains) as int64
 * [n_chains][len], or with FW_MAP_SUM its sum over those chains [len]; len is
 * n_edges for FW_MAP_CUT_TIMES and n otherwise.  Values are current through the
 * last yield; FW_MAP_FINALIZE applies the reference's end-of-run rule. */
int fw_chains_read_map(fw_chains* c, int32_t what, int32_t chain0, int32_t n_chains,
                       int32_t flags, int64_t* dst, size_t bytes);

/* Batched per-flip evaluation on ONE state — the bit-exact per-step contract
 * (cut_edges updater, single_flip_contiguous, Bounds, b_nodes_bi):
 * for each i < m, flipping v[i] to target[i] gives
 *   dcut[i]      = len(cut_edges) after - before
 *   contig[i]    = 1 iff the old district of v[i] stays connected and non-empty
 *   pop_ok[i]    = 1 iff both changed districts stay inside [pop_lo, pop_hi]
 *   dboundary[i] = number of boundary nodes after - before
 * Flips with target == labels[v] or out-of-range values fail with FW_EINVAL. */
int fw_eval_flips(fw_graph* g, const int16_t* labels, int32_t k, const int32_t* v,
                  const int16_t* target, int32_t m, int64_t pop_lo, int64_t pop_hi,
                  int32_t* dcut, uint8_t* contig, uint8_t* pop_ok, int32_t* dboundary);

#ifdef __cplusplus
}
#endif

#endif /* FLIPWALK_H */
