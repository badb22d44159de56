/* rescan_hip.h — C ABI of librescan_hip.so, the MI355X (gfx950) implementation of Rescan's
 * per-scan geometric hot path.  Plain pointers and sizes only; no C++/torch types.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference tree, mhalber/Rescan).  Matrices are column-major float[16] exactly like
 * msh_mat4_t (lib/msh/msh_vec_math.h:187-191); point arrays are AoS float[3*n] exactly like
 * msh_vec3_t* (lib/msh/msh_vec_math.h:159-164).
 *
 * Return convention: functions returning int give 0 on success and a negative RS_HIP_E_*
 * code otherwise; rs_hip_last_error() describes the failure.  There is NO CPU fallback:
 * without a usable HIP device every compute entry point fails with RS_HIP_E_NODEVICE.
 */
#ifndef RESCAN_HIP_H
#define RESCAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_HIP_OK            0
#define RS_HIP_E_NODEVICE   -1   /* no HIP device / runtime error at init */
#define RS_HIP_E_ARG        -2   /* bad argument */
#define RS_HIP_E_RUNTIME    -3   /* HIP runtime error during the call */
#define RS_HIP_E_CAPACITY   -4   /* problem exceeds a documented limit */

/* ---- runtime ----------------------------------------------------------------------- */

/* Bind the calling process to HIP device `device` (one process per GPU). */
int         rs_hip_init( int device );
const char* rs_hip_last_error( void );
/* Use an existing hipStream_t (e.g. torch's current stream) for all launches; NULL = the
 * library's own stream. */
int         rs_hip_set_stream( void* hip_stream );
int         rs_hip_synchronize( void );
/* Restrict the calling thread's own stream to the compute units whose bits are set in mask (n_words x 32 bits, CU 0 = bit 0 of
 * word 0): independent operators issued from different threads can be kept off each other's CUs (a latency-bound chain beside
 * a throughput-bound batch).  Replaces the thread's stream; pending work on the old one is waited for.  (NULL, 0) goes back to an
 * unrestricted stream — do that before the process exits when a profiler is attached: rocprofv3 crashes in its finalisation when
 * masked streams are still alive. */
int         rs_hip_stream_cu_mask( const uint32_t* mask, int32_t n_words );
/* The HIP stream (hipStream_t) the calling thread's launches go to: its own, or the one given to rs_hip_set_stream.  NULL if the
 * library cannot be initialised. */
void*       rs_hip_get_stream( void );
/* ABI/version string, e.g. "rescan_hip 0.1 gfx950". */
const char* rs_hip_version( void );
/* The value the library would use now for one of its environment switches (RS_HIP_..., the table of rescan_amd/csrc/rs_switches.h:
 * the environment as read at the time that switch is read, or what its setter stored since).  A flag gives 0 or 1, a word 1 when
 * set.  RS_HIP_E_ARG for a name that is not in the table.  Needs no device. */
int         rs_hip_switch_get( const char* name, double* value );

/* Per-kernel timing with HIP events recorded on the launch stream.  While enabled, each
 * launch of a hot kernel is bracketed by an event pair; rs_hip_profile_read() synchronises
 * and returns launch count and summed milliseconds for kernel `name`
 * ("nn_icp", "icp_moments", "nn_score", "nn_label", "nn_rows", "edges", "coverage", "isect", "footprints").  The name "candidates" is
 * not a kernel: its launch count is the number of candidates the search kernels staged and evaluated
 * since the last reset (each of them by the 64 query lanes of its wave) — SURVEY.md §8d's second figure. */
int         rs_hip_profile_enable( int on );
int         rs_hip_profile_reset( void );
int         rs_hip_profile_read( const char* name, int64_t* launches, double* total_ms );
/* A named no-op kernel (rs::k_step_marker) on the calling thread's stream: marks where a caller's unit of work begins in a kernel trace. */
int         rs_hip_profile_marker( void );

/* ---- device-resident clouds -------------------------------------------------------- */

/* A cloud = positions (+ optional normals) laid out in HBM as 16-byte records
 * {x,y,z,orig_index} sorted by uniform-grid cell, plus the cell offset table: the device
 * counterpart of a cloud level and its msh_hash_grid_t
 * (lib/rs/rs_pointcloud.h:77-97,849-863; lib/msh/msh_hash_grid.h:248-269,388-541).
 * cell_size > 0 : grid cell edge in metres (msh_hash_grid uses 2*radius; any value gives the
 *                 same search results, it only changes speed).
 * cell_size < 0 : chosen from the cloud's sampling density (about two sample spacings) —
 *                 the fastest choice for the staged search.
 * cell_size = 0 : one cell holding everything ("brute-tile" layout). */
typedef struct rs_hip_cloud rs_hip_cloud_t;

rs_hip_cloud_t* rs_hip_cloud_create( const float* pos, const float* nor /* may be NULL */,
                                     int32_t n, float cell_size );
/* rs_hip_cloud_create for n_clouds clouds in one call. pos[k] / nor[k]: n[k] x 3 floats (nor == NULL: no cloud has normals;
 * nor[k] == NULL: cloud k has none; n[k] == 0: an empty cloud, pos[k] may be NULL). cell_sizes[k] as rs_hip_cloud_create's
 * cell_size (NULL: -1 for all). out[k]: a cloud whose layouts, host copies and reported sizes are those of
 * rs_hip_cloud_create( pos[k], nor[k], n[k], cell_sizes[k] ), to the byte. All or nothing: RS_HIP_OK, or an error code with out
 * untouched and nothing left allocated.  The stages of the build run once for the whole batch (the number of launches and
 * synchronisations does not grow with n_clouds), and the clouds of a batch share one device allocation, which is freed when the
 * last of them is destroyed; each is destroyed by rs_hip_cloud_destroy like any other. */
int             rs_hip_cloud_create_many( const float* const* pos, const float* const* nor, const int32_t* n, const float* cell_sizes,
                                          int32_t n_clouds, rs_hip_cloud_t** out );
/* A cloud of more than n points inside a batch is built alone, by rs_hip_cloud_create's own path (the result is the same).  Process-wide;
 * n < 0 only reads; returns the previous value.  Default: 499 999 — at 500 000 points the batch no longer beat the single builds
 * (profiles/r25/build_many_timing.txt). */
int32_t         rs_hip_cloud_many_single_above( int32_t n );
void            rs_hip_cloud_destroy( rs_hip_cloud_t* c );
int32_t         rs_hip_cloud_size( const rs_hip_cloud_t* c );
/* query tiles of the cloud: runs of at most 64 points of its Hilbert order, what one wave of a search takes */
int32_t         rs_hip_cloud_tiles( const rs_hip_cloud_t* c );
/* bytes of HBM held by the cloud */
int64_t         rs_hip_cloud_bytes( const rs_hip_cloud_t* c );
/* The cloud's points in the order they were given or produced: 3 * size floats each (either may be NULL; nor only of a cloud
 * with normals).  A copy of what the cloud keeps on the host: no device work.  For clouds that were built on the device
 * (rs_hip_cloud_create_level, rs_hip_cloud_create_resampled) this is how the caller sees their points. */
int             rs_hip_cloud_points( const rs_hip_cloud_t* c, float* pos, float* nor );
/* (tests, diagnostics) The two layouts a cloud was built into, read back as they are; changes nothing.  Two calls, sizes first:
 * with every array pointer NULL the call fills the scalars only (no device work); the caller then sizes its arrays from them, sets
 * the pointers it wants and calls again.  A pointer left NULL is skipped; nor / qnor only of a cloud with normals (RS_HIP_E_ARG).
 *   min, cell, inv_cell, dims   the uniform grid; cell = inv_cell = 0 and dims = {1, 1, 1} for the brute layout and an empty cloud.
 *                               cell is what was used: an explicit or derived cell doubled until the table has at most 48e6 cells
 *   n_cells                     dims[0] * dims[1] * dims[2]
 *   occupied                    the occupied-cell count the tile extent limit was derived from (brute layout: an estimate)
 *   extent_limit                the largest extent of a query tile on any axis (FLT_MAX for an empty cloud)
 *   cell_start[n_cells + 1]     offsets into the cell-sorted records; cell (x, y, z) has index (z * dims[1] + y) * dims[0] + x
 *   order[n], qorder[n]         original index of cell-sorted slot s / of Hilbert slot s; by_orig[n]: Hilbert slot of an original index
 *   tiles[n_tiles + 1]          first Hilbert slot of every query tile, then n
 *   pos, qpos (nor, qnor)       the 16-byte records of the two layouts as 4 * n words: the point's (normal's) bits and, in the
 *                               fourth word of a position record, its original index (0 in a normal record)
 * Inside a cell, and among equal Hilbert keys, points keep the order they were given in.  The bounds min / max are taken over
 * the finite coordinates of each axis ([0, 0] for an axis that has none).  A point with a coordinate that is not finite is stored
 * and counted like any other: on that axis it lies in cell 0 (NaN, -Inf) or in cell dims - 1 (+Inf), and no search returns it. */
typedef struct rs_hip_layout
{
  float    min[3], cell, inv_cell;
  int32_t  dims[3];
  int64_t  n, n_cells, occupied;
  float    extent_limit;
  int32_t  n_tiles, has_normals;
  uint32_t *cell_start;
  int32_t  *order, *qorder;
  uint32_t *tiles;
  int32_t  *by_orig;
  uint32_t *pos, *qpos, *nor, *qnor;
} rs_hip_layout_t;
int             rs_hip_cloud_layout( const rs_hip_cloud_t* c, rs_hip_layout_t* out );
/* (diagnostics) Where cloud construction went, in seconds of the calling threads' wall clock, summed over every cloud the process
 * built since the last reset: out[0] host copy of the arrays, [1] upload + bounds, [2] cell index (sort by cell, offset table),
 * [3] Hilbert order + tiles.  Returns the number of clouds counted; reset != 0 clears the counters. */
int64_t         rs_hip_cloud_build_seconds( double out[4], int32_t reset );

/* ---- bounded-K radius search ------------------------------------------------------- */

/* msh_hash_grid_radius_search (lib/msh/msh_hash_grid.h:1090-1259): for every query the
 * (at most) k nearest target points with dist² < radius², row-major rows of stride k.
 * Rows are always written in ascending (dist², index) order (the reference sorts when
 * search_desc.sort != 0 and leaves heap order otherwise; ascending is a valid answer to
 * both).  n_neighbors may be NULL.  Host pointers in, host pointers out.
 * Returns the total neighbour count through *total (may be NULL). */
int rs_hip_radius_search( const rs_hip_cloud_t* target, const float* query, int64_t n_query,
                          float radius, int32_t k,
                          float* distances_sq, int32_t* indices, size_t* n_neighbors,
                          uint64_t* total );

/* ---- k-nearest search on the reference's own grid ------------------------------------ */

/* msh_hash_grid_knn_search (lib/msh/msh_hash_grid.h:1291-1447), which is NOT an exact k-nearest
 * search: it walks the bins of a grid whose geometry comes from the init radius (the points' box
 * grown by 1e-4; cell = 2 radius, or max_dim / (32 sqrt 3) when radius <= 0; :413-449), shell by
 * shell around the query's bin, skips a bin beyond the k-th distance held after the previous shell
 * and stops one shell after k points are held.  A knn grid is that geometry over a device cloud's
 * points (built on the device; the cloud may be destroyed afterwards).  dim = 2: a cloud of
 * msh_hash_grid_init_2d points, (x, y, 0); its queries carry z = 0.  NULL on failure
 * (rs_hip_last_error(); a radius so small against the box that the grid would need more than 2^26
 * bins is refused rather than allocated). */
#define RS_HIP_KNN_MAX_K 64      /* k cap of rs_hip_knn_search (one 64-lane wave holds a query's rows) */
typedef struct rs_hip_knn_grid rs_hip_knn_grid_t;
rs_hip_knn_grid_t* rs_hip_knn_grid_create( const rs_hip_cloud_t* cloud, float radius, int32_t dim );
void               rs_hip_knn_grid_destroy( rs_hip_knn_grid_t* grid );
/* the grid's bins per axis (w, h, d), cell edge and origin (min_pt: the grown box's corner); cell / min_pt may be NULL */
int                rs_hip_knn_grid_geometry( const rs_hip_knn_grid_t* grid, int64_t dims[3], double* cell, float min_pt[3] );
/* The same geometry computed on the host from n AoS points (no device needed); RS_HIP_E_CAPACITY
 * where rs_hip_knn_grid_create would refuse the grid. */
int                rs_hip_knn_geometry( const float* pos, int64_t n, float radius, int32_t dim,
                                        int64_t dims[3], double* cell, float min_pt[3] );
/* For every query (3 floats; host pointers in and out, any n_query) the reference's rows: row i
 * holds n_neighbors[i] = min(k, points in the bins visited) entries, ascending in (dist², index),
 * at distances_sq / indices + i*k; entries past n_neighbors[i] are left untouched.  Where the
 * reference is undefined (a shell of more than 128 bins, fewer than k points, a query outside the
 * box) the walk has no bin cap and ends once every bin has been visited.  k <= RS_HIP_KNN_MAX_K,
 * else RS_HIP_E_CAPACITY.  n_neighbors and total may be NULL. */
int rs_hip_knn_search( const rs_hip_knn_grid_t* grid, const float* query, int64_t n_query, int32_t k,
                       float* distances_sq, int32_t* indices, size_t* n_neighbors, uint64_t* total );

/* ---- point-to-plane ICP ------------------------------------------------------------- */

/* icp_align (lib/rs/icp.h:416-500): aligns T1*source to T2*target; *T1 is updated in place,
 * the last RMS error is returned through *err (1e6 if no iteration produced one).
 * `source` and `target` must have normals.  max_iter: the reference uses 100.
 * fixed_iters != 0 disables the convergence test at icp.h:489 (benchmark mode).
 * n_iters (may be NULL) receives the number of correspondence searches made. */
int rs_hip_icp_align( const rs_hip_cloud_t* source, const rs_hip_cloud_t* target,
                      float* T1, const float* T2, float max_dist, float max_angle,
                      int32_t max_iter, int32_t fixed_iters, float* err, int32_t* n_iters );

/* The same call, also leaving the error after every iteration in errs_per_iter[0 .. *n_iters) (room for max_iter floats): what
 * icp_align( ..., verbose = true ) prints per iteration (icp.h:482-486).  Same result; the loop state is read after every iteration
 * instead of every few, so it is slower by a synchronisation per iteration. */
int rs_hip_icp_align_traced( const rs_hip_cloud_t* source, const rs_hip_cloud_t* target,
                             float* T1, const float* T2, float max_dist, float max_angle,
                             int32_t max_iter, int32_t fixed_iters, float* err, int32_t* n_iters, float* errs_per_iter );

/* Per-iteration trace of the calling thread's ICP calls (rs_hip_icp_align, _batch — slices included — and _multi) from
 * rs_hip_icp_trace_begin to rs_hip_icp_trace_end.  For problem p (its index in the call) and iteration i < max_iter, row
 * r = p * max_iter + i receives the pose after the iteration (poses[16 r ..]), its error (errs[r]) and the estimator step that
 * ran (kinds[r], RS_HIP_ICP_STEP_*); rows of iterations that did not run keep kind RS_HIP_ICP_STEP_NONE and NaN.  A problem run
 * again in the reference's order by the stop test's guard has the rows of the run whose result is returned and redone[p] = 1.
 * Same results as untraced; the loop state is read after every iteration.  Begin fills every row and redone[] afresh. */
#define RS_HIP_ICP_STEP_NONE        -1
#define RS_HIP_ICP_STEP_REF_ORDER    0   /* the reference's own accumulation order (k_icp_faithful): its bits */
#define RS_HIP_ICP_STEP_REPLAY       1   /* the same bits in parallel (rs_hip_icp_replay_below) */
#define RS_HIP_ICP_STEP_LANE_CHAINS  2   /* the reference's fp32 centroid chains by one wave per chain + fp64 moments */
#define RS_HIP_ICP_STEP_GRID_CHAINS  3   /* the same chains spread over the chip + fp64 moments */
#define RS_HIP_ICP_STEP_PLAIN        4   /* early plain step: fp64 moments centred on their own fp64 centroids (rs_hip_icp_early_plain) */
#define RS_HIP_ICP_STEP_RECORDS      5   /* the chains' sums by pass 2 of the replay from the searches' records (after the chains gave up) */
#define RS_HIP_ICP_STEP_MOMENTS      6   /* plain k_icp_moments (rs_hip_icp_exact_centroids( 0 )) */
int rs_hip_icp_trace_begin( float* poses, float* errs, int32_t* kinds, int32_t* redone, int32_t max_iter, int32_t n_problems );
int rs_hip_icp_trace_end( void );

/* The estimator step (icp.h:136-148,210-298,393-402), by source size (round 6; priced against the bar on every reference fixture:
 * profiles/r06/estimator_policy.txt).  Sources of at most `n_points` points use the reference's own accumulation order and
 * precisions (one sequential fp32 chain per accumulator): poses, errors and iteration counts are bit-identical to the
 * reference's.  Default 16384 — every level-2 object of the reference's call sites — (environment RS_HIP_REF_ORDER_BELOW); 65536 covers all of them, at
 * 520 instead of 110 us per iteration on a 50 k-point source.  Larger sources: see rs_hip_icp_replay_below (opt-in),
 * rs_hip_icp_lane_chains_below (default up to 65536 points), beyond that the grid chains — all three centre the step on the
 * reference's own fp32 centroid sums, bit for bit, and differ from it only where it rounds the 33 accumulators of the normal
 * equations after every addition (<= 3e-6 in the pose on its fixtures, equal iteration counts).  n_points < 0 only reads.  Returns
 * the previous threshold.  Applies to rs_hip_icp_align, _batch, _multi and rs_hip_icp_estimate_pt2pl. */
int32_t rs_hip_icp_reference_order_below( int32_t n_points );
/* Sources larger than that, up to `n_points` points (default 0 = off since round 6; environment RS_HIP_REPLAY_BELOW), get the SAME sums —
 * the reference's sequential fp32 / fp64 chains, bit for bit — computed in parallel: segments of 128 points are added
 * speculatively from a guessed start, for both parities of its last mantissa bit, and a walk over the segments with the exact
 * value accepts a segment when the accumulator provably stayed inside its binade.  0 = never; n_points < 0 only
 * reads.  Returns the previous threshold.  rs_hip_icp_replay_redone(): segments the last call's walks had to re-add one addend
 * after the other (a diagnostic: binade crossings, chain starts). */
int32_t rs_hip_icp_replay_below( int32_t n_points );
int32_t rs_hip_icp_replay_redone( void );
/* Round 6.  Sources above both thresholds and of at most `n_points` points take the LANE chains: the reference's 2.5 sigma cut, its
 * seven weighted-centroid sums (lib/rs/icp.h:136-148) as the sequential fp32 chains they are, bit for bit — one wave per chain, 256
 * addends per step on the integer grid of the running sum's binade, in fp32 one after the other wherever that does not hold — and the
 * normal equations (:226-252) as a parallel fp64 reduction centred on those centroids.  Not the reference's bits: measured on every
 * reference fixture of that size at most 3e-6 from its pose, equal iteration counts (profiles/r06/estimator_policy.txt).  Any
 * number of differently sized problems run side by side (rs_hip_icp_align_multi).  Larger sources take the grid chains (the same
 * sums spread over the chip) — and so does a call with ONE problem from 28672 points on: same sums, same poses bit for bit, faster with
 * the chip to itself (tools/lane_vs_grid.py); a threshold set beyond 65536 keeps such calls on the lane chains too.  n_points < 0 only
 * reads; returns the previous threshold.  Environment: RS_HIP_LANE_CHAINS_BELOW.
 * rs_hip_icp_lane_chains_sequential(): addends those walks added one by one since rs_hip_init (a diagnostic: chain starts, binade
 * changes, ties, sums that hover around zero). */
int32_t rs_hip_icp_lane_chains_below( int32_t n_points );
int64_t rs_hip_icp_lane_chains_sequential( void );
/* The stop test's guard (round 6).  The estimators above that are not the reference's own order follow its per-iteration errors to
 * 1e-8 ... 6e-7; icp_align's stop test |err - prev_err| < 1e-5 (icp.h:489) decided by less than that can fall the other way (one
 * iteration more or less: 1e-4 in the pose).  A problem whose decisive difference comes within 1.5e-6 of the threshold (environment
 * RS_HIP_STOP_GUARD, 0 = off) is run AGAIN in the reference's own order — its bits — where one exists (sources up to 262144 points).
 * Returns how many problems were, since rs_hip_init. */
int64_t rs_hip_icp_stop_guard_redone( void );
/* Plain early iterations (round 6).  The chains above fix where the iteration CONVERGES; far from the end an iteration only has to bring the
 * pose near.  With this on (default; environment RS_HIP_EARLY_PLAIN=0 turns it off) a call on a scan-sized source (more than 65536 points) runs the
 * plain step — fp64 moments centred on their own fp64 centroids, two launches instead of six — in its early iterations, keeping chain
 * iterations before any iteration whose result can be returned: a fixed-length call (fixed_iters) runs plain until TWO before its end; a call
 * with the stop test in its first four iterations (three chain iterations before the first decision), and only for sources above 262144
 * points (below, the stop test's guard wants the reference's errors from the start).  Measured on six 1 M-point rooms: <= 3.7e-6 from the
 * reference's pose (<= 1.2e-6 without; with ONE chain iteration 1.1e-5: not shipped; profiles/r06/early_plain.txt).
 * Object-sized sources (up to 65536 points, whichever kernels run their chains) keep them in every iteration.  on < 0 only reads; returns the previous setting. */
int32_t rs_hip_icp_early_plain( int32_t on );
/* Plain iterations without records (round 10).  A plain step sums its moments in no particular order, so its search writes no 48-byte
 * record per source point: it leaves matched slot, dist² and dot (12 B per point) and the moments are formed from those in the source's
 * tile order, in fp64, by a fixed schedule (two runs give the same bits; against the step from records only the order of the fp64
 * additions differs).  on = 1 (environment RS_HIP_PLAIN_RECORDS=1) brings the plain step from records back: for A/B runs and tests.
 * on < 0 only reads; returns the previous setting.  The trace kind of both is RS_HIP_ICP_STEP_PLAIN. */
int32_t rs_hip_icp_plain_from_records( int32_t on );
/* The launch that ends an iteration of a scan-sized source (35 workgroups sum the moments' partials, the last one to finish solves)
 * hands its 35 sums over by agent-scope atomic stores, a relaxed ticket and atomic loads.  on = 1 (environment RS_HIP_UPDATE_FENCED=1)
 * brings back the hand-over by two full memory fences: the same bits, for A/B runs and tests.  on < 0 only reads; returns the previous
 * setting. */
int32_t rs_hip_icp_update_fenced( int32_t on );
/* (tests) The loop state an ICP call keeps on the device: 4-byte words per problem, and the largest state block, in words, that is written by
 * the call's fill launch from its argument block (larger batches: a host-to-device copy).  The results do not depend on which. */
void    rs_hip_icp_state_layout( int32_t* words_per_problem, int32_t* launch_max_words );
float   rs_hip_icp_stop_guard( float guard );      /* sets the guard's width (0: off); < 0 only reads; returns the previous width */
/* The sequential estimator (sources up to rs_hip_icp_reference_order_below) runs the reference's dist² statistics and its weighted
 * centroids in ONE pass, the 2.5 sigma cut of the weights (lib/rs/icp.h:396-401) taken at a guess of sigma; the pass stands when no
 * dist² lies between the guessed and the real cut, else the centroids are summed again.  Iterations that had to, over every calling
 * thread of the process, since the first ICP call (diagnostics). */
int32_t rs_hip_icp_faith_redone( void );
/* Test switch of that guess, in thousandths: 1000 (default) the guess as made, 0 no guess (statistics, centroids and normal equations
 * in three passes, as up to round 3), any other value scales the guessed cut — a guess that fails, for the tests of the check and of
 * the fallback.  Returns the previous value; < 0 only queries. */
int32_t rs_hip_icp_faith_guess( int32_t permille );
/* Sources above both thresholds (whole million-point scans): the parallel fp64 reduction, centred on the REFERENCE'S centroids —
 * the seven sums behind icp__compute_weighted_centroid (icp.h:136-148: Σw, Σw·p, Σw·q) are computed as the reference's own
 * sequential fp32 chains, bit for bit.  Those chains carry a systematic rounding drift (parts in a thousand of Σw once the running
 * sum's grid is coarser than the spread of the addends) that moves the reference's converged pose by up to 3e-4 from the exact
 * least-squares one; with its centroids the fp64 step lands within ~1e-6 of the reference's pose.  on = 0: plain fp64
 * moments (faster by the chains' cost, within 1e-4 of the reference in most runs only); on < 0 only reads; environment
 * RS_HIP_EXACT_CENTROIDS.  Returns the previous setting. */
int32_t rs_hip_icp_exact_centroids( int32_t on );
/* How many rs_hip_icp_align[_batch] calls the grid chains gave up so far (sums that keep changing binade — coordinates that straddle
 * the origin in a cancelling order) and ran again with the centroid sums by pass 2 of the replay: same result, ~10x the estimator time. */
int32_t rs_hip_icp_chains_gave_up( void );
/* A source cloud whose chains gave a problem up goes straight to the replay on its next `calls` calls as an ICP source (default 15;
 * environment RS_HIP_CHAINS_RETRY_AFTER) instead of paying for the failed attempt each time; 0 = every call tries the chains first
 * (tests that compare the two paths on centred scans use this); calls < 0 only reads.  The skip is per source cloud, whatever the
 * poses and the target.  Returns the previous value. */
int32_t rs_hip_icp_chains_retry_after( int32_t calls );

/* Many independent icp_align problems of one (source, target) pair, one per start pose
 * (apps/pose_proposal/main.cpp:190-202 runs exactly this loop): T1s is float[16*n], errs
 * float[n], iters int32[n] (may be NULL).  All problems advance in lock-step launches. */
int rs_hip_icp_align_batch( const rs_hip_cloud_t* source, const rs_hip_cloud_t* target,
                            float* T1s, int32_t n, const float* T2, float max_dist, float max_angle,
                            int32_t max_iter, int32_t fixed_iters, float* errs, int32_t* iters );

/* Many independent icp_align problems with a DIFFERENT source each against one target — the per-placement refine loop of
 * lib/rs/rs_database.h:220-230 (rsdb_refine_alignment_of_objects_to_scene) and apps/pose_proposal/main.cpp:190-202 — as one
 * call: problem p aligns sources[p] from T1s[16 p].  Sources of at most rs_hip_icp_reference_order_below() points (every call
 * site of the reference) advance in lock-step launches, grid.y = problem, each problem on its own source view; a batch that
 * holds a larger source runs problem by problem.  Every problem's pose, error and iteration count are what rs_hip_icp_align
 * returns for it alone, bit for bit. */
int rs_hip_icp_align_multi( const rs_hip_cloud_t* const* sources, const rs_hip_cloud_t* target,
                            float* T1s, int32_t n, const float* T2, float max_dist, float max_angle,
                            int32_t max_iter, int32_t fixed_iters, float* errs, int32_t* iters );

/* icp_find_corrs (lib/rs/icp.h:306-412), one call: compacted correspondences in source
 * order.  Output arrays are caller-allocated with capacity 3*n_source floats (weights:
 * n_source); *n_corrs receives the count. */
int rs_hip_icp_find_corrs( const rs_hip_cloud_t* source, const rs_hip_cloud_t* target,
                           const float* T1, const float* T2, float max_dist, float max_angle,
                           float* corr_pts1, float* corr_nor1, float* corr_pts2, float* corr_nor2,
                           float* weights, int32_t* n_corrs );

/* ---- alignment score ---------------------------------------------------------------- */

/* mgs_compute_object_alignment_score (apps/pose_proposal/pose_proposal.cpp:93-158) for
 * n_poses poses at once: scores[p] = score of `object` placed by poses[16*p..] against
 * `scene`.  radius = search_radii[search_lvl] (0.1 at the reference's search_lvl = 1, also
 * used as the distance sigma), max_n_neigh = 64 (proposal/verification) or 32 (refinement). */
int rs_hip_alignment_scores( const rs_hip_cloud_t* object, const rs_hip_cloud_t* scene,
                             const float* poses, int32_t n_poses, float radius, int32_t max_n_neigh,
                             float* scores );
/* Batches of at least `n_queries` (poses x object points) on a scene with a cell grid take the scene-space route: every transformed
 * query is keyed by the scene-aligned block it falls in (and the way its normal faces), the keys are radix-sorted, and a wave
 * searches 64 queries of one block whatever poses they come from — a third of the candidate evaluations of the object-space
 * launch for the same bits.  Default 65536 (environment RS_HIP_SCORE_SCENE_MIN; RS_HIP_SCORE_SCENE=0: never), and only
 * batches whose queries are dense in the scene take it (>= 128 per 0.1 m block of the lattice they span, RS_HIP_SCORE_SCENE_DENSITY: a
 * proposal's verification, not a grid search over the whole room); a threshold of 0 takes it whatever the density.
 * n_queries < 0 only reads.  Returns the previous threshold. */
int64_t rs_hip_score_scene_space_from( int64_t n_queries );

/* ---- label transfer ----------------------------------------------------------------- */

typedef struct rs_hip_placement
{
  float                 pose[16];   /* rs_obj_plcmnt_t.pose */
  const rs_hip_cloud_t* object;     /* the placed object's level-1 cloud */
  float                 radius;     /* search radius for this placement */
} rs_hip_placement_t;

/* rspf__assign_temporary_labels (lib/rs/rs_pointcloud_filters.cpp:738-778) over
 * placements[0..n) in the given order, continuing from the caller's labels / min_dists
 * (int8 / float, length = scene size, scene input order).  labels[j] receives
 * label_base + i + 1 for the winning placement i. */
int rs_hip_assign_labels( const rs_hip_cloud_t* scene, const rs_hip_placement_t* placements,
                          int32_t n, int32_t label_base, int8_t* labels, float* min_dists );

/* The per-placement "unary cost rows" of the same loop, for sharding placements across
 * GPUs: rows[i*scene_n + j] = dist² of scene point j to placement i's nearest object point
 * if one lies within the radius AND passes the 70° normal gate, +inf otherwise.
 * rows_device = 0: `rows` is a host pointer.  rows_device = 1: a device pointer (e.g. a torch tensor that will be
 * all-gathered), rows indexed by scene point in input order like the host form.  rows_device = 2: a device pointer, rows
 * indexed by the scene cloud's QUERY slot — the order the kernel produces them in (coalesced, no re-ordering pass);
 * rs_hip_fold_label_rows_device takes such rows when it is given the same scene cloud (every rank of the multi-GPU route
 * builds the same cloud from the same scene, so the rows of all ranks share that order). */
int rs_hip_label_rows( const rs_hip_cloud_t* scene, const rs_hip_placement_t* placements,
                       int32_t n, float* rows, int rows_device );

/* Ordered arg-min over gathered rows, host side: applies rows 0..n-1 in order with the
 * strict `<` of rs_pointcloud_filters.cpp:763 (earlier placement wins ties). */
void rs_hip_combine_label_rows( const float* rows, int32_t n_rows, int64_t scene_n, int32_t label_base,
                                int8_t* labels, float* min_dists );

/* The same ordered arg-min over rows that already sit in DEVICE memory — the gathered send buffers of the multi-GPU
 * route (placements sharded across GPUs, rows all-gathered over RCCL, then folded in the sorted order of
 * rs_pointcloud_filters.cpp:823-848).  Row k starts at rows_device + row_offsets[k] (in floats; row_offsets is a host
 * array, so rows of different ranks may sit anywhere in one gathered buffer) and holds scene_n floats.  labels / min_dists
 * are host arrays: continued from the caller's values like rs_hip_assign_labels, or — fresh != 0 — started on the device
 * from the loop's initial state (label 0, min_dist 1e9: rs_pointcloud_filters.cpp:799-802,820) without an upload. */
int rs_hip_fold_label_rows_device( const float* rows_device, const int64_t* row_offsets, int32_t n_rows, int64_t scene_n,
                                   int32_t label_base, int8_t* labels, float* min_dists, int32_t fresh,
                                   const rs_hip_cloud_t* rows_in_query_order_of /* NULL: rows in input order */ );

/* The lighter exchange of the same split: instead of one row per placement, a rank sends the PARTIAL of its own contiguous run of
 * the sorted arrangement — the loop's running (min_dist, label) after that run, started from (1e9, 0): 5 bytes per scene point
 * whatever the number of placements (4.9 MB instead of 31 MB per rank at 8 placements per rank and 1 M scene points).  Folding the
 * ranks' partials in rank order with the loop's strict `<` gives the bits of the sequential loop, because the runs are contiguous
 * and in order.  rs_hip_label_partial_device writes the partial of placements[0..n) into device memory (e.g. the RCCL send
 * buffer), indexed by the scene cloud's query slot; labels carry label_base + i + 1.  rs_hip_fold_label_partials_device folds
 * n_parts gathered partials (rank r's min_dists at base_device + min_offsets[r] floats, its labels at (int8*)base_device +
 * label_offsets[r] bytes; host arrays of offsets) and returns the result in input order. */
int rs_hip_label_partial_device( const rs_hip_cloud_t* scene, const rs_hip_placement_t* placements, int32_t n, int32_t label_base,
                                 float* min_dists_device, int8_t* labels_device );
int rs_hip_fold_label_partials_device( const float* base_device, const int64_t* min_offsets, const int64_t* label_offsets, int32_t n_parts,
                                       int64_t scene_n, int8_t* labels, float* min_dists, const rs_hip_cloud_t* in_query_order_of );

/* rspf_arrangement_to_labels ordering + two passes (lib/rs/rs_pointcloud_filters.cpp:780-848):
 * sorts placement indices (dynamic first, then by class index; stable), runs the dynamic
 * pass with `radius` and the static pass with 1.5*radius (or resets min_dists when
 * prioritize_static).  is_static / class_idx are per placement.  sorted_order (may be NULL)
 * receives the permutation; labels index into the sorted order, 1-based, 0 = unlabelled.  min_dists may be NULL (the reference
 * frees its own before it returns, :871-872: the shim's rsd_arrangement_to_labels does not download them). */
int rs_hip_arrangement_to_labels( const rs_hip_cloud_t* scene,
                                  const float* poses /* 16*n */, const rs_hip_cloud_t* const* objects /* n */,
                                  const int32_t* is_static, const int32_t* class_idx, int32_t n,
                                  float radius, int prioritize_static,
                                  int8_t* labels, float* min_dists, int32_t* sorted_order );

/* The same plus the function's tail (lib/rs/rs_pointcloud_filters.cpp:851-869): temporary labels -> in_pc->class_ids[lvl] /
 * instance_ids[lvl] — class of the labelled placement's object and the placement's uidx; label 0 gives
 * (unlabelled_class_idx = rsdb_get_class_idx( rsdb, "unlabelled" ), RSPF_MAX_INSTANCES = 1024).  uidx is per placement
 * (rs_obj_plcmnt_t.uidx).  labels / min_dists / sorted_order may be NULL. */
int rs_hip_arrangement_to_ids( const rs_hip_cloud_t* scene,
                               const float* poses /* 16*n */, const rs_hip_cloud_t* const* objects /* n */,
                               const int32_t* is_static, const int32_t* class_idx, const int32_t* uidx, int32_t n,
                               float radius, int prioritize_static, int32_t unlabelled_class_idx,
                               int32_t* class_ids, int32_t* instance_ids, int8_t* labels, float* min_dists, int32_t* sorted_order );

/* ---- level builder ---------------------------------------------------- */

/* rs_pointcloud__compute_level_poisson (lib/rs/rs_pointcloud.h:984-1106): Poisson-disk subsample of
 * `cloud` in INPUT order — the first point no earlier sample has marked becomes a sample and marks
 * every point within `radius` of it (the reference's searches return at most max_n_neigh points;
 * for level L it uses radius = voxel_size[L] = 0.005·2^L and max_n_neigh = 1024·L/4, 256 for L = 0,
 * :995-996,1011).  sample_idx (capacity = cloud size) receives the sample indices in increasing
 * order — the order in which the reference fills the level's arrays (:1090-1099); n_rounds (may be
 * NULL) the number of decision rounds the device needed.  If some point has more than max_n_neigh
 * points within the radius a reference search would be truncated to its max_n_neigh nearest; that
 * case is not reproduced: the call fails with RS_HIP_E_CAPACITY and writes nothing. */
int rs_hip_level_samples( const rs_hip_cloud_t* cloud, float radius, int32_t max_n_neigh,
                          int32_t* sample_idx, int32_t* n_samples, int32_t* n_rounds );

/* The level as a cloud of its own, built without leaving the device: the samples of `base` (as above), the gather of
 * their positions / normals (rs_pointcloud.h:1090-1099) and the level's search index
 * (rs_pointcloud_compute_search_grid, :849-863; cell_size as for rs_hip_cloud_create).  sample_idx (may be NULL,
 * capacity = size of base) and n_samples (may be NULL) receive the samples.  NULL on failure. */
rs_hip_cloud_t* rs_hip_cloud_create_level( const rs_hip_cloud_t* base, float radius, int32_t max_n_neigh, float cell_size,
                                           int32_t* sample_idx, int32_t* n_samples );

/* Levels of many clouds in one call. Problem (c, l) = level l of bases[c]: the samples rs_hip_level_samples( bases[c], radii[l],
 * max_n_neigh[l] ) returns, and out[c * n_levels + l] the cloud rs_hip_cloud_create_level( bases[c], radii[l], max_n_neigh[l],
 * cell_sizes ? cell_sizes[l] : -1 ) makes of them, to the byte (layouts, host copies, reported sizes).  The reference samples every
 * level from level 0 (rs_pointcloud.h:989-1011, :1305-1315), so the problems are independent and are decided side by side: one
 * neighbourhood sweep per base at the largest radius, one frontier launch per step for all problems, one batched index build; the
 * launches and read-backs of a call do not grow with n_clouds or n_levels.
 *   All or nothing: RS_HIP_OK, or an error code with out / sample_idx / n_samples untouched and nothing left allocated.
 *   Over-cap: if any point of any problem has more than that level's max_n_neigh points within that level's radius the whole call
 *   fails with RS_HIP_E_CAPACITY; the text names the lowest (cloud index, level index) that is over.  Decided after the counting
 *   pass, before anything is written through the counts.
 *   Accepted: an empty base (each of its levels is an empty cloud), the same base listed more than once, bases with and without
 *   normals in one batch (a level has normals iff its base has), n_clouds == 0 or n_levels == 0 (RS_HIP_OK, nothing done), radii in
 *   any order, equal radii with different caps.
 *   RS_HIP_E_ARG, before any launch: a NULL base, a radius that is not > 0, a cap <= 0, n_levels > 8, n_clouds * n_levels > 32768.
 *   RS_HIP_E_CAPACITY, before any launch: the bases decided together have more than 2^30 = 1 073 741 824 (points x n_levels) in sum
 *   — a frontier item is (global id << 1) | flag in an int.  (A base of more than 1 000 000 points is not decided with the others
 *   but by rs_hip_level_samples' own path inside the call, and does not count.)
 *   The clouds of a call share device allocations, freed with the last of them; each is destroyed by rs_hip_cloud_destroy.  The
 *   bases may be destroyed right after the call. */
int rs_hip_level_samples_many( const rs_hip_cloud_t* const* bases, int32_t n_clouds,
                               const float* radii, const int32_t* max_n_neigh, int32_t n_levels,
                               int32_t* const* sample_idx,   /* [c * n_levels + l], capacity size of bases[c]; an entry may be NULL */
                               int32_t* n_samples,           /* n_clouds * n_levels */
                               int32_t* n_rounds );          /* may be NULL: frontier steps the batch needed */
int rs_hip_cloud_create_levels_many( const rs_hip_cloud_t* const* bases, int32_t n_clouds,
                                     const float* radii, const int32_t* max_n_neigh, const float* cell_sizes /* may be NULL */, int32_t n_levels,
                                     rs_hip_cloud_t** out,   /* n_clouds * n_levels */
                                     int32_t* const* sample_idx /* may be NULL as a whole or per entry */, int32_t* n_samples /* may be NULL */ );

/* The gathers that end the level builder (lib/rs/rs_pointcloud.h:1090-1099): for each of n_arrays per-point arrays of the
 * base level (host pointers, `words[a]` 32-bit words per point: 3 for positions / normals / colours, 1 for radii, qualities,
 * class and instance ids), dst[a][i] = src[a][sample_idx[i]].  Entries with a NULL src or dst are skipped. */
int rs_hip_gather_attributes( const int32_t* sample_idx, int32_t count, int32_t n_src,
                              const void* const* src, const int32_t* words, void* const* dst, int32_t n_arrays );

/* ---- mesh resampler: the level-0 cloud of a mesh ---------------------------- */

/* rs_pointcloud_uniform_resample (lib/rs/rs_pointcloud.h:1132-1227), the call rs_pointcloud_from_files sends every PLY
 * with faces through (:1268-1276), bit for bit: positions, normals, colours, radii, class and instance ids of the
 * n_samples = (size_t)( 0.5 * total_area * 12800.0 ) samples.  The reference threads two PCG32 generators
 * (lib/msh/msh_std.h:1413-1470; seeds 12346 for the barycentric draws, 64321 for the alias sampler) through its loop and
 * takes exactly two draws from each per sample, so sample i is computed on its own from the states 2 i steps after the
 * seeding.  Face areas (:1143-1154; msh_vec3_cross / msh_vec3_norm, msh_vec_math.h:974,988), their double sum, the sample
 * count and the alias table (msh_distrib2pdf + msh_discrete_distribution_update, msh_std.h:1843-1849,1863-1925 — with
 * the normaliser msh_accumulated rounds to float) are made on the host; the samples on the device.  Qualities, which the
 * reference leaves unset, are not an output.
 *
 * Refusals, all decided on the host before any launch (rs_hip_last_error() says which):
 *   RS_HIP_E_ARG       a vertex index outside [0, n_vertices); n_faces <= 0; a total area that is not finite; an fp32 area
 *                      sum <= 1e-8 (the reference then samples from an uninitialised pdf, msh_std.h:1846)
 *   RS_HIP_E_CAPACITY  n_faces > 2^24 (beyond it (float)n_faces is inexact and the reference's alias column can reach
 *                      n_faces); n_samples > INT32_MAX
 *
 * pos: 3 * n_vertices floats; faces: 3 * n_faces vertex indices. */

/* The host part alone; needs no device.  n_samples, total_area (the double sum), and the alias table: prob / alias
 * (each may be NULL, n_faces entries).  An alias entry the reference never writes (its prob is 1.0) holds its own index. */
int rs_hip_resample_plan( const float* pos, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                          int64_t* n_samples, double* total_area,
                          double* prob /* may be NULL, n_faces */, int32_t* alias /* may be NULL, n_faces */ );

/* Samples first .. first + count - 1 of the reference's sequence; host pointers in and out.  An attribute whose input or
 * output pointer is NULL is skipped; pos and out_pos are required.  The window must lie inside [0, n_samples]
 * (RS_HIP_E_ARG otherwise); count = 0 succeeds and writes nothing.  out_face (may be NULL): the face each sample lies on.
 * A sample does not depend on the window it is asked for in, so windows that partition [0, n_samples) give the whole
 * sequence.  A normal whose interpolated sum is zero is NaN, as in the reference (1 / sqrtf( 0 ) times 0). */
int rs_hip_uniform_resample( const float* pos, const float* nor, const float* col, const float* radii,
                             const int32_t* class_ids, const int32_t* instance_ids, int64_t n_vertices,
                             const int32_t* faces, int64_t n_faces, int64_t first, int64_t count,
                             float* out_pos, float* out_nor, float* out_col, float* out_radii,
                             int32_t* out_class, int32_t* out_instance, int32_t* out_face /* may be NULL */ );

/* The whole level-0 cloud, sampled and indexed without leaving the device: the samples' positions (and normals, where
 * nor is not NULL) are written where the index build of rs_hip_cloud_create_level reads them (cell_size as for
 * rs_hip_cloud_create).  n_samples may be NULL.  NULL on failure; rs_hip_cloud_points hands the points to the host. */
rs_hip_cloud_t* rs_hip_cloud_create_resampled( const float* pos, const float* nor, int64_t n_vertices,
                                               const int32_t* faces, int64_t n_faces, float cell_size, int64_t* n_samples );

/* The step before the resampler, for a mesh that comes without normals (surface reconstruction hands such meshes back):
 * rs_pointcloud__compute_normals (lib/rs/rs_pointcloud.h:556-596), which rs_pointcloud__load_ply calls for a PLY with faces and
 * no normals (:716-723); loader_pass != 0 adds the loader's own pass over the result (:743-751).  Bit for bit, all fp32:
 *   face normal   cross( p2 - p1, p3 - p1 ), not normalised (msh_vec_math.h:974-979)
 *   vertex chain  faces in ascending index, corners 1, 2, 3: n[v] = lerp( n[v], normal, 1.0f / ( (float)counts[v] + 1.0f ) )
 *                 (msh_vec3_lerp: u = 1.0f - t, t * b + u * a); counts advance after the face's three corners, so a face that
 *                 names a vertex twice or three times applies the lerp that often with one t and adds 2 or 3 to the count
 *   finish        norm > 0 -> n * ( 1.0f / sqrtf( sum ) ); otherwise (0, 1, 0): a vertex no face names, a sum that cancels to
 *                 zero, a NaN (it fails the compare).  An infinite norm passes and normalises to NaN, as in the reference
 *   loader pass   msh_vec3_normalize once more; a normal with a NaN component becomes (0, 0, 0)
 * Where the reference's value is NaN the device's is NaN too; its sign and payload are the multiplier's.
 * Host pointers; out_nor 3 * n_vertices floats; counts (may be NULL) n_vertices: the corners that name each vertex.
 *
 * Refusals, each RS_HIP_E_ARG and decided before a device is touched, with nothing written: a NULL pos, faces or out_nor;
 * n_vertices <= 0; n_faces <= 0 (the reference then leaves malloc'ed memory unwritten, :718-722); a vertex index outside
 * [0, n_vertices) (the reference reads out of bounds); 3 * n_faces or n_vertices above INT32_MAX.  Coordinates that are not
 * finite are NOT refused: the reference's function is defined on them. */
int rs_hip_vertex_normals( const float* pos, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                           int32_t loader_pass, float* out_nor, int32_t* counts /* may be NULL */ );

/* A mesh as a PLY without normals holds it -> the indexed level-0 cloud, without leaving the device: the normals above with
 * the loader pass, written into the vertex records the sampler reads, then exactly what rs_hip_cloud_create_resampled does
 * with them.  Refuses what rs_hip_vertex_normals refuses and what the resampler refuses.  n_samples may be NULL.  NULL on
 * failure. */
rs_hip_cloud_t* rs_hip_cloud_create_from_mesh( const float* pos, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                                               float cell_size, int64_t* n_samples );

/* ---- model fusion: the row that closes a timestep ------------------------- */

/* rsdu_augment_database (apps/segment_transfer/database_update.cpp:22-91) for one placement: the scan's points that carry
 * the placement's instance id (rs_pointcloud_copy_by_ids, lib/rs/rs_pointcloud.h:239-297), aligned to the object's level-0
 * model by icp_align( .., 0.05, 10 deg ) from inverse( pose ) unless the object is static, moved into the model's frame
 * (rs_pointcloud_transform, :1367-1378), concatenated with the model and shuffled by the Fisher-Yates pass of
 * rs_pointcloud_merge (:383-446; PCG32, seed 12346).  Bit for bit wherever the ICP pose is: the library's ICP runs in the
 * reference's order up to 16 384 source points; above that its pose is within 1e-4 of the reference's, and the merged
 * positions of such an object inherit that difference.
 *
 * Refusals, all decided on the host before any launch (rs_hip_last_error() says which):
 *   RS_HIP_E_ARG       a negative count; a required array that is NULL; an id listed twice (the reference would emit
 *                      its points once per entry); a cloud without normals
 *   RS_HIP_E_CAPACITY  more than 2^24 merged points: up to there (float)i is exact and the shuffle's j < i for every
 *                      draw; beyond it the reference's j can exceed i */

/* The shuffle's permutation, made by the reference's loop on the host; needs no device.  perm[i] (n entries): the index,
 * in the concatenation "A then B", of the element that ends at position i.  n = 0 and n = 1 succeed. */
int rs_hip_shuffle_plan( int64_t n, uint32_t seed, int32_t* perm );

/* The same array made on the device: every step's draw by jumping the generator ahead, a sort of the steps by the
 * position they target, and one walk per output position (rs_fuse.hip). */
int rs_hip_shuffle_permutation( int64_t n, uint32_t seed, int32_t* perm );

/* index[0 .. *count): the i, increasing, with point_ids[i] among the n_ids entries of ids — the order
 * rs_pointcloud_copy_by_ids emits.  Host pointers in and out; index has room for n entries.  A count of 0 is no error. */
int rs_hip_select_by_ids( const int32_t* point_ids, int64_t n, const int32_t* ids, int32_t n_ids, int32_t* index, int64_t* count );

/* The merge stage alone on host arrays, with the pose given: A's points and normals through xform (msh_mat4_vec3_mul,
 * points with w = 1, normals with w = 0, not renormalised), then B's as they are, shuffled.  out_pos / out_nor:
 * 3 * (n_a + n_b) floats; source (may be NULL, n_a + n_b entries): source[i] < n_a names A's point, otherwise B's point
 * source[i] - n_a — the permutation of rs_hip_shuffle_plan.  Either count may be 0. */
int rs_hip_merge_shuffled( const float* a_pos, const float* a_nor, int64_t n_a, const float xform[16],
                           const float* b_pos, const float* b_nor, int64_t n_b, uint32_t seed,
                           float* out_pos, float* out_nor, int32_t* source /* may be NULL */ );

/* The whole row without leaving the device: the merged level-0 cloud, indexed (cell_size as for rs_hip_cloud_create);
 * rs_hip_cloud_create_level builds its levels and rs_hip_cloud_points hands its points to the host.
 *   scan, scan_instance_ids   the scan's level-1 cloud and one id per point, in the order the points were given to it
 *   uidx                      the placement's instance id
 *   model, pose               the object's level-0 cloud and the placement's pose; xform = rs_hip_mat4_inverse( pose )
 *   refine                    0 for a static object; otherwise rs_hip_icp_align( extracted, model, xform, identity,
 *                             max_dist, max_angle, 100 iterations ) — the reference passes 0.05 and 10 degrees
 * Out, each may be NULL: xform_out, the pose used; icp_err, what the ICP returned (0 without it); source, as for
 * rs_hip_merge_shuffled (n_extracted + the model's size entries); scan_index (room for the scan's size), the scan point
 * behind extracted point k; n_extracted.  The other attributes follow on the host through source / scan_index and
 * rs_hip_gather_attributes; the instance ids of the result are all uidx (database_update.cpp:79-85).
 * No point carries uidx: NULL with rs_hip_last_error() empty and *n_extracted = 0 — the reference leaves the model as it
 * is (database_update.cpp:58).  NULL with a message on failure. */
rs_hip_cloud_t* rs_hip_cloud_create_fused( const rs_hip_cloud_t* scan, const int32_t* scan_instance_ids, int32_t uidx,
                                           const rs_hip_cloud_t* model, const float pose[16], int32_t refine,
                                           float max_dist, float max_angle, float cell_size,
                                           float xform_out[16], float* icp_err, int32_t* source, int32_t* scan_index,
                                           int64_t* n_extracted );

/* Diagnostics: where the time of rs_hip_cloud_create_fused / rs_hip_cloud_fuse_arrangement went on the calling thread since
 * the last call of this function — extraction | ICP | permutation | merge | index build, seconds (out may be NULL) — and
 * whether the next calls keep the clock (enable != 0: they then synchronise after every stage). */
void rs_hip_fuse_seconds( double out[5], int32_t enable );

/* ---- the whole arrangement in one call -------------------------------------------------------- */

/* The permutations of n_placements independent shuffles, concatenated: perm[off_p + i] (off_p = n[0] + .. + n[p - 1]) is
 * rs_hip_shuffle_permutation( n[p], seed )[i], a LOCAL index.  Every placement restarts the generator at `seed`
 * (rs_pointcloud_merge seeds it itself).  One draw, one sort and one walk for all of them.  A size may be 0 or 1.
 * RS_HIP_E_ARG: a negative count, NULL arrays; RS_HIP_E_CAPACITY: an n[p] above 2^24, or a sum above 2^31 - 2. */
int rs_hip_shuffle_permutations( const int64_t* n, int32_t n_placements, uint32_t seed, int32_t* perm );

/* rs_hip_merge_shuffled for n_placements placements in one permutation pass and one merge launch.  a_pos / a_nor / b_pos /
 * b_nor: n_placements host pointers each (an entry may be NULL where its count is 0); xforms: 16 floats per placement;
 * out_pos / out_nor / source (may be NULL): the placements' results one after the other, placement p's at element
 * sum( n_a[q] + n_b[q], q < p ); source is local to its placement, as rs_hip_merge_shuffled returns it.  Refuses what
 * rs_hip_merge_shuffled and rs_hip_shuffle_permutations refuse. */
int rs_hip_merge_shuffled_multi( int32_t n_placements, const float* const* a_pos, const float* const* a_nor, const int64_t* n_a,
                                 const float* xforms, const float* const* b_pos, const float* const* b_nor, const int64_t* n_b,
                                 uint32_t seed, float* out_pos, float* out_nor, int32_t* source /* may be NULL */ );

/* One placement of an arrangement.  model_from names the model:
 *   -1            `model`, the object's level-0 cloud
 *   q, 0 <= q < p the shape placement q of the same call leaves: its merged cloud, or — when no scan point carries q's uidx
 *                 and the object stays as it is (database_update.cpp:58) — q's own model, resolved the same way.  This is the
 *                 reference's loop where the same object_idx is placed twice, or where a novel object copies a shape an
 *                 earlier placement already replaced (:51 after :89).  `model` is ignored. */
typedef struct rs_hip_fuse_placement {
  int32_t uidx;                 /* the placement's instance id */
  int32_t refine;               /* 0 for a static object */
  int32_t model_from;
  int32_t reserved;
  const rs_hip_cloud_t* model;
  float pose[16];
} rs_hip_fuse_placement_t;

/* What rs_hip_cloud_create_fused returns for the placement alone, given the same model.  source and scan_index are the
 * caller's arrays (each may be NULL): source has room for n_extracted + the model's size entries (the scan's size + the
 * model's always suffices; a dependent placement's model is as large as what its model_from left), scan_index for the
 * scan's size.  The call writes the other fields: cloud is NULL and n_extracted 0 where no scan point carries uidx (xform
 * and icp_err are then 0).  The caller destroys every cloud. */
typedef struct rs_hip_fuse_result {
  rs_hip_cloud_t* cloud;
  int64_t n_extracted;
  float xform[16];
  float icp_err;
  int32_t reserved;
  int32_t* source;
  int32_t* scan_index;
} rs_hip_fuse_result_t;

/* rsdu_augment_database's loop over all placements of an arrangement (database_update.cpp:28-91) without the points leaving
 * the device: the scan's instance ids are uploaded once and cut by the split's table and stable partition (segment k of its
 * order is what rs_hip_select_by_ids returns for that id); the placements run in rounds by the depth of their model_from
 * chains (an ordinary arrangement is one round); a round runs one rs_hip_icp_align per dynamic placement, then ONE
 * permutation pass and ONE merge launch for all its placements, then one batched index build for its merged clouds.  Two placements with
 * the same uidx extract the same points.  Every result is bit for bit rs_hip_cloud_create_fused's for that placement alone
 * wherever that call is bit for bit the reference; above 16 384 extracted points xform is within the ICP's 1e-4 bar and
 * the merged arrays are bit for bit the merge under the xform returned.
 * Refusals, decided on the host before any fuse kernel is launched, results untouched: RS_HIP_E_ARG for a negative
 * n_placements, NULL scan / placements / results / ids, a model_from outside [-1, p), model_from == -1 without a model, a
 * cloud without normals; RS_HIP_E_CAPACITY for more than 4096 distinct instance ids (the split's table finds that; there is
 * no fallback walk), more than 2^24 merged points in one placement, more than 2^31 - 2 merged points in one round.
 * n_placements == 0 succeeds.  A failure part of the way destroys the clouds already made and writes no result record
 * (the contents of source / scan_index arrays are then unspecified). */
int rs_hip_cloud_fuse_arrangement( const rs_hip_cloud_t* scan, const int32_t* scan_instance_ids,
                                   const rs_hip_fuse_placement_t* placements, int32_t n_placements,
                                   float max_dist, float max_angle, float cell_size, rs_hip_fuse_result_t* results );

/* ---- scan to object models: the row that opens a sequence ----------------- */

/* seg2rsdb's pointcloud_to_rsdb (apps/seg2rsdb/main.cpp:80-136): a labelled scan cut into one object model per instance.
 *   table     the distinct values of instance_ids, in order of first appearance (hashtable_keys returns insertion order);
 *             an id is the int32 itself, negative values included; each comes with its count and the index of its first point
 *   segment   instance k's points, in input order (rs_pointcloud_copy_by_ids, lib/rs/rs_pointcloud.h:239-297); the object's
 *             class is the class id of the segment's FIRST point (main.cpp:114), whatever the others carry
 *   centroid  per axis  double c = 0; c += (double)p[i]  over the segment in order, divided by (double)n, cast to float
 *             (rs_pointcloud_centroid, :1318-1339); then y = 0 (main.cpp:119)
 *   xform     identity for an object whose class is among static_classes (the caller's restatement of rsdb_is_class_static,
 *             which needs a class table); otherwise msh_translate( identity, ( -cx, -0.0f, -cz ) ), and every position goes
 *             through msh_mat4_vec3_mul( xform, p, 1 ), every normal through ( xform, n, 0 ) — the general product, so a -0.0
 *             normal component comes out +0.0 and an infinite coordinate makes NaN.  A static object's points are NOT passed
 *             through the product: their bits are the scan's
 *   pose      msh_mat4_inverse( xform ), for the identity too
 * Bit for bit the reference's; where its value is a NaN, a NaN (sign and payload are the adder's or the multiplier's).
 * The object's bounding box, which the reference computes before the transform and never again, is not an output.
 *
 * Refusals, each with a rs_hip_last_error() text and nothing written:
 *   RS_HIP_E_ARG       n < 0; a required array that is NULL; a static list of negative length, or NULL with n_static > 0
 *   RS_HIP_E_CAPACITY  more than max_instances (4096) distinct ids; more than 2^31 - 2 points
 * n = 0 succeeds with no instances. */

/* Where the results go.  Every member but n_instances may be NULL (the plan takes a NULL n_instances too).  With I the number
 * of instances, which the caller does not know beforehand: arrays "per instance" need room for min( n, max_instances )
 * entries, offsets for one more.
 *   inst_ids, counts, first     the table
 *   offsets                     offsets[k] .. offsets[k + 1]: instance k's part of order, out_pos, out_nor
 *   order                       n entries: the scan index of every output point, instance-major
 *   class_of, is_static         per instance
 *   sums                        3 per instance: the doubles before the division
 *   centroids                   3 per instance, with y = 0 as the reference leaves it
 *   xforms, poses               16 per instance, column-major
 *   out_pos, out_nor            3 n floats: the objects' points, in `order`; out_nor needs the scan's normals
 * The colour, radius, quality and id arrays follow on the host through order and rs_hip_gather_attributes. */
typedef struct rs_hip_split_out
{
  int32_t* n_instances; int32_t* inst_ids; int64_t* counts; int64_t* first; int64_t* offsets; int32_t* order;
  int32_t* class_of; int32_t* is_static; double* sums; float* centroids; float* xforms; float* poses;
  float* out_pos; float* out_nor;
} rs_hip_split_out_t;

/* The whole of the above by the reference's loops on the HOST; makes no device call.  The checker on machines without a
 * GPU and the reference of the device route. */
int rs_hip_split_plan( const float* pos, const float* nor /* may be NULL */, const int32_t* class_ids, const int32_t* instance_ids,
                       int64_t n, const int32_t* static_classes, int32_t n_static, const rs_hip_split_out_t* out );

/* The table alone, on the device: one atomic per distinct id of a wave into an open-addressed table; only the table comes
 * back.  inst_ids / counts / first (each may be NULL): room for min( n, max_instances ) entries. */
int rs_hip_instance_table( const int32_t* instance_ids, int64_t n, int32_t* inst_ids, int64_t* counts, int64_t* first,
                           int32_t* n_instances );

/* The stable multiway partition, on the device: for every k, order[offsets[k] .. offsets[k + 1]) is what
 * rs_hip_select_by_ids returns for { inst_ids[k] }.  inst_ids and offsets may be NULL. */
int rs_hip_split_by_instance( const int32_t* instance_ids, int64_t n, int32_t* inst_ids, int64_t* offsets, int32_t* order,
                              int32_t* n_instances );

/* The centroid chains alone, on the device: sums[3 k + a] = the sequential fp64 sum of pos[3 order[j] + a] over
 * j = offsets[k] .. offsets[k + 1] - 1; centroids (may be NULL) the cast quotient BEFORE y = 0.  pos: 3 n floats.  Refused
 * (RS_HIP_E_ARG): offsets that do not start at 0 or decrease, an entry of order outside [0, n). */
int rs_hip_segment_centroids( const float* pos, int64_t n, const int32_t* order, const int64_t* offsets, int32_t n_instances,
                              double* sums, float* centroids /* may be NULL */ );

/* The plan's outputs made on the device end to end (rs_split.hip): table, partition, chains, and one lane per output point
 * for the transform. */
int rs_hip_scan_to_objects( const float* pos, const float* nor /* may be NULL */, const int32_t* class_ids,
                            const int32_t* instance_ids, int64_t n, const int32_t* static_classes, int32_t n_static,
                            const rs_hip_split_out_t* out );

/* The same from a level-0 cloud with normals, without the points visiting the host: objects[k] (room for
 * min( size of scan, max_instances ) handles) is instance k's model as an indexed cloud of its own (cell_size as for
 * rs_hip_cloud_create); rs_hip_cloud_points hands its points out.  class_ids / instance_ids: one per point, in the order the
 * points were given to the scan.  out: the table, order, class_of, is_static, sums, centroids, xforms and poses; out_pos and
 * out_nor must be NULL.  The caller owns the clouds and destroys them; a failure part of the way destroys those already made
 * and returns none. */
int rs_hip_cloud_split_objects( const rs_hip_cloud_t* scan, const int32_t* class_ids, const int32_t* instance_ids,
                                const int32_t* static_classes, int32_t n_static, float cell_size,
                                rs_hip_cloud_t** objects, const rs_hip_split_out_t* out );

/* For tests: the partition's tile (points per column of its [rank][tile] matrix), the largest instance count its LDS route
 * serves on the calling thread, the refusal cap, and the addends of one step of a centroid chain.  Each may be NULL. */
void rs_hip_split_layout( int32_t* tile, int32_t* lds_ranks, int32_t* max_instances, int32_t* chain_block );

/* Sets the largest instance count of the partition's LDS route on the calling thread (0: every call takes the sort route;
 * clamped to 2048) and returns the previous value; a negative argument only reads. */
int32_t rs_hip_split_lds_ranks( int32_t ranks );

/* Sets the form of the centroid chains on the calling thread — 0 (default): a wave per chain whose steps are order-free where
 * that is provably exact; 1: a lone lane per chain adding in the reference's order, kept to be measured against — and
 * returns the previous value; a negative argument only reads.  Both give the same doubles. */
int32_t rs_hip_split_chains_form( int32_t form );

/* Diagnostic: how many addends the chains of the calling thread's last call added one by one. */
int64_t rs_hip_split_chains_sequential( void );

/* Diagnostics: where the time of rs_hip_scan_to_objects / rs_hip_cloud_split_objects went on the calling thread since the
 * last call of this function — table | partition | chains | transform with its copies | index builds, seconds (out may be
 * NULL) — and whether the next calls keep the clock (enable != 0: they then synchronise after every stage). */
void rs_hip_split_seconds( double out[5], int32_t enable );

/* ---- neighbourhood graph ------------------------------------------ */

/* rspf_compute_neighborhood (lib/rs/rs_pointcloud_filters.cpp:674-722): K = max_nn self-search
 * within sqrt(radius_sq) over `cloud` (needs normals), one weighted edge per (point, neighbour),
 * de-duplicated so that every undirected pair appears once, oriented as the reference's insertion
 * order leaves it ({i,j}, i<j, is (i,j) when j is among i's neighbours, (j,i) otherwise); self pairs
 * (i,i) are included, as in the reference.  weight = (1 - pow(d²/(4 r²), dist_exp)) *
 * powf(clamp(n·m,0,1), angle_exp) (the reference calls it with 8, 0.05², 15, 16).
 * Edges are written ordered by idx1, then by (dist², idx2); capacity must be >= n*max_nn. */
int rs_hip_compute_neighborhood( const rs_hip_cloud_t* cloud, int32_t max_nn, float radius_sq,
                                 float dist_exp, float angle_exp,
                                 int32_t* idx1, int32_t* idx2, float* weight, int64_t capacity, int64_t* n_edges );

/* ---- scene-coverage term of the arrangement optimiser ---------------- */

/* The voxel grid of lib/rs/intersect.h:59-109 over a scene's bounding box (isect_grid3d_init: fattened by
 * 0.3, ceilf(extent/voxel)+1 cells per axis) with the scene's level-2 points rasterised into it
 * (rsao_rasterize_scene_to_grid, apps/segment_transfer/arrangement_optimization.cpp:1064-1079: points
 * with quality < threshold are skipped; quality may be NULL).  One bit per voxel on the device.
 * In rs_hip_coverage_create, _scores and _extensions a point with a NaN or infinite coordinate (after its pose) lies outside the
 * grid, like any point whose floored cell coordinate is not in [0, res): it sets, clears and reads no cell. */
typedef struct rs_hip_coverage rs_hip_coverage_t;
rs_hip_coverage_t* rs_hip_coverage_create( const float bbox_min[3], const float bbox_max[3], float voxel_size,
                                           const float* scene_pos, const float* scene_quality, int64_t n_scene,
                                           float quality_threshold );
void rs_hip_coverage_destroy( rs_hip_coverage_t* c );
int  rs_hip_coverage_info( const rs_hip_coverage_t* c, int32_t res[3], float origin[3], int64_t* n_cells, int64_t* valid_cells );
/* Copies the scene grid out as the reference's byte array (1 = RSAO_CELL_ACTIVE), n_cells bytes. */
int  rs_hip_coverage_scene_grid( const rs_hip_coverage_t* c, uint8_t* data );

/* rsao__compute_scene_coverage_score (:344-373) for a batch of arrangements in one launch: arrangement a
 * consists of the placements [first_placement[a], first_placement[a+1]); placement k puts objects[k] (its
 * level-2 cloud) at poses[16k..] and is skipped when is_static[k] (rsdb_is_object_static, :1095-1096).
 * scores[a] = agreeing / valid scene voxels (0 when the scene grid is empty); agree (optional) receives
 * the integer numerators.  The simulated-annealing loop evaluates one arrangement per iteration
 * (:388); candidate moves can be scored together. */
int  rs_hip_coverage_scores( rs_hip_coverage_t* c, const rs_hip_cloud_t* const* objects, const float* poses,
                             const int32_t* is_static, const int32_t* first_placement, int32_t n_arrangements,
                             float* scores, int32_t* agree );

/* rsao_greedy_step's trial arrangements (:1012-1020) in one call: candidate k is scored as the arrangement "base + candidate k",
 * without a plane of the grid per candidate.  The base's placements are (base_objects[i], base_poses[16i..], base_static[i]),
 * static ones skipped (:1095-1096); candidate k places cand_objects[k] (level-2 cloud) at cand_poses[16k..] and is always
 * rasterised (the greedy step proposes no static object).  agree[k] (may be NULL) = base's agreeing voxels + the distinct
 * scene-active voxels candidate k hits that the base does not; scores[k] = (float)agree[k] / (float)valid, 0 when the scene grid
 * has no valid cell (:366-368); *base_agree (may be NULL) = the base's own count.  Every agree[k] and every bit of scores[k]
 * equals what rs_hip_coverage_scores returns for base + candidate k, and what rsao__compute_scene_coverage_score (:344-373) does.
 * The base is rasterised once; a candidate's bits live in the sub-box of its cells, in LDS (rs_arrange.hip). */
int  rs_hip_coverage_extensions( rs_hip_coverage_t* c,
                                 const rs_hip_cloud_t* const* base_objects, const float* base_poses, const int32_t* base_static, int32_t n_base,
                                 const rs_hip_cloud_t* const* cand_objects, const float* cand_poses, int32_t n_candidates,
                                 float* scores, int32_t* agree, int32_t* base_agree );
/* (tests, diagnostics) Candidates whose sub-box needs at most `bytes` of LDS keep it there (default and maximum 16384); larger ones
 * use a slab of global memory, same code, same bits.  0 sends every candidate there; bytes < 0 only reads.  Returns the previous budget. */
int32_t rs_hip_coverage_lds_budget( int32_t bytes );
/* (diagnostics) Candidates the process scored on the LDS route and on the slab route since the last reset. */
void    rs_hip_coverage_extension_routes( int64_t* lds, int64_t* slab, int32_t reset );
/* rs_hip_coverage_extensions, rs_hip_coverage_footprints and rs_hip_scene_saliency keep their device and pinned buffers per calling thread between calls (a bit
 * plane of the grid, the placements, the scene points; a slab of up to 256 MB once a call took the global route).  They are not
 * freed when the thread ends: a thread that ends while the process goes on calls this first.  Later calls allocate again. */
int     rs_hip_arrange_release( void );

/* ---- coverage footprints: the coverage term of the simulated-annealing loop without a device call per iteration ---- */

/* rsao_simulated_annealing (arrangement_optimization.cpp:388 ff.) scores one arrangement per iteration, and every placement it can
 * ever hold is known before the loop: the scene's pose proposals and the placements of the starting arrangement.  The coverage of an
 * arrangement (:344-373) depends only on WHICH scene-active voxels its non-static placements hit (:1083-1106, :359-367):
 *   agree = | union of footprint( k ) over its placements |,   score = (float)agree / (float)valid,
 * footprint( k ) = the distinct cells the transformed level-2 points of placement k fall into that are active in the scene grid.
 * rs_hip_coverage_footprints computes the footprints of n_placements placements in one device call: placement k puts objects[k] at
 * poses[16k..]; a static placement (is_static[k], :1095-1096) has the empty footprint and its object may be NULL; so has an empty
 * cloud.  A point with a NaN or infinite coordinate, or off the grid, has no cell (as in rs_hip_coverage_scores).  The result holds,
 * per placement, its cells as ascending, duplicate-free int32 indices of the reference's grid (y * x_res * z_res + z * x_res + x),
 * with the grid's n_cells and valid_cells.  One workgroup per placement, bits in a sub-box in LDS (rs_hip_coverage_lds_budget, as
 * for rs_hip_coverage_extensions; larger sub-boxes on a slab of global memory), compacted on the device; two blocking read-backs
 * on the LDS route.  NULL on failure (rs_hip_last_error): RS_HIP_E_ARG conditions are refused before a device is touched.
 * The buffers are the calling thread's (rs_hip_arrange_release).
 * A footprints handle lives in host memory.  rs_hip_footprints_scores writes to it (its marks): one thread at a time per handle. */
typedef struct rs_hip_footprints rs_hip_footprints_t;
rs_hip_footprints_t* rs_hip_coverage_footprints( rs_hip_coverage_t* c,
    const rs_hip_cloud_t* const* objects, const float* poses, const int32_t* is_static,
    int32_t n_placements );
/* Host only: the same object from arrays (tests, callers that cache footprints).  offsets: n_placements + 1 values from 0 that do not
 * decrease; placement k's cells are cells[offsets[k] .. offsets[k+1]), strictly ascending, each in [0, n_cells); 0 <= valid_cells <=
 * n_cells.  Anything else: NULL with RS_HIP_E_ARG's text in rs_hip_last_error (n_cells beyond 2e9: RS_HIP_E_CAPACITY's). */
rs_hip_footprints_t* rs_hip_footprints_from_arrays( int64_t n_cells, int64_t valid_cells,
    const int64_t* offsets /* n+1 */, const int32_t* cells, int32_t n_placements );
void rs_hip_footprints_destroy( rs_hip_footprints_t* f );
/* Any of the four outputs may be NULL.  total_cells = offsets[n_placements]. */
int  rs_hip_footprints_info( const rs_hip_footprints_t* f, int32_t* n_placements,
                             int64_t* n_cells, int64_t* valid_cells, int64_t* total_cells );
/* offsets: n_placements + 1 values; cells: total_cells values (may be NULL when there are none). */
int  rs_hip_footprints_arrays( const rs_hip_footprints_t* f, int64_t* offsets, int32_t* cells );
/* Host only: rsao__compute_scene_coverage_score (:344-373) of arrangement a = members[first[a] .. first[a+1]) (indices into the
 * footprint set), bit for bit: agree[a] (may be NULL) = the number of distinct cells in its members' footprints, scores[a] =
 * (float)agree[a] / (float)valid_cells in one fp32 division, 0 when valid_cells is 0 (:367-368).  A member may repeat and counts
 * once; an empty arrangement scores 0 / valid.  A member outside [0, n_placements) or first[] that decreases: RS_HIP_E_ARG with
 * nothing written.  The cost of an arrangement is the length of its members' lists: nothing of the grid's size is cleared or read. */
int  rs_hip_footprints_scores( rs_hip_footprints_t* f, const int32_t* members, const int32_t* first,
                               int32_t n_arrangements, float* scores, int32_t* agree /* may be NULL */ );
/* (diagnostics) Placements footprinted on the LDS route and on the slab route since the last reset (static and empty ones count
 * for the LDS route: they need no sub-box). */
void rs_hip_coverage_footprint_routes( int64_t* lds, int64_t* slab, int32_t reset );

/* ---- scene saliency: the per-point quality that gates the scene grid (arrangement_optimization.cpp:1109-1160) ---- */

/* isect_grid3d_init (lib/rs/intersect.h:59-75) for a box, on the host: cells per axis, origin (the fattened box's minimum) and the
 * number of cells — the size of the byte array rs_hip_scene_saliency can hand back.  RS_HIP_E_CAPACITY beyond 2e9 cells. */
int  rs_hip_voxel_grid_shape( const float bbox_min[3], const float bbox_max[3], float voxel_size, int32_t res[3], float origin[3], int64_t* n_cells );

/* rsao__compute_scene_saliency_grid (:1109-1160, called through rsao_compute_scene_saliency from apps/segment_transfer/main.cpp:337)
 * for one scene: a grid over the scene's box (main.cpp:327 passes voxel_size 0.15f) in which ALL proposals of dynamic objects
 * set their cells first and then ALL proposals of static objects clear theirs (:1126-1131; rsao__rasterize_proposals_to_grid,
 * :1038-1062, level 2 of the object, msh_mat4_vec3_mul( pose, p, 1 ), cell by isect_grid3d_cell_from_world_space, intersect.h:97-109).
 * Proposal k places objects[prop_object[k]] (its level-2 device cloud) at prop_poses[16k..]; prop_static[k] =
 * rsdb_is_object_static of that object.  scene_pos / scene_class are the scene's LEVEL-0 positions (AoS xyz) and class ids, host
 * arrays; wall_class / floor_class = rsdb_get_class_idx( "wall" / "floor" ), -1 where the class is absent.  quality[i] = 0.0f
 * for a wall or floor point whatever its cell holds (:1141-1145), else 1.0f if its cell is lit and 0.0f if not or if the point
 * lies outside the grid (:1146-1154).  grid (may be NULL; grid_capacity >= the grid's cells) receives the grid as the reference's
 * byte array (1 = RSAO_CELL_ACTIVE).  Any number of proposals (launches of 65535 each).  Arguments are checked before a device
 * is touched.  A point with a NaN or infinite coordinate (after its pose) lies outside the grid, like any point whose floored cell
 * coordinate is not in [0, res): it sets, clears and reads no cell. */
int  rs_hip_scene_saliency( const float bbox_min[3], const float bbox_max[3], float voxel_size,
                            const rs_hip_cloud_t* const* objects, int32_t n_objects,
                            const int32_t* prop_object, const float* prop_poses, const int32_t* prop_static, int32_t n_proposals,
                            const float* scene_pos, const int32_t* scene_class, int64_t n_scene,
                            int32_t wall_class, int32_t floor_class, float* quality, uint8_t* grid, int64_t grid_capacity );

/* ---- voxel overlap of placed shapes, non-maximum suppression of pose proposals ---- */

/* A shape is two device clouds of one object: its BOUNDARY cloud (the reference's level 1: the points that are rasterised,
 * lib/rs/intersect.h:215) and its EXTENT cloud (level 3: the points whose transformed box sizes the grid, :114). */
typedef struct rs_hip_isect_shape { const rs_hip_cloud_t* boundary; const rs_hip_cloud_t* extent; } rs_hip_isect_shape_t;

/* isect_get_overlap_factor (lib/rs/intersect.h:309-368) for n_pairs pairs in one call, bit for bit: pair k places
 * shapes[shape_a[k]] by poses_a[16k..] and shapes[shape_b[k]] by poses_b[16k..]; overlap[k] = cells occupied in both grids /
 * max (normalize_by_smaller: min) of the two grids' occupied cells, 0 when the extent boxes do not intersect, 1 when that
 * count is 0.  voxelize_inside = 0 counts boundary cells only (isect_compute_boundary_grid).  counts (may be NULL) =
 * {count_a, count_b, both} per pair.  Refused, with nothing written: a pair whose grid has an x or z line of more than 4096
 * cells while voxelize_inside is set — the reference's scanline arrays, :132-133 — or more than 2^20 cells along an axis or
 * planes beyond 256 MB (RS_HIP_E_CAPACITY); a pair with a boundary point outside the grid of its extent boxes — the
 * reference's assert, :227-229; impossible for a level pyramid, whose level 1 lies within 4 cm of level 3 and the grid is
 * grown by 0.3 — (RS_HIP_E_ARG; rs_hip_last_error() names the pair). */
int rs_hip_overlap_factors( const rs_hip_isect_shape_t* shapes, int32_t n_shapes,
                            const int32_t* shape_a, const float* poses_a, const int32_t* shape_b, const float* poses_b,
                            int32_t n_pairs, float voxel_size, int voxelize_inside, int normalize_by_smaller,
                            float* overlap, int32_t* counts );

/* mgs_non_maxima_suppresion for ONE object's proposals (apps/pose_proposal/pose_proposal.cpp:377-451): until every proposal
 * is marked, the first unmarked proposal with the strictly largest score is kept, and every unmarked proposal i is discarded
 * whose overlap with it (voxel 0.1, inside fill, normalised by the larger count) is > 0.5f, or whose transformed centroid lies
 * closer than dist_threshold to the keep's, or whose score is < 0.01f.  centroid is rs_pointcloud_centroid( shape, 0 )
 * (lib/rs/rs_pointcloud.h:1318-1340: a sequential fp64 sum over level 0, rounded to fp32): the caller's, like the reference's
 * cached one.  marks[i] = 1 keep, 2 discard; keep_idx[0 .. *n_keep) ascending (:441-447); n_rounds (may be NULL) = rounds =
 * keeps.  Scores that are NaN or <= -1e9 give RS_HIP_E_ARG (the reference would index with -1).  The rounds run on the host,
 * one launch and one read-back of 12 bytes per evaluated pair each; the overlap is evaluated only where neither cheap test
 * discards and the two extent boxes (computed once per proposal) intersect. */
int rs_hip_nms( const rs_hip_isect_shape_t* shape, const float centroid[3], const float* poses, const float* scores, int32_t n,
                float dist_threshold, int32_t* marks /* n: 1 keep, 2 discard */, int32_t* keep_idx, int32_t* n_keep, int32_t* n_rounds );
/* (tests, diagnostics) Pairs whose four bit planes need at most `bytes` of LDS keep them there (default and maximum 61440); larger
 * ones use a slab of global memory, same code, same bits.  0 sends every pair there; bytes < 0 only reads.  Returns the previous budget. */
int32_t rs_hip_isect_lds_budget( int32_t bytes );
/* (diagnostics) Pairs the process rasterised since the last reset, and pairs rs_hip_nms settled without (cheap tests, disjoint boxes). */
void    rs_hip_isect_pairs( int64_t* evaluated, int64_t* skipped, int32_t reset );

/* ---- floor and wall planes: RANSAC votes, inlier gather, relabel ---- */

/* rspf__detect_floor / rspf__detect_walls, rspf__gather_model_inliers and rspf_relabel_walls_and_floors
 * (lib/rs/rs_pointcloud_filters.cpp:116-323, 617-671), bit for bit.  Everything is fp32 in the reference's association, compiled
 * without contraction; msh_abs is x < 0 ? -x : x, so a NaN fails every compare.  Not covered, and why:
 * rspf__split_by_connected_components and what needs its output (rspf__refine_plane_models, rspf_compute_plane_features,
 * rspf_classify_planes).
 *
 * Refusals, all decided on the host with nothing written (rs_hip_last_error() says which):
 *   RS_HIP_E_ARG       null arrays or negative counts; a round whose candidate set is empty (the reference's pdf would stay
 *                      uninitialised); a wall round with fewer than 2 candidates (the reference's redraw loop never ends); a
 *                      detection that would pop an empty model array (undefined in the reference)
 *   RS_HIP_E_CAPACITY  n > 2^24 ((float)n is inexact in msh_rand_range); more models than the caller's capacity */

/* One round's sampling on the host (no device needed): the alias table over weights 1.0 (active[i] != 0) / 0.0, the PCG32
 * seeded with `seed` (the reference: 12346), n_iter triples idx[3h..3h+2] — distinct = 0 the floor's three plain samples,
 * distinct = 1 the walls' redraws (b while b == a, c while c == b; c == a is allowed) — and per triple (each may be NULL)
 * center = p_a and normal = normalize( cross( p_b - p_a, p_c - p_a ) ), NaN for a degenerate triple. */
int rs_hip_plane_hypotheses( const float* pos, int64_t n, const uint8_t* active, int32_t n_iter, int32_t distinct, uint32_t seed,
                             int32_t* idx, float* center, float* normal );

/* evaluate_plane_model (:116-134) for n_hyp hypotheses at once, host arrays in and out: counts[h] = the number of points i with
 * active[i] != 0 and msh_abs( dot( normal_h, pos_i - center_h ) ) < dist_threshold.  valid (may be NULL): a hypothesis with
 * valid[h] == 0 is not scored (the walls' up test) and counts 0.  n = 0 or n_hyp = 0 succeed. */
int rs_hip_plane_votes( const float* pos, int64_t n, const uint8_t* active, const float* center, const float* normal,
                        const uint8_t* valid, int32_t n_hyp, float dist_threshold, int32_t* counts );

/* What a detection did, round by round (round 0 is the floor's, rounds 1.. are the walls'), for tests and diagnostics.  The
 * caller sets capacity_rounds, max_iters (>= both iteration counts) and the arrays, each of which may be NULL; round r's
 * entries start at r * 3 * max_iters (idx), r * max_iters (valid, counts), r (best, n_iters) and r * n (mask_before,
 * mask_after: the candidate mask the round sampled from, and the mask after its remove_inliers; the floor removes nothing).
 * counts of hypotheses that failed the up test are 0; best is -1 where the round detected nothing.  Rounds beyond
 * capacity_rounds are counted in n_rounds and not recorded. */
typedef struct rs_hip_plane_trace
{
  int32_t capacity_rounds, max_iters;
  int32_t n_rounds;
  int32_t* idx; uint8_t* valid; int32_t* counts; int32_t* best; int32_t* n_iters;
  uint8_t* mask_before; uint8_t* mask_after;
} rs_hip_plane_trace_t;

/* rspf__detect_floor then rspf__detect_walls on a cloud with normals (the reference: level 2 with ( 0.8f, 0.033f, 250, 2500,
 * 5000 )).  The points stay on the device; per round the candidate mask comes to the host, the triples go back, and the best
 * hypothesis' index and count come back.  Models in the reference's order (the floor first if one was found), n_inliers = the
 * votes of each; *n_floors and *n_walls are the two functions' return values, *n_models the length of the array they leave.
 * Kept as the reference has it: a wall round that detects nothing pushes nothing, removes the inliers of the previous best
 * model (before any wall: the zero plane, which removes every candidate), ends the loop, and the final pop then removes a
 * model that was legitimate — the previous wall or the floor. */
int rs_hip_detect_planes( const rs_hip_cloud_t* cloud, float dot_threshold, float dist_threshold, int64_t count_threshold,
                          int32_t floor_iters, int32_t wall_iters, int32_t capacity,
                          float* centers /* 3 * capacity */, float* normals /* 3 * capacity */, int64_t* n_inliers /* capacity */,
                          int32_t* n_floors, int32_t* n_walls, int32_t* n_models, rs_hip_plane_trace_t* trace /* may be NULL */ );

/* A plane model crosses as plain arrays, model m at: centers[3m], normals[3m], axes[9m] (column-major: axes[9m + 3c + r]),
 * extends[4m] (x, y, z, w), valid[m], normal_up_dot[m].  Arrays a call does not read may be NULL. */

/* rspf__gather_model_inliers (:277-323) on a cloud with normals: for each model in order (skipped, with an empty range, if
 * check_validity and valid[m] == 0) the indices i, increasing, with msh_abs( dot( nrm_i, n ) ) > dot_threshold and
 * msh_abs( dot( n, p_i - c ) ) < dist_threshold and, with check_extends, rspf__is_point_within_convex_poly of the model's quad
 * as written there (three of the four corners).  index[offsets[m] .. offsets[m + 1]) are model m's; offsets has n_models + 1
 * entries.  More than `capacity` indices: RS_HIP_E_CAPACITY, nothing written. */
int rs_hip_gather_plane_inliers( const rs_hip_cloud_t* cloud, const float* centers, const float* normals, const float* axes,
                                 const float* extends, const int8_t* valid, int32_t n_models, float dot_threshold,
                                 float dist_threshold, int32_t check_validity, int32_t check_extends,
                                 int32_t* index, int64_t capacity, int64_t* offsets );

/* rspf_relabel_walls_and_floors (:617-671) on a cloud with normals (the reference: level 1): the gather with dist_threshold
 * 0.05f, dot_threshold 0 (the reference's params struct is zero-initialised and the function never sets it), validity and
 * extends checked, and for every valid model in order and each of its inliers: normal_up_dot > 0.8f — instance >= 1024 -> 0,
 * class == unlabelled_idx -> floor_idx; else instance >= 1024 -> 1, class == unlabelled_idx -> wall_idx.  class_ids and
 * instance_ids (host, one entry per point of the cloud in the order it was created from) are rewritten in place. */
int rs_hip_relabel_walls_and_floors( const rs_hip_cloud_t* cloud, const float* centers, const float* normals, const float* axes,
                                     const float* extends, const int8_t* valid, const float* normal_up_dot, int32_t n_models,
                                     int32_t floor_idx, int32_t wall_idx, int32_t unlabelled_idx,
                                     int32_t* class_ids, int32_t* instance_ids );
/* (measurements) 0: the votes kernel stages each tile of points in LDS (the default); 1: it reads them through wave-uniform global
 * loads.  Same counts.  form < 0 only reads.  Returns the previous form. */
int32_t rs_hip_plane_votes_form( int32_t form );

/* ---- pose proposals: the multi-resolution grid search (SURVEY.md §2 row 5, §3.2 "hot loop A") ---- */

/* mgs_propose_poses (apps/pose_proposal/pose_proposal.cpp:325-369): a grid search over (cell x, cell z, yaw) with the objects'
 * coarsest level, the survivors scored again with the finer ones.  The constants are the caller's, never the library's; the
 * reference's are spacing 0.10f, angle_delta (float)( MSH_TWO_PI / 10.0f ), height 0, thresholds { 0.25f, 0.35f, 0.40f } for levels
 * 4, 3, 2, radius 0.1f (the scene's level 1), max_n_neigh 64.  Static objects are the caller's to leave out (rsdb_is_object_static).
 * Not covered: the distance-field gate (:223-227), which mgs_propose_poses never passes. */

/* The host part alone; needs no device.  The tables of the grid, by the reference's loops as written (:203-222): ox / oz start at
 * -spacing and are accumulated with fp32 += while < length + spacing, compared in fp32 (a length of 3.2 at spacing 0.1 gives 35
 * steps, one more than the real numbers); the yaw angle starts at 0.0f and is accumulated in fp32 while < the double 6.2831853072;
 * yaw[16 k ..] = msh_rotate( identity, angle_k, (0,1,0) ), column-major, with the host libm's sinf / cosf.  Two passes: the
 * counts are always written; a table that is NULL is not asked for; a table shorter than its count (cap_*) gives
 * RS_HIP_E_CAPACITY and no table is written.  RS_HIP_E_ARG: a box that is not finite, spacing or angle_delta not > 0, or a step so
 * small that its fp32 counter would not advance (the reference's loop would not end); RS_HIP_E_CAPACITY: more than 2^20 steps. */
int rs_hip_pose_grid_plan( const float bbox_min[3], const float bbox_max[3], float spacing, float angle_delta,
                           int32_t* n_x, int32_t* n_z, int32_t* n_yaw,
                           float* ox /* may be NULL */, int32_t cap_x, float* oz /* may be NULL */, int32_t cap_z,
                           float* yaw /* may be NULL, 16 per step */, int32_t cap_yaw );

/* What a search did, for tests and diagnostics; each array may be NULL.  Entry [o * n_levels + l]: n_scored = the poses of object o
 * scored at level l (level 0: the whole grid; later: the proposals whose score was > 0.0f), n_kept = its proposals with a score
 * > 0.0f after the level.  n_proposed[o] = the length of the object's proposal storage (it never shrinks, :292). */
typedef struct rs_hip_propose_trace
{
  int32_t* n_scored; int32_t* n_kept;    /* n_objects * n_levels */
  int32_t* n_proposed;                   /* n_objects */
} rs_hip_propose_trace_t;

/* The search for n_objects objects at once.  objects[o * n_levels + l]: object o's cloud of level l, coarsest first (the reference:
 * levels 4, 3, 2), each with normals; n_levels 1..4.  scene: the cloud that is searched (the reference: level 1), bbox_*: the
 * scan's bounding box, whose min is the grid's origin.  Kept as the reference has it:
 *   level 0      the pose of (cell i, j; yaw k) is yaw[k] with col[3] = ( min.x + ox[i], height, min.z + oz[j], 1 ), cells x-outer and
 *                z-inner; per cell the best score starts at 0 and is replaced by strict > in yaw order (the first of equals wins, a
 *                NaN never); the cell proposes where best > thresholds[0], in cell order
 *   level l      only proposals with score > 0.0f are scored again and become score > thresholds[l] ? score : -1.0f
 *   final lists  every proposal with fabsf( score ) > 0.000001f, in order — the ones marked -1 included, which the reference hands
 *                to its non-maximum suppression
 *   an object level of 0 points scores NaN: at level 0 nothing is proposed, later its proposals become -1
 * counts[o] = the length of object o's list, poses[( o * capacity + i ) * 16 ..] and scores[o * capacity + i] its entries.  An
 * object with more than `capacity` entries: RS_HIP_E_CAPACITY, counts hold what is needed, poses and scores are not written.
 * The poses are made on the device from the planner's tables and scored by the launches of rs_hip_alignment_scores (more than
 * 65 535 in chunks); between levels only counts come to the host, n_levels waits per call whatever n_objects is. */
int rs_hip_propose_poses( const rs_hip_cloud_t* const* objects, int32_t n_objects, int32_t n_levels, const rs_hip_cloud_t* scene,
                          const float bbox_min[3], const float bbox_max[3], float spacing, float angle_delta, float height,
                          const float* thresholds /* n_levels */, float radius, int32_t max_n_neigh, int32_t capacity,
                          int32_t* counts /* n_objects */, float* poses /* n_objects * capacity * 16 */,
                          float* scores /* n_objects * capacity */, rs_hip_propose_trace_t* trace /* may be NULL */ );

/* The two judging stages on host arrays (the device kernels of the search, run on uploaded scores).
 * rs_hip_cell_best: scores[c * n_yaw + k]; best_yaw[c] = the winning k (-1: no score > 0), best_score[c] (0 then),
 * keep[c] = the cell's slot in the proposal list — the number of proposing cells before it — or -1 where best_score[c] is not
 * > threshold.
 * rs_hip_verify_marks: out[i] = old[i] > 0.0f ? ( new[i] > threshold ? new[i] : -1.0f ) : old[i]; out may be old_scores. */
int rs_hip_cell_best( const float* scores, int32_t n_cells, int32_t n_yaw, float threshold,
                      int32_t* best_yaw, float* best_score, int32_t* keep );
int rs_hip_verify_marks( const float* old_scores, const float* new_scores, int32_t n, float threshold, float* out );
/* Frees the search's buffers of the calling thread (they are kept between calls otherwise). */
int rs_hip_propose_release( void );

/* ---- host-side helpers shared by the drop-in shim (exact reference arithmetic) ------- */

/* msh_mat4_inverse / msh_mat4_mul (lib/msh/msh_vec_math.h:1818-1905, 1441-1476) */
void rs_hip_mat4_inverse( const float* m, float* out );
void rs_hip_mat4_mul( const float* a, const float* b, float* out );
/* The device's sinf/cosf — a restatement of the host libm's algorithm, since the reference's poses carry libm's bits
 * (msh_rotate, msh_vec_math.h:2091-2092) — evaluated on the host for n arguments, so that a CPU test can hold it
 * against the libm of the machine (no GPU needed). */
void rs_hip_sincosf_model( const float* x, int64_t n, float* sin_out, float* cos_out );
/* icp_estimate_rigid_xform_pt2pl (lib/rs/icp.h:210-298) on host arrays (device reduction).  The estimator is chosen by n and the
 * thresholds above, as for rs_hip_icp_align.  Weights that vanish (their sum <= 1e-7: all zero, for instance): the reference's
 * estimator has no guard of its own there — it divides by the sum and returns NaN — while its caller, icp_align, tests the sum
 * first and keeps the pose (icp.h:466-470).  This entry point does what the caller does, whichever estimator runs: T1 is left as
 * it came, *err = 0 and RS_HIP_OK comes back. */
int  rs_hip_icp_estimate_pt2pl( const float* pts1, const float* pts2, const float* nor2,
                                const float* weights, int32_t n, float* T1, float* err );

#ifdef __cplusplus
}
#endif
#endif /* RESCAN_HIP_H */
