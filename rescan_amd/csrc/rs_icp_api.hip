// librescan_hip host side: the ICP entry points of include/rescan_hip.h.
//
// Owns the ICP outer loop (searches and reductions on the GPU; the 6x6 LDLᵀ solve and the pose composition on the host in the
// reference's own arithmetic, lib/rs/icp.h:267-295), the estimator policy that loop applies (icp_choose, icp_plain_iterations),
// the call's one fill launch, the per-iteration traces and the diagnostics.  Runtime state and profiling: rs_api.hip, clouds:
// rs_cloud_api.hip, both through rs_api.h.

#include "../../include/rescan_hip.h"
#include "rs_api.h"
#include "rs_device.h"
#include "rs_math.h"
#include "rs_switches.h"
#include "rs_xcdmap.h"      // the census of icp_debug_after by XCD class

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <array>
#include <atomic>

using namespace rs;

// ------------------------------------------------------------------------------------------
// ICP
// ------------------------------------------------------------------------------------------

namespace {

struct IcpWorkspace
{
  DevBuf state, slot, d2, dot, stat_acc, mom_part, res, wexp, queue, queue_count, multi;   // (multi: the per-problem views of a multi-source batch)
  DevBuf cert_r, cert_dot, cert_slack;                                                    // ICP certificates
  DevBuf order_a, order_b;                                                      // ICP phase A slow-tile lists (ping-pong)
  DevBuf tmp_pos, tmp_pos2, tmp_nor2;                                           // estimate-only
  DevBuf faith;                                                                 // reference-order estimator: correspondences in source order
  DevBuf rp_segsum, rp_guess, rp_seg, rp_super, rp_totals, rp_redone;                     // ... its parallel form (replay)
  DevBuf ch_rec, ch_segsum, ch_prefix, ch_seg, ch_blk, ch_guess, ch_dbg, ch_done, ch_chk;                                    // the centroid chains of large sources (grid chains)
  PinBuf h_a, h_b, h_multi;      // h_multi: a multi-source batch's problem views
};
thread_local IcpWorkspace g_ws;
// rs_hip_icp_align_traced: the calling thread's next single-problem alignment leaves its per-iteration errors here (the loop then
// reads its state after every iteration instead of every few)
thread_local float* g_icp_trace = nullptr;
thread_local int g_icp_trace_cap = 0;
// rs_hip_icp_trace_begin: the calling thread's ICP calls leave, per problem and iteration, the pose after it, its error and the
// estimator that ran (RS_HIP_ICP_STEP_*), until rs_hip_icp_trace_end.  A call's problem index reaches the trace's through
// g_tr_map / g_tr_off (slices, groups of a multi-source batch, problems run again): global = map ? map[off + p] : off + p.
struct IcpStepTrace { float* poses = nullptr; float* errs = nullptr; int32_t* kinds = nullptr; int32_t* redone = nullptr; int max_iter = 0, n_prob = 0; };
thread_local IcpStepTrace g_tr;
thread_local const int* g_tr_map = nullptr;
thread_local int g_tr_off = 0;
struct TrShift      // problem p of the calls below is problem d + p of the caller
{
  int saved; TrShift( int d ) : saved( g_tr_off ) { g_tr_off += d; } ~TrShift() { g_tr_off = saved; }
};
struct TrMap        // problem p of the calls below is the caller's problem map[p]
{
  const int* saved_map; int saved_off;
  TrMap( const int* map ) : saved_map( g_tr_map ), saved_off( g_tr_off ) { g_tr_map = map; g_tr_off = 0; }
  ~TrMap() { g_tr_map = saved_map; g_tr_off = saved_off; }
};
inline int tr_global( int p )
{
  const int g = g_tr_map ? g_tr_map[g_tr_off + p] : g_tr_off + p;
  return ( g >= 0 && g < g_tr.n_prob ) ? g : -1;
}
void tr_clear_row( int g )
{
  for( int i = 0; i < g_tr.max_iter; ++i )
  {
    const size_t r = (size_t)g * g_tr.max_iter + i;
    for( int k = 0; k < 16; ++k ) g_tr.poses[r * 16 + k] = NAN;
    g_tr.errs[r] = NAN; g_tr.kinds[r] = RS_HIP_ICP_STEP_NONE;
  }
}
// a call starts over for its problems 0 .. n-1: whatever an earlier attempt left in their rows goes
void tr_clear( int n ) { if( g_tr.kinds ) for( int p = 0; p < n; ++p ) { const int g = tr_global( p ); if( g >= 0 ) tr_clear_row( g ); } }
// The ICP loop's device-resident state, one 4-byte word array after the other (n = n_prob); array X starts at word ICP_ST_X * n:
//   T1 16n | active n | T1_prev 16n | iters n | err n | prev_err n | queued n | ticket n | failed n
// ticket carries the stop guard's flags: [p] = 1 when a stop test of problem p came within L.stop_guard of its threshold
// (k_icp_update); failed the grid chains' (ChainBufs::failed: [p] = 1 when a walk gave problem p up) — in the state block, so that the
// give-up decision comes out of the copy and the synchronisation that end every call anyway.
enum : size_t { ICP_ST_T1 = 0, ICP_ST_ACTIVE = 16, ICP_ST_T1_PREV = 17, ICP_ST_ITERS = 33, ICP_ST_ERR = 34, ICP_ST_PREV_ERR = 35,
                ICP_ST_QUEUED = 36, ICP_ST_TICKET = 37, ICP_ST_FAILED = 38, ICP_STATE_WORDS = 39 };
// iteration i has just run for every problem with was_active[p]: its pose and error as the state holds them now (hS: the n-problem state)
void tr_record( int n, int i, int kind, const float* hS, std::vector<char>& was_active )
{
  const size_t np = (size_t)n;
  const int* hActive = (const int*)( hS + np * ICP_ST_ACTIVE );
  for( int p = 0; p < n; ++p )
  {
    if( !was_active[p] ) continue;
    was_active[p] = hActive[p] ? 1 : 0;
    const int g = tr_global( p );
    if( g < 0 || i >= g_tr.max_iter ) continue;
    const size_t r = (size_t)g * g_tr.max_iter + i;
    std::memcpy( g_tr.poses + r * 16, hS + np * ICP_ST_T1 + 16 * p, 64 ); g_tr.errs[r] = hS[np * ICP_ST_ERR + p]; g_tr.kinds[r] = kind;
  }
}
void tr_mark_redone( int p ) { if( g_tr.redone ) { const int g = tr_global( p ); if( g >= 0 ) g_tr.redone[g] = 1; } }
DevBuf g_faith_redone;            // (a process-wide counter: rs_hip_icp_faith_redone)
std::mutex g_faith_redone_mu;

// The estimator of icp_estimate_rigid_xform_pt2pl (lib/rs/icp.h:210-298) by source size — round 6: the policy priced against the bar on every
// reference fixture (profiles/r06/estimator_policy.txt):
//   n <= REF_ORDER_BELOW (16 384)    the reference's own accumulation order and precisions (k_icp_faithful): its bits.  Every level-2 object of the
//                                    reference's call sites (2-10 k points); up to ~10 k points the sequential chains cost no more than the launches of
//                                    anything parallel (60-90 us per iteration either way), at 16 k 150 against 75.
//   n <= REPLAY_BELOW (0: off)       the same bits computed in parallel ("replay"): opt-in.
//   n <= LANE_CHAINS_BELOW (65 536)  LANE chains: the reference's 2.5 sigma cut and its seven centroid sums bit for bit by one wave per chain +
//                                    fp64 moments; any number of differently sized problems per launch (rs_hip_icp_align_multi) — every icp_align
//                                    call site of the reference (level-2 objects 2-10 k points, scene extracts up to ~50 k: SURVEY §8 a6).
//                                    <= 3e-6 from the reference's pose on its fixtures, equal iteration counts; 110 instead of 520 us per iteration at 50 k.
//   larger                           GRID chains: the same seven sums spread over the chip (k_chain_*) + fp64 moments; <= 1.5e-6 on ten 1 M-point
//                                    rooms, <= 9e-7 on the 24 scan-sized sweep runs.  A chain that hovers around zero gives the call up: again with
//                                    the sums by pass 2 of the replay.
// RS_HIP_EXACT_CENTROIDS=0: plain fp64 moments for everything above the first two thresholds (up to 2e-4 from the reference: NOT within the bar's
// margin — kept for measurements).  rs_hip_icp_reference_order_below( 65536 ) brings the reference's bits back for every call site.
// After a source's centroid chains gave a problem up, its next CHAINS_RETRY_AFTER calls go straight to the replay (rs_hip_icp_chains_retry_after).
// (The thresholds are rows of rs_switches.h: read when the library is loaded, changed by their setters.)
std::atomic<int> g_chains_gave_up{ 0 };
// ... of a call with ONE problem, whose grid chains have the chip to themselves: the same sums — the same poses, bit for bit — faster from
// ~28 k points on (tools/lane_vs_grid.py, us per iteration lane | grid: 17 k 74 | 80, 25 k 80 | 80, 30 k 84 | 80, 40 k 101 | 90, 50 k 111 | 91,
// 65 k 130 | 97); batches keep the lane chains up to LANE_CHAINS_BELOW (a walk per problem side by side: eight 50 k-point refines 20 us per
// problem and iteration).  A threshold set beyond 65 536 (rs_hip_icp_lane_chains_below) means "the lane chains, whatever the call" and
// holds for single calls too; any other setting caps them at 28 672.
// The two source sizes the policy is keyed on: object-sized sources (the sequential reference order of a bit-exact run, the lane chains'
// default range; larger ones are scan-sized: early plain iterations) and the largest source with a bit-exact estimator (the replay).
constexpr int ICP_OBJECT_PTS = 65536, ICP_EXACT_PTS = 262144;
inline int lane_single_cap( int lane_below ) { return lane_below > ICP_OBJECT_PTS ? lane_below : std::min( lane_below, 28672 ); }
// The estimators, by the RS_HIP_ICP_STEP_* code of their iterations (RS_HIP_ICP_STEP_PLAIN: the early iterations of GRID_CHAINS and
// RECORDS, icp_plain_iterations).
enum IcpEstimator
{
  ICP_EST_REF_ORDER   = RS_HIP_ICP_STEP_REF_ORDER,     // k_icp_faithful
  ICP_EST_REPLAY      = RS_HIP_ICP_STEP_REPLAY,        // launch_icp_replay
  ICP_EST_LANE_CHAINS = RS_HIP_ICP_STEP_LANE_CHAINS,   // launch_icp_lane_chains (object-sized: one wave per chain)
  ICP_EST_GRID_CHAINS = RS_HIP_ICP_STEP_GRID_CHAINS,   // launch_icp_chain_centroids
  ICP_EST_RECORDS     = RS_HIP_ICP_STEP_RECORDS,       // launch_icp_exact_centroids_from_records (centroid_mode 2: the cross-check, and a give-up's re-run)
  ICP_EST_MOMENTS     = RS_HIP_ICP_STEP_MOMENTS,       // launch_icp_moments (centroid_mode 0)
};
struct IcpChoice { IcpEstimator est; bool guard; };
// The estimator of a call of n_problems problems whose largest source has n_source points (centroid_mode: rs_hip_icp_exact_centroids;
// force_bits: the reference's own order, sequential or parallel, whatever the thresholds say), and whether the stop test's guard
// applies: only where the estimator is not the reference's order AND a bit-exact one exists to run the problem again with.
IcpChoice icp_choose( int n_source, int n_problems, int centroid_mode, bool force_bits )
{
  if( n_source <= ( force_bits ? ICP_OBJECT_PTS : sw_int( SW_REF_ORDER_BELOW ) ) ) return { ICP_EST_REF_ORDER, false };
  if( n_source <= ( force_bits ? ICP_EXACT_PTS : sw_int( SW_REPLAY_BELOW ) ) ) return { ICP_EST_REPLAY, false };
  if( centroid_mode == 0 ) return { ICP_EST_MOMENTS, false };
  const int below = sw_int( SW_LANE_CHAINS_BELOW );
  const IcpEstimator est = n_source <= ( n_problems > 1 ? below : lane_single_cap( below ) ) ? ICP_EST_LANE_CHAINS
                         : centroid_mode == 1 ? ICP_EST_GRID_CHAINS : ICP_EST_RECORDS;
  return { est, n_source <= ICP_EXACT_PTS };
}
// The stop test's guard (round 6).  icp_align stops when |err - prev_err| < 1e-5 (icp.h:489).  The lane / grid chains follow the
// reference's errors to 1e-8 ... 6e-7 (their moments are exact where the reference rounds): when a decisive difference passes within
// that of 1e-5 the decision can fall the other way — one iteration more or less, 1e-4 ... 2e-4 in the pose; measured: 2 of 49
// object-sized runs, profiles/r06/stop_test_guard.txt.  A problem whose |delta err| comes within STOP_GUARD of the threshold in any
// iteration that can stop (i > 5) is therefore RUN AGAIN in the reference's own order (sequential chains up to 65 536 points, their
// parallel form up to 262 144): the reference's bits.  ~20 % of stop-test calls at 1.5e-6; larger sources have no bit-exact estimator
// to fall back on (0.5 ms per iteration at 1 M points were never the default) and keep their result.  RS_HIP_STOP_GUARD=0: off.
std::atomic<long long> g_stop_guard_redone{ 0 };      // (diagnostics: rs_hip_icp_stop_guard_redone)
// PLAIN early iterations (round 6).  The reference's centroid chains decide where the iteration CONVERGES; an iteration far from the end only has
// to bring the pose near, and ICP forgets how it got there at its own contraction rate (measured on the headline, the chains in the last m
// iterations of ten: m = 10 / 7 / 5 / 3 / 1 -> 9.9e-7 / 6.9e-7 / 1.3e-6 / 2.5e-6 / 1.0e-5 from the reference's pose; profiles/r06/early_plain.txt).
// Rule, for scan-sized sources (more than 65 536 points): chain iterations precede any iteration whose result can be returned — TWO in a
// call of fixed length, which runs the plain step (fp64 moments centred on their own fp64 centroids: two launches instead of six) until two
// iterations before its end (m = 2 and m = 3 are the same few 1e-6 from the reference's pose on six rooms — <= 3.7e-6 / <= 2.6e-6, neither
// monotone in m — m = 1 is not: 1.1e-5, outside the 1e-5 this policy is held to); three in a call with the stop test (first decision at
// i = 6, icp.h:489), which runs plain in its first four iterations, and only where no bit-exact estimator guards the decision anyway
// (sources above 262 144 points: STOP_GUARD).  A ten-iteration call at 1 M points: 2.52 -> 2.14 ms.  RS_HIP_EARLY_PLAIN=0: off;
// rs_hip_icp_early_plain().  RS_HIP_EARLY_TAIL=m: m chain iterations kept in both kinds of call (tools/early_plain_table.py).
inline int icp_plain_iterations( int n_source, int max_iter, bool fixed_iters )
{
  if( !sw_int( SW_EARLY_PLAIN ) ) return 0;
  const int forced = sw_int( SW_EARLY_TAIL );
  const int keep = forced > 0 ? forced : ( fixed_iters ? 2 : 3 );      // chain iterations before a result can be returned
  const int tail = std::max( 0, max_iter - keep );
  // (by SIZE, not by which kernels run the chains: an object refine contracts too slowly for this — rs_hip_icp_lane_chains_below( 0 ) puts
  //  50 k-point refines on the grid chains, and they keep them in every iteration)
  if( n_source <= ICP_OBJECT_PTS ) return 0;
  if( fixed_iters ) return tail;
  return n_source > ICP_EXACT_PTS ? std::min( std::max( 0, 7 - keep ), tail ) : 0;
}
// PLAIN iterations without records (round 10).  A plain step is a sum in no particular order: nothing in it needs the 48-byte record a
// search scatters to every source point's ORIGINAL index for the chains (icp_emit: pose and source reload, two gathers, three 16-byte
// stores — 78 MB written per 1 M-point search, read back by k_chain_moments).  The search of a plain iteration therefore runs with
// L.rec == null and k_plain_moments forms the moments from m_slot / m_d2 / m_dot in tile order (rs_icp_chain.hip); the iterations that
// keep the chains, or the RECORDS estimator's own, get their records from their own search as before.  RS_HIP_PLAIN_RECORDS=1 /
// rs_hip_icp_plain_from_records( 1 ): the plain step from records again (A/B runs, tests).

// Consecutive segments of one stream sharing their boundary events: one event per boundary instead of
// two (an event between two dependent launches costs a few microseconds of their back-to-back dispatch,
// which matters for the ICP loop's chain of short kernels).
// The ICP loop may be sampled: one call in RS_HIP_PROF_EVERY (default 1: every call) carries the events and the averages
// per launch are taken over those — two events per iteration are ~12 us of a ~180 us iteration, 3-4 % of a bench step.
struct ProfChain
{
  const char* cur = nullptr; hipEvent_t at = nullptr;
  bool on = true;
  ProfChain()
  {
    const unsigned every = (unsigned)sw_int( SW_PROF_EVERY );
    thread_local unsigned tick = 0;
    if( g_prof ) on = ( tick++ % every ) == 0;
  }
  void mark( const char* name )
  {
    if( !g_prof || !on ) return;
    hipEvent_t ev = prof_event();
    if( cur ) prof_span( cur, at, ev );
    cur = name; at = ev;
  }
  ~ProfChain() { if( cur ) mark( nullptr ); }
};

} // namespace

// The fills an ICP call begins with (queue lengths, tickets, statistics accumulators, the two lists of slow tiles, "no certificate") as ONE
// launch.  Each was a hipMemsetAsync — a kernel of the runtime's, 7-9 us apart on the stream: ten of them put 84 us in front of the first
// search of every call (profiles/r06/trace_one_serial_step.txt before this), 3 % of the headline's step.
extern "C" {
namespace rs {
// ... and the call's initial loop state (round 11): a state block of up to STATE_MAX words — six problems — rides in the launch's argument
// block and is written from there, instead of a host-to-device copy packet of its own in front of the launch (icp_upload_state).
struct FillRanges
{
  static constexpr int MAX = 16, STATE_MAX = 256;
  uint32_t* p[MAX]; unsigned long long words[MAX]; uint32_t value[MAX]; int n;
  uint32_t* state_dst; int state_words; uint32_t state[STATE_MAX];
};
__global__ __launch_bounds__( 256 ) void k_fill_ranges( FillRanges R )
{
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
  for( int r = 0; r < R.n; ++r )
    for( size_t i = t; i < R.words[r]; i += step ) R.p[r][i] = R.value[r];
  if( blockIdx.x == 0 && (int)threadIdx.x < R.state_words ) R.state_dst[threadIdx.x] = R.state[threadIdx.x];
}
}
}
namespace {
thread_local rs::FillRanges g_fills{};
int icp_fills_flush()
{
  if( g_fills.n == 0 && g_fills.state_words == 0 ) return RS_HIP_OK;
  unsigned long long most = 0;
  for( int r = 0; r < g_fills.n; ++r ) most = std::max( most, g_fills.words[r] );
  const int blocks = (int)std::min<unsigned long long>( 1024ull, std::max<unsigned long long>( 1ull, ( most + 1023 ) / 1024 ) );
  hipLaunchKernelGGL( rs::k_fill_ranges, dim3( blocks ), dim3( 256 ), 0, g_stream, g_fills );
  g_fills.n = 0; g_fills.state_words = 0;
  return RS_HIP_OK;      // (a failed launch surfaces at the call's synchronisation, like every other kernel's)
}
// hipMemsetAsync( p, byte, bytes, g_stream ), deferred to the call's one fill launch (icp_fills_flush: before the first kernel that reads p)
int icp_fill( void* p, int byte, size_t bytes )
{
  if( bytes == 0 ) return RS_HIP_OK;
  if( ( bytes & 3 ) || ( (uintptr_t)p & 3 ) ) { HIP_TRY( hipMemsetAsync( p, byte, bytes, g_stream ), RS_HIP_E_RUNTIME ); return RS_HIP_OK; }
  if( g_fills.n == rs::FillRanges::MAX ) { if( int rc = icp_fills_flush() ) return rc; }
  const uint32_t b = (uint32_t)( byte & 0xff );
  g_fills.p[g_fills.n] = (uint32_t*)p; g_fills.words[g_fills.n] = bytes / 4; g_fills.value[g_fills.n] = b | ( b << 8 ) | ( b << 16 ) | ( b << 24 ); ++g_fills.n;
  return RS_HIP_OK;
}
}

namespace {

struct IcpCtx
{
  IcpLaunch L{};
  int n_waves = 0;             // tiles of the (largest) source: the searches' grid
  size_t total_pts = 0;        // rows of the per-point arrays over all problems (one source: n_prob x n)
  size_t total_tiles = 0;      // likewise per tile
  size_t heavy_words = 0;      // words of one slow-tile buffer over all problems
};

// One source for all problems (src), or one per problem (srcs[n_prob], src == null: a multi-source batch — the kernels then bind
// their problem's view on the device, rs_icp.h: icp_bind).
int icp_prepare( IcpCtx& cx, const rs_hip_cloud_t* src, const rs_hip_cloud_t* tgt, int n_prob, const float* T2, const rs_hip_cloud_t* const* srcs = nullptr )
{
  if( n_prob <= 0 ) { set_err( "icp: empty batch" ); return RS_HIP_E_ARG; }
  if( !tgt || !tgt->has_nor || ( !src && !srcs ) ) { set_err( "icp: source and target clouds need normals" ); return RS_HIP_E_ARG; }
  for( int p = 0; p < ( srcs ? n_prob : 1 ); ++p )
  {
    const rs_hip_cloud_t* c = srcs ? srcs[p] : src;
    if( !c || !c->has_nor ) { set_err( "icp: source and target clouds need normals" ); return RS_HIP_E_ARG; }
  }
  IcpLaunch& L = cx.L;
  L.tgt = tgt->view; L.tgt.evals = g_prof ? g_evals : nullptr; L.n_prob = n_prob; L.K = 16;   // icp.h:330
  Mat4 t2; std::memcpy( t2.m, T2, 64 );
  Mat4 t2i = mat4_inverse( t2 );                                                                             // icp.h:329
  std::memcpy( L.T2i.m, t2i.m, 64 );
  const size_t np = (size_t)n_prob;
  int rc;
  L.multi = nullptr;
  if( srcs )
  {
    if( ( rc = g_ws.h_multi.ensure( np * sizeof( IcpProblem ) ) ) || ( rc = g_ws.multi.ensure( np * sizeof( IcpProblem ) ) ) ) return rc;
    // (pinned and only ever written here: every ICP entry point ends with a stream synchronisation, so the upload of the previous
    //  call's views is over before this one overwrites them)
    IcpProblem* P = g_ws.h_multi.as<IcpProblem>();
    size_t pts = 0, tiles = 0, heavy = 0; int max_n = 0, max_tiles = 0;
    for( size_t p = 0; p < np; ++p )
    {
      P[p].src = srcs[p]->qview; P[p].by_orig = srcs[p]->d_qby_orig;
      P[p].pt_off = (long long)pts; P[p].tile_off = (long long)tiles; P[p].heavy_off = (long long)heavy;
      pts += (size_t)srcs[p]->n; tiles += (size_t)srcs[p]->qview.n_tiles; heavy += heavy_stride( srcs[p]->qview.n_tiles );
      max_n = std::max( max_n, (int)srcs[p]->n ); max_tiles = std::max( max_tiles, srcs[p]->qview.n_tiles );
    }
    HIP_TRY( hipMemcpyAsync( g_ws.multi.p, P, np * sizeof( IcpProblem ), hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
    L.multi = (const IcpProblem*)g_ws.multi.p; L.src = QueryView{}; L.by_orig = nullptr;
    L.max_n = max_n; L.max_tiles = max_tiles;
    cx.total_pts = std::max<size_t>( 1, pts ); cx.total_tiles = std::max<size_t>( 1, tiles ); cx.heavy_words = heavy;
  }
  else
  {
    L.src = src->qview; L.by_orig = src->d_qby_orig; L.max_n = src->n; L.max_tiles = src->qview.n_tiles;
    cx.total_pts = np * std::max<size_t>( 1, (size_t)src->n ); cx.total_tiles = np * (size_t)std::max( 1, src->qview.n_tiles );
    cx.heavy_words = np * heavy_stride( src->qview.n_tiles );
  }
  cx.n_waves = L.max_tiles;
  L.n_mom_blocks = std::max( 1, std::min( 512, ( L.max_n + 255 ) / 256 ) );    // (the fp64 moments' own grid; a plain iteration's is plain_moment_blocks: at most 512 workgroups too)
  if( ( rc = g_ws.state.ensure( np * ICP_STATE_WORDS * 4 ) ) ||
      ( rc = g_ws.slot.ensure( cx.total_pts * 4 ) ) || ( rc = g_ws.d2.ensure( cx.total_pts * 4 ) ) || ( rc = g_ws.dot.ensure( cx.total_pts * 4 ) ) ||
      ( rc = g_ws.stat_acc.ensure( np * STAT_SHARDS * 4 * 8 ) ) ||
      ( rc = g_ws.mom_part.ensure( np * L.n_mom_blocks * ICP_NMOM * 8 ) ) || ( rc = g_ws.res.ensure( np * ICP_NRES * 8 ) ) ||
      ( rc = g_ws.h_a.ensure( np * ICP_NRES * 8 ) ) || ( rc = g_ws.h_b.ensure( np * ICP_STATE_WORDS * 4 ) ) ||
      ( rc = g_ws.queue.ensure( cx.total_tiles * 4 ) ) || ( rc = g_ws.queue_count.ensure( np * 4 ) ) )
    return rc;
  L.queue = g_ws.queue.as<int>(); L.queue_count = g_ws.queue_count.as<int>();
  L.solo_stages = handoff_threshold( (long long)cx.total_tiles );
  L.heavy_streamed = sw_int( SW_HEAVY_STREAMED ); L.heavy_handoff = sw_int( SW_HEAVY_HANDOFF ); L.heavy_total = sw_int( SW_HEAVY_TOTAL );
  float* w = g_ws.state.as<float>();
  L.T1 = w + np * ICP_ST_T1; L.active = (int*)( w + np * ICP_ST_ACTIVE ); L.T1_prev = w + np * ICP_ST_T1_PREV;
  L.iters = (int*)( w + np * ICP_ST_ITERS ); L.err = w + np * ICP_ST_ERR; L.prev_err = w + np * ICP_ST_PREV_ERR;
  L.queued = (int*)( w + np * ICP_ST_QUEUED ); L.ticket = (int*)( w + np * ICP_ST_TICKET );
  L.solve = 0; L.iter_index = 0; L.fixed_iters = 0;
  L.seed = sw_flag( SW_NO_SEED ) ? 0 : 1;
  L.by_rows = sw_flag( SW_NO_BY_ROWS ) ? 0 : 1;
  L.bounded_only = sw_flag( SW_NO_BOUNDED_ONLY ) ? 0 : 1;
  L.cert_r = nullptr; L.cert_dot = nullptr; L.cert_slack = nullptr; L.tgt_nor_max = tgt->nor_max;
  L.m_slot = g_ws.slot.as<int>(); L.m_d2 = g_ws.d2.as<float>(); L.m_dot = g_ws.dot.as<float>();
  L.stat_acc = nullptr;       // set by the align loop (fp64 estimator only)
  L.mom_part = g_ws.mom_part.as<double>(); L.res = g_ws.res.as<double>();
  L.w_explicit = nullptr;
  L.faith = nullptr;
  {
    // one counter for the process (every calling thread's kernels add to it; rs_hip_icp_faith_redone reads it from any thread)
    std::lock_guard<std::mutex> lk( g_faith_redone_mu );
    if( !g_faith_redone.p )
    {
      if( int rc = g_faith_redone.ensure( 64 ) ) return rc;
      HIP_TRY( hipMemset( g_faith_redone.p, 0, 64 ), RS_HIP_E_RUNTIME );
    }
  }
  L.faith_redone = g_faith_redone.as<int>();
  L.faith_guess_scale = (float)sw_int( SW_FAITH_GUESS ) / 1000.0f;
  g_fills.n = 0; g_fills.state_words = 0;      // (fills an earlier call queued and never launched — it failed before its first kernel — are not this call's)
  if( int rcf = icp_fill( g_ws.queue_count.p, 0, np * 4 ) ) return rcf;
  return RS_HIP_OK;
}

// Waves per queued tile in the cooperative kernel.  A short queue is bound by its heaviest tile (8 waves: from the third iteration on the
// certificates have emptied it; launches that skip phase A: while there are few tiles), a long one by throughput (4).  Batches of many
// problems (round 6): object refines keep a long queue in every iteration — the rim of every object has nothing to match — and the
// launch is throughput-bound however late: 512 50 k-point refines (410 k tiles) 33.8 ms per step with 8 waves per tile, 30.2 with 4,
// 28.9 with 2.
inline int icp_coop_waves( const IcpLaunch& L, long long total_tiles, int n_prob, int i )
{
  if( n_prob > 8 && total_tiles >= 131072 ) return 2;
  if( n_prob > 8 && total_tiles >= 32768 ) return 4;
  return L.coop_all ? ( total_tiles <= 1536 ? 8 : 4 ) : ( ( i >= 2 && L.cert_r ) ? 8 : 4 );
}

// buffers of the parallel reference-order estimator for n_prob problems of n_source points
int replay_prepare( ReplayBufs& B, int n_prob, int n_source )
{
  B.n_seg = replay_segments( n_source ); B.n_super = replay_superblocks( n_source );
  const size_t rows = (size_t)n_prob * ICP_NMOM * (size_t)B.n_seg, srows = (size_t)n_prob * ICP_NMOM * (size_t)B.n_super;
  int rc;
  if( ( rc = g_ws.rp_segsum.ensure( rows * 8 ) ) || ( rc = g_ws.rp_guess.ensure( 3 * rows * 8 ) ) || ( rc = g_ws.rp_seg.ensure( rows * replay_seg_bytes() ) ) ||
      ( rc = g_ws.rp_super.ensure( srows * replay_seg_bytes() ) ) ||
      ( rc = g_ws.rp_totals.ensure( (size_t)n_prob * 3 * ICP_NMOM * 8 ) ) || ( rc = g_ws.rp_redone.ensure( (size_t)n_prob * 4 + 64 ) ) ) return rc;
  B.segsum = g_ws.rp_segsum.as<double>(); B.guess = g_ws.rp_guess.as<double>(); B.seg = (ReplaySeg*)g_ws.rp_seg.p; B.super = (ReplaySeg*)g_ws.rp_super.p;
  B.totals = g_ws.rp_totals.as<double>(); B.redone = g_ws.rp_redone.as<int>();
  if( int rcf = icp_fill( g_ws.rp_redone.p, 0, (size_t)n_prob * 4 + 64 ) ) return rcf;
  return RS_HIP_OK;
}

// initial loop state (icp.h:441-442: errors start at 1e6): with the call's fill launch when it fits in its argument block (the launch
// is enqueued by icp_fills_flush, before the first kernel of the call), else by a copy from the pinned block
int icp_upload_state( IcpCtx& cx, const float* T1s, size_t np )
{
  const bool by_launch = np * ICP_STATE_WORDS <= (size_t)rs::FillRanges::STATE_MAX;
  float* h = by_launch ? reinterpret_cast<float*>( g_fills.state ) : g_ws.h_b.as<float>();
  std::memset( h, 0, np * ICP_STATE_WORDS * 4 );
  int* hi = (int*)h;
  for( size_t p = 0; p < np; ++p )
  {
    std::memcpy( h + np * ICP_ST_T1 + 16 * p, T1s + 16 * p, 64 ); hi[np * ICP_ST_ACTIVE + p] = 1;
    std::memcpy( h + np * ICP_ST_T1_PREV + 16 * p, T1s + 16 * p, 64 );
    h[np * ICP_ST_ERR + p] = 1e6f; h[np * ICP_ST_PREV_ERR + p] = 1e6f;
  }
  if( by_launch )
  {
    // (the pinned block too: a call that enqueues no iteration — max_iter <= 0 — reads its results from there without a copy back)
    std::memcpy( g_ws.h_b.as<float>(), h, np * ICP_STATE_WORDS * 4 );
    g_fills.state_dst = g_ws.state.as<uint32_t>(); g_fills.state_words = (int)( np * ICP_STATE_WORDS ); return RS_HIP_OK;
  }
  HIP_TRY( hipMemcpyAsync( g_ws.state.p, h, np * ICP_STATE_WORDS * 4, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  return RS_HIP_OK;
}

// Certificates on (rs_icp_search.hip: icp_certificate): two floats per (problem, source point).
int icp_enable_certificates( IcpCtx& cx )
{
  int rc;
  const size_t words = cx.total_pts;
  if( sw_flag( SW_NO_CERT ) || !std::isfinite( cx.L.tgt_nor_max ) ) return RS_HIP_OK;
  if( ( rc = g_ws.cert_r.ensure( words * 4 ) ) || ( rc = g_ws.cert_dot.ensure( words * 4 ) ) ) return rc;
  if( int rcf = icp_fill( g_ws.cert_r.p, 0xFF, words * 4 ) ) return rcf;      // NaN: no certificate
  cx.L.cert_r = g_ws.cert_r.as<float>(); cx.L.cert_dot = g_ws.cert_dot.as<float>();
  if( !sw_flag( SW_NO_RANK_CERT ) )            // read only next to a valid cert_r, written with every fresh one: no initialisation
  {
    if( ( rc = g_ws.cert_slack.ensure( words * 4 ) ) ) return rc;
    cx.L.cert_slack = g_ws.cert_slack.as<float>();
  }
  return RS_HIP_OK;
}

// ---- diagnostics (RS_HIP_DEBUG / RS_HIP_DEBUG_CYCLES): one iteration per chunk, device timers per tile ----
void icp_debug_before( IcpCtx& cx, int n, bool cycles )
{
  static DevBuf dbgbuf;
#ifndef RS_DBG
#define RS_DBG 0
#endif
  if( cycles && !RS_DBG )
  { static bool told = false; if( !told ) fprintf( stderr, "[rs_hip] RS_HIP_DEBUG_CYCLES needs the diagnostic build: tools/variant.sh dbg -DRS_DBG=1, then RS_HIP_LIB=.../librescan_hip_dbg.so\n" ); told = true; }
  if( RS_DBG && cycles && n == 1 )
  {
    if( dbgbuf.ensure( (size_t)cx.n_waves * 48 + 64 ) ) return;
    (void)hipMemsetAsync( (char*)dbgbuf.p + (size_t)cx.n_waves * 48, 0, 64, g_stream );
    cx.L.dbg = dbgbuf.as<unsigned long long>();
  }
}

void icp_debug_after( IcpCtx& cx, int n_src, int n, int i, float max_dist )
{
  (void)hipStreamSynchronize( g_stream );
  std::vector<int> qc( n ), ms( (size_t)n_src ); std::vector<float> cr( cx.L.cert_r ? (size_t)n_src : 0 );
  (void)hipMemcpy( qc.data(), cx.L.queue_count, (size_t)n * 4, hipMemcpyDeviceToHost );      // (reset when the iteration ends)
  (void)hipMemcpy( ms.data(), cx.L.m_slot, ms.size() * 4, hipMemcpyDeviceToHost );
  if( cx.L.cert_r ) (void)hipMemcpy( cr.data(), cx.L.cert_r, cr.size() * 4, hipMemcpyDeviceToHost );
  size_t unm = 0, cert = 0;
  for( int v : ms ) unm += v < 0;
  for( float v : cr ) cert += v > 0.0f;
  long long st_sum = 0, st_cnt = 0;
  if( cx.L.heavy_out )
  {
    std::vector<int> words( (size_t)cx.n_waves );
    (void)hipMemcpy( words.data(), cx.L.heavy_out + HEAVY_HDR + HEAVY_SLOTS, words.size() * 4, hipMemcpyDeviceToHost );
    for( int v : words ) if( (unsigned)v >> 2 ) { st_sum += (unsigned)v >> 2; ++st_cnt; }
    long long heavy = 0; for( int v : words ) heavy += ( v & 3 ) == 2;
    fprintf( stderr, "[rs_hip icp]   of the queued tiles, handed off as HEAVY bounded tiles (flag 2): %lld\n", heavy );
  }
  fprintf( stderr, "[rs_hip icp] it %d (max_dist %g, coop waves %d): prob 0 queued tiles %d of %d, unmatched %zu of %d, certificates %zu, candidates streamed per tile of phase A %lld\n",
           i, (double)max_dist, cx.L.coop_waves, qc[0], cx.n_waves, unm, n_src, cert, st_cnt ? st_sum / st_cnt : 0ll );
  if( !cx.L.dbg ) return;
  std::vector<unsigned long long> h( (size_t)cx.n_waves * 2 );
  (void)hipMemcpy( h.data(), cx.L.dbg, h.size() * 8, hipMemcpyDeviceToHost );
  struct Row { unsigned long long start, ticks; unsigned uns, handoff, stages, streamed, rank_streamed; };
  std::vector<Row> t;
  unsigned long long sum = 0, ho = 0, tiles_uns = 0, n_rank = 0, t0 = ~0ull, t1 = 0;
  for( int k = 0; k < cx.n_waves; ++k )
  {
    const unsigned long long v = h[2*k+1];
    Row r{ h[2*k], v & 0xfffff, (unsigned)( v >> 57 ), (unsigned)( ( v >> 20 ) & 1 ), (unsigned)( ( v >> 21 ) & 15 ), (unsigned)( ( v >> 25 ) & 0xffff ), (unsigned)( ( v >> 41 ) & 0xffff ) };
    t.push_back( r ); sum += r.ticks; ho += r.uns; tiles_uns += r.uns ? 1 : 0; n_rank += r.rank_streamed ? 1 : 0;
    t0 = std::min( t0, r.start ); t1 = std::max( t1, r.start + r.ticks );
  }
  fprintf( stderr, "[rs_hip dbg] phase A: %.1f us from first wave start to last wave end; unsettled lanes after shell 1: %llu in %llu tiles; rank pass in %llu tiles; mean tile %.1f us\n",
           ( t1 - t0 ) / 100.0, ho, tiles_uns, n_rank, (double)sum / cx.n_waves / 100.0 );
  {
    // waves in flight over time (10 slices) and the tiles that end last
    const double span = (double)( t1 - t0 );
    int live[10] = { 0 };
    for( const Row& r : t ) for( int b = 0; b < 10; ++b ) { const double at = t0 + span * ( b + 0.5 ) / 10; if( r.start <= at && at < r.start + r.ticks ) live[b]++; }
    fprintf( stderr, "[rs_hip dbg]   waves in flight at 5%%,15%%,..95%% of the span:" ); for( int b = 0; b < 10; ++b ) fprintf( stderr, " %d", live[b] ); fprintf( stderr, "\n" );
    std::vector<Row> byend = t; std::sort( byend.begin(), byend.end(), []( const Row& a, const Row& b ) { return a.start + a.ticks > b.start + b.ticks; } );
    for( int k = 0; k < 5 && k < (int)byend.size(); ++k )
      fprintf( stderr, "[rs_hip dbg]   late finisher: starts at %.1f us, runs %.1f us, shells %u, streamed %u, rank-pass %u, handoff %u\n",
               ( byend[k].start - t0 ) / 100.0, byend[k].ticks / 100.0, byend[k].stages, byend[k].streamed, byend[k].rank_streamed, byend[k].handoff );
  }
  {
    // per XCD class of phase A's tile map (rs_xcdmap.h): each XCD dispatches its own class, so a class that ends long after the
    // others is a launch that ends with slots empty.  Times in us from the launch's first start; a tile handed to the cooperative
    // kernel without a search (flag 2) has a start and no time.  The list is the one this launch wrote for the next one's front slots.
    struct Cls { long long tiles = 0; unsigned long long sum = 0, first = ~0ull, last_start = 0, last_end = 0; } cls[XCD_CLASSES];
    const int nb = xm_blocks( cx.n_waves, RS_PA_WAVES ), map_k = ( cx.L.warm && cx.L.bounded_only ) ? RS_XCD_CHUNK_WARM_LOG2 : RS_XCD_CHUNK_LOG2;      // (this launch's: launch_icp_corr)
    for( int k = 0; k < cx.n_waves; ++k )
    {
      Cls& c = cls[RS_XCD_MAP ? xm_class( k / RS_PA_WAVES, nb, map_k ) : ( k / RS_PA_WAVES ) & ( XCD_CLASSES - 1 )];
      c.tiles++; c.sum += t[k].ticks; c.first = std::min( c.first, t[k].start ); c.last_start = std::max( c.last_start, t[k].start ); c.last_end = std::max( c.last_end, t[k].start + t[k].ticks );
    }
    int fill[XCD_CLASSES] = { 0 };
    if( cx.L.heavy_out ) (void)hipMemcpy( fill, cx.L.heavy_out, sizeof( fill ), hipMemcpyDeviceToHost );
    fprintf( stderr, "[rs_hip dbg]   tile map: %s, chunk log2 %d, %d natural blocks\n", RS_XCD_MAP ? ( map_k < 0 ? "contiguous eighths" : "chunks dealt to the classes" ) : "none", map_k, nb );
    for( int c = 0; c < XCD_CLASSES; ++c )
      fprintf( stderr, "[rs_hip dbg]   class %d: tiles %lld, tile time %.1f ms, first start %.1f us, last start %.1f us, last end %.1f us, slow-tile list %d of %d\n", c, cls[c].tiles, cls[c].sum / 1e5,
               cls[c].tiles ? ( cls[c].first - t0 ) / 100.0 : 0.0, cls[c].tiles ? ( cls[c].last_start - t0 ) / 100.0 : 0.0, cls[c].tiles ? ( cls[c].last_end - t0 ) / 100.0 : 0.0, fill[c], HEAVY_PER_CLASS );
  }
  std::sort( t.begin(), t.end(), []( const Row& a, const Row& b ) { return a.ticks < b.ticks; } );
  for( double q : { 0.5, 0.9, 0.99, 0.999, 1.0 } )
  {
    const Row& r = t[std::min( t.size() - 1, (size_t)( q * t.size() ) )];
    fprintf( stderr, "[rs_hip dbg]   phase A p%g: %.1f us, shells %u, streamed %u, rank-pass streamed %u, handoff %u\n", q * 100, r.ticks / 100.0, r.stages, r.streamed, r.rank_streamed, r.handoff );
  }
  std::vector<unsigned long long> c( (size_t)qc[0] * 4 );
  (void)hipMemcpy( c.data(), cx.L.dbg + 2 * (size_t)cx.n_waves, c.size() * 8, hipMemcpyDeviceToHost );
  std::vector<std::array<unsigned long long, 4>> rows;
  for( int b = 0; b < qc[0]; ++b ) rows.push_back( { c[4*b], c[4*b+1], c[4*b+2], c[4*b+3] } );
  std::sort( rows.begin(), rows.end() );
  auto pr = [&]( const char* tag, size_t k ) { if( rows.empty() ) return; k = std::min( k, rows.size() - 1 );
    fprintf( stderr, "[rs_hip dbg]   coop %s: %.1f us (setup %.1f, shell k=2 %.1f, full shell %.1f, rest %.1f), wave-0 streamed %llu cand, searching lanes %llu, unmatched %llu\n", tag, rows[k][0] / 100.0,
             ( rows[k][3] & 0xffff ) / 100.0, ( ( rows[k][3] >> 16 ) & 0xffff ) / 100.0, ( ( rows[k][3] >> 32 ) & 0xffff ) / 100.0, ( rows[k][3] >> 48 ) / 100.0,
             rows[k][1], rows[k][2] & 0xff, ( rows[k][2] >> 8 ) & 0xff ); };
  // cell rows per sweep (the first three of a tile; 0: no such sweep) and row-table loads per tile, over the queued tiles
  {
    std::vector<unsigned> v[4];
    for( const auto& r : rows )
    {
      for( int s = 0; s < 3; ++s ) { const unsigned n = (unsigned)( ( r[2] >> ( 16 + 14 * s ) ) & 0x3fff ); if( n ) v[s].push_back( n ); }
      v[3].push_back( (unsigned)( r[2] >> 58 ) );
    }
    const char* what[4] = { "cell rows of sweep 1", "cell rows of sweep 2", "cell rows of sweep 3", "row-table loads per tile" };
    for( int s = 0; s < 4; ++s )
    {
      if( v[s].empty() ) continue;
      std::sort( v[s].begin(), v[s].end() );
      fprintf( stderr, "[rs_hip dbg]   coop %s: p50 %u, p90 %u, max %u (%zu tiles)\n", what[s], v[s][v[s].size() / 2], v[s][v[s].size() * 9 / 10], v[s].back(), v[s].size() );
    }
  }
  unsigned long long cat[4]; (void)hipMemcpy( cat, cx.L.dbg + 6 * (size_t)cx.n_waves, 32, hipMemcpyDeviceToHost );
  if( RS_DBG >= 2 ) fprintf( stderr, "[rs_hip dbg]   unmatched lanes: skipped by certificate %llu, freshly certified %llu, rank-rejected %llu, loose-band only %llu\n", cat[0], cat[1], cat[2], cat[3] );
  pr( "p10", rows.size() / 10 ); pr( "p50", rows.size() / 2 ); pr( "p90", rows.size() * 9 / 10 ); pr( "p99", rows.size() * 99 / 100 ); pr( "max", rows.size() - 1 );
}

void icp_set_radius( IcpCtx& cx, float max_dist, float tmin )
{
  cx.L.radius = max_dist; cx.L.radius_sq = radius_sq_of( max_dist ); cx.L.gate_tmin = tmin;
  // fixed-point scales of the dist² statistics: r²·2^e1 and r⁴·2^e2 just below 2^36, so that a tile's sum (64 terms)
  // and the sum over 2^22 tiles stay below 2^64, with 36 bits below the radius
  const double r2 = cx.L.radius_sq;
  int e1 = 0, e2 = 0;
  if( r2 > 0.0 && std::isfinite( r2 ) ) { e1 = 35 - std::ilogb( r2 ); e2 = 35 - std::ilogb( r2 * r2 ); }
  e1 = std::max( -900, std::min( 900, e1 ) ); e2 = std::max( -900, std::min( 900, e2 ) );
  cx.L.stat_s1 = std::ldexp( 1.0, e1 ); cx.L.stat_i1 = std::ldexp( 1.0, -e1 );
  cx.L.stat_s2 = std::ldexp( 1.0, e2 ); cx.L.stat_i2 = std::ldexp( 1.0, -e2 );
}

// Buffers of the lane-chain estimator for the problems of cx (cx.total_pts source points in all, the largest cx.L.max_n): the searches'
// records, the seven totals per problem, the moments' partials (one per 1 024 source points of the largest problem), the update's ticket.
std::atomic<long long> g_lane_seq_addends{ 0 }, g_lane_addends{ 0 };      // (diagnostics: rs_hip_icp_lane_chains_sequential)
int icp_lane_prepare( IcpCtx& cx, ChainBufs& CB )
{
  int rc;
  const size_t np = (size_t)cx.L.n_prob, rows = cx.total_pts;
  const int max_n = cx.L.max_n;
  CB.n_seg = chain_segments( max_n ); CB.n_blk = chain_blocks( max_n ); CB.refresh = 0;
  cx.L.n_mom_blocks = CB.n_blk * 4;
  if( ( rc = g_ws.ch_rec.ensure( std::max<size_t>( 1, rows ) * REC_F4 * 16 ) ) || ( rc = g_ws.rp_totals.ensure( np * 3 * ICP_NMOM * 8 ) ) ||
      ( rc = g_ws.rp_redone.ensure( np * 4 + 64 ) ) || ( rc = g_ws.ch_done.ensure( np * 8 ) ) ||
      ( rc = g_ws.mom_part.ensure( np * (size_t)cx.L.n_mom_blocks * ICP_NMOM * 8 ) ) ||
      ( rc = g_ws.ch_segsum.ensure( 8 * ( rows + 4 * np ) * 4 ) ) ) return rc;
  CB.addends = g_ws.ch_segsum.as<float>();      // (the grid chains' buffer: the two estimators never run in one call)
  if( sw_flag( SW_LANE_DEBUG ) )
  {
    if( ( rc = g_ws.ch_dbg.ensure( np * CH_ROWS * 16 ) ) ) return rc;
    HIP_TRY( hipMemsetAsync( g_ws.ch_dbg.p, 0, np * CH_ROWS * 16, g_stream ), RS_HIP_E_RUNTIME );
    CB.dbg = g_ws.ch_dbg.as<int>();
  }
  if( int rcf = icp_fill( g_ws.rp_redone.p, 0, np * 4 + 64 ) ) return rcf;
  if( int rcf = icp_fill( g_ws.ch_done.p, 0, np * 8 ) ) return rcf;
  CB.totals = g_ws.rp_totals.as<double>(); CB.resolved = g_ws.rp_redone.as<int>(); CB.done = g_ws.ch_done.as<int>(); CB.failed = nullptr;
  cx.L.rec = (float4*)g_ws.ch_rec.p; cx.L.mom_part = g_ws.mom_part.as<double>();
  g_lane_addends.fetch_add( (long long)rows * CH_ROWS );      // (per iteration; the diagnostic divides by what it counted the same way)
  return RS_HIP_OK;
}
// (diagnostics) addends the walks of this call added one by one, over all its iterations
void icp_lane_account( const ChainBufs& CB, int n_prob )
{
  std::vector<int> r( (size_t)n_prob );
  if( hipMemcpy( r.data(), CB.resolved, r.size() * 4, hipMemcpyDeviceToHost ) != hipSuccess ) return;
  long long t = 0; for( int v : r ) t += v;
  g_lane_seq_addends.fetch_add( t );
  if( CB.dbg )
  {
    std::vector<int> d( (size_t)n_prob * CH_ROWS * 4 );
    if( hipMemcpy( d.data(), CB.dbg, d.size() * 4, hipMemcpyDeviceToHost ) != hipSuccess ) return;
    for( int p = 0; p < std::min( n_prob, 4 ); ++p )
      for( int row = 0; row < CH_ROWS; ++row )
      {
        const int* o = d.data() + ( (size_t)p * CH_ROWS + row ) * 4;
        fprintf( stderr, "[rs_hip lane] problem %d chain %d: %d points, walk %.2f us, %d attempts (%d stretches), %d addends one by one\n", p, row, o[3], o[0] / 100.0, o[1], ( o[3] + 511 ) / 512, o[2] );
      }
  }
}

// One call's estimator: which (icp_choose), its buffers, its early plain iterations (icp_plain_iterations).
struct IcpEst
{
  IcpEstimator est;
  ReplayBufs RB{};
  ChainBufs CB{};
  int n_plain = 0;
};
inline bool icp_exact_centroids( IcpEstimator e ) { return e == ICP_EST_LANE_CHAINS || e == ICP_EST_GRID_CHAINS || e == ICP_EST_RECORDS; }

// The buffers of E.est for the problems of cx (cx.total_pts source points in all, the largest cx.L.max_n), their fills queued.
int icp_estimator_prepare( IcpCtx& cx, IcpEst& E )
{
  int rc;
  const int n = cx.L.n_prob, max_n = cx.L.max_n;
  const size_t np = (size_t)n, pts = cx.total_pts;
  ReplayBufs& RB = E.RB;
  ChainBufs& CB = E.CB;
  switch( E.est )
  {
  case ICP_EST_REF_ORDER:
  case ICP_EST_REPLAY:
    if( ( rc = g_ws.faith.ensure( (size_t)FAITH_REC * pts * 4 ) ) ) return rc;
    cx.L.faith = g_ws.faith.as<float>();
    if( E.est == ICP_EST_REPLAY && ( rc = replay_prepare( RB, n, max_n ) ) ) return rc;
    return RS_HIP_OK;
  case ICP_EST_LANE_CHAINS:
    if( ( rc = icp_lane_prepare( cx, CB ) ) ) return rc;
    RB.totals = CB.totals;
    break;
  case ICP_EST_GRID_CHAINS:
  {
    if( ( rc = g_ws.rp_totals.ensure( np * 3 * ICP_NMOM * 8 ) ) || ( rc = g_ws.rp_redone.ensure( np * 4 + 64 ) ) ) return rc;
    RB.totals = g_ws.rp_totals.as<double>(); RB.redone = g_ws.rp_redone.as<int>();
    if( int rcf = icp_fill( g_ws.rp_redone.p, 0, np * 4 + 64 ) ) return rcf;
    CB.n_seg = chain_segments( max_n ); CB.n_blk = chain_blocks( max_n );
    const size_t rows = np * CH_ROWS;
    if( ( rc = g_ws.ch_rec.ensure( pts * REC_F4 * 16 ) ) || ( rc = g_ws.ch_segsum.ensure( rows * CB.n_seg * 8 ) ) ||
        ( rc = g_ws.ch_prefix.ensure( rows * CB.n_blk * 4 * 8 ) ) || ( rc = g_ws.ch_seg.ensure( rows * CB.n_seg * sizeof( ChainRec ) ) ) ||
        ( rc = g_ws.ch_blk.ensure( rows * CB.n_blk * sizeof( ChainRec ) ) ) ||
        ( rc = g_ws.ch_guess.ensure( rows * CB.n_seg * 4 ) ) ) return rc;
    CB.segsum = g_ws.ch_segsum.as<double>(); CB.blksum = g_ws.ch_prefix.as<double>(); CB.seg = (ChainRec*)g_ws.ch_seg.p; CB.blk = (ChainRec*)g_ws.ch_blk.p; CB.guess = g_ws.ch_guess.as<int>();
    CB.totals = RB.totals; CB.resolved = RB.redone;
    if( ( rc = g_ws.ch_done.ensure( np * 8 ) ) ) return rc;
    if( int rcf = icp_fill( g_ws.ch_done.p, 0, np * 8 ) ) return rcf;
    CB.done = g_ws.ch_done.as<int>(); CB.failed = (int*)( g_ws.state.as<float>() + np * ICP_ST_FAILED );      // (zero since icp_upload_state)
    if( const int dbg_reps = sw_int( SW_CHAIN_DEBUG ) )      // (at least 1 when the name is set)
    {
      if( ( rc = g_ws.ch_dbg.ensure( rows * ( 4 + 64 * 8 ) * 4 ) ) ) return rc;
      CB.dbg = g_ws.ch_dbg.as<int>(); CB.dbg_reps = dbg_reps;
      // the walk writes its mismatch marker only where it finds 0: a fresh (or an earlier call's) buffer must not speak for this one
      HIP_TRY( hipMemsetAsync( g_ws.ch_dbg.p, 0, rows * ( 4 + 64 * 8 ) * 4, g_stream ), RS_HIP_E_RUNTIME );
      if( !sw_flag( SW_CHAIN_DEBUG_NO_SELFCHECK ) )      // (the self-check redoes every step the slow way: without it the stamps are the walk's real times)
      {
        if( ( rc = g_ws.ch_chk.ensure( rows * ( 4 + 3 * 4096 ) * 4 ) ) ) return rc;
        HIP_TRY( hipMemsetAsync( g_ws.ch_chk.p, 0, rows * ( 4 + 3 * 4096 ) * 4, g_stream ), RS_HIP_E_RUNTIME );
        CB.chk = g_ws.ch_chk.as<int>();
      }
    }
    cx.L.rec = (float4*)g_ws.ch_rec.p;
    cx.L.n_mom_blocks = CB.n_blk * 4;              // k_chain_moments: one workgroup, one partial, per quarter block (1 024 source points)
    // (the larger of the two layouts: a plain iteration's k_plain_moments leaves plain_moment_blocks partials per moment)
    if( ( rc = g_ws.mom_part.ensure( np * (size_t)std::max( CB.n_blk * 4, plain_moment_blocks( cx.L.max_tiles ) ) * ICP_NMOM * 8 ) ) ) return rc;
    cx.L.mom_part = g_ws.mom_part.as<double>();
    break;
  }
  case ICP_EST_RECORDS:
    // the replay's buffers, the searches' records, the chains' moment kernel and update (launch_icp_exact_centroids_from_records)
    if( ( rc = replay_prepare( RB, n, max_n ) ) ) return rc;
    CB.n_seg = chain_segments( max_n ); CB.n_blk = chain_blocks( max_n ); CB.refresh = 0;
    if( ( rc = g_ws.ch_rec.ensure( pts * REC_F4 * 16 ) ) || ( rc = g_ws.ch_done.ensure( np * 8 ) ) ||
        ( rc = g_ws.mom_part.ensure( np * (size_t)std::max( CB.n_blk * 4, plain_moment_blocks( cx.L.max_tiles ) ) * ICP_NMOM * 8 ) ) ) return rc;
    if( int rcf = icp_fill( g_ws.ch_done.p, 0, np * 8 ) ) return rcf;
    CB.done = g_ws.ch_done.as<int>();
    cx.L.rec = (float4*)g_ws.ch_rec.p;
    cx.L.n_mom_blocks = CB.n_blk * 4;
    cx.L.mom_part = g_ws.mom_part.as<double>();
    break;
  case ICP_EST_MOMENTS:
    break;
  }
  if( icp_exact_centroids( E.est ) ) { cx.L.exact_centroids = 1; cx.L.centroid_totals = RB.totals; }
  // (the fp64 moments' integer statistics)
  if( int rcf = icp_fill( g_ws.stat_acc.p, 0, np * STAT_SHARDS * 4 * 8 ) ) return rcf;
  cx.L.stat_acc = g_ws.stat_acc.as<unsigned long long>();
  return RS_HIP_OK;
}

// Enqueues the estimator launches of iteration i; returns the RS_HIP_ICP_STEP_* kind of what it launched.
int icp_step( IcpCtx& cx, IcpEst& E, int i )
{
  const int chain_refresh = sw_int( SW_CHAIN_REFRESH );
  switch( E.est )
  {
  case ICP_EST_REF_ORDER:   launch_icp_faithful( cx.L, g_stream ); break;
  case ICP_EST_REPLAY:      launch_icp_replay( cx.L, E.RB, g_stream ); break;
  case ICP_EST_LANE_CHAINS: launch_icp_lane_chains( cx.L, E.CB, g_stream ); break;
  case ICP_EST_MOMENTS:     launch_icp_moments( cx.L, g_stream ); break;
  case ICP_EST_GRID_CHAINS:
  case ICP_EST_RECORDS:
    if( i < E.n_plain )
    {
      IcpLaunch Lp = cx.L; Lp.exact_centroids = 0;
      if( Lp.rec ) launch_icp_plain_from_records( Lp, E.CB, g_stream );
      else
      {
        // (its search ran without records, icp_align_impl: the moments from the matches, one partial per workgroup)
        Lp.n_mom_blocks = plain_moment_blocks( Lp.max_tiles );
        launch_icp_plain_from_matches( Lp, E.CB, g_stream );
      }
      return RS_HIP_ICP_STEP_PLAIN;
    }
    if( E.est == ICP_EST_RECORDS ) { launch_icp_exact_centroids_from_records( cx.L, E.RB, E.CB, g_stream ); break; }
    // the binade guesses of the chains' records: made from the sums of the iteration before (k_chain_walk_and_moments) — in the first
    // chain iteration from its own, so the records and the walks wait for the moments there (RS_HIP_CHAIN_REFRESH=k: in every k-th as well)
    E.CB.refresh = ( i == E.n_plain || ( chain_refresh > 0 && ( i % chain_refresh ) == 0 ) ) ? 1 : 0;
    launch_icp_chain_centroids( cx.L, E.CB, g_stream );
    break;
  }
  return E.est;
}

// (diagnostics after the loop of a one-source call) RS_HIP_DEBUG_TOTALS: the seven centroid sums of the last iteration, as the estimator
// used them (bits); RS_HIP_CHAIN_DEBUG: which segments the last iteration's chain walks added up addend by addend, and why their record
// did not fit, then — unless the chains gave the call up — the walks' self-check.
void icp_debug_report( const IcpEst& E, int n, int centroid_mode, bool gave_up )
{
  if( icp_exact_centroids( E.est ) && sw_flag( SW_DEBUG_TOTALS ) )
  {
    std::vector<double> t( (size_t)n * 3 * ICP_NMOM );
    (void)hipMemcpy( t.data(), E.RB.totals, t.size() * 8, hipMemcpyDeviceToHost );
    for( int p = 0; p < n; ++p )
    {
      fprintf( stderr, "[rs_hip totals] mode %d problem %d:", centroid_mode, p );
      for( int r = 0; r < CH_ROWS; ++r ) { const float f = (float)t[( (size_t)p * 3 + 1 ) * ICP_NMOM + r]; uint32_t u; std::memcpy( &u, &f, 4 ); fprintf( stderr, " %08x", u ); }
      fprintf( stderr, "\n" );
    }
  }
  if( E.CB.dbg )
  {
    std::vector<int> d( (size_t)CH_ROWS * ( 4 + 64 * 8 ) );
    (void)hipMemcpy( d.data(), E.CB.dbg, d.size() * 4, hipMemcpyDeviceToHost );
    for( int r = 0; r < CH_ROWS; ++r )
    {
      const int* q = d.data() + (size_t)r * ( 4 + 64 * 8 );
      fprintf( stderr, "[rs_hip chains] chain %d: %d segments added one by one (%d with their addends fetched ahead), %d steps by one record, %d wave-wide scans%s; fetches done after %.2f us, walk after %.2f us\n", r, q[0] & 0xffff, q[2] & 0xffff, q[2] >> 16, ( q[0] >> 16 ) & 0x3fff,
               ( q[0] >> 30 ) ? " (STUCK)" : "", q[1] / 100.0, q[3] / 100.0 );
      fprintf( stderr, "   cut + block 0 after %.2f us, block forecasts after %.2f us, segment records + forecasts after %.2f us; %d shader cycles in the walk itself\n", q[4 + 63 * 8] / 100.0, q[4 + 63 * 8 + 1] / 100.0, q[4 + 63 * 8 + 2] / 100.0, q[4 + 63 * 8 + 3] );
      if( q[4 + 63 * 8 + 4] )
        fprintf( stderr, "   step %d taken by its record DIFFERS from the same step by scans: record es %x lo %d hi %d D %d tp %x | start %08x -> by scans %08x, by record %08x | kind type %d chunk %d block %d from %d to %d\n",
                 q[4 + 63 * 8 + 4] - 1, q[4 + 63 * 8 + 5], q[4 + 63 * 8 + 6], q[4 + 63 * 8 + 7], q[4 + 62 * 8], q[4 + 62 * 8 + 1], (unsigned)q[4 + 62 * 8 + 2], (unsigned)q[4 + 62 * 8 + 3], (unsigned)q[4 + 62 * 8 + 4],
                 q[4 + 62 * 8 + 5] & 3, ( q[4 + 62 * 8 + 5] >> 2 ) & 7, ( q[4 + 62 * 8 + 5] >> 5 ) & 63, ( q[4 + 62 * 8 + 5] >> 11 ) & 63, ( q[4 + 62 * 8 + 5] >> 17 ) & 127 );
      for( int k = 0; k < std::min( q[0] & 0xffff, 62 ); ++k )
      {
        const int* e = q + 4 + 8 * k; const unsigned sb = (unsigned)e[1];
        fprintf( stderr, "   segment %6d (at %6.2f us): value exp %3u mantissa %8u sign %u | %d cycles for the 64 adds | %s, %s\n", e[0], e[7] / 100.0, ( sb >> 23 ) & 255u,
                 ( sb & 0x7fffffu ) | 0x800000u, sb >> 31, e[3],
                 ( e[2] & 2 ) ? "block forecast" : "block NOT forecast", ( e[2] & 1 ) ? "addends ahead" : "addends fetched now" );
      }
    }
  }
  if( E.CB.chk && !gave_up )
  {
    std::vector<int> c( (size_t)CH_ROWS * ( 4 + 3 * 4096 ) );
    (void)hipMemcpy( c.data(), E.CB.chk, c.size() * 4, hipMemcpyDeviceToHost );
    for( int r = 0; r < CH_ROWS; ++r )
    {
      const int* q = c.data() + (size_t)r * ( 4 + 3 * 4096 );
      if( q[1] < 0 ) { fprintf( stderr, "[rs_hip chains] chain %d self-check: %d steps, all as the plain sum (%08x); %d segments end in another binade than they start in\n", r, q[0], (unsigned)q[3], q[2] ); continue; }
      const int k = q[1];
      auto show = [&]( int j ) { const int* e = q + 4 + 3 * j; const int kind = e[2]; fprintf( stderr, "      step %d: ends at segment %d with %08x; type %d chunk %d block %d from %d to %d slot %d, %s\n", j, e[0], (unsigned)e[1], kind & 3, ( kind >> 2 ) & 7, ( kind >> 5 ) & 63, ( kind >> 11 ) & 63, ( kind >> 17 ) & 127, ( kind >> 24 ) & 63, ( kind >> 30 ) & 1 ? "by its record" : "by scans / addend by addend" ); };
      fprintf( stderr, "[rs_hip chains] chain %d self-check: step %d of %d differs from the plain sum (%08x there)\n", r, k, q[0], (unsigned)q[2] );
      if( k > 0 ) show( k - 1 );
      show( k );
    }
  }
}

enum { ICP_CHAINS_GAVE_UP = -1000 };      // (internal) a centroid chain's walk gave the problem up: again, the seven sums by pass 2 of the replay

enum { ICP_STOP_EDGE = -1001 };           // (internal) a stop test of some problem came within the guard of its threshold: *edge lists them

// the problems whose stop test was decided inside the guard, with their start poses (16 floats each, in the order of p)
struct StopEdges { std::vector<int> p; std::vector<float> T_in; };

// One ICP call for n problems: one source for all (src), or one per problem (srcs[n], src == null: a multi-source
// batch — the reference-order and lane-chain estimators only, see rs_hip_icp_align_multi).  Writes T1s, errs and iters, except when a
// grid chain gave a problem up (ICP_CHAINS_GAVE_UP: nothing written yet).  With the stop test and the guard armed (icp_choose), the
// problems decided inside the guard go to *edge and ICP_STOP_EDGE comes back; their results are written all the same.
int icp_align_impl( const rs_hip_cloud_t* src, const rs_hip_cloud_t* const* srcs, const rs_hip_cloud_t* target,
                    float* T1s, int32_t n, const float* T2, float max_dist, float max_angle,
                    int32_t max_iter, int32_t fixed_iters, float* errs, int32_t* iters, int centroid_mode,
                    bool force_bits /* the reference's own order (sequential / parallel) whatever the thresholds say */, StopEdges* edge )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( !T1s || !T2 || !errs ) { set_err( "icp_align: null argument" ); return RS_HIP_E_ARG; }
  IcpCtx cx;
  if( ( rc = icp_prepare( cx, src, target, n, T2, srcs ) ) ) return rc;
  tr_clear( n );
  const float tmin = icp_gate_threshold( max_angle );
  if( src && src->n == 0 ) { for( int p = 0; p < n; ++p ) { errs[p] = 1e6f; if( iters ) iters[p] = 1; } return RS_HIP_OK; }   // n_corrs == 0 on the first search
  if( ( rc = icp_enable_certificates( cx ) ) ) return rc;
  if( ( rc = icp_upload_state( cx, T1s, (size_t)n ) ) ) return rc;
  const IcpChoice choice = icp_choose( cx.L.max_n, n, centroid_mode, force_bits );
  // (the other estimators' kernels are built for one source per launch)
  if( srcs && choice.est != ICP_EST_REF_ORDER && choice.est != ICP_EST_LANE_CHAINS ) { set_err( "icp_align_multi: the estimator thresholds changed during the call" ); return RS_HIP_E_ARG; }
  IcpEst E{ choice.est };
  if( ( rc = icp_estimator_prepare( cx, E ) ) ) return rc;
  // (see icp_plain_iterations.  Scan-sized sources only: the eight 50 k-point refines of bench.py --scaling strong end 2.2e-6 from the reference with the
  //  chains throughout, 8.7e-6 with three plain iterations, 2.0e-5 with seven or eight — an object refine contracts more slowly than a scan-to-scan fit)
  if( E.est == ICP_EST_GRID_CHAINS || E.est == ICP_EST_RECORDS ) E.n_plain = icp_plain_iterations( cx.L.max_n, max_iter, fixed_iters != 0 );
  cx.L.stop_guard = ( choice.guard && !fixed_iters && edge ) ? sw_float( SW_STOP_GUARD ) : 0.0f;
  const size_t heavy_words = cx.heavy_words;
  const bool reorder = !sw_flag( SW_NO_LPT ), warm = !sw_flag( SW_NO_WARM );
  if( !warm ) cx.L.bounded_only = 0;      // (no launch of this call takes the warm form: rs_device.h)
  if( reorder )
  {
    if( ( rc = g_ws.order_a.ensure( heavy_words * 4 ) ) || ( rc = g_ws.order_b.ensure( heavy_words * 4 ) ) ) return rc;
    if( int rcf = icp_fill( g_ws.order_a.p, 0, heavy_words * 4 ) ) return rcf;
    if( int rcf = icp_fill( g_ws.order_b.p, 0, heavy_words * 4 ) ) return rcf;
  }

  // The whole iteration runs on the device (search, statistics, moments, solve, pose update, stop
  // tests), so iterations are enqueued back to back and the host looks at the state only once per
  // chunk; problems that stopped inside a chunk turn the rest of its launches into no-ops
  // (every kernel returns at once for an inactive problem).
  const bool debug_cycles = sw_flag( SW_DEBUG_CYCLES ), debug = !srcs && ( sw_flag( SW_DEBUG ) || debug_cycles );
  const int chunk_env = sw_int( SW_ICP_CHUNK );
  const size_t np = (size_t)n, state_bytes = np * ICP_STATE_WORDS * 4;
  float* hS = g_ws.h_b.as<float>();
  const int* hActive = (const int*)( hS + np * ICP_ST_ACTIVE );
  const long long total_tiles = (long long)cx.total_tiles;
  const long long coop_all_below = sw_i64( SW_COOP_ALL_BELOW );
  const int coop_waves_forced = sw_int( SW_COOP_WAVES );
  cx.L.solve = 1; cx.L.fixed_iters = fixed_iters ? 1 : 0;
  // (per ITERATION, not per chunk or call: a traced call runs one iteration per chunk, and the RECORDS estimator's own iterations follow plain ones)
  float4* const rec_all = cx.L.rec;
  const bool plain_matches = !sw_int( SW_PLAIN_RECORDS ) && ( E.est == ICP_EST_GRID_CHAINS || E.est == ICP_EST_RECORDS );
  if( ( rc = icp_fills_flush() ) ) return rc;      // everything the call's first kernels expect zeroed, in one launch
  ProfChain prof;
  int kind = RS_HIP_ICP_STEP_NONE;                  // (rs_hip_icp_trace_begin: the estimator of the iteration just enqueued)
  std::vector<char> was_active( g_tr.kinds ? np : 0, 1 );
  for( int i = 0; i < max_iter; )                                       // icp.h:444
  {
    // (the stop test looks at i > 5, icp.h:489: the first seven iterations go out in one piece, then chunk_env at a time — an iteration enqueued
    //  behind the one that stopped is six empty launches, a look at the state a copy and a synchronisation)
    const int chunk = ( debug || g_icp_trace || g_tr.kinds ) ? 1 : ( fixed_iters ? max_iter - i : std::min( i == 0 ? std::max( 7, chunk_env ) : std::max( 1, chunk_env ), max_iter - i ) );
    for( int c = 0; c < chunk; ++c, ++i )
    {
      icp_set_radius( cx, max_dist, tmin );
      cx.L.iter_index = i;
      cx.L.warm = ( i > 0 && warm ) ? 1 : 0;   // every active problem wrote m_slot in iteration i-1
      // launches of a few thousand tiles go straight to the cooperative kernel (launch_icp_corr); it is bound by its
      // heaviest tile while the list is short (8 waves per tile), by throughput beyond (4)
      cx.L.coop_all = total_tiles <= coop_all_below ? 1 : 0;
      cx.L.coop_waves = icp_coop_waves( cx.L, total_tiles, n, i );
      if( coop_waves_forced ) cx.L.coop_waves = coop_waves_forced;
      if( reorder )
      {
        cx.L.heavy_in = i == 0 ? nullptr : ( ( i & 1 ) ? g_ws.order_a.as<int>() : g_ws.order_b.as<int>() );
        cx.L.heavy_out = ( i & 1 ) ? g_ws.order_b.as<int>() : g_ws.order_a.as<int>();
      }
      cx.L.rec = ( plain_matches && i < E.n_plain ) ? nullptr : rec_all;      // a plain iteration's search leaves slot, dist² and dot only
      if( debug ) icp_debug_before( cx, n, debug_cycles );
      prof.mark( "nn_icp" ); launch_icp_corr( cx.L, g_stream );
      if( debug ) icp_debug_after( cx, cx.L.max_n, n, i, max_dist );
      prof.mark( "icp_moments" ); kind = icp_step( cx, E, i );
      double nd = max_dist * 0.95;                                      // icp.h:493
      max_dist = (float)( nd > 0.05 ? nd : 0.05 );
    }
    prof.mark( nullptr );
    HIP_TRY( hipMemcpyAsync( hS, g_ws.state.p, state_bytes, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
    HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
    if( g_icp_trace && n == 1 && i >= 1 && i - 1 < g_icp_trace_cap ) g_icp_trace[i - 1] = hS[np * ICP_ST_ERR];      // the error after iteration i - 1
    if( g_tr.kinds ) tr_record( n, i - 1, kind, hS, was_active );
    int n_active = 0;
    for( int p = 0; p < n; ++p ) n_active += hActive[p] ? 1 : 0;
    if( n_active == 0 ) break;
  }
  if( E.est == ICP_EST_LANE_CHAINS ) icp_lane_account( E.CB, n );
  bool gave_up = false;
  if( E.est == ICP_EST_GRID_CHAINS )
  {
    const int* hFailed = (const int*)( hS + np * ICP_ST_FAILED );      // (part of the state block the loop's last look copied)
    for( int p = 0; p < n; ++p ) gave_up = gave_up || hFailed[p] != 0;
  }
  if( !srcs ) icp_debug_report( E, n, centroid_mode, gave_up );
  if( gave_up ) { g_chains_gave_up.fetch_add( 1 ); return ICP_CHAINS_GAVE_UP; }      // (nothing written to the caller's arrays yet)
  const int* hIters = (const int*)( hS + np * ICP_ST_ITERS );
  const int* hEdge = (const int*)( hS + np * ICP_ST_TICKET );
  const bool guarded = edge && cx.L.stop_guard > 0.0f;
  for( int p = 0; p < n; ++p )
  {
    if( guarded && hEdge[p] ) { edge->p.push_back( p ); edge->T_in.insert( edge->T_in.end(), T1s + 16 * p, T1s + 16 * p + 16 ); }   // (its start pose, still there)
    std::memcpy( T1s + 16 * p, hS + np * ICP_ST_T1 + 16 * p, 64 ); errs[p] = hS[np * ICP_ST_ERR + p]; if( iters ) iters[p] = hIters[p];
  }
  return guarded && !edge->p.empty() ? ICP_STOP_EDGE : RS_HIP_OK;
}

// The stop guard's re-runs: every problem of `edge` again, alone, from its start pose and the caller's max_dist (the loop shrinks its own,
// icp.h:493), in the reference's own order — its decisions, its bits.  Problem q's source: srcs ? srcs[q] : src.
int icp_stop_guard_rerun( const StopEdges& edge, const rs_hip_cloud_t* src, const rs_hip_cloud_t* const* srcs, const rs_hip_cloud_t* target,
                          float* T1s, const float* T2, float max_dist, float max_angle, int32_t max_iter, int32_t fixed_iters,
                          float* errs, int32_t* iters, int centroid_mode )
{
  for( size_t k = 0; k < edge.p.size(); ++k )
  {
    const int q = edge.p[k];
    float* T = T1s + 16 * (size_t)q;
    std::memcpy( T, edge.T_in.data() + 16 * k, 64 );
    { TrShift ts( q ); if( int rc = icp_align_impl( srcs ? srcs[q] : src, nullptr, target, T, 1, T2, max_dist, max_angle, max_iter, fixed_iters, errs + q, iters ? iters + q : nullptr, centroid_mode, true, nullptr ) ) return rc; }
    tr_mark_redone( q );
    g_stop_guard_redone.fetch_add( 1 );
  }
  return RS_HIP_OK;
}
} // namespace

extern "C" {

int rs_hip_icp_align_batch( const rs_hip_cloud_t* source, const rs_hip_cloud_t* target,
                            float* T1s, int32_t n, const float* T2, float max_dist, float max_angle,
                            int32_t max_iter, int32_t fixed_iters, float* errs, int32_t* iters )
{
  // Scan-sized sources: the reference's centroid sums by the grid chains — which give a problem up when a sum keeps changing
  // binade (coordinates that straddle the origin in a cancelling order: rs_icp_chain.hip, chain_walk_row); the batch is then run
  // again with those sums by pass 2 of the replay: the same bits, 0.9 ms per iteration at a million points instead of 0.09.
  // The estimators of large sources keep per-point records per problem (48 B with the chains, 44 B + the replay's rows when they
  // give up): many start poses of a whole scan are run in slices of problems whose records stay below RS_HIP_ICP_BATCH_BYTES
  // (default 4 GB) — the problems are independent, so the results are those of the one batch.
  // (the arguments first: nothing below may read through them before they are known to be there)
  if( !source || !target || !T1s || !T2 || !errs || n < 0 ) { set_err( "icp_align_batch: bad arguments" ); return RS_HIP_E_ARG; }
  const double cap = sw_double( SW_ICP_BATCH_BYTES );
  const bool per_point_records = source && source->n > sw_int( SW_REF_ORDER_BELOW );
  // (96 B per point: the 48-byte records + what a slice that falls back to the replay adds — its segment rows, ~35 / 128 x ( 8 + 24 + sizeof( ReplaySeg ) ) ≈ 48 B per point)
  const int slice = per_point_records ? std::max( 1, (int)std::min<double>( (double)std::max( n, 1 ), cap / ( 96.0 * (double)std::max( source->n, 1 ) ) ) ) : std::max( n, 1 );
  for( int p0 = 0; p0 < std::max( n, 1 ); p0 += slice )
  {
    const int np = std::min( slice, n - p0 );
    float* T = T1s ? T1s + 16 * (size_t)p0 : nullptr; float* e = errs ? errs + p0 : nullptr; int32_t* it = iters ? iters + p0 : nullptr;
    // (a source whose chains gave up lately: the attempt — a cold search, the iterations up to the give-up, the launches that idle
    //  through the rest of the call: ~1.4 ms at a million points — is skipped; every 16th such call tries the chains again)
    int mode = sw_int( SW_EXACT_CENTROIDS );
    if( mode == 1 && per_point_records && sw_int( SW_CHAINS_RETRY_AFTER ) > 0 && source->chains_wander.load() > 0 ) { source->chains_wander.fetch_sub( 1 ); mode = 2; }
    StopEdges edge;
    TrShift ts( p0 );
    int rc = icp_align_impl( source, nullptr, target, T, np, T2, max_dist, max_angle, max_iter, fixed_iters, e, it, mode, false, &edge );
    // (a problem of the slice whose chains gave up: that slice again, its seven sums by pass 2 of the replay — nothing of it was written yet)
    if( rc == ICP_CHAINS_GAVE_UP )
    {
      source->chains_wander.store( sw_int( SW_CHAINS_RETRY_AFTER ) );
      rc = icp_align_impl( source, nullptr, target, T, np, T2, max_dist, max_angle, max_iter, fixed_iters, e, it, 2, false, &edge );
    }
    if( rc == ICP_STOP_EDGE ) rc = icp_stop_guard_rerun( edge, source, nullptr, target, T, T2, max_dist, max_angle, max_iter, fixed_iters, e, it, mode );
    if( rc ) return rc;
  }
  return RS_HIP_OK;
}

// The per-placement refine loop as one call (lib/rs/rs_database.h:220-230, apps/pose_proposal/main.cpp:190-202 with a different
// object per proposal): problem p aligns sources[p] to the target from T1s[p].  Sources within the reference-order estimator's
// range (rs_hip_icp_reference_order_below: every call site of the reference) run as ONE batch — grid.y = problem, the kernels bind
// their problem's source view on the device (rs_icp.h: icp_bind), so the sequential chains of all problems run side by side;
// every problem's result is what rs_hip_icp_align returns for it alone, bit for bit.  A batch with a larger source is run
// problem by problem (their estimators are built for one source per launch).
int rs_hip_icp_align_multi( const rs_hip_cloud_t* const* sources, const rs_hip_cloud_t* target,
                            float* T1s, int32_t n, const float* T2, float max_dist, float max_angle,
                            int32_t max_iter, int32_t fixed_iters, float* errs, int32_t* iters )
{
  if( !sources || !target || !T1s || !T2 || !errs || n < 0 ) { set_err( "icp_align_multi: bad arguments" ); return RS_HIP_E_ARG; }
  int rc = ensure_ready(); if( rc ) return rc;
  if( n == 0 ) return RS_HIP_OK;
  // Every problem gets the estimator its own rs_hip_icp_align would (icp_choose), so that its result is that call's bit for bit: the
  // problems within the reference-order range run as one batch (k_icp_faithful), those within the lane chains' range as another
  // (launch_icp_lane_chains), the rest — estimators built for one source per launch — one by one.
  const int mode = sw_int( SW_EXACT_CENTROIDS );
  std::vector<int> group[3];
  for( int p = 0; p < n; ++p )
  {
    if( !sources[p] ) { set_err( "icp_align_multi: null source" ); return RS_HIP_E_ARG; }
    const IcpEstimator est = icp_choose( sources[p]->n, n, mode, false ).est;
    group[sources[p]->n <= 0 ? 2 : est == ICP_EST_REF_ORDER ? 0 : est == ICP_EST_LANE_CHAINS ? 1 : 2].push_back( p );
  }
  // m >= 2 problems of one group in the same launches, then the stop guard's re-runs
  auto run_group = [&]( const rs_hip_cloud_t* const* src, float* T, int m, float* e, int32_t* it )
  {
    StopEdges edge;
    const int r = icp_align_impl( nullptr, src, target, T, m, T2, max_dist, max_angle, max_iter, fixed_iters, e, it, mode, false, &edge );
    return r == ICP_STOP_EDGE ? icp_stop_guard_rerun( edge, nullptr, src, target, T, T2, max_dist, max_angle, max_iter, fixed_iters, e, it, mode ) : r;
  };
  for( int p : group[2] )
  {
    TrShift ts( p );
    if( ( rc = rs_hip_icp_align_batch( sources[p], target, T1s + 16 * p, 1, T2, max_dist, max_angle, max_iter, fixed_iters, errs + p, iters ? iters + p : nullptr ) ) ) return rc;
  }
  for( int cls = 0; cls < 2; ++cls )
  {
    const std::vector<int>& g = group[cls];
    if( g.empty() ) continue;
    if( g.size() == 1 )
    {
      const int p = g[0];
      TrShift ts( p );
      if( ( rc = rs_hip_icp_align_batch( sources[p], target, T1s + 16 * p, 1, T2, max_dist, max_angle, max_iter, fixed_iters, errs + p, iters ? iters + p : nullptr ) ) ) return rc;
      continue;
    }
    if( (int)g.size() == n )      // (the common case: one group, in place)
      return run_group( sources, T1s, n, errs, iters );
    std::vector<const rs_hip_cloud_t*> src( g.size() ); std::vector<float> T( 16 * g.size() ), e( g.size() ); std::vector<int32_t> it( g.size() );
    for( size_t k = 0; k < g.size(); ++k ) { src[k] = sources[g[k]]; std::memcpy( T.data() + 16 * k, T1s + 16 * g[k], 64 ); }
    { TrMap tm( g.data() ); if( ( rc = run_group( src.data(), T.data(), (int)g.size(), e.data(), it.data() ) ) ) return rc; }
    for( size_t k = 0; k < g.size(); ++k ) { std::memcpy( T1s + 16 * g[k], T.data() + 16 * k, 64 ); errs[g[k]] = e[k]; if( iters ) iters[g[k]] = it[k]; }
  }
  return RS_HIP_OK;
}

// (diagnostics) problems run again in the reference's order because a stop test of theirs was decided inside the guard, since rs_hip_init
int64_t rs_hip_icp_stop_guard_redone( void ) { return g_stop_guard_redone.load(); }
// The setters of the switches that have one (rs_switches.h: sw_set — a negative argument only reads; the previous value comes back).
int32_t rs_hip_icp_early_plain( int32_t on )              { return sw_set( SW_EARLY_PLAIN, on ); }
int32_t rs_hip_icp_plain_from_records( int32_t on )       { return sw_set( SW_PLAIN_RECORDS, on ); }
int32_t rs_hip_icp_update_fenced( int32_t on )            { return sw_set( SW_UPDATE_FENCED, on ); }
float   rs_hip_icp_stop_guard( float guard )              { return sw_set( SW_STOP_GUARD, guard ); }
int32_t rs_hip_icp_lane_chains_below( int32_t n_points )  { return sw_set( SW_LANE_CHAINS_BELOW, n_points ); }
int32_t rs_hip_icp_chains_retry_after( int32_t calls )    { return sw_set( SW_CHAINS_RETRY_AFTER, calls ); }
int32_t rs_hip_icp_reference_order_below( int32_t n_points ) { return sw_set( SW_REF_ORDER_BELOW, n_points ); }
int32_t rs_hip_icp_replay_below( int32_t n_points )       { return sw_set( SW_REPLAY_BELOW, n_points ); }
int32_t rs_hip_icp_exact_centroids( int32_t on )          { return sw_set( SW_EXACT_CENTROIDS, on ); }
int32_t rs_hip_icp_faith_guess( int32_t permille )        { return sw_set( SW_FAITH_GUESS, permille ); }
void rs_hip_icp_state_layout( int32_t* words_per_problem, int32_t* launch_max_words )
{
  if( words_per_problem ) *words_per_problem = ICP_STATE_WORDS;
  if( launch_max_words ) *launch_max_words = rs::FillRanges::STATE_MAX;
}
// (diagnostics) of all addends the lane chains have summed since rs_hip_init, how many were added one by one in fp32 (per mille)
int64_t rs_hip_icp_lane_chains_sequential( void ) { return g_lane_seq_addends.load(); }

int32_t rs_hip_icp_chains_gave_up( void ) { return g_chains_gave_up.load(); }

int32_t rs_hip_icp_faith_redone( void )
{
  int v = 0;
#ifdef RS_FAITH_TIMING
  { int t[16]; (void)hipStreamSynchronize( g_stream ); if( g_faith_redone.p && hipMemcpy( t, g_faith_redone.p, sizeof t, hipMemcpyDeviceToHost ) == hipSuccess )
    for( int w = 0; w < 4; ++w ) fprintf( stderr, "[rs_hip faith timing] pass %d wave %d: %d cycles at work, %d at the barrier, %d chunks\n", RS_FAITH_TIMING, w, t[2 + 3 * w], t[3 + 3 * w], t[4 + 3 * w] ); }
#endif
  if( g_faith_redone.p && ( hipStreamSynchronize( g_stream ) != hipSuccess || hipMemcpy( &v, g_faith_redone.p, 4, hipMemcpyDeviceToHost ) != hipSuccess ) ) return -1;
  return v;
}

int32_t rs_hip_icp_replay_redone( void )
{
  int v = 0;
  if( g_ws.rp_redone.p && hipMemcpy( &v, g_ws.rp_redone.p, 4, hipMemcpyDeviceToHost ) != hipSuccess ) return -1;
  return v;
}

int rs_hip_icp_align_traced( const rs_hip_cloud_t* source, const rs_hip_cloud_t* target,
                             float* T1, const float* T2, float max_dist, float max_angle,
                             int32_t max_iter, int32_t fixed_iters, float* err, int32_t* n_iters, float* errs_per_iter )
{
  g_icp_trace = errs_per_iter; g_icp_trace_cap = errs_per_iter ? std::max( 0, max_iter ) : 0;
  const int rc = rs_hip_icp_align( source, target, T1, T2, max_dist, max_angle, max_iter, fixed_iters, err, n_iters );
  g_icp_trace = nullptr; g_icp_trace_cap = 0;
  return rc;
}

int rs_hip_icp_trace_begin( float* poses, float* errs, int32_t* kinds, int32_t* redone, int32_t max_iter, int32_t n_problems )
{
  if( !poses || !errs || !kinds || !redone || max_iter < 1 || n_problems < 1 ) { set_err( "icp_trace_begin: bad arguments" ); return RS_HIP_E_ARG; }
  g_tr.poses = poses; g_tr.errs = errs; g_tr.kinds = kinds; g_tr.redone = redone; g_tr.max_iter = max_iter; g_tr.n_prob = n_problems;
  for( int g = 0; g < n_problems; ++g ) { tr_clear_row( g ); redone[g] = 0; }
  return RS_HIP_OK;
}

int rs_hip_icp_trace_end( void )
{
  g_tr = IcpStepTrace{};
  return RS_HIP_OK;
}

int rs_hip_icp_align( const rs_hip_cloud_t* source, const rs_hip_cloud_t* target,
                      float* T1, const float* T2, float max_dist, float max_angle,
                      int32_t max_iter, int32_t fixed_iters, float* err, int32_t* n_iters )
{
  float e = 1e6f; int32_t it = 0;
  int rc = rs_hip_icp_align_batch( source, target, T1, 1, T2, max_dist, max_angle, max_iter, fixed_iters, &e, &it );
  if( err ) *err = e;
  if( n_iters ) *n_iters = it;
  return rc;
}

int rs_hip_icp_find_corrs( const rs_hip_cloud_t* source, const rs_hip_cloud_t* target,
                           const float* T1, const float* T2, float max_dist, float max_angle,
                           float* corr_pts1, float* corr_nor1, float* corr_pts2, float* corr_nor2,
                           float* weights, int32_t* n_corrs )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( !T1 || !T2 || !n_corrs ) { set_err( "icp_find_corrs: null argument" ); return RS_HIP_E_ARG; }
  IcpCtx cx;
  if( ( rc = icp_prepare( cx, source, target, 1, T2 ) ) ) return rc;
  *n_corrs = 0;
  const int nq = source->n;
  if( nq == 0 ) return RS_HIP_OK;
  std::vector<Mat4> T( 1 ); std::memcpy( T[0].m, T1, 64 );
  if( ( rc = icp_upload_state( cx, T1, 1 ) ) ) return rc;
  icp_set_radius( cx, max_dist, icp_gate_threshold( max_angle ) );
  if( ( rc = icp_fills_flush() ) ) return rc;
  { ProfScope ps( "nn_icp" ); launch_icp_corr( cx.L, g_stream ); }
  std::vector<int> slot( nq ); std::vector<float> d2( nq ), dot( nq );
  HIP_TRY( hipMemcpyAsync( slot.data(), cx.L.m_slot, (size_t)nq * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( d2.data(), cx.L.m_d2, (size_t)nq * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( dot.data(), cx.L.m_dot, (size_t)nq * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );

  // Back to source order and compact (icp.h:381-391).  The query positions/normals are
  // re-derived on the host with the same two mat·vec products the kernel used.
  std::vector<int> by_orig( nq );
  for( int s = 0; s < nq; ++s ) by_orig[source->qorder[s]] = s;
  Mat4 t2; std::memcpy( t2.m, T2, 64 ); Mat4 t2i = mat4_inverse( t2 );
  auto apply = []( const Mat4& M, const float* v, float w, float* o ) {
    o[0] = M.m[0] * v[0] + M.m[4] * v[1] + M.m[ 8] * v[2] + w * M.m[12];
    o[1] = M.m[1] * v[0] + M.m[5] * v[1] + M.m[ 9] * v[2] + w * M.m[13];
    o[2] = M.m[2] * v[0] + M.m[6] * v[1] + M.m[10] * v[2] + w * M.m[14]; };
  std::vector<float> dists; dists.reserve( nq );
  int ic = 0;
  for( int i = 0; i < nq; ++i )
  {
    const int s = by_orig[i];
    if( slot[s] < 0 ) continue;
    const int i2 = target->order[slot[s]];
    float t[3], qp[3], qn[3];
    apply( T[0], &source->h_pos[3*i], 1.0f, t ); apply( t2i, t, 1.0f, qp );
    apply( T[0], &source->h_nor[3*i], 0.0f, t ); apply( t2i, t, 0.0f, qn );
    if( corr_pts1 ) std::memcpy( corr_pts1 + 3*ic, qp, 12 );
    if( corr_nor1 ) std::memcpy( corr_nor1 + 3*ic, qn, 12 );
    if( corr_pts2 ) std::memcpy( corr_pts2 + 3*ic, &target->h_pos[3*i2], 12 );
    if( corr_nor2 ) std::memcpy( corr_nor2 + 3*ic, &target->h_nor[3*i2], 12 );
    if( weights ) weights[ic] = ( 1.0f - d2[s] / max_dist ) * dot[s];       // icp.h:387
    dists.push_back( d2[s] );
    ic++;
  }
  // icp.h:393-402 with msh_compute_mean / msh_compute_stddev in source order (msh_std.h:1800-1825)
  if( weights && ic > 0 )
  {
    float acc = 0; for( int i = 0; i < ic; ++i ) acc += dists[i];
    float mean = acc / (float)ic;
    float sq = 0.0f; for( int i = 0; i < ic; ++i ) sq += dists[i] * dists[i];
    float sd = (float)std::sqrt( sq / (float)ic - mean * mean );
    if( sd > 0.000001 ) for( int i = 0; i < ic; ++i ) if( dists[i] > 2.5f * sd ) weights[i] = 0.0;
  }
  *n_corrs = ic;
  return RS_HIP_OK;
}

int rs_hip_icp_estimate_pt2pl( const float* pts1, const float* pts2, const float* nor2,
                               const float* weights, int32_t n, float* T1, float* err )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( !pts1 || !pts2 || !nor2 || !weights || !T1 || n <= 0 ) { set_err( "icp_estimate: bad arguments" ); return RS_HIP_E_ARG; }
  g_fills.n = 0; g_fills.state_words = 0;      // (see icp_prepare)
  // Present the correspondences to k_icp_moments as "query i matched slot i" with explicit weights.
  const size_t nn = (size_t)n;
  if( ( rc = g_ws.tmp_pos.ensure( nn * 16 ) ) || ( rc = g_ws.tmp_pos2.ensure( nn * 16 ) ) || ( rc = g_ws.tmp_nor2.ensure( nn * 16 ) ) ||
      ( rc = g_ws.wexp.ensure( nn * 4 ) ) || ( rc = g_ws.slot.ensure( nn * 4 ) ) || ( rc = g_ws.d2.ensure( nn * 4 ) ) || ( rc = g_ws.dot.ensure( nn * 4 ) ) ||
      ( rc = g_ws.state.ensure( ICP_STATE_WORDS * 4 ) ) ||
      ( rc = g_ws.mom_part.ensure( 256 * ICP_NMOM * 8 ) ) || ( rc = g_ws.res.ensure( ICP_NRES * 8 ) ) || ( rc = g_ws.h_a.ensure( ICP_NRES * 8 ) ) )
    return rc;
  std::vector<float4> a( nn ), b( nn ), c( nn ); std::vector<int> sl( nn );
  for( size_t i = 0; i < nn; ++i )
  {
    a[i] = make_float4( pts1[3*i], pts1[3*i+1], pts1[3*i+2], 0 );
    b[i] = make_float4( pts2[3*i], pts2[3*i+1], pts2[3*i+2], 0 );
    c[i] = make_float4( nor2[3*i], nor2[3*i+1], nor2[3*i+2], 0 );
    sl[i] = (int)i;
  }
  Mat4 I = mat4_identity(); double zeros[ICP_NRES]; std::memset( zeros, 0, sizeof(zeros) );
  float st_host[ICP_STATE_WORDS]; std::memset( st_host, 0, sizeof( st_host ) );       // identity pose, active, tickets zero
  std::memcpy( st_host, I.m, 64 ); { int one = 1; std::memcpy( st_host + 16, &one, 4 ); }
  HIP_TRY( hipMemcpyAsync( g_ws.tmp_pos.p, a.data(), nn * 16, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( g_ws.tmp_pos2.p, b.data(), nn * 16, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( g_ws.tmp_nor2.p, c.data(), nn * 16, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( g_ws.wexp.p, weights, nn * 4, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( g_ws.slot.p, sl.data(), nn * 4, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( g_ws.state.p, st_host, sizeof( st_host ), hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( g_ws.res.p, zeros, ICP_NRES * 8, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );     // host staging vectors go out of scope below
  IcpLaunch L{};
  L.tgt.pos = g_ws.tmp_pos2.as<float4>(); L.tgt.nor = g_ws.tmp_nor2.as<float4>(); L.tgt.n = n;
  L.src.pos = g_ws.tmp_pos.as<float4>(); L.src.nor = nullptr; L.src.tiles = nullptr; L.src.n = n; L.src.n_tiles = 0; L.n_prob = 1;
  L.multi = nullptr; L.max_n = n; L.max_tiles = 0;
  L.T1 = g_ws.state.as<float>(); L.active = (int*)( g_ws.state.as<float>() + 16 ); std::memcpy( L.T2i.m, I.m, 64 );
  L.ticket = (int*)( g_ws.state.as<float>() + 37 ); L.solve = 0;       // reductions only: the solve below runs on the host
  L.radius = 1.0f; L.m_slot = g_ws.slot.as<int>(); L.m_d2 = g_ws.d2.as<float>(); L.m_dot = g_ws.dot.as<float>();
  L.mom_part = g_ws.mom_part.as<double>(); L.res = g_ws.res.as<double>();
  L.n_mom_blocks = std::max( 1, std::min( 256, ( n + 255 ) / 256 ) ); L.w_explicit = g_ws.wexp.as<float>();
  // (a single estimator step on the caller's own correspondences: wherever the ICP loop would centre on the reference's chains — the lane
  //  chains' range — this entry point simply runs the reference's order: one call, its cost does not matter, its bits do)
  const int seq_below = std::max( sw_int( SW_REF_ORDER_BELOW ), sw_int( SW_EXACT_CENTROIDS ) != 0 ? sw_int( SW_LANE_CHAINS_BELOW ) : 0 );
  if( n <= std::max( seq_below, sw_int( SW_REPLAY_BELOW ) ) )
  {
    // the reference's own accumulation order (k_icp_faithful, or its parallel form): solve and pose update on the device too
    if( ( rc = g_ws.faith.ensure( nn * FAITH_REC * 4 ) ) ) return rc;
    L.faith = g_ws.faith.as<float>(); L.by_orig = nullptr; L.err = g_ws.state.as<float>() + 34;
    // (the points are presented untransformed, so the state's pose stays the identity uploaded above and T1 is multiplied in afterwards)
    if( n <= seq_below || n > sw_int( SW_REPLAY_BELOW ) ) { ProfScope ps( "icp_moments" ); launch_icp_faithful( L, g_stream ); }
    else
    {
      ReplayBufs RB{};
      if( ( rc = replay_prepare( RB, 1, n ) ) || ( rc = icp_fills_flush() ) ) return rc;
      ProfScope ps( "icp_moments" ); launch_icp_replay( L, RB, g_stream );
    }
    float out[ICP_STATE_WORDS];
    HIP_TRY( hipMemcpyAsync( out, g_ws.state.p, sizeof( out ), hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
    HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
    Mat4 step, T; std::memcpy( step.m, out, 64 ); std::memcpy( T.m, T1, 64 );
    T = mat4_mul( step, T );                      // icp.h:295: *T1 = T * *T1 (step = T * I, exact)
    std::memcpy( T1, T.m, 64 );
    if( err ) *err = out[34];
    return RS_HIP_OK;
  }
  { ProfScope ps( "icp_moments" ); launch_icp_moments( L, g_stream ); }
  double* hM = g_ws.h_a.as<double>();
  HIP_TRY( hipMemcpyAsync( hM, g_ws.res.p, ICP_NMOM * 8, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  Mat4 T; std::memcpy( T.m, T1, 64 );
  float e = 0.0f;
  // the reference has no Σw guard inside the estimator itself; keep T1 when the system is empty
  if( icp_solve( hM, T, e ) ) std::memcpy( T1, T.m, 64 );
  if( err ) *err = e;
  return RS_HIP_OK;
}

} // extern "C"
