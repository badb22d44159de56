// librescan_hip host side: the part of the C ABI of include/rescan_hip.h that every other part stands on.
//
// Owns the runtime state (error text, device, the calling thread's stream), profiling (per-kernel HIP-event timing used by
// bench.py) and device clouds (cell-sorted 16-byte records + cell offset table, built on the device), and defines what rs_api.h
// declares for the other three host units: rs_icp_api.hip (the ICP host driver), rs_score.hip (alignment scores) and
// rs_rows_api.hip (labels, rows, neighbourhood graph, level builder, coverage).  There is no CPU fallback: every compute entry
// point fails with RS_HIP_E_NODEVICE when no HIP device is usable.

#include "../../include/rescan_hip.h"
#include "rs_api.h"
#include "rs_buildplan.h"
#include "rs_device.h"
#include "rs_host.h"
#include "rs_math.h"
#include "rs_switches.h"

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
// runtime state
// ------------------------------------------------------------------------------------------

namespace {

char g_err[512] = "";
int g_device = -1;
bool g_ready = false;
thread_local hipStream_t g_own_stream = nullptr;
// (profiling: the spans booked since the last read, by name, and the pool their events come from)
std::mutex g_prof_mutex;
struct ProfEntry { std::vector<std::pair<hipEvent_t, hipEvent_t>> spans; int64_t launches = 0; double ms = 0.0; };
std::map<std::string, ProfEntry> g_profmap;
std::vector<hipEvent_t> g_evpool;      // events are handed out in order and recycled by prof_collect
size_t g_evnext = 0;

struct BuildWorkspace
{
  DevBuf bld_pos, bld_nor, bld_k0, bld_k1, bld_v0, bld_v1, bld_v2, bld_small, bld_bits, bld_tmp;   // cloud construction
  DevBuf many_pos, many_nor, many_segid, many_k0, many_k1, many_v0, many_v1, many_v2, many_segs, many_trial, many_small, many_bits, many_tmp;   // ... of a batch
  PinBuf many_stage;     // the small clouds of a batch, packed for one upload per run of them
};
thread_local BuildWorkspace g_ws;

} // namespace

namespace rs {

thread_local hipStream_t g_stream = nullptr;

void set_err( const char* fmt, ... )
{
  va_list ap; va_start( ap, fmt ); vsnprintf( g_err, sizeof(g_err), fmt, ap ); va_end( ap );
}

int ensure_ready()
{
  if( !g_ready ) { int rc = rs_hip_init( g_device >= 0 ? g_device : 0 ); if( rc ) return rc; }
  if( !g_own_stream )       // first call from this host thread
  {
    HIP_TRY( hipSetDevice( g_device ), RS_HIP_E_NODEVICE );
    HIP_TRY( hipStreamCreateWithFlags( &g_own_stream, hipStreamNonBlocking ), RS_HIP_E_NODEVICE );
  }
  if( !g_stream ) g_stream = g_own_stream;
  return RS_HIP_OK;
}

// ---- profiling ---------------------------------------------------------------------------
bool g_prof = false;
unsigned long long* g_evals = nullptr;  // device counter of staged-and-evaluated candidates (all threads, all kernels) while profiling

// one event recorded on the calling thread's stream (null if profiling is off or events ran out)
hipEvent_t prof_event()
{
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> lock( g_prof_mutex );
    if( g_evnext == g_evpool.size() ) { hipEvent_t x; if( hipEventCreate( &x ) != hipSuccess ) return nullptr; g_evpool.push_back( x ); }
    ev = g_evpool[g_evnext++];
  }
  (void)hipEventRecord( ev, g_stream );
  return ev;
}
void prof_span( const char* name, hipEvent_t a, hipEvent_t b )
{
  if( !a || !b ) return;
  std::lock_guard<std::mutex> lock( g_prof_mutex );
  g_profmap[name].spans.emplace_back( a, b );
}

// Hand-off policy of the two-phase search.  A lone wave that is still unsettled after streaming
// this many candidates sits in a cluttered neighbourhood and would need ~0.5 ms for the rest of
// its box; it is queued for the cooperative kernel instead.  That only pays when the launch has
// too few tiles to hide such stragglers behind other work (measured on MI355X: 1 M-query ICP,
// 15.6 k tiles: 0.60 -> 0.47 ms per search with hand-off; 256-pose score batch, 40 k tiles:
// 1.5 -> 3.0 ms, i.e. worse), so big launches keep everything in phase A.
// Hand-off rule of a search launch (rs_search.h: tile_search): low 16 bits = candidates a lone wave may
// stream while a lane is unsettled, high bits = the shell after which an unsettled tile is handed off whatever it
// streamed.  A wave that runs almost alone on its SIMD (few tiles in flight) is latency-bound, so the fewer tiles a
// launch has, the earlier the cooperative kernel takes over; launches with > 24 k tiles (score batches) keep
// everything in phase A — there the stragglers hide behind other tiles and the hand-off measured slower.
int handoff_threshold( long long total_tiles )
{
  const int forced = sw_int( SW_SOLO_STAGES ), forced_k = sw_int( SW_HANDOFF_K );
  if( forced > 0 ) return forced | ( std::max( 0, forced_k ) << 16 );
  if( total_tiles > 24000 ) return 0x7fffffff;
  const int k_always = forced_k >= 0 ? forced_k : 1;
  return ( total_tiles <= 12000 ? 128 : 192 ) | ( k_always << 16 );
}

} // namespace rs

namespace {

void prof_collect()
{
  std::lock_guard<std::mutex> lock( g_prof_mutex );
  for( auto& kv : g_profmap )
  {
    ProfEntry& e = kv.second;
    for( auto& sp : e.spans )
    {
      float ms = 0.0f;
      (void)hipEventSynchronize( sp.second );
      if( hipEventElapsedTime( &ms, sp.first, sp.second ) == hipSuccess ) { e.ms += ms; e.launches++; }
    }
    e.spans.clear();
  }
  g_evnext = 0;
}

} // namespace

// ------------------------------------------------------------------------------------------
// clouds
// ------------------------------------------------------------------------------------------

// (struct rs_hip_cloud: rs_api.h)

namespace {

// ---- query layout ---------------------------------------------------------------------------
// (Hilbert order + greedy tiling are computed on the device: rs_build.hip.)

// (The tile extent limit, from the cloud's own sampling density: query_extent_limit, rs_buildplan.h.  Its cap, RS_HIP_TILE_EXTENT_MAX:
//  a sparse cloud (a subsampled level, a random subset) searched in a denser one would otherwise get tiles whose box is mostly the
//  empty space between its points — 1000 points against a 200 k scan: 404 -> 60 us per ICP iteration with the cap.)

} // namespace

extern "C" {

const char* rs_hip_version( void ) { return "rescan_hip 0.1 gfx950"; }
const char* rs_hip_last_error( void ) { return g_err; }

int rs_hip_init( int device )
{
  int count = 0;
  hipError_t e = hipGetDeviceCount( &count );
  if( e != hipSuccess || count <= 0 )
  {
    set_err( "rs_hip_init: no HIP device (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString( e ) );
    return RS_HIP_E_NODEVICE;
  }
  if( device < 0 || device >= count ) { set_err( "rs_hip_init: device %d out of range (%d devices)", device, count ); return RS_HIP_E_ARG; }
  HIP_TRY( hipSetDevice( device ), RS_HIP_E_NODEVICE );
  // RS_HIP_SCHEDULE=spin: completion waits of THIS device busy-wait instead of sleeping — for callers that wait for small results
  // thousands of times per second (librescan_dropin.so asks for it: the unchanged pose_proposal issues ~37 k searches per run; so
  // does bench.py).  Opt-in: a library does not change a process's scheduling policy by itself (8 ranks x 3 busy-waiting threads on
  // a host with a CPU quota would starve each other).  Refused (harmlessly) when the process has set the device up already.
  {
    const char* sch = sw_word( SW_SCHEDULE );
    if( sch && !std::strcmp( sch, "spin" ) ) (void)hipSetDeviceFlags( hipDeviceScheduleSpin );
    (void)hipGetLastError();
  }
  g_device = device;
  g_ready = true;
  return RS_HIP_OK;
}

int rs_hip_set_stream( void* s )
{
  int rc = ensure_ready(); if( rc ) return rc;
  g_stream = s ? (hipStream_t)s : g_own_stream;
  return RS_HIP_OK;
}

int rs_hip_stream_cu_mask( const uint32_t* mask, int32_t n_words )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( ( !mask ) != ( n_words <= 0 ) ) { set_err( "stream_cu_mask: bad arguments" ); return RS_HIP_E_ARG; }
  hipStream_t s = nullptr;
  if( mask ) HIP_TRY( hipExtStreamCreateWithCUMask( &s, (uint32_t)n_words, mask ), RS_HIP_E_RUNTIME );
  else       HIP_TRY( hipStreamCreateWithFlags( &s, hipStreamNonBlocking ), RS_HIP_E_RUNTIME );          // (null, 0): back to an unrestricted stream
  if( g_own_stream ) { (void)hipStreamSynchronize( g_own_stream ); (void)hipStreamDestroy( g_own_stream ); }
  const bool was_own = g_stream == g_own_stream || !g_stream;
  g_own_stream = s;
  if( was_own ) g_stream = s;
  return RS_HIP_OK;
}

void* rs_hip_get_stream( void )
{
  if( ensure_ready() ) return nullptr;
  return (void*)g_stream;
}

int rs_hip_synchronize( void )
{
  int rc = ensure_ready(); if( rc ) return rc;
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  return RS_HIP_OK;
}

int rs_hip_profile_enable( int on )
{
  if( on && !g_evals )
  {
    int rc = ensure_ready(); if( rc ) return rc;
    HIP_TRY( hipMalloc( (void**)&g_evals, EVAL_SHARDS * 64 ), RS_HIP_E_RUNTIME );
    HIP_TRY( hipMemset( g_evals, 0, EVAL_SHARDS * 64 ), RS_HIP_E_RUNTIME );
  }
  if( on )
  {
    // events are created ahead of the timed region (creating them one by one inside it shows up as stalls of a step)
    std::lock_guard<std::mutex> lock( g_prof_mutex );
    while( g_evpool.size() < 8192 ) { hipEvent_t x; if( hipEventCreate( &x ) != hipSuccess ) break; g_evpool.push_back( x ); }
  }
  g_prof = on != 0;
  return RS_HIP_OK;
}
// A named no-op on the calling thread's stream: where a caller's unit of work begins in a kernel trace (tools/pmc_summary.py --trace
// cuts a `rocprofv3 --kernel-trace` of bench.py at these; VERDICT r05, weak 6: a trace must show a step of the TIMED workload).
namespace rs { __global__ void k_step_marker() {} }
int rs_hip_profile_marker( void )
{
  int rc = ensure_ready(); if( rc ) return rc;
  hipLaunchKernelGGL( rs::k_step_marker, dim3( 1 ), dim3( 1 ), 0, g_stream );
  return RS_HIP_OK;
}
int rs_hip_profile_reset( void )
{
  prof_collect();
  std::lock_guard<std::mutex> lock( g_prof_mutex );
  for( auto& kv : g_profmap ) { kv.second.launches = 0; kv.second.ms = 0.0; }
  if( g_evals ) (void)hipMemset( g_evals, 0, EVAL_SHARDS * 64 );
  return RS_HIP_OK;
}
int rs_hip_profile_read( const char* name, int64_t* launches, double* total_ms )
{
  prof_collect();
  if( name && !std::strcmp( name, "candidates" ) )
  {
    // not a kernel: the number of candidates staged and evaluated since the last reset (each by the 64 lanes of its wave)
    unsigned long long v = 0;
    if( g_evals )
    {
      std::vector<unsigned long long> h( (size_t)EVAL_SHARDS * 8 );
      (void)hipMemcpy( h.data(), g_evals, h.size() * 8, hipMemcpyDeviceToHost );
      for( int k = 0; k < EVAL_SHARDS; ++k ) v += h[(size_t)k * 8];
    }
    if( launches ) *launches = (int64_t)v;
    if( total_ms ) *total_ms = 0.0;
    return RS_HIP_OK;
  }
  std::lock_guard<std::mutex> lock( g_prof_mutex );
  auto it = g_profmap.find( name ? name : "" );
  if( it == g_profmap.end() ) { if( launches ) *launches = 0; if( total_ms ) *total_ms = 0.0; return RS_HIP_OK; }
  if( launches ) *launches = it->second.launches;
  if( total_ms ) *total_ms = it->second.ms;
  return RS_HIP_OK;
}

} // extern "C"

// ---- cloud build -------------------------------------------------------------------------
// The caller's raw arrays are uploaded once and everything else happens on the device (rs_build.hip):
// bounds, the density-derived cell size, a stable sort by cell (input order inside a cell, like
// msh_hash_grid.h:511-532) with a dense offset table, and the Hilbert-ordered, tiled query layout.
// The host only takes the few decisions in between (cell size, table size, number of tiles).
// The index is built once per cloud level and reused by every search.
// pos / nor: packed xyz, host pointers — or device pointers when from_device (a level gathered on the device: the
// host copies the shim and the find_corrs entry point use are then downloaded instead of uploaded)
// (diagnostics, rs_hip_cloud_build_seconds: where a cloud's construction goes — host copy | upload + bounds | cell index | Hilbert order + tiles;
//  wall clock of the calling thread between the build's own synchronisations, summed over every cloud built by the process)
static std::mutex g_build_mu;
static double g_build_s[4] = { 0, 0, 0, 0 };
static long long g_build_n = 0;
struct BuildClock
{
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now(); double acc[4] = { 0, 0, 0, 0 };
  void lap( int k ) { const auto now = std::chrono::steady_clock::now(); acc[k] += std::chrono::duration<double>( now - t ).count(); t = now; }
  void commit( long long clouds = 1 ) { std::lock_guard<std::mutex> lk( g_build_mu ); for( int k = 0; k < 4; ++k ) g_build_s[k] += acc[k]; g_build_n += clouds; }
};
// rs_hip_cloud_many_single_above: a cloud of more points than this is built alone inside a batch.  The default is the timing's
// (profiles/r25/build_many_timing.txt, 16 clouds): the batch wins 8.7x at 1 000 points and 1.8x at 50 000; at 500 000 it is a tie
// (65.7 against 65.6 ms, the interquartile ranges overlap), so clouds of 500 000 points and more keep the single build, whose
// workspace is one cloud's and not the batch's.
static std::atomic<int32_t> g_many_single_above{ 499999 };
namespace rs {
rs_hip_cloud_t* cloud_create_impl( const float* pos, const float* nor, int32_t n, float cell_size, bool from_device )
{
  if( ensure_ready() != RS_HIP_OK ) return nullptr;
  if( n < 0 || ( n > 0 && !pos ) ) { set_err( "rs_hip_cloud_create: bad arguments" ); return nullptr; }
  BuildClock clk;
  rs_hip_cloud* c = new rs_hip_cloud();
  c->n = n; c->has_nor = nor != nullptr;
  if( !from_device )
  {
    c->h_pos.assign( pos, pos + (size_t)3 * n );
    if( nor ) c->h_nor.assign( nor, nor + (size_t)3 * n );
  }
  else
  {
    c->h_pos.resize( (size_t)3 * n );
    if( nor ) c->h_nor.resize( (size_t)3 * n );
  }
  clk.lap( 0 );
  auto fail = [&]( hipError_t e ) { set_err( "rs_hip_cloud_create: %s", hipGetErrorString( e ) ); rs_hip_cloud_destroy( c ); return (rs_hip_cloud_t*)nullptr; };
  auto failrc = [&]( const char* what ) { set_err( "rs_hip_cloud_create: %s", what ); rs_hip_cloud_destroy( c ); return (rs_hip_cloud_t*)nullptr; };
#define CC( expr ) do { hipError_t e_ = ( expr ); if( e_ != hipSuccess ) return fail( e_ ); } while( 0 )
  const size_t nn = (size_t)std::max( 1, n );
  BuildWorkspace& W = g_ws;
  if( W.bld_pos.ensure( nn * 12 ) || ( nor && W.bld_nor.ensure( nn * 12 ) ) || W.bld_k0.ensure( ( nn + 1 ) * 4 ) || W.bld_k1.ensure( ( nn + 1 ) * 4 ) ||
      W.bld_v0.ensure( nn * 4 ) || W.bld_v1.ensure( nn * 4 ) || W.bld_v2.ensure( nn * 4 ) || W.bld_small.ensure( 64 ) )
    return failrc( "workspace allocation failed" );
  float* d_raw = W.bld_pos.as<float>(); float* d_rawn = nor ? W.bld_nor.as<float>() : nullptr;
  uint32_t *k0 = W.bld_k0.as<uint32_t>(), *k1 = W.bld_k1.as<uint32_t>(), *v0 = W.bld_v0.as<uint32_t>(), *v1 = W.bld_v1.as<uint32_t>(), *v2 = W.bld_v2.as<uint32_t>();
  unsigned* d_small = W.bld_small.as<unsigned>();
  if( n > 0 )
  {
    CC( hipMemcpyAsync( d_raw, pos, (size_t)n * 12, from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, g_stream ) );
    if( nor ) CC( hipMemcpyAsync( d_rawn, nor, (size_t)n * 12, from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, g_stream ) );
    if( from_device )
    {
      CC( hipMemcpyAsync( c->h_pos.data(), pos, (size_t)n * 12, hipMemcpyDeviceToHost, g_stream ) );
      if( nor ) CC( hipMemcpyAsync( c->h_nor.data(), nor, (size_t)n * 12, hipMemcpyDeviceToHost, g_stream ) );
    }
  }

  // bounds (+ the largest normal, which bounds how fast a gate value can change with the query normal)
  float mn[3] = { 0, 0, 0 }, mx[3] = { 0, 0, 0 };
  if( n > 0 )
  {
    const unsigned init[8] = { ~0u, ~0u, ~0u, 0u, 0u, 0u, 0u, 0u };
    unsigned got[8];
    CC( hipMemcpyAsync( d_small, init, 32, hipMemcpyHostToDevice, g_stream ) );
    launch_build_bounds( d_raw, d_rawn, n, d_small, g_stream );
    CC( hipMemcpyAsync( got, d_small, 32, hipMemcpyDeviceToHost, g_stream ) );
    CC( hipStreamSynchronize( g_stream ) );
    auto dec = []( unsigned u ) { unsigned b = ( u & 0x80000000u ) ? ( u ^ 0x80000000u ) : ~u; float f; std::memcpy( &f, &b, 4 ); return f; };
    for( int a = 0; a < 3; ++a ) { mn[a] = dec( got[a] ); mx[a] = dec( got[3 + a] ); }
    bp_sanitise_bounds( mn, mx );           // (the kernel took the finite coordinates only; an axis without one: [0, 0])
    if( nor )
    {
      float n2; std::memcpy( &n2, &got[6], 4 );
      c->nor_max = ( got[7] || !std::isfinite( n2 ) ) ? INFINITY : std::sqrt( n2 ) * 1.00001f;
    }
  }

  clk.lap( 1 );
  // cell_size < 0: pick the cell from the cloud's own sampling density (about two sample
  // spacings: a surface patch then holds ~4 points per cell, the first search shell ~100-300).
  if( cell_size < 0.0f )
  {
    cell_size = 0.1f;
    if( n > 0 )
    {
      float c0 = bp_trial_first_cell( mn, mx );
      for( int attempt = 0; attempt < RS_BP_TRIAL_ATTEMPTS; ++attempt, c0 *= 2.0f )
      {
        const TrialGrid tg = bp_trial_grid( mn, mx, c0 );
        if( !tg.countable() && attempt < RS_BP_TRIAL_ATTEMPTS - 1 ) continue;          // trial grid too fine to count (huge, sparse extent): coarsen
        float per_cell = RS_BP_PER_CELL_WANTED;
        if( tg.countable() )
        {
          const size_t words = tg.words();
          if( W.bld_bits.ensure( words * 4 ) ) return failrc( "workspace allocation failed" );
          CC( hipMemsetAsync( W.bld_bits.p, 0, words * 4, g_stream ) );
          CC( hipMemsetAsync( d_small, 0, 4, g_stream ) );
          launch_build_mark( d_raw, n, mn, tg.inv, tg.top, tg.td[1], tg.td[2], W.bld_bits.as<uint32_t>(), g_stream );
          launch_popcount( W.bld_bits.as<uint32_t>(), (int)words, (int*)d_small, g_stream );
          int occ = 0;
          CC( hipMemcpyAsync( &occ, d_small, 4, hipMemcpyDeviceToHost, g_stream ) );
          CC( hipStreamSynchronize( g_stream ) );
          per_cell = bp_per_cell( n, occ );
        }
        if( per_cell >= RS_BP_PER_CELL_WANTED || attempt == RS_BP_TRIAL_ATTEMPTS - 1 ) { cell_size = bp_auto_cell_of( per_cell, c0 ); break; }
      }
      cell_size = bp_auto_cell_scaled( cell_size, sw_float( SW_AUTO_CELL_SCALE ) );
    }
  }
  int dims[3] = { 1, 1, 1 };
  float inv_cell = 0.0f, cell = cell_size;
  if( cell_size > 0.0f && n > 0 )
  {
    // (in double before any cast: an extent of any size is coarsened into the table; one that overflows a float gets the brute layout)
    if( bp_table_dims( mn, mx, cell, dims ) ) inv_cell = 1.0f / cell;
    else cell_size = cell = 0.0f;
  }
  c->cell = ( cell_size > 0.0f ) ? cell : 0.0f;
  const size_t n_cells = (size_t)dims[0] * dims[1] * dims[2];

  const size_t pb = nn * sizeof(float4);
  CC( hipMalloc( (void**)&c->d_pos, pb ) );
  if( nor ) CC( hipMalloc( (void**)&c->d_nor, pb ) );
  CC( hipMalloc( (void**)&c->d_cell_start, ( n_cells + 1 ) * 4 ) );
  CC( hipMemsetAsync( c->d_cell_start, 0, ( n_cells + 1 ) * 4, g_stream ) );
  size_t occupied = 0;
  int key_bits = 1; while( ( 1ull << key_bits ) < n_cells && key_bits < 32 ) ++key_bits;
  const size_t tmp_bytes = std::max( std::max( build_sort_temp_bytes( (int)nn, 32 ), build_scan_temp_bytes( n_cells + 1 ) ), build_scan_temp_bytes( nn + 1 ) );
  if( W.bld_tmp.ensure( tmp_bytes + 256 ) ) return failrc( "workspace allocation failed" );
  if( n > 0 )
  {
    // cell ids + per-cell counts -> offsets; stable sort of the point indices by cell
    launch_build_cellids( d_raw, n, mn, inv_cell, dims, k0, v0, c->d_cell_start, g_stream );
    if( build_exclusive_scan( W.bld_tmp.p, tmp_bytes, c->d_cell_start, c->d_cell_start, n_cells + 1, g_stream ) ) return failrc( "device scan failed" );
    if( build_sort_pairs( W.bld_tmp.p, tmp_bytes, k0, k1, v0, v1, n, key_bits, g_stream ) ) return failrc( "device sort failed" );
    launch_build_gather( d_raw, d_rawn, v1, n, c->d_pos, c->d_nor, g_stream );
    CC( hipMemsetAsync( d_small, 0, 4, g_stream ) );
    launch_build_count_runs( k1, n, (int*)d_small, g_stream );
    int occ = 0;
    CC( hipMemcpyAsync( &occ, d_small, 4, hipMemcpyDeviceToHost, g_stream ) );
    c->order.resize( (size_t)n );
    CC( hipMemcpyAsync( c->order.data(), v1, (size_t)n * 4, hipMemcpyDeviceToHost, g_stream ) );
    CC( hipStreamSynchronize( g_stream ) );
    occupied = (size_t)occ;
  }
  c->bytes = (int64_t)( pb * ( nor ? 2 : 1 ) + ( n_cells + 1 ) * 4 );

  clk.lap( 2 );
  GridView& v = c->view;
  v.pos = c->d_pos; v.nor = c->d_nor; v.cell_start = c->d_cell_start;
  v.minx = mn[0]; v.miny = mn[1]; v.minz = mn[2]; v.inv_cell = inv_cell; v.cell = inv_cell > 0.0f ? cell : 0.0f;
  v.w = dims[0]; v.h = dims[1]; v.d = dims[2]; v.n = n;

  // query layout: Hilbert order (10 bits per axis over the largest extent), tiles of <= 64 points
  float lim_cell = cell_size > 0.0f ? cell : 0.1f;
  if( !( cell_size > 0.0f ) )
  {
    // brute layout has one cell: estimate the occupancy of a 0.1 m grid instead
    occupied = bp_brute_occupied( n, mn, mx );
  }
  c->occupied = (int64_t)occupied;
  c->extent_limit = query_extent_limit( n, occupied, lim_cell, sw_float( SW_TILE_EXTENT_MAX ) );
  CC( hipMalloc( (void**)&c->d_qpos, pb ) );
  if( nor ) CC( hipMalloc( (void**)&c->d_qnor, pb ) );
  int n_tiles = 0;
  if( n > 0 )
  {
    const float scale = bp_hilbert_scale( mn, mx );
    launch_build_hilbert( d_raw, n, mn, scale, k0, v0, g_stream );
    if( build_sort_pairs( W.bld_tmp.p, tmp_bytes, k0, k1, v0, v2, n, 30, g_stream ) ) return failrc( "device sort failed" );
    launch_build_gather( d_raw, d_rawn, v2, n, c->d_qpos, c->d_qnor, g_stream );
    CC( hipMalloc( (void**)&c->d_qby_orig, (size_t)n * 4 ) );
    launch_build_inverse( c->d_qpos, n, c->d_qby_orig, g_stream );
    // tile starts: flags -> exclusive scan -> scatter
    uint32_t* flags = k0; uint32_t* scanned = k1;
    CC( hipMemsetAsync( flags + n, 0, 4, g_stream ) );
    launch_build_tile_flags( c->d_qpos, n, c->extent_limit, flags, v0, v1, g_stream );   // (order / v1 is on the host by now)
    if( build_exclusive_scan( W.bld_tmp.p, tmp_bytes, flags, scanned, (size_t)n + 1, g_stream ) ) return failrc( "device scan failed" );
    unsigned total = 0;
    CC( hipMemcpyAsync( &total, scanned + n, 4, hipMemcpyDeviceToHost, g_stream ) );
    c->qorder.resize( (size_t)n );
    CC( hipMemcpyAsync( c->qorder.data(), v2, (size_t)n * 4, hipMemcpyDeviceToHost, g_stream ) );
    CC( hipStreamSynchronize( g_stream ) );
    n_tiles = (int)total;
    CC( hipMalloc( (void**)&c->d_tiles, ( (size_t)n_tiles + 1 ) * 4 ) );
    launch_build_tile_scatter( flags, scanned, n, c->d_tiles, g_stream );
    const uint32_t last = (uint32_t)n;
    CC( hipMemcpyAsync( c->d_tiles + n_tiles, &last, 4, hipMemcpyHostToDevice, g_stream ) );
    CC( hipStreamSynchronize( g_stream ) );
  }
  else
  {
    CC( hipMalloc( (void**)&c->d_tiles, 4 ) );
    CC( hipMemsetAsync( c->d_tiles, 0, 4, g_stream ) );
    CC( hipStreamSynchronize( g_stream ) );
  }
  c->bytes += (int64_t)( pb * ( nor ? 2 : 1 ) + ( (size_t)n_tiles + 1 ) * 4 + (size_t)n * 4 );
  c->qview.pos = c->d_qpos; c->qview.nor = c->d_qnor; c->qview.tiles = c->d_tiles;
  c->qview.n = n; c->qview.n_tiles = n_tiles;
  clk.lap( 3 ); clk.commit();
#undef CC
  return c;
}
} // namespace rs

// ---- the build of many clouds in one call -------------------------------------------------------------------
// cloud_create_impl's stages, each once for a whole group of clouds (rs_build.hip: the k_many_* kernels): the points lie concatenated
// in the workspace, a segment table says where each cloud's points start and where its arrays go, and the host takes cloud_create_impl's
// decisions per cloud, with the same bp_* functions in the same order.  The synchronisations of a group are the single build's —
// bounds, one per trial attempt, cells, tiles — whatever the number of clouds; a group whose trial tables or offset tables pass
// their budget (rs_buildplan.h: bp_many_groups) takes those stages in several ranges of consecutive clouds.
namespace {

inline size_t up256( size_t b ) { return ( b + 255 ) & ~(size_t)255; }

struct ManyState       // what the host decides for one cloud
{
  float mn[3] = { 0, 0, 0 }, mx[3] = { 0, 0, 0 };
  float cell_size = 0.0f, cell = 0.0f, c0 = 0.0f, inv_cell = 0.0f;
  bool undecided = false;
  int dims[3] = { 1, 1, 1 };
  size_t n_cells = 1, occupied = 0;
};

int many_fail( int rc, const char* what, hipError_t e = hipSuccess )
{
  set_err( "rs_hip_cloud_create_many: %s%s%s", what, e != hipSuccess ? ": " : "", e != hipSuccess ? hipGetErrorString( e ) : "" );
  (void)hipStreamSynchronize( g_stream );       // copies into the clouds' vectors may be in flight, and the caller frees them next
  return rc;
}

// the points of the group's clouds into the workspace: a large cloud by a copy of its own, a run of small ones packed into one
void many_upload( const ManyInput* in, const int* idx, int m, const std::vector<int>& off, bool normals, bool from_device, float* dst, char* stage, hipStream_t st, hipError_t& err )
{
  const size_t small = 16384;
  size_t filled = 0, run_at = 0, run_bytes = 0; int run_first = -1;
  const char* d_src = nullptr; char* d_dst = nullptr; size_t d_bytes = 0;        // a copy of its own that waits for the next: segments that
  auto flush_direct = [&] {                                                      // follow each other in memory (a consumer's workspace) go as one
    if( d_bytes && err == hipSuccess ) err = hipMemcpyAsync( d_dst, d_src, d_bytes, from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st );
    d_bytes = 0;
  };
  auto flush = [&] {
    if( run_first >= 0 && run_bytes && err == hipSuccess ) err = hipMemcpyAsync( dst + (size_t)3 * off[run_first], stage + run_at, run_bytes, hipMemcpyHostToDevice, st );
    run_first = -1; run_bytes = 0; run_at = filled;
  };
  for( int j = 0; j < m && err == hipSuccess; ++j )
  {
    const ManyInput& s = in[idx[j]];
    const float* src = normals ? s.nor : s.pos;
    const size_t bytes = (size_t)s.n * 12;
    if( !bytes ) continue;                              // (takes no room: a run goes on across it)
    if( !src ) { flush(); continue; }                   // a cloud without normals leaves a hole
    if( from_device || bytes >= small )
    {
      flush();
      char* to = (char*)( dst + (size_t)3 * off[j] );
      if( d_bytes && (const char*)src == d_src + d_bytes && to == d_dst + d_bytes ) { d_bytes += bytes; continue; }
      flush_direct();
      d_src = (const char*)src; d_dst = to; d_bytes = bytes;
      continue;
    }
    flush_direct();
    if( run_first < 0 ) run_first = j;
    std::memcpy( stage + filled, src, bytes ); filled += bytes; run_bytes += bytes;
  }
  flush(); flush_direct();
}

int many_build_group( const ManyInput* in, const int* idx, int m, bool from_device, rs_hip_cloud** made, BuildClock& clk )
{
#define MT( expr, what ) do { hipError_t e_ = ( expr ); if( e_ != hipSuccess ) return many_fail( RS_HIP_E_RUNTIME, what, e_ ); } while( 0 )
  BuildWorkspace& W = g_ws;
  hipStream_t st = g_stream;
  std::vector<int> off( (size_t)m + 1, 0 );
  bool any_nor = false;
  size_t small_pos = 0, small_nor = 0;
  for( int j = 0; j < m; ++j )
  {
    const ManyInput& s = in[idx[j]];
    off[j + 1] = off[j] + s.n;
    any_nor |= s.nor && s.n > 0;
    if( !from_device && (size_t)s.n * 12 < 16384 ) { small_pos += (size_t)s.n * 12; if( s.nor ) small_nor += (size_t)s.n * 12; }
  }
  const int N = off[m];
  const size_t NN = (size_t)std::max( 1, N ), M = (size_t)m;
  // the small arrays, one buffer: bounds (8 words per cloud) | occupied | n_tiles | point offsets | the trial tables' clouds | their starts
  const size_t o_occ = 32 * M, o_ntiles = o_occ + 4 * M, o_off = o_ntiles + 4 * M, o_tseg = o_off + 4 * ( M + 1 ), o_tstart = ( o_tseg + 4 * M + 7 ) & ~(size_t)7;
  if( W.many_pos.ensure( NN * 12 ) || ( any_nor && W.many_nor.ensure( NN * 12 ) ) || W.many_segid.ensure( NN * 4 ) || W.many_k0.ensure( ( NN + 1 ) * 8 ) ||
      W.many_k1.ensure( ( NN + 1 ) * 8 ) || W.many_v0.ensure( NN * 4 ) || W.many_v1.ensure( NN * 4 ) || W.many_v2.ensure( NN * 4 ) ||
      W.many_segs.ensure( M * sizeof(ManySeg) ) || W.many_trial.ensure( M * sizeof(ManyTrial) ) || W.many_small.ensure( o_tstart + 8 * ( M + 1 ) ) ||
      W.many_stage.ensure( small_pos + small_nor + 16 ) )
    return many_fail( RS_HIP_E_RUNTIME, "workspace allocation failed" );
  float* d_raw = W.many_pos.as<float>(); float* d_rawn = any_nor ? W.many_nor.as<float>() : nullptr;
  int* segid = W.many_segid.as<int>();
  unsigned long long *k0 = W.many_k0.as<unsigned long long>(), *k1 = W.many_k1.as<unsigned long long>();
  uint32_t *v0 = W.many_v0.as<uint32_t>(), *v1 = W.many_v1.as<uint32_t>(), *v2 = W.many_v2.as<uint32_t>();
  ManySeg* d_segs = W.many_segs.as<ManySeg>(); ManyTrial* d_trial = W.many_trial.as<ManyTrial>();
  char* sm = (char*)W.many_small.p;
  unsigned* d_bounds = (unsigned*)sm; int* d_occ = (int*)( sm + o_occ ); int* d_ntiles = (int*)( sm + o_ntiles ); int* d_off = (int*)( sm + o_off );
  int* d_tseg = (int*)( sm + o_tseg ); unsigned long long* d_tstart = (unsigned long long*)( sm + o_tstart );

  std::vector<ManySeg> segs( M );
  std::memset( (void*)segs.data(), 0, M * sizeof(ManySeg) );
  for( int j = 0; j < m; ++j ) { segs[j].base = off[j]; segs[j].n = in[idx[j]].n; segs[j].has_nor = in[idx[j]].nor ? 1 : 0; segs[j].dims[0] = segs[j].dims[1] = segs[j].dims[2] = 1; }
  std::vector<float> all_pos, all_nor;       // from_device: the host copies come back in one piece
  std::vector<unsigned> bounds( 8 * M );
  std::vector<ManyState> S( M );
  if( N > 0 )
  {
    hipError_t e = hipSuccess;
    many_upload( in, idx, m, off, false, from_device, d_raw, (char*)W.many_stage.p, st, e );
    if( any_nor ) many_upload( in, idx, m, off, true, from_device, d_rawn, (char*)W.many_stage.p + small_pos, st, e );
    MT( e, "upload" );
    if( from_device )
    {
      all_pos.resize( (size_t)3 * N );
      MT( hipMemcpyAsync( all_pos.data(), d_raw, (size_t)N * 12, hipMemcpyDeviceToHost, st ), "host copy" );
      if( any_nor ) { all_nor.resize( (size_t)3 * N ); MT( hipMemcpyAsync( all_nor.data(), d_rawn, (size_t)N * 12, hipMemcpyDeviceToHost, st ), "host copy" ); }
    }
    MT( hipMemcpyAsync( d_off, off.data(), ( M + 1 ) * 4, hipMemcpyHostToDevice, st ), "segment offsets" );
    launch_many_segids( d_off, m, N, segid, st );
    MT( hipMemcpyAsync( d_segs, segs.data(), M * sizeof(ManySeg), hipMemcpyHostToDevice, st ), "segment table" );
    // bounds (+ the largest normal) of every cloud
    for( size_t j = 0; j < M; ++j ) for( int a = 0; a < 8; ++a ) bounds[8 * j + a] = a < 3 ? ~0u : 0u;
    MT( hipMemcpyAsync( d_bounds, bounds.data(), 32 * M, hipMemcpyHostToDevice, st ), "bounds" );
    launch_many_bounds( d_raw, d_rawn, segid, d_segs, N, d_bounds, st );
    MT( hipMemcpyAsync( bounds.data(), d_bounds, 32 * M, hipMemcpyDeviceToHost, st ), "bounds" );
    MT( hipStreamSynchronize( st ), "bounds" );
    auto dec = []( unsigned u ) { unsigned b = ( u & 0x80000000u ) ? ( u ^ 0x80000000u ) : ~u; float f; std::memcpy( &f, &b, 4 ); return f; };
    for( int j = 0; j < m; ++j )
    {
      if( segs[j].n <= 0 ) continue;
      const unsigned* got = bounds.data() + 8 * (size_t)j;
      for( int a = 0; a < 3; ++a ) { S[j].mn[a] = dec( got[a] ); S[j].mx[a] = dec( got[3 + a] ); }
      bp_sanitise_bounds( S[j].mn, S[j].mx );
      if( segs[j].has_nor )
      {
        float n2; std::memcpy( &n2, &got[6], 4 );
        made[j]->nor_max = ( got[7] || !std::isfinite( n2 ) ) ? INFINITY : std::sqrt( n2 ) * 1.00001f;
      }
    }
    if( from_device )
      for( int j = 0; j < m; ++j )
      {
        const size_t b = (size_t)3 * off[j], c = (size_t)3 * segs[j].n;
        if( c ) std::memcpy( made[j]->h_pos.data(), all_pos.data() + b, c * 4 );
        if( c && segs[j].has_nor ) std::memcpy( made[j]->h_nor.data(), all_nor.data() + b, c * 4 );
      }
  }
  clk.lap( 1 );

  // the density-derived cells: the undecided clouds advance attempt by attempt, their bit tables side by side
  std::vector<int> occ( M, 0 ), gend( M + 1, 0 );
  for( int j = 0; j < m; ++j )
  {
    S[j].cell_size = in[idx[j]].cell_size;
    if( S[j].cell_size < 0.0f ) { S[j].cell_size = 0.1f; if( segs[j].n > 0 ) { S[j].undecided = true; S[j].c0 = bp_trial_first_cell( S[j].mn, S[j].mx ); } }
  }
  {
    std::vector<ManyTrial> trial( M );
    std::vector<TrialGrid> grid( M );
    std::vector<int> act, tseg; std::vector<double> words; std::vector<unsigned long long> tstart;
    for( int attempt = 0; attempt < RS_BP_TRIAL_ATTEMPTS; ++attempt )
    {
      const bool last = attempt == RS_BP_TRIAL_ATTEMPTS - 1;
      act.clear(); words.clear();
      for( int j = 0; j < m; ++j )
      {
        if( !S[j].undecided ) continue;
        const TrialGrid tg = bp_trial_grid( S[j].mn, S[j].mx, S[j].c0 );
        if( !tg.countable() )               // too fine to count: coarsen, or, at the last attempt, stand for the wanted density
        {
          if( !last ) S[j].c0 *= 2.0f;
          else { S[j].cell_size = bp_auto_cell_of( RS_BP_PER_CELL_WANTED, S[j].c0 ); S[j].undecided = false; }
          continue;
        }
        grid[j] = tg; act.push_back( j ); words.push_back( (double)tg.words() );
      }
      if( act.empty() ) continue;
      const int ng = bp_many_groups( nullptr, words.data(), (int)act.size(), 0.0, RS_BP_MANY_TRIAL_WORDS_MAX, gend.data() );
      for( int g = 0; g < ng; ++g )
      {
        const int ga = g ? gend[g - 1] : 0, gb = gend[g];
        for( auto& t : trial ) t.active = 0;
        tseg.clear(); tstart.clear();
        unsigned long long total = 0;
        for( int t = ga; t < gb; ++t )
        {
          const int j = act[t]; const TrialGrid& tg = grid[j]; ManyTrial& T = trial[j];
          for( int a = 0; a < 3; ++a ) { T.mn[a] = S[j].mn[a]; T.top[a] = tg.top[a]; }
          T.inv = tg.inv; T.db = tg.td[1]; T.dc = tg.td[2]; T.word = total; T.active = 1;
          tseg.push_back( j ); tstart.push_back( total ); total += tg.words();
        }
        tstart.push_back( total );
        if( W.many_bits.ensure( (size_t)total * 4 ) ) return many_fail( RS_HIP_E_RUNTIME, "workspace allocation failed" );
        MT( hipMemsetAsync( W.many_bits.p, 0, (size_t)total * 4, st ), "trial grid" );
        MT( hipMemsetAsync( d_occ, 0, 4 * M, st ), "trial grid" );
        MT( hipMemcpyAsync( d_trial, trial.data(), M * sizeof(ManyTrial), hipMemcpyHostToDevice, st ), "trial grid" );
        MT( hipMemcpyAsync( d_tseg, tseg.data(), tseg.size() * 4, hipMemcpyHostToDevice, st ), "trial grid" );
        MT( hipMemcpyAsync( d_tstart, tstart.data(), tstart.size() * 8, hipMemcpyHostToDevice, st ), "trial grid" );
        const int first = off[act[ga]], end = off[act[gb - 1] + 1];
        launch_many_mark( d_raw, segid, d_trial, first, end - first, W.many_bits.as<uint32_t>(), st );
        launch_many_popcount( W.many_bits.as<uint32_t>(), total, d_tstart, d_tseg, (int)tseg.size(), d_occ, st );
        MT( hipMemcpyAsync( occ.data(), d_occ, 4 * M, hipMemcpyDeviceToHost, st ), "trial grid" );
        MT( hipStreamSynchronize( st ), "trial grid" );
        for( int t = ga; t < gb; ++t )
        {
          const int j = act[t];
          const float per_cell = bp_per_cell( segs[j].n, occ[j] );
          if( per_cell >= RS_BP_PER_CELL_WANTED || last ) { S[j].cell_size = bp_auto_cell_of( per_cell, S[j].c0 ); S[j].undecided = false; }
          else S[j].c0 *= 2.0f;
        }
      }
    }
  }
  const float auto_scale = sw_float( SW_AUTO_CELL_SCALE ), extent_max = sw_float( SW_TILE_EXTENT_MAX );
  std::vector<double> table_words( M );
  for( int j = 0; j < m; ++j )
  {
    ManyState& s = S[j];
    if( in[idx[j]].cell_size < 0.0f && segs[j].n > 0 ) s.cell_size = bp_auto_cell_scaled( s.cell_size, auto_scale );
    s.cell = s.cell_size;
    if( s.cell_size > 0.0f && segs[j].n > 0 )
    {
      if( bp_table_dims( s.mn, s.mx, s.cell, s.dims ) ) s.inv_cell = 1.0f / s.cell;
      else s.cell_size = s.cell = 0.0f;
    }
    made[j]->cell = ( s.cell_size > 0.0f ) ? s.cell : 0.0f;
    s.n_cells = (size_t)s.dims[0] * s.dims[1] * s.dims[2];
    table_words[j] = (double)( up256( ( s.n_cells + 2 ) * 4 ) / 4 );     // n_cells + 1 offsets and the word that starts the next table at 0
    for( int a = 0; a < 3; ++a ) { segs[j].mn[a] = s.mn[a]; segs[j].dims[a] = s.dims[a]; }
    segs[j].inv_cell = s.inv_cell;
  }

  // the rest, for one range of clouds after the other whose offset tables fit the budget together (as a rule: all at once)
  int seg_bits = 0; while( ( 1ull << seg_bits ) < (unsigned long long)m ) ++seg_bits;
  std::vector<int32_t> all_order( NN ), all_qorder( NN );
  std::vector<int> n_tiles( M, 0 );
  const int ng = bp_many_groups( nullptr, table_words.data(), m, 0.0, RS_BP_MANY_CELL_WORDS_MAX, gend.data() );
  std::vector<int> range_end( gend.begin(), gend.begin() + ng );
  for( int g = 0; g < ng; ++g )
  {
    const int a = g ? range_end[g - 1] : 0, b = range_end[g];
    const int first = off[a], cnt = off[b] - off[a];
    // one allocation: the offset tables first and side by side, then every cloud's records, tile list and inverse
    size_t total = 0;
    for( int j = a; j < b; ++j ) { segs[j].cell_word = total / 4; total += (size_t)table_words[j] * 4; }
    const size_t region_words = total / 4;
    std::vector<size_t> at( (size_t)( b - a ) * 6 );
    for( int j = a; j < b; ++j )
    {
      const size_t pb = (size_t)std::max( 1, segs[j].n ) * sizeof(float4);
      size_t* o = at.data() + (size_t)( j - a ) * 6;
      o[0] = total; total += up256( pb );
      o[1] = total; if( segs[j].has_nor ) total += up256( pb );
      o[2] = total; total += up256( pb );
      o[3] = total; if( segs[j].has_nor ) total += up256( pb );
      o[4] = total; total += up256( ( (size_t)segs[j].n + 1 ) * 4 );        // (at most a tile per point)
      o[5] = total; if( segs[j].n > 0 ) total += up256( (size_t)segs[j].n * 4 );
    }
    CloudBlock* blk = new CloudBlock();
    { const hipError_t e = hipMalloc( &blk->p, total ); if( e != hipSuccess ) { delete blk; return many_fail( RS_HIP_E_RUNTIME, "allocation of the clouds failed", e ); } }
    char* base = (char*)blk->p;
    uint32_t* tables = (uint32_t*)base;
    for( int j = a; j < b; ++j )
    {
      rs_hip_cloud* c = made[j]; const size_t* o = at.data() + (size_t)( j - a ) * 6;
      c->block = blk; blk->clouds.fetch_add( 1 );
      c->d_cell_start = tables + segs[j].cell_word;
      c->d_pos = (float4*)( base + o[0] ); c->d_nor = segs[j].has_nor ? (float4*)( base + o[1] ) : nullptr;
      c->d_qpos = (float4*)( base + o[2] ); c->d_qnor = segs[j].has_nor ? (float4*)( base + o[3] ) : nullptr;
      c->d_tiles = (uint32_t*)( base + o[4] ); c->d_qby_orig = segs[j].n > 0 ? (int*)( base + o[5] ) : nullptr;
      segs[j].pos = c->d_pos; segs[j].nor = c->d_nor; segs[j].qpos = c->d_qpos; segs[j].qnor = c->d_qnor; segs[j].tiles = c->d_tiles; segs[j].by_orig = c->d_qby_orig;
    }
    const size_t tmp_bytes = std::max( std::max( build_sort64_temp_bytes( std::max( 1, cnt ), 32 + seg_bits ), build_scan_temp_bytes( region_words ) ), build_scan_temp_bytes( (size_t)cnt + 1 ) );
    if( W.many_tmp.ensure( tmp_bytes + 256 ) ) return many_fail( RS_HIP_E_RUNTIME, "workspace allocation failed" );
    MT( hipMemsetAsync( tables, 0, region_words * 4, st ), "cell tables" );
    MT( hipMemcpyAsync( d_segs, segs.data(), M * sizeof(ManySeg), hipMemcpyHostToDevice, st ), "segment table" );
    if( cnt > 0 )
    {
      // cell ids + per-cell counts -> offsets (one scan over all tables); stable sort of the point indices by (cloud, cell)
      launch_many_cellids( d_raw, segid, d_segs, first, cnt, k0, v0, tables, st );
      if( build_exclusive_scan( W.many_tmp.p, tmp_bytes, tables, tables, region_words, st ) ) return many_fail( RS_HIP_E_RUNTIME, "device scan failed" );
      if( build_sort64_pairs( W.many_tmp.p, tmp_bytes, k0 + first, k1 + first, v0 + first, v1 + first, cnt, 32 + seg_bits, st ) ) return many_fail( RS_HIP_E_RUNTIME, "device sort failed" );
      launch_many_gather( d_raw, d_rawn, segid, d_segs, v1, first, cnt, false, st );
      MT( hipMemsetAsync( d_occ, 0, 4 * M, st ), "cell index" );
      launch_many_count_runs( k1, segid, first, cnt, d_occ, st );
      MT( hipMemcpyAsync( occ.data() + a, d_occ + a, (size_t)( b - a ) * 4, hipMemcpyDeviceToHost, st ), "cell index" );
      MT( hipMemcpyAsync( all_order.data() + first, v1 + first, (size_t)cnt * 4, hipMemcpyDeviceToHost, st ), "cell index" );
    }
    MT( hipStreamSynchronize( st ), "cell index" );
    clk.lap( 2 );

    // query layouts: Hilbert order, tiles
    for( int j = a; j < b; ++j )
    {
      ManyState& s = S[j]; rs_hip_cloud* c = made[j];
      const int n = segs[j].n;
      s.occupied = n > 0 ? (size_t)occ[j] : 0;
      const float lim_cell = s.cell_size > 0.0f ? s.cell : 0.1f;
      if( !( s.cell_size > 0.0f ) ) s.occupied = bp_brute_occupied( n, s.mn, s.mx );
      c->occupied = (int64_t)s.occupied;
      c->extent_limit = query_extent_limit( n, s.occupied, lim_cell, extent_max );
      segs[j].extent_limit = c->extent_limit;
      segs[j].hscale = n > 0 ? bp_hilbert_scale( s.mn, s.mx ) : 0.0f;
    }
    MT( hipMemcpyAsync( d_segs, segs.data(), M * sizeof(ManySeg), hipMemcpyHostToDevice, st ), "segment table" );
    if( cnt > 0 )
    {
      launch_many_hilbert( d_raw, segid, d_segs, first, cnt, k0, v0, st );
      if( build_sort64_pairs( W.many_tmp.p, tmp_bytes, k0 + first, k1 + first, v0 + first, v2 + first, cnt, 32 + seg_bits, st ) ) return many_fail( RS_HIP_E_RUNTIME, "device sort failed" );
      launch_many_gather( d_raw, d_rawn, segid, d_segs, v2, first, cnt, true, st );
      // tile starts: flags -> exclusive scan -> scatter (the keys and the cell order, which is on the host by now, are scratch from here)
      uint32_t* flags = (uint32_t*)k0; uint32_t* scanned = (uint32_t*)k1;
      launch_many_tile_flags( segid, d_segs, first, cnt, flags, v0, v1, st );
      if( build_exclusive_scan( W.many_tmp.p, tmp_bytes, flags, scanned, (size_t)cnt + 1, st ) ) return many_fail( RS_HIP_E_RUNTIME, "device scan failed" );
      launch_many_tile_scatter( flags, scanned, segid, d_segs, first, cnt, a, b - a, d_ntiles, st );
      MT( hipMemcpyAsync( all_qorder.data() + first, v2 + first, (size_t)cnt * 4, hipMemcpyDeviceToHost, st ), "tiles" );
    }
    else launch_many_tile_scatter( nullptr, nullptr, segid, d_segs, first, 0, a, b - a, d_ntiles, st );
    MT( hipMemcpyAsync( n_tiles.data() + a, d_ntiles + a, (size_t)( b - a ) * 4, hipMemcpyDeviceToHost, st ), "tiles" );
    MT( hipStreamSynchronize( st ), "tiles" );
    clk.lap( 3 );
  }

  for( int j = 0; j < m; ++j )
  {
    rs_hip_cloud* c = made[j]; const ManyState& s = S[j];
    const int n = segs[j].n; const bool nor = segs[j].has_nor != 0;
    const size_t pb = (size_t)std::max( 1, n ) * sizeof(float4);
    if( n > 0 )
    {
      c->order.assign( all_order.begin() + off[j], all_order.begin() + off[j + 1] );
      c->qorder.assign( all_qorder.begin() + off[j], all_qorder.begin() + off[j + 1] );
    }
    c->bytes = (int64_t)( pb * ( nor ? 2 : 1 ) + ( s.n_cells + 1 ) * 4 ) + (int64_t)( pb * ( nor ? 2 : 1 ) + ( (size_t)n_tiles[j] + 1 ) * 4 + (size_t)n * 4 );
    GridView& v = c->view;
    v.pos = c->d_pos; v.nor = c->d_nor; v.cell_start = c->d_cell_start;
    v.minx = s.mn[0]; v.miny = s.mn[1]; v.minz = s.mn[2]; v.inv_cell = s.inv_cell; v.cell = s.inv_cell > 0.0f ? s.cell : 0.0f;
    v.w = s.dims[0]; v.h = s.dims[1]; v.d = s.dims[2]; v.n = n;
    c->qview.pos = c->d_qpos; c->qview.nor = c->d_qnor; c->qview.tiles = c->d_tiles;
    c->qview.n = n; c->qview.n_tiles = n_tiles[j];
  }
#undef MT
  return RS_HIP_OK;
}

} // namespace

namespace rs {
int cloud_create_many_impl( const ManyInput* in, int32_t K, bool from_device, rs_hip_cloud_t** out )
{
  if( K < 0 || !out || ( K > 0 && !in ) ) { set_err( "rs_hip_cloud_create_many: bad arguments" ); return RS_HIP_E_ARG; }
  for( int k = 0; k < K; ++k )
    if( in[k].n < 0 || ( in[k].n > 0 && !in[k].pos ) ) { set_err( "rs_hip_cloud_create_many: cloud %d: a negative size, or points without an array", k ); return RS_HIP_E_ARG; }
  if( K == 0 ) return RS_HIP_OK;
  int rc = ensure_ready(); if( rc ) return rc;
  BuildClock clk;
  std::vector<rs_hip_cloud*> made( (size_t)K, nullptr );
  auto undo = [&] { for( rs_hip_cloud* c : made ) rs_hip_cloud_destroy( c ); };
  // a cloud above the threshold gains nothing from the batch and is built alone, to the same bytes
  const int32_t single_above = g_many_single_above.load();
  std::vector<int> batch;
  std::vector<double> points;
  int below = 0;
  for( int k = 0; k < K; ++k ) below += in[k].n <= single_above ? 1 : 0;
  for( int k = 0; k < K; ++k )
  {
    if( below < 2 || in[k].n > single_above ) continue;      // (a batch of one is the single build)
    rs_hip_cloud* c = new rs_hip_cloud();
    c->n = in[k].n; c->has_nor = in[k].nor != nullptr;
    const size_t f = (size_t)3 * in[k].n;
    if( !from_device ) { c->h_pos.assign( in[k].pos, in[k].pos + f ); if( in[k].nor ) c->h_nor.assign( in[k].nor, in[k].nor + f ); }
    else { c->h_pos.resize( f ); if( in[k].nor ) c->h_nor.resize( f ); }
    made[k] = c; batch.push_back( k ); points.push_back( (double)in[k].n );
  }
  clk.lap( 0 );
  if( !batch.empty() )
  {
    std::vector<int> gend( batch.size() );
    const int ng = bp_many_groups( points.data(), nullptr, (int)batch.size(), RS_BP_MANY_POINTS_MAX, 0.0, gend.data() );
    std::vector<rs_hip_cloud*> group;
    for( int g = 0; g < ng; ++g )
    {
      const int a = g ? gend[g - 1] : 0, b = gend[g];
      group.clear();
      for( int t = a; t < b; ++t ) group.push_back( made[batch[t]] );
      rc = many_build_group( in, batch.data() + a, b - a, from_device, group.data(), clk );
      if( rc ) { undo(); return rc; }
    }
    clk.commit( (long long)batch.size() );
  }
  for( int k = 0; k < K; ++k )
  {
    if( made[k] ) continue;
    made[k] = cloud_create_impl( in[k].pos, in[k].nor, in[k].n, in[k].cell_size, from_device );      // (its own laps and error text)
    if( !made[k] ) { undo(); return RS_HIP_E_RUNTIME; }
  }
  for( int k = 0; k < K; ++k ) out[k] = made[k];
  return RS_HIP_OK;
}
} // namespace rs

extern "C" {

extern "C" int64_t rs_hip_cloud_build_seconds( double out[4], int32_t reset )
{
  std::lock_guard<std::mutex> lk( g_build_mu );
  if( out ) for( int k = 0; k < 4; ++k ) out[k] = g_build_s[k];
  const long long n = g_build_n;
  if( reset ) { for( int k = 0; k < 4; ++k ) g_build_s[k] = 0.0; g_build_n = 0; }
  return n;
}

rs_hip_cloud_t* rs_hip_cloud_create( const float* pos, const float* nor, int32_t n, float cell_size )
{
  return cloud_create_impl( pos, nor, n, cell_size, false );
}

int rs_hip_cloud_create_many( const float* const* pos, const float* const* nor, const int32_t* n, const float* cell_sizes, int32_t n_clouds, rs_hip_cloud_t** out )
{
  if( n_clouds < 0 || !out || ( n_clouds > 0 && ( !pos || !n ) ) ) { set_err( "rs_hip_cloud_create_many: bad arguments" ); return RS_HIP_E_ARG; }
  std::vector<ManyInput> in( (size_t)n_clouds );
  for( int k = 0; k < n_clouds; ++k ) in[k] = ManyInput{ pos[k], nor ? nor[k] : nullptr, n[k], cell_sizes ? cell_sizes[k] : -1.0f };
  return cloud_create_many_impl( in.data(), n_clouds, false, out );
}

int32_t rs_hip_cloud_many_single_above( int32_t n )
{
  return n < 0 ? g_many_single_above.load() : g_many_single_above.exchange( n );
}

int rs_hip_cloud_points( const rs_hip_cloud_t* c, float* pos, float* nor )
{
  if( !c || ( nor && !c->has_nor ) ) { set_err( "cloud_points: no cloud, or normals asked of a cloud without them" ); return RS_HIP_E_ARG; }
  if( pos ) std::memcpy( pos, c->h_pos.data(), c->h_pos.size() * 4 );
  if( nor ) std::memcpy( nor, c->h_nor.data(), c->h_nor.size() * 4 );
  return RS_HIP_OK;
}

void rs_hip_cloud_destroy( rs_hip_cloud_t* c )
{
  if( !c ) return;
  if( c->block )         // made by a batched build: its arrays are sub-ranges of the block, which goes with its last cloud
  {
    if( c->block->clouds.fetch_sub( 1 ) == 1 ) { if( c->block->p ) (void)hipFree( c->block->p ); delete c->block; }
    delete c;
    return;
  }
  if( c->d_pos ) (void)hipFree( c->d_pos );
  if( c->d_nor ) (void)hipFree( c->d_nor );
  if( c->d_cell_start ) (void)hipFree( c->d_cell_start );
  if( c->d_qpos ) (void)hipFree( c->d_qpos );
  if( c->d_qnor ) (void)hipFree( c->d_qnor );
  if( c->d_tiles ) (void)hipFree( c->d_tiles );
  if( c->d_qby_orig ) (void)hipFree( c->d_qby_orig );
  delete c;
}

int32_t rs_hip_cloud_size( const rs_hip_cloud_t* c ) { return c ? c->n : 0; }
int32_t rs_hip_cloud_tiles( const rs_hip_cloud_t* c ) { return c ? c->qview.n_tiles : 0; }
int64_t rs_hip_cloud_bytes( const rs_hip_cloud_t* c ) { return c ? c->bytes : 0; }

// What the build left, read back as it is: changes nothing and books no profile span.
int rs_hip_cloud_layout( const rs_hip_cloud_t* c, rs_hip_layout_t* out )
{
  if( !c || !out ) { set_err( "cloud_layout: no cloud, or nowhere to write" ); return RS_HIP_E_ARG; }
  if( ( out->nor || out->qnor ) && !c->has_nor ) { set_err( "cloud_layout: normals asked of a cloud without them" ); return RS_HIP_E_ARG; }
  const GridView& v = c->view;
  out->min[0] = v.minx; out->min[1] = v.miny; out->min[2] = v.minz; out->cell = v.cell; out->inv_cell = v.inv_cell;
  out->dims[0] = v.w; out->dims[1] = v.h; out->dims[2] = v.d;
  out->n = c->n; out->n_cells = (int64_t)v.w * v.h * v.d; out->occupied = c->occupied; out->extent_limit = c->extent_limit;
  out->n_tiles = c->qview.n_tiles; out->has_normals = c->has_nor ? 1 : 0;
  const size_t n = (size_t)c->n;
  if( out->order && n ) std::memcpy( out->order, c->order.data(), n * 4 );
  if( out->qorder && n ) std::memcpy( out->qorder, c->qorder.data(), n * 4 );
  if( !( out->cell_start || out->tiles || out->by_orig || out->pos || out->qpos || out->nor || out->qnor ) ) return RS_HIP_OK;
  int rc = ensure_ready(); if( rc ) return rc;
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  if( out->cell_start ) HIP_TRY( hipMemcpy( out->cell_start, c->d_cell_start, ( (size_t)out->n_cells + 1 ) * 4, hipMemcpyDeviceToHost ), RS_HIP_E_RUNTIME );
  if( out->tiles ) HIP_TRY( hipMemcpy( out->tiles, c->d_tiles, ( (size_t)out->n_tiles + 1 ) * 4, hipMemcpyDeviceToHost ), RS_HIP_E_RUNTIME );
  if( n )
  {
    if( out->by_orig ) HIP_TRY( hipMemcpy( out->by_orig, c->d_qby_orig, n * 4, hipMemcpyDeviceToHost ), RS_HIP_E_RUNTIME );
    if( out->pos ) HIP_TRY( hipMemcpy( out->pos, c->d_pos, n * 16, hipMemcpyDeviceToHost ), RS_HIP_E_RUNTIME );
    if( out->qpos ) HIP_TRY( hipMemcpy( out->qpos, c->d_qpos, n * 16, hipMemcpyDeviceToHost ), RS_HIP_E_RUNTIME );
    if( out->nor ) HIP_TRY( hipMemcpy( out->nor, c->d_nor, n * 16, hipMemcpyDeviceToHost ), RS_HIP_E_RUNTIME );
    if( out->qnor ) HIP_TRY( hipMemcpy( out->qnor, c->d_qnor, n * 16, hipMemcpyDeviceToHost ), RS_HIP_E_RUNTIME );
  }
  return RS_HIP_OK;
}

void rs_hip_sincosf_model( const float* x, int64_t n, float* sin_out, float* cos_out )
{
  for( int64_t i = 0; i < n; ++i ) rs_sincosf_model( x[i], sin_out[i], cos_out[i] );
}
void rs_hip_mat4_inverse( const float* m, float* out ) { Mat4 a; std::memcpy( a.m, m, 64 ); Mat4 r = mat4_inverse( a ); std::memcpy( out, r.m, 64 ); }
void rs_hip_mat4_mul( const float* a_, const float* b_, float* out ) { Mat4 a, b; std::memcpy( a.m, a_, 64 ); std::memcpy( b.m, b_, 64 ); Mat4 r = mat4_mul( a, b ); std::memcpy( out, r.m, 64 ); }

// The value the library would use now for a name of the table (a flag, or a word that is set: 1); no device needed.
int rs_hip_switch_get( const char* name, double* value )
{
  const int k = sw_find( name );
  if( k < 0 || !value ) { set_err( "switch_get: %s is no switch of rs_switches.h", name ? name : "(null)" ); return RS_HIP_E_ARG; }
  *value = sw_value( (SwId)k ).d;
  return RS_HIP_OK;
}

} // extern "C"

// ------------------------------------------------------------------------------------------
// what the translation units with entry points of their own need from this one (declared in rs_host.h)
// ------------------------------------------------------------------------------------------

namespace rs {
int api_ready( hipStream_t* st ) { const int rc = ensure_ready(); if( rc == RS_HIP_OK ) *st = g_stream; return rc; }
void api_set_err( const char* what ) { set_err( "%s", what ); }
const GridView* api_cloud_view( const rs_hip_cloud* c ) { return c ? &c->view : nullptr; }
void* api_prof_begin() { return g_prof ? (void*)prof_event() : nullptr; }
void api_prof_end( const char* name, void* begin ) { if( begin ) prof_span( name, (hipEvent_t)begin, prof_event() ); }
bool api_cloud_has_normals( const rs_hip_cloud* c ) { return c->has_nor; }
int api_clouds_from_device( const float* pos, const float* nor, const int64_t* first, const int64_t* count, int32_t n_segments, float cell_size, rs_hip_cloud** out )
{
  std::vector<ManyInput> in( (size_t)std::max( 0, n_segments ) );
  for( int32_t k = 0; k < n_segments; ++k )
    in[(size_t)k] = ManyInput{ pos + 3 * (size_t)first[k], nor ? nor + 3 * (size_t)first[k] : nullptr, (int32_t)count[k], cell_size };
  return cloud_create_many_impl( in.data(), n_segments, true, out );
}
CloudPoints api_cloud_points( const rs_hip_cloud* c )
{
  return CloudPoints{ c->d_qpos, c->has_nor ? c->d_qnor : nullptr, c->d_qby_orig, c->n };
}
} // namespace rs
