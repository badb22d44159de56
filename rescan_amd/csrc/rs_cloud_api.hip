// librescan_hip host side: device clouds (cell-sorted 16-byte records + cell offset table, and the same points in Hilbert order cut
// into tiles, built on the device) — rs_hip_cloud_create, rs_hip_cloud_create_many and what reads a cloud back.  Host only: no kernel
// is defined here; the build's kernels are rs_build.hip's, and every decision the host takes between them is rs_buildplan.h's
// CloudPlan: one plan, two drivers — cloud_create_impl builds one cloud, many_build_group a group of them in the same launches.
// Runtime state and profiling: rs_api.hip, through rs_api.h.

#include "../../include/rescan_hip.h"
#include "rs_api.h"
#include "rs_buildplan.h"
#include "rs_device.h"
#include "rs_host.h"
#include "rs_switches.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <vector>

using namespace rs;

namespace {

struct BuildWorkspace
{
  DevBuf bld_pos, bld_nor, bld_k0, bld_k1, bld_v0, bld_v1, bld_v2, bld_small, bld_bits, bld_tmp;   // cloud construction
  DevBuf many_pos, many_nor, many_segid, many_k0, many_k1, many_v0, many_v1, many_v2, many_segs, many_trial, many_small, many_bits, many_tmp;   // ... of a batch
  PinBuf many_stage;     // the small clouds of a batch, packed for one upload per run of them
};
thread_local BuildWorkspace g_ws;

} // namespace

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

namespace {

// ---- what both builds do alike ---------------------------------------------------------------
// the cloud object with its original-order host copies: the caller's arrays, or, from_device, room for what the build downloads
rs_hip_cloud* cloud_new( const float* pos, const float* nor, int32_t n, bool from_device )
{
  rs_hip_cloud* c = new rs_hip_cloud();
  c->n = n; c->has_nor = nor != nullptr;
  const size_t f = (size_t)3 * n;
  if( !from_device ) { c->h_pos.assign( pos, pos + f ); if( nor ) c->h_nor.assign( nor, nor + f ); }
  else { c->h_pos.resize( f ); if( nor ) c->h_nor.resize( f ); }
  return c;
}
// what a finished build leaves in the object around its arrays (the d_* pointers are set): the plan's results, both views, the size
void cloud_fill( rs_hip_cloud* c, const CloudPlan& p, int n_tiles )
{
  c->nor_max = p.nor_max;
  c->cell = ( p.cell_size > 0.0f ) ? p.cell : 0.0f;
  c->occupied = (int64_t)p.occupied;
  c->extent_limit = p.extent_limit;
  c->bytes = bp_plan_bytes( c->n, c->has_nor, p.n_cells, n_tiles );
  GridView& v = c->view;
  v.pos = c->d_pos; v.nor = c->d_nor; v.cell_start = c->d_cell_start;
  v.minx = p.mn[0]; v.miny = p.mn[1]; v.minz = p.mn[2]; v.inv_cell = p.inv_cell; v.cell = p.inv_cell > 0.0f ? p.cell : 0.0f;
  v.w = p.dims[0]; v.h = p.dims[1]; v.d = p.dims[2]; v.n = c->n;
  c->qview.pos = c->d_qpos; c->qview.nor = c->d_qnor; c->qview.tiles = c->d_tiles;
  c->qview.n = c->n; c->qview.n_tiles = n_tiles;
}

} // namespace

// ---- cloud build -------------------------------------------------------------------------
// The caller's raw arrays are uploaded once and everything else happens on the device (rs_build.hip):
// bounds, the density-derived cell size, a stable sort by cell (input order inside a cell, like
// msh_hash_grid.h:511-532) with a dense offset table, and the Hilbert-ordered, tiled query layout.
// The host only takes the few decisions in between (cell size, table size, number of tiles: the CloudPlan).
// The index is built once per cloud level and reused by every search.
// pos / nor: packed xyz, host pointers — or device pointers when from_device (a level gathered on the device: the
// host copies the shim and the find_corrs entry point use are then downloaded instead of uploaded)
namespace rs {
rs_hip_cloud_t* cloud_create_impl( const float* pos, const float* nor, int32_t n, float cell_size, bool from_device )
{
  if( ensure_ready() != RS_HIP_OK ) return nullptr;
  if( n < 0 || ( n > 0 && !pos ) ) { set_err( "rs_hip_cloud_create: bad arguments" ); return nullptr; }
  BuildClock clk;
  rs_hip_cloud* c = cloud_new( pos, nor, n, from_device );
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
  CloudPlan P;
  if( n > 0 )
  {
    const unsigned init[8] = { ~0u, ~0u, ~0u, 0u, 0u, 0u, 0u, 0u };
    unsigned got[8];
    CC( hipMemcpyAsync( d_small, init, 32, hipMemcpyHostToDevice, g_stream ) );
    launch_build_bounds( d_raw, d_rawn, n, d_small, g_stream );
    CC( hipMemcpyAsync( got, d_small, 32, hipMemcpyDeviceToHost, g_stream ) );
    CC( hipStreamSynchronize( g_stream ) );
    bp_plan_bounds( P, got, n, nor != nullptr );
  }

  clk.lap( 1 );
  // the density-derived cell: one trial grid after the other is counted until one is coarse enough
  const bool asked_auto = cell_size < 0.0f;
  bp_plan_cell_begin( P, cell_size, n );
  for( int attempt = 0; P.undecided; ++attempt )
  {
    const bool last = attempt == RS_BP_TRIAL_ATTEMPTS - 1;
    TrialGrid tg;
    if( !bp_plan_trial( P, last, tg ) ) continue;
    const size_t words = tg.words();
    if( W.bld_bits.ensure( words * 4 ) ) return failrc( "workspace allocation failed" );
    CC( hipMemsetAsync( W.bld_bits.p, 0, words * 4, g_stream ) );
    CC( hipMemsetAsync( d_small, 0, 4, g_stream ) );
    launch_build_mark( d_raw, n, P.mn, tg.inv, tg.top, tg.td[1], tg.td[2], W.bld_bits.as<uint32_t>(), g_stream );
    launch_popcount( W.bld_bits.as<uint32_t>(), (int)words, (int*)d_small, g_stream );
    int occ = 0;
    CC( hipMemcpyAsync( &occ, d_small, 4, hipMemcpyDeviceToHost, g_stream ) );
    CC( hipStreamSynchronize( g_stream ) );
    bp_plan_trial_counted( P, n, occ, last );
  }
  // (the scale is read, and with that fixed for the process, by the first build that needs it)
  bp_plan_table( P, n, asked_auto, asked_auto && n > 0 ? sw_float( SW_AUTO_CELL_SCALE ) : 1.0f );

  const size_t pb = nn * sizeof(float4);
  CC( hipMalloc( (void**)&c->d_pos, pb ) );
  if( nor ) CC( hipMalloc( (void**)&c->d_nor, pb ) );
  CC( hipMalloc( (void**)&c->d_cell_start, ( P.n_cells + 1 ) * 4 ) );
  CC( hipMemsetAsync( c->d_cell_start, 0, ( P.n_cells + 1 ) * 4, g_stream ) );
  size_t occupied = 0;
  int key_bits = 1; while( ( 1ull << key_bits ) < P.n_cells && key_bits < 32 ) ++key_bits;
  const size_t tmp_bytes = std::max( std::max( build_sort_temp_bytes( (int)nn, 32 ), build_scan_temp_bytes( P.n_cells + 1 ) ), build_scan_temp_bytes( nn + 1 ) );
  if( W.bld_tmp.ensure( tmp_bytes + 256 ) ) return failrc( "workspace allocation failed" );
  if( n > 0 )
  {
    // cell ids + per-cell counts -> offsets; stable sort of the point indices by cell
    launch_build_cellids( d_raw, n, P.mn, P.inv_cell, P.dims, k0, v0, c->d_cell_start, g_stream );
    if( build_exclusive_scan( W.bld_tmp.p, tmp_bytes, c->d_cell_start, c->d_cell_start, P.n_cells + 1, g_stream ) ) return failrc( "device scan failed" );
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

  clk.lap( 2 );
  // query layout: Hilbert order (10 bits per axis over the largest extent), tiles of <= 64 points
  // (The tile extent limit, from the cloud's own sampling density: query_extent_limit, rs_buildplan.h.  Its cap, RS_HIP_TILE_EXTENT_MAX:
  //  a sparse cloud (a subsampled level, a random subset) searched in a denser one would otherwise get tiles whose box is mostly the
  //  empty space between its points — 1000 points against a 200 k scan: 404 -> 60 us per ICP iteration with the cap.)
  bp_plan_query_layout( P, n, occupied, sw_float( SW_TILE_EXTENT_MAX ) );
  CC( hipMalloc( (void**)&c->d_qpos, pb ) );
  if( nor ) CC( hipMalloc( (void**)&c->d_qnor, pb ) );
  int n_tiles = 0;
  if( n > 0 )
  {
    launch_build_hilbert( d_raw, n, P.mn, P.hscale, k0, v0, g_stream );
    if( build_sort_pairs( W.bld_tmp.p, tmp_bytes, k0, k1, v0, v2, n, 30, g_stream ) ) return failrc( "device sort failed" );
    launch_build_gather( d_raw, d_rawn, v2, n, c->d_qpos, c->d_qnor, g_stream );
    CC( hipMalloc( (void**)&c->d_qby_orig, (size_t)n * 4 ) );
    launch_build_inverse( c->d_qpos, n, c->d_qby_orig, g_stream );
    // tile starts: flags -> exclusive scan -> scatter
    uint32_t* flags = k0; uint32_t* scanned = k1;
    CC( hipMemsetAsync( flags + n, 0, 4, g_stream ) );
    launch_build_tile_flags( c->d_qpos, n, P.extent_limit, flags, v0, v1, g_stream );   // (order / v1 is on the host by now)
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
  cloud_fill( c, P, n_tiles );
  clk.lap( 3 ); clk.commit();
#undef CC
  return c;
}
} // namespace rs

// ---- the build of many clouds in one call -------------------------------------------------------------------
// cloud_create_impl's stages, each once for a whole group of clouds (rs_build.hip: the k_many_* kernels): the points lie concatenated
// in the workspace, a segment table says where each cloud's points start and where its arrays go, and every cloud has its own
// CloudPlan, advanced by the functions that advance cloud_create_impl's.  The synchronisations of a group are the single build's —
// bounds, one per trial attempt, cells, tiles — whatever the number of clouds; a group whose trial tables or offset tables pass
// their budget (rs_buildplan.h: bp_many_groups) takes those stages in several ranges of consecutive clouds.
namespace {

inline size_t up256( size_t b ) { return ( b + 255 ) & ~(size_t)255; }

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
  std::vector<CloudPlan> S( M );
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
    for( int j = 0; j < m; ++j ) bp_plan_bounds( S[j], bounds.data() + 8 * (size_t)j, segs[j].n, segs[j].has_nor != 0 );
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
  for( int j = 0; j < m; ++j ) bp_plan_cell_begin( S[j], in[idx[j]].cell_size, segs[j].n );
  {
    std::vector<ManyTrial> trial( M );
    std::vector<TrialGrid> grid( M );
    std::vector<int> act, tseg; std::vector<double> words; std::vector<unsigned long long> tstart;
    for( int attempt = 0; attempt < RS_BP_TRIAL_ATTEMPTS; ++attempt )
    {
      const bool last = attempt == RS_BP_TRIAL_ATTEMPTS - 1;
      act.clear(); words.clear();
      for( int j = 0; j < m; ++j )
        if( S[j].undecided && bp_plan_trial( S[j], last, grid[j] ) ) { act.push_back( j ); words.push_back( (double)grid[j].words() ); }
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
        for( int t = ga; t < gb; ++t ) bp_plan_trial_counted( S[act[t]], segs[act[t]].n, occ[act[t]], last );
      }
    }
  }
  const float auto_scale = sw_float( SW_AUTO_CELL_SCALE ), extent_max = sw_float( SW_TILE_EXTENT_MAX );
  std::vector<double> table_words( M );
  for( int j = 0; j < m; ++j )
  {
    CloudPlan& s = S[j];
    bp_plan_table( s, segs[j].n, in[idx[j]].cell_size < 0.0f, auto_scale );
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
      bp_plan_query_layout( S[j], segs[j].n, segs[j].n > 0 ? (size_t)occ[j] : 0, extent_max );
      segs[j].extent_limit = S[j].extent_limit;
      segs[j].hscale = S[j].hscale;
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
    rs_hip_cloud* c = made[j];
    if( segs[j].n > 0 )
    {
      c->order.assign( all_order.begin() + off[j], all_order.begin() + off[j + 1] );
      c->qorder.assign( all_qorder.begin() + off[j], all_qorder.begin() + off[j + 1] );
    }
    cloud_fill( c, S[j], n_tiles[j] );
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
    made[k] = cloud_new( in[k].pos, in[k].nor, in[k].n, from_device );
    batch.push_back( k ); points.push_back( (double)in[k].n );
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

int64_t rs_hip_cloud_build_seconds( double out[4], int32_t reset )
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

} // extern "C"

// ------------------------------------------------------------------------------------------
// what the translation units with entry points of their own need of a cloud (declared in rs_host.h)
// ------------------------------------------------------------------------------------------

namespace rs {
const GridView* api_cloud_view( const rs_hip_cloud* c ) { return c ? &c->view : nullptr; }
bool api_cloud_has_normals( const rs_hip_cloud* c ) { return c->has_nor; }
int api_clouds_from_device( const float* pos, const float* nor, const int64_t* first, const int64_t* count, int32_t n_segments, float cell_size, rs_hip_cloud** out )
{
  std::vector<ManyInput> in( (size_t)std::max( 0, n_segments ) );
  for( int32_t k = 0; k < n_segments; ++k )
    in[(size_t)k] = ManyInput{ pos + 3 * (size_t)first[k], nor ? nor + 3 * (size_t)first[k] : nullptr, (int32_t)count[k], cell_size };
  return cloud_create_many_impl( in.data(), n_segments, true, out );
}
int api_clouds_from_device_each( const float* pos, const float* nor, const int64_t* first, const int64_t* count, const int32_t* has_nor, const float* cell_sizes,
                                 int32_t n_segments, rs_hip_cloud** out )
{
  std::vector<ManyInput> in( (size_t)std::max( 0, n_segments ) );
  for( int32_t k = 0; k < n_segments; ++k )
    in[(size_t)k] = ManyInput{ pos + 3 * (size_t)first[k], has_nor[k] ? nor + 3 * (size_t)first[k] : nullptr, (int32_t)count[k], cell_sizes[k] };
  return cloud_create_many_impl( in.data(), n_segments, true, out );
}
const QueryView* api_cloud_query( const rs_hip_cloud* c ) { return c ? &c->qview : nullptr; }
CloudPoints api_cloud_points( const rs_hip_cloud* c )
{
  return CloudPoints{ c->d_qpos, c->has_nor ? c->d_qnor : nullptr, c->d_qby_orig, c->n };
}
} // namespace rs
