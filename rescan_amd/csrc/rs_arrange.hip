// The arrangement optimiser's set-up and its greedy step on the scene voxel grid (apps/segment_transfer/arrangement_optimization.cpp):
// rsao__compute_scene_saliency_grid (:1038-1062, :1109-1160) — rs_hip_scene_saliency — and the coverage term of rsao_greedy_step's
// C trial arrangements "current + proposal k" (:1012-1020 through :344-373, :1083-1106) — rs_hip_coverage_extensions.
//
// Everything the reference decides here is a cell index, a 0 / 1 cell value, a count of cells or one fp32 division of two counts,
// so the results are the reference's, bit for bit.  The fp32 arithmetic that leads to a cell keeps its operations and their order:
// xform3 (msh_mat4_vec3_mul) and voxel_of (isect_grid3d_cell_from_world_space: the MULTIPLY by 1.0f / voxel), -ffp-contract=off.
//
// Saliency: one bit per cell.  Stores of the reference are idempotent within a phase (every dynamic proposal writes 1, every
// static one 0), so the order inside a phase is free and the order BETWEEN the phases is all there is to keep: k_saliency_raster
// runs once over the dynamic proposals (atomicOr) and then once over the static ones (atomicAnd), two launches on one stream.
// k_saliency_lookup reads the finished plane per level-0 scene point.
//
// Extensions: agree( base + k ) = agree( base ) + fresh[k], fresh[k] = the distinct cells candidate k hits that are scene-active
// and that no base placement hits.
//   1. the base is rasterised ONCE into one plane with the coverage term's own kernel (k_coverage, one arrangement): it sets
//      scene-active cells only and counts them, so the plane is "base AND scene" and the count is agree( base ).
//   2. k_extend<false>: one workgroup per candidate.  A first walk over the candidate's points finds the box of its LIVE cells
//      (scene-active, not in the base plane: the only cells that can count); the sub-box's bits are cleared in LDS; a second
//      walk sets them with an LDS atomicOr, the first setter counts.  No per-candidate plane of the grid, no global memset.
//      A candidate whose sub-box exceeds the LDS budget writes nothing but its name and its size to an overflow list.
//   3. only if that list is not empty: k_extend<true>, the same code on a slab of global memory, one workgroup per listed
//      candidate (a wall seen at an angle at 5 cm is ~11 KB and still fits; the route exists for small voxels and for tests).
//   4. the host adds, divides (:366-367) and reports.  One read-back per call on the LDS route.
// (rs_isect.hip takes the boxes in a launch of their own and routes on the host before the main launch.  Here the box needs the
//  two planes, not the pose alone, and the common case is "every candidate fits": deciding inside the workgroup saves that launch
//  and its read-back for all of them.)
#include "rs_host.h"
#include "rs_search.h"
#include "rs_voxel.h"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstring>
#include <vector>

using namespace rs;

// 256 threads: a level-2 object is tens to a few hundred points, one or two trips of the point loops; 4 waves and 16 KiB of LDS
// per workgroup let 8 workgroups share a CU (32 waves: the wave cap binds before the 160 KiB of LDS do).
#define ARR_BLOCK 256
#define ARR_LDS_BYTES 16384
#define ARR_MAX_GRID_Y 65535
#define ARR_SLAB_BYTES ( (size_t)256 << 20 )      // global route: sub-boxes of one launch (one plane of the largest grid is 250 MB)

namespace {

struct ArrProposal { const float4* pos; int n; int pad; Xform pose; };
struct ArrOverflow { int cand; int pad; unsigned long long words; };
struct ArrSlabJob  { int cand; int pad; unsigned long long off, words; };

struct ExtLaunch
{
  VoxGrid grid;
  const uint32_t* scene_bits; const uint32_t* base_bits;
  const CoveragePlacement* cand;
  int lds_bytes;
  int* fresh;                      // per candidate
  int* n_overflow; ArrOverflow* overflow;       // written by the LDS route
  const ArrSlabJob* jobs; uint32_t* slab;       // read by the global route
};

__device__ __forceinline__ int wave_sum( int v ) { for( int o = 32; o; o >>= 1 ) v += __shfl_xor( v, o, 64 ); return v; }
__device__ __forceinline__ int wave_min( int v ) { for( int o = 32; o; o >>= 1 ) v = min( v, __shfl_xor( v, o, 64 ) ); return v; }
__device__ __forceinline__ int wave_max( int v ) { for( int o = 32; o; o >>= 1 ) v = max( v, __shfl_xor( v, o, 64 ) ); return v; }

// rsao__rasterize_proposals_to_grid (:1038-1062) for the proposals of one phase: blockIdx.y = proposal
__global__ __launch_bounds__( ARR_BLOCK ) void k_saliency_raster( VoxGrid g, const ArrProposal* props, int set, uint32_t* bits )
{
  const ArrProposal P = props[blockIdx.y];
  for( int i = blockIdx.x * ARR_BLOCK + threadIdx.x; i < P.n; i += gridDim.x * ARR_BLOCK )
  {
    const float4 p = P.pos[i];
    float x, y, z;
    xform3( P.pose, p.x, p.y, p.z, 1.0f, x, y, z );            // :1056
    const int c = voxel_of( g, x, y, z );
    if( c < 0 ) continue;                                       // :1058
    if( set ) atomicOr( bits + ( c >> 5 ), 1u << ( c & 31 ) );
    else      atomicAnd( bits + ( c >> 5 ), ~( 1u << ( c & 31 ) ) );
  }
}

// :1137-1156 — wall and floor points are 0 whatever their cell holds; the others are their cell's value
__global__ __launch_bounds__( ARR_BLOCK ) void k_saliency_lookup( VoxGrid g, const float* pos, const int* cls, long long n, int wall, int floor_idx,
                                                                 const uint32_t* bits, float* quality )
{
  const long long i = (long long)blockIdx.x * ARR_BLOCK + threadIdx.x;
  if( i >= n ) return;
  const int k = cls[i];
  float q = 0.0f;
  if( !( k == wall || k == floor_idx ) )                        // :1141 (a class id of -1 equals an absent class's -1 there too)
  {
    const int c = voxel_of( g, pos[3*i], pos[3*i+1], pos[3*i+2] );
    if( c >= 0 && ( ( bits[c >> 5] >> ( c & 31 ) ) & 1u ) ) q = 1.0f;
  }
  quality[i] = q;
}

// the cell of point i of a placed candidate if it can still count (scene-active, not hit by the base), else -1
__device__ __forceinline__ int live_cell( const ExtLaunch& L, const CoveragePlacement& P, int i )
{
  const float4 p = P.pos[i];
  float x, y, z;
  xform3( P.pose, p.x, p.y, p.z, 1.0f, x, y, z );              // msh_mat4_vec3_mul( pose, p, 1 ), :1101
  const int c = voxel_of( L.grid, x, y, z );
  if( c < 0 ) return -1;
  const uint32_t m = 1u << ( c & 31 );
  if( !( L.scene_bits[c >> 5] & m ) || ( L.base_bits[c >> 5] & m ) ) return -1;     // :363-364
  return c;
}

// One workgroup per candidate.  GLOBAL: the sub-box lives in `slab` (candidates of L.jobs), else in LDS (every candidate).
template <bool GLOBAL>
__global__ __launch_bounds__( ARR_BLOCK ) void k_extend( ExtLaunch L )
{
  __shared__ uint32_t s_bits[GLOBAL ? 1 : ARR_LDS_BYTES / 4];
  __shared__ int s_box[6], s_fresh;
  const int tid = threadIdx.x;
  const int cand = GLOBAL ? L.jobs[blockIdx.x].cand : (int)blockIdx.x;
  const CoveragePlacement P = L.cand[cand];                    // (uniform: scalar registers)
  const int xz = L.grid.x_res * L.grid.z_res, xr = L.grid.x_res;
  if( tid < 3 ) { s_box[tid] = INT_MAX; s_box[3 + tid] = INT_MIN; }
  if( tid == 0 ) s_fresh = 0;
  __syncthreads();
  int lo[3] = { INT_MAX, INT_MAX, INT_MAX }, hi[3] = { INT_MIN, INT_MIN, INT_MIN };
  for( int i = tid; i < P.n; i += ARR_BLOCK )
  {
    const int c = live_cell( L, P, i );
    if( c < 0 ) continue;
    const int cy = c / xz, r = c - cy * xz, cz = r / xr, cx = r - cz * xr;          // :108 backwards
    lo[0] = min( lo[0], cx ); hi[0] = max( hi[0], cx ); lo[1] = min( lo[1], cy ); hi[1] = max( hi[1], cy ); lo[2] = min( lo[2], cz ); hi[2] = max( hi[2], cz );
  }
  for( int a = 0; a < 3; ++a ) { lo[a] = wave_min( lo[a] ); hi[a] = wave_max( hi[a] ); }
  if( ( tid & 63 ) == 0 ) for( int a = 0; a < 3; ++a ) { atomicMin( &s_box[a], lo[a] ); atomicMax( &s_box[3 + a], hi[a] ); }
  __syncthreads();
  const int x0 = s_box[0], y0 = s_box[1], z0 = s_box[2];
  if( s_box[3] < x0 ) { if( tid == 0 ) L.fresh[cand] = 0; return; }                  // no live cell (uniform)
  const int sx = s_box[3] - x0 + 1, sy = s_box[4] - y0 + 1, sz = s_box[5] - z0 + 1;
  const unsigned long long words = ( (unsigned long long)sx * sy * sz + 31ull ) >> 5;   // (at most the grid's own plane: below 2^26)
  if( !GLOBAL && words * 4ull > (unsigned long long)L.lds_bytes )
  {
    if( tid == 0 ) { const int slot = atomicAdd( L.n_overflow, 1 ); L.overflow[slot] = ArrOverflow{ cand, 0, words }; }
    return;
  }
  if( GLOBAL && words != L.jobs[blockIdx.x].words ) { if( tid == 0 ) L.fresh[cand] = -1; return; }     // (the same walk over the same planes: cannot differ)
  uint32_t* bits = GLOBAL ? L.slab + L.jobs[blockIdx.x].off : s_bits;
  for( unsigned long long w = tid; w < words; w += ARR_BLOCK ) bits[w] = 0u;
  __syncthreads();
  int fresh = 0;
  for( int i = tid; i < P.n; i += ARR_BLOCK )
  {
    const int c = live_cell( L, P, i );
    if( c < 0 ) continue;
    const int cy = c / xz, r = c - cy * xz, cz = r / xr, cx = r - cz * xr;
    const unsigned long long b = ( (unsigned long long)( cy - y0 ) * sz + ( cz - z0 ) ) * sx + ( cx - x0 );
    const uint32_t m = 1u << ( b & 31ull );
    if( !( atomicOr( bits + ( b >> 5 ), m ) & m ) ) ++fresh;                         // the first point in a cell counts it
  }
  fresh = wave_sum( fresh );
  if( ( tid & 63 ) == 0 && fresh ) atomicAdd( &s_fresh, fresh );
  __syncthreads();
  if( tid == 0 ) L.fresh[cand] = s_fresh;
}

// ---- footprints: the distinct scene-active cells of every placement, as sorted lists ------

// Placement k of rs_hip_coverage_footprints: its cloud (n = 0 for a static placement or an empty cloud), its pose and where its
// cells start in FpLaunch::cells — the sum of the n before it: a placement hits no more cells than it has points.
struct FpPlacement { const float4* pos; int n; int pad; long long first; Xform pose; };

struct FpLaunch
{
  VoxGrid grid;
  const uint32_t* scene_bits;
  const FpPlacement* plc;
  int lds_bytes;
  int* count; int* cells;                       // per placement: its number of cells (-1: more cells than points, cannot happen); its cells from plc[k].first
  int* n_overflow; ArrOverflow* overflow;       // written by the LDS route
  const ArrSlabJob* jobs; uint32_t* slab;       // read by the global route
};

#define FP_RUN 16                                // words per thread and trip of the compaction: ARR_BLOCK * FP_RUN words are the whole LDS budget
#define FP_CHUNK ( ARR_BLOCK * FP_RUN )

// the cell of point i of a placement if the scene grid is active there (:363-364 without an arrangement plane), else -1
__device__ __forceinline__ int scene_cell( const FpLaunch& L, const FpPlacement& P, int i )
{
  const float4 p = P.pos[i];
  float x, y, z;
  xform3( P.pose, p.x, p.y, p.z, 1.0f, x, y, z );              // msh_mat4_vec3_mul( pose, p, 1 ), :1101
  const int c = voxel_of( L.grid, x, y, z );
  if( c < 0 ) return -1;
  if( !( L.scene_bits[c >> 5] & ( 1u << ( c & 31 ) ) ) ) return -1;
  return c;
}

// One workgroup per placement, k_extend's skeleton: box of the placement's scene-active cells, the sub-box's bits cleared (LDS, or
// the slab for the placements of L.jobs), one atomicOr per point.  Then the compaction: the sub-box is (y, z, x)-major like the grid's
// own cell index, so its set bits in order ARE the placement's cells in ascending order.  A trip covers FP_CHUNK words: every thread
// popcounts a contiguous run of them, an exclusive scan over the workgroup (DPP wave scan, the four waves' totals through LDS) gives
// its offset, and it writes the global index of each of its set bits from there.  The LDS route needs one trip.
template <bool GLOBAL>
__global__ __launch_bounds__( ARR_BLOCK ) void k_footprint( FpLaunch L )
{
  __shared__ uint32_t s_bits[GLOBAL ? 1 : ARR_LDS_BYTES / 4];
  __shared__ int s_box[6];
  __shared__ uint32_t s_wave[ARR_BLOCK / 64];
  const int tid = threadIdx.x;
  const int k = GLOBAL ? L.jobs[blockIdx.x].cand : (int)blockIdx.x;
  const FpPlacement P = L.plc[k];                              // (uniform: scalar registers)
  const int xz = L.grid.x_res * L.grid.z_res, xr = L.grid.x_res;
  if( tid < 3 ) { s_box[tid] = INT_MAX; s_box[3 + tid] = INT_MIN; }
  __syncthreads();
  int lo[3] = { INT_MAX, INT_MAX, INT_MAX }, hi[3] = { INT_MIN, INT_MIN, INT_MIN };
  for( int i = tid; i < P.n; i += ARR_BLOCK )
  {
    const int c = scene_cell( L, P, i );
    if( c < 0 ) continue;
    const int cy = c / xz, r = c - cy * xz, cz = r / xr, cx = r - cz * xr;          // :108 backwards
    lo[0] = min( lo[0], cx ); hi[0] = max( hi[0], cx ); lo[1] = min( lo[1], cy ); hi[1] = max( hi[1], cy ); lo[2] = min( lo[2], cz ); hi[2] = max( hi[2], cz );
  }
  for( int a = 0; a < 3; ++a ) { lo[a] = wave_min( lo[a] ); hi[a] = wave_max( hi[a] ); }
  if( ( tid & 63 ) == 0 ) for( int a = 0; a < 3; ++a ) { atomicMin( &s_box[a], lo[a] ); atomicMax( &s_box[3 + a], hi[a] ); }
  __syncthreads();
  const int x0 = s_box[0], y0 = s_box[1], z0 = s_box[2];
  if( s_box[3] < x0 ) { if( tid == 0 ) L.count[k] = 0; return; }                     // no scene-active cell (uniform)
  const int sx = s_box[3] - x0 + 1, sy = s_box[4] - y0 + 1, sz = s_box[5] - z0 + 1;
  const unsigned long long words = ( (unsigned long long)sx * sy * sz + 31ull ) >> 5;   // (at most the grid's own plane: below 2^26)
  if( !GLOBAL && words * 4ull > (unsigned long long)L.lds_bytes )
  {
    if( tid == 0 ) { const int slot = atomicAdd( L.n_overflow, 1 ); L.overflow[slot] = ArrOverflow{ k, 0, words }; L.count[k] = 0; }
    return;
  }
  if( GLOBAL && words != L.jobs[blockIdx.x].words ) { if( tid == 0 ) L.count[k] = -2; return; }     // (the same walk over the same plane: cannot differ)
  uint32_t* bits = GLOBAL ? L.slab + L.jobs[blockIdx.x].off : s_bits;
  for( unsigned long long w = tid; w < words; w += ARR_BLOCK ) bits[w] = 0u;
  __syncthreads();
  for( int i = tid; i < P.n; i += ARR_BLOCK )
  {
    const int c = scene_cell( L, P, i );
    if( c < 0 ) continue;
    const int cy = c / xz, r = c - cy * xz, cz = r / xr, cx = r - cz * xr;
    const unsigned long long b = ( (unsigned long long)( cy - y0 ) * sz + ( cz - z0 ) ) * sx + ( cx - x0 );
    atomicOr( bits + ( b >> 5 ), 1u << ( b & 31ull ) );                              // several points in one cell: one bit
  }
  __syncthreads();
  // (the slab's words were written by atomics of other waves: read them where the atomics were made, past this CU's vector cache)
  auto word = [&]( unsigned long long w ) -> uint32_t { return GLOBAL ? __hip_atomic_load( bits + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT ) : bits[w]; };
  const uint32_t sxz = (uint32_t)sx * (uint32_t)sz;
  int* out = L.cells + P.first;
  uint32_t done = 0;                                                                  // cells of the trips before this one
  for( unsigned long long w_base = 0; w_base < words; w_base += FP_CHUNK )            // (uniform)
  {
    const uint32_t span = (uint32_t)min( words - w_base, (unsigned long long)FP_CHUNK );
    const uint32_t per = ( span + ARR_BLOCK - 1 ) / ARR_BLOCK;                        // <= FP_RUN
    const uint32_t w0 = min( (uint32_t)tid * per, span ), w1 = min( w0 + per, span );
    uint32_t mine = 0;
    for( uint32_t w = w0; w < w1; ++w ) mine += __popc( word( w_base + w ) );
    const uint32_t incl = wave_scan( mine, tid & 63 );
    if( ( tid & 63 ) == 63 ) s_wave[tid >> 6] = incl;
    __syncthreads();
    uint32_t o = done + incl - mine, total = 0;
    for( int v = 0; v < ARR_BLOCK / 64; ++v ) { const uint32_t t = s_wave[v]; if( v < ( tid >> 6 ) ) o += t; total += t; }
    for( uint32_t w = w0; w < w1; ++w )
    {
      uint32_t v = word( w_base + w );
      while( v )
      {
        const uint32_t b = (uint32_t)( w_base + w ) * 32u + (uint32_t)( __ffs( v ) - 1 );
        v &= v - 1u;
        const uint32_t dy = b / sxz, r = b - dy * sxz, dz = r / (uint32_t)sx, dx = r - dz * (uint32_t)sx;
        if( o < (uint32_t)P.n ) out[o] = ( y0 + (int)dy ) * xz + ( z0 + (int)dz ) * xr + x0 + (int)dx;     // (never past the placement's own region)
        ++o;
      }
    }
    done += total;
    __syncthreads();                                                                  // (s_wave is written again by the next trip)
  }
  if( tid == 0 ) L.count[k] = done <= (uint32_t)P.n ? (int)done : -1;
}

// The tight CSR: placement k's cells copied from its region of `cells` to tight[ sum of the counts before k ...).  Every workgroup
// sums the counts before its own (a few hundred placements: one or two trips); a negative count (an overflowed placement's 0 is
// not one) copies nothing.
__global__ __launch_bounds__( ARR_BLOCK ) void k_footprint_pack( const FpPlacement* plc, const int* count, const int* cells, int* tight )
{
  __shared__ long long s_before[ARR_BLOCK / 64];
  const int k = blockIdx.x, tid = threadIdx.x;
  long long before = 0;
  for( int j = tid; j < k; j += ARR_BLOCK ) before += max( count[j], 0 );
  for( int o = 32; o; o >>= 1 ) before += __shfl_xor( before, o, 64 );
  if( ( tid & 63 ) == 0 ) s_before[tid >> 6] = before;
  __syncthreads();
  before = 0;
  for( int v = 0; v < ARR_BLOCK / 64; ++v ) before += s_before[v];
  const int n = min( count[k], plc[k].n );
  const int* src = cells + plc[k].first;
  for( int i = tid; i < n; i += ARR_BLOCK ) tight[before + i] = src[i];
}

// ------------------------------------------------------------------------------------------

// The calling thread's buffers, grown on demand and kept between calls (a base plane, the placements, the footprints' cells, and a
// slab of up to ARR_SLAB_BYTES once a call took the global route).  No destructor frees them (rs_host.h: Buf); a thread that ends
// while the process goes on gives them back with rs_hip_arrange_release().
struct ArrWorkspace
{
  Buf props, bits, pos, cls, quality, base, plc, out, over, jobs, slab, fp_cells, fp_tight, h_in{ nullptr, 0, true }, h_out{ nullptr, 0, true };
  hipError_t release()
  {
    hipError_t first = hipSuccess;
    for( Buf* b : { &props, &bits, &pos, &cls, &quality, &base, &plc, &out, &over, &jobs, &slab, &fp_cells, &fp_tight, &h_in, &h_out } )
    {
      const hipError_t e = b->release();
      if( first == hipSuccess ) first = e;
    }
    return first;
  }
};
thread_local ArrWorkspace g_arr_ws;
// process-wide, read and written by any calling thread
std::atomic<int> g_arr_lds_bytes{ ARR_LDS_BYTES };
std::atomic<int64_t> g_arr_lds_route{ 0 }, g_arr_slab_route{ 0 }, g_fp_lds_route{ 0 }, g_fp_slab_route{ 0 };

// The device part of rs_hip_coverage_footprints, arguments checked by its caller: offsets (n + 1) and the cells of every placement.
// Stream order of the LDS route: upload, k_footprint<false>, k_footprint_pack, read-back 1 (overflow count and counts), read-back
// 2 (the tight cells, whose number read-back 1 told).  Overflowed placements count 0 in the first launch; with any of them the
// overflow list is read, k_footprint<true> fills their regions, and the pack and the two read-backs are made again.
int footprints_device( rs_hip_coverage_t* c, const rs_hip_cloud_t* const* objects, const float* poses, const int32_t* is_static, int32_t n,
                       std::vector<int64_t>& offsets, std::vector<int32_t>& cells )
{
  offsets.assign( (size_t)n + 1, 0 ); cells.clear();
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  if( n == 0 ) return RS_HIP_OK;
  ArrWorkspace& W = g_arr_ws;
  std::vector<FpPlacement> plc( (size_t)n );
  long long total = 0;
  for( int32_t k = 0; k < n; ++k )
  {
    FpPlacement p{}; p.first = total;
    if( !is_static[k] )                                          // :1095-1096
    {
      const GridView* v = api_cloud_view( objects[k] );
      if( v->n > 0 ) { p.pos = v->pos; p.n = v->n; }
    }
    std::memcpy( p.pose.m, poses + 16 * (size_t)k, 64 );
    plc[k] = p; total += p.n;
  }
  // device words of a call: [0] placements on the overflow list, [1] unused, [2 ..) cells per placement
  const size_t out_ints = 2 + (size_t)n, cell_bytes = std::max<size_t>( 1, (size_t)total ) * 4;
  RS_TRY_DRAIN( st, W.out.ensure( out_ints * 4 ), "coverage_footprints: buffers" );
  RS_TRY_DRAIN( st, W.over.ensure( (size_t)n * sizeof(ArrOverflow) ), "coverage_footprints: buffers" );
  RS_TRY_DRAIN( st, W.plc.ensure( (size_t)n * sizeof(FpPlacement) ), "coverage_footprints: buffers" );
  RS_TRY_DRAIN( st, W.fp_cells.ensure( cell_bytes ), "coverage_footprints: buffers" );
  RS_TRY_DRAIN( st, W.fp_tight.ensure( cell_bytes ), "coverage_footprints: buffers" );
  RS_TRY_DRAIN( st, W.h_in.ensure( (size_t)n * sizeof(FpPlacement) ), "coverage_footprints: buffers" );
  RS_TRY_DRAIN( st, W.h_out.ensure( out_ints * 4 + 8 + (size_t)n * sizeof(ArrOverflow) ), "coverage_footprints: buffers" );
  RS_TRY_DRAIN( st, hipMemsetAsync( W.out.p, 0, 8, st ), "coverage_footprints: clear" );
  std::memcpy( W.h_in.p, plc.data(), (size_t)n * sizeof(FpPlacement) );
  RS_TRY_DRAIN( st, hipMemcpyAsync( W.plc.p, W.h_in.p, (size_t)n * sizeof(FpPlacement), hipMemcpyHostToDevice, st ), "coverage_footprints: upload" );
  int* d_out = (int*)W.out.p;
  FpLaunch L{};
  L.grid = c->grid; L.scene_bits = c->d_bits; L.plc = (const FpPlacement*)W.plc.p; L.lds_bytes = g_arr_lds_bytes.load();
  L.count = d_out + 2; L.cells = (int*)W.fp_cells.p; L.n_overflow = d_out; L.overflow = (ArrOverflow*)W.over.p;
  int* h_out = (int*)W.h_out.p;
  // the pack, read-back 1 and, once every count is final, read-back 2
  auto pack_and_read = [&]( bool final ) -> int
  {
    {
      ProfSpan span( "footprints" );
      hipLaunchKernelGGL( k_footprint_pack, dim3( (unsigned)n ), dim3( ARR_BLOCK ), 0, st, L.plc, (const int*)L.count, (const int*)L.cells, (int*)W.fp_tight.p );
    }
    RS_TRY_DRAIN( st, hipGetLastError(), "coverage_footprints: launch" );
    RS_TRY_DRAIN( st, hipMemcpyAsync( h_out, d_out, out_ints * 4, hipMemcpyDeviceToHost, st ), "coverage_footprints: download" );
    RS_TRY_DRAIN( st, hipStreamSynchronize( st ), "coverage_footprints" );
    if( !final && h_out[0] != 0 ) return RS_HIP_OK;              // (the slab route comes first)
    for( int32_t k = 0; k < n; ++k )
    {
      const int cnt = h_out[2 + k];
      if( cnt == -2 ) return fail( RS_HIP_E_RUNTIME, "coverage_footprints: a sub-box changed between the two routes" );
      if( cnt < 0 || cnt > plc[k].n ) return fail( RS_HIP_E_RUNTIME, "coverage_footprints: a placement with more cells than points" );
      offsets[(size_t)k + 1] = offsets[k] + cnt;
    }
    cells.resize( (size_t)offsets[n] );
    if( !cells.empty() )
    {
      RS_TRY_DRAIN( st, hipMemcpyAsync( cells.data(), W.fp_tight.p, cells.size() * 4, hipMemcpyDeviceToHost, st ), "coverage_footprints: download" );
      RS_TRY_DRAIN( st, hipStreamSynchronize( st ), "coverage_footprints" );
    }
    return RS_HIP_OK;
  };
  {
    ProfSpan span( "footprints" );
    hipLaunchKernelGGL( k_footprint<false>, dim3( (unsigned)n ), dim3( ARR_BLOCK ), 0, st, L );
  }
  rc = pack_and_read( false ); if( rc ) return rc;
  const int n_over = h_out[0];
  if( n_over < 0 || n_over > n ) return fail( RS_HIP_E_RUNTIME, "coverage_footprints: overflow list out of range" );
  if( n_over > 0 )
  {
    ArrOverflow* ho = (ArrOverflow*)( h_out + out_ints + ( out_ints & 1 ) );
    RS_TRY_DRAIN( st, hipMemcpyAsync( ho, W.over.p, (size_t)n_over * sizeof(ArrOverflow), hipMemcpyDeviceToHost, st ), "coverage_footprints: download" );
    RS_TRY_DRAIN( st, hipStreamSynchronize( st ), "coverage_footprints" );
    std::sort( ho, ho + n_over, []( const ArrOverflow& a, const ArrOverflow& b ) { return a.cand < b.cand; } );       // (the list's order is the workgroups')
    std::vector<ArrSlabJob> jobs( n_over );
    std::vector<std::pair<int, int>> chunks;                       // launches of at most ARR_SLAB_BYTES of sub-boxes
    size_t slab_words = 0;
    for( int i = 0; i < n_over; )
    {
      size_t used = 0; int j = i;
      while( j < n_over && ( j == i || ( used + ho[j].words ) * 4 <= ARR_SLAB_BYTES ) )
      {
        if( ho[j].cand < 0 || ho[j].cand >= n || ho[j].words > (unsigned long long)c->n_words ) return fail( RS_HIP_E_RUNTIME, "coverage_footprints: overflow entry out of range" );
        jobs[j] = ArrSlabJob{ ho[j].cand, 0, used, ho[j].words }; used += ho[j].words; ++j;
      }
      chunks.emplace_back( i, j ); slab_words = std::max( slab_words, used ); i = j;
    }
    RS_TRY_DRAIN( st, W.slab.ensure( slab_words * 4 ), "coverage_footprints: scratch slab" );
    RS_TRY_DRAIN( st, W.jobs.ensure( jobs.size() * sizeof(ArrSlabJob) ), "coverage_footprints: buffers" );
    RS_TRY_DRAIN( st, hipMemcpyAsync( W.jobs.p, jobs.data(), jobs.size() * sizeof(ArrSlabJob), hipMemcpyHostToDevice, st ), "coverage_footprints: upload" );
    L.slab = (uint32_t*)W.slab.p;
    {
      ProfSpan span( "footprints" );
      for( const auto& ch : chunks )
      {
        L.jobs = (const ArrSlabJob*)W.jobs.p + ch.first;
        hipLaunchKernelGGL( k_footprint<true>, dim3( (unsigned)( ch.second - ch.first ) ), dim3( ARR_BLOCK ), 0, st, L );
      }
    }
    rc = pack_and_read( true ); if( rc ) return rc;                // (its first synchronisation also keeps `jobs` alive until the upload is done)
  }
  g_fp_lds_route += n - n_over; g_fp_slab_route += n_over;
  return RS_HIP_OK;
}

} // namespace

// rs_hip_coverage_footprints' result, or the same from arrays: host memory only.  `dense` holds every cell as its rank among the
// set's distinct cells, so that a union is counted on a stamp array as long as that set, not as the grid: rs_hip_footprints_scores
// marks a cell with the arrangement's epoch and counts the first mark; nothing is cleared between arrangements.
struct rs_hip_footprints
{
  int64_t n_cells = 0, valid = 0;
  std::vector<int64_t> offsets{ 0 };
  std::vector<int32_t> cells, dense;
  std::vector<uint32_t> stamp;
  uint32_t epoch = 0;
  void index()
  {
    std::vector<int32_t> u( cells );
    std::sort( u.begin(), u.end() );
    u.erase( std::unique( u.begin(), u.end() ), u.end() );
    dense.resize( cells.size() );
    for( size_t i = 0; i < cells.size(); ++i ) dense[i] = (int32_t)( std::lower_bound( u.begin(), u.end(), cells[i] ) - u.begin() );
    stamp.assign( u.size(), 0u ); epoch = 0;
  }
};

extern "C" {

int rs_hip_voxel_grid_shape( const float bbox_min[3], const float bbox_max[3], float voxel_size, int32_t res[3], float origin[3], int64_t* n_cells )
{
  if( !bbox_min || !bbox_max || !( voxel_size > 0.0f ) ) return fail( RS_HIP_E_ARG, "voxel_grid_shape: bad arguments" );
  VoxGrid g{};
  if( !vox_grid_init( bbox_min, bbox_max, voxel_size, g, nullptr ) ) return fail( RS_HIP_E_CAPACITY, "voxel_grid_shape: the cells do not fit the reference's int32 cell index" );
  if( res ) { res[0] = g.x_res; res[1] = g.y_res; res[2] = g.z_res; }
  if( origin ) { origin[0] = g.ox; origin[1] = g.oy; origin[2] = g.oz; }
  if( n_cells ) *n_cells = g.n_cells;
  return RS_HIP_OK;
}

int rs_hip_scene_saliency( const float bbox_min[3], const float bbox_max[3], float voxel_size,
                           const rs_hip_cloud_t* const* objects, int32_t n_objects,
                           const int32_t* prop_object, const float* prop_poses, const int32_t* prop_static, int32_t n_props,
                           const float* scene_pos, const int32_t* scene_class, int64_t n_scene,
                           int32_t wall_class, int32_t floor_class, float* quality, uint8_t* grid, int64_t grid_capacity )
{
  if( !bbox_min || !bbox_max || !( voxel_size > 0.0f ) || n_objects < 0 || n_props < 0 || n_scene < 0 ||
      ( n_props > 0 && ( !objects || !prop_object || !prop_poses || !prop_static ) ) || ( n_scene > 0 && ( !scene_pos || !scene_class || !quality ) ) )
    return fail( RS_HIP_E_ARG, "scene_saliency: bad arguments" );
  for( int32_t k = 0; k < n_props; ++k )
    if( prop_object[k] < 0 || prop_object[k] >= n_objects || !objects[prop_object[k]] )
    {
      char msg[128]; snprintf( msg, sizeof(msg), "scene_saliency: proposal %d names an object outside [0, %d) or without a cloud", k, n_objects );
      return fail( RS_HIP_E_ARG, msg );
    }
  VoxGrid g{};
  if( !vox_grid_init( bbox_min, bbox_max, voxel_size, g, nullptr ) ) return fail( RS_HIP_E_CAPACITY, "scene_saliency: the cells do not fit the reference's int32 cell index" );
  if( grid && grid_capacity < (int64_t)g.n_cells ) return fail( RS_HIP_E_CAPACITY, "scene_saliency: the grid array is smaller than the grid (rs_hip_voxel_grid_shape)" );
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  ArrWorkspace& W = g_arr_ws;
  // the proposals of the two phases, dynamic ones first (:1126-1131)
  std::vector<ArrProposal> props; props.reserve( n_props );
  int n_dyn = 0, max_pts[2] = { 0, 0 };
  for( int phase = 0; phase < 2; ++phase )
    for( int32_t k = 0; k < n_props; ++k )
    {
      if( ( prop_static[k] != 0 ) != ( phase == 1 ) ) continue;
      const GridView* v = api_cloud_view( objects[prop_object[k]] );
      if( v->n <= 0 ) continue;
      ArrProposal P{}; P.pos = v->pos; P.n = v->n; std::memcpy( P.pose.m, prop_poses + 16 * (size_t)k, 64 );
      props.push_back( P ); max_pts[phase] = std::max( max_pts[phase], v->n );
      if( phase == 0 ) ++n_dyn;
    }
  const size_t n_words = ( (size_t)g.n_cells + 31 ) / 32;
  RS_TRY_DRAIN( st, W.bits.ensure( n_words * 4 ), "scene_saliency: buffers" );
  RS_TRY_DRAIN( st, hipMemsetAsync( W.bits.p, 0, n_words * 4, st ), "scene_saliency: clear" );              // isect_grid3d_init's memset (intersect.h:74)
  if( !props.empty() )
  {
    RS_TRY_DRAIN( st, W.props.ensure( props.size() * sizeof(ArrProposal) ), "scene_saliency: buffers" );
    RS_TRY_DRAIN( st, W.h_in.ensure( props.size() * sizeof(ArrProposal) ), "scene_saliency: buffers" );
    std::memcpy( W.h_in.p, props.data(), props.size() * sizeof(ArrProposal) );
    RS_TRY_DRAIN( st, hipMemcpyAsync( W.props.p, W.h_in.p, props.size() * sizeof(ArrProposal), hipMemcpyHostToDevice, st ), "scene_saliency: upload" );
  }
  if( n_scene > 0 )
  {
    RS_TRY_DRAIN( st, W.pos.ensure( (size_t)n_scene * 12 ), "scene_saliency: buffers" );
    RS_TRY_DRAIN( st, W.cls.ensure( (size_t)n_scene * 4 ), "scene_saliency: buffers" );
    RS_TRY_DRAIN( st, W.quality.ensure( (size_t)n_scene * 4 ), "scene_saliency: buffers" );
    RS_TRY_DRAIN( st, hipMemcpyAsync( W.pos.p, scene_pos, (size_t)n_scene * 12, hipMemcpyHostToDevice, st ), "scene_saliency: upload" );
    RS_TRY_DRAIN( st, hipMemcpyAsync( W.cls.p, scene_class, (size_t)n_scene * 4, hipMemcpyHostToDevice, st ), "scene_saliency: upload" );
  }
  {
    ProfSpan span( "saliency" );
    const int n_phase[2] = { n_dyn, (int)props.size() - n_dyn };
    for( int phase = 0; phase < 2; ++phase )
    {
      const int bx = std::max( 1, std::min( 64, ( max_pts[phase] + ARR_BLOCK - 1 ) / ARR_BLOCK ) );
      for( int first = 0; first < n_phase[phase]; first += ARR_MAX_GRID_Y )          // (any number of proposals: launches of at most 65535)
        hipLaunchKernelGGL( k_saliency_raster, dim3( bx, std::min( ARR_MAX_GRID_Y, n_phase[phase] - first ) ), dim3( ARR_BLOCK ), 0, st, g,
                            (const ArrProposal*)W.props.p + ( phase ? n_dyn : 0 ) + first, phase == 0 ? 1 : 0, (uint32_t*)W.bits.p );
    }
    if( n_scene > 0 )
      hipLaunchKernelGGL( k_saliency_lookup, dim3( blocks_for( n_scene, ARR_BLOCK ) ), dim3( ARR_BLOCK ), 0, st, g,
                          (const float*)W.pos.p, (const int*)W.cls.p, (long long)n_scene, (int)wall_class, (int)floor_class, (const uint32_t*)W.bits.p, (float*)W.quality.p );
  }
  RS_TRY_DRAIN( st, hipGetLastError(), "scene_saliency: launch" );
  if( n_scene > 0 ) RS_TRY_DRAIN( st, hipMemcpyAsync( quality, W.quality.p, (size_t)n_scene * 4, hipMemcpyDeviceToHost, st ), "scene_saliency: download" );
  std::vector<uint32_t> hb;
  if( grid ) { hb.resize( n_words ); RS_TRY_DRAIN( st, hipMemcpyAsync( hb.data(), W.bits.p, n_words * 4, hipMemcpyDeviceToHost, st ), "scene_saliency: download" ); }
  RS_TRY_DRAIN( st, hipStreamSynchronize( st ), "scene_saliency" );       // (also keeps the caller's arrays and `hb` in use until the copies are done)
  if( grid ) for( int i = 0; i < g.n_cells; ++i ) grid[i] = ( hb[(size_t)i >> 5] >> ( i & 31 ) ) & 1u;      // 1 = RSAO_CELL_ACTIVE
  return RS_HIP_OK;
}

int rs_hip_coverage_extensions( rs_hip_coverage_t* c,
                                const rs_hip_cloud_t* const* base_objects, const float* base_poses, const int32_t* base_static, int32_t n_base,
                                const rs_hip_cloud_t* const* cand_objects, const float* cand_poses, int32_t n_cand,
                                float* scores, int32_t* agree, int32_t* base_agree )
{
  if( !c || n_base < 0 || n_cand < 0 || ( n_base > 0 && ( !base_objects || !base_poses || !base_static ) ) ||
      ( n_cand > 0 && ( !cand_objects || !cand_poses || !scores ) ) )
    return fail( RS_HIP_E_ARG, "coverage_extensions: bad arguments" );
  for( int32_t k = 0; k < n_base; ++k )
    if( !base_static[k] && !base_objects[k] )
    {
      char msg[128]; snprintf( msg, sizeof(msg), "coverage_extensions: base placement %d has no object cloud", k );
      return fail( RS_HIP_E_ARG, msg );
    }
  for( int32_t k = 0; k < n_cand; ++k )
    if( !cand_objects[k] )
    {
      char msg[128]; snprintf( msg, sizeof(msg), "coverage_extensions: candidate %d has no object cloud", k );
      return fail( RS_HIP_E_ARG, msg );
    }
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  ArrWorkspace& W = g_arr_ws;
  // placements: the base's non-static ones (:1095-1096), then the candidates
  std::vector<CoveragePlacement> plc; plc.reserve( (size_t)n_base + n_cand );
  int base_max = 0;
  for( int32_t k = 0; k < n_base; ++k )
  {
    if( base_static[k] ) continue;
    const GridView* v = api_cloud_view( base_objects[k] );
    if( v->n <= 0 ) continue;
    CoveragePlacement p{}; p.pos = v->pos; p.n = v->n; p.arrangement = 0; std::memcpy( p.pose.m, base_poses + 16 * (size_t)k, 64 );
    plc.push_back( p ); base_max = std::max( base_max, v->n );
  }
  const size_t n_base_plc = plc.size();
  for( int32_t k = 0; k < n_cand; ++k )
  {
    const GridView* v = api_cloud_view( cand_objects[k] );
    CoveragePlacement p{}; p.pos = v->pos; p.n = v->n; p.arrangement = 0; std::memcpy( p.pose.m, cand_poses + 16 * (size_t)k, 64 );
    plc.push_back( p );
  }
  // device words of a call: [0] agree( base ), [1] candidates on the overflow list, [2 ..) fresh per candidate
  const size_t out_ints = 2 + (size_t)n_cand, plane_bytes = (size_t)c->n_words * 4;
  RS_TRY_DRAIN( st, W.base.ensure( plane_bytes ), "coverage_extensions: buffers" );
  RS_TRY_DRAIN( st, W.out.ensure( out_ints * 4 ), "coverage_extensions: buffers" );
  RS_TRY_DRAIN( st, W.over.ensure( std::max<size_t>( 1, n_cand ) * sizeof(ArrOverflow) ), "coverage_extensions: buffers" );
  RS_TRY_DRAIN( st, W.plc.ensure( std::max<size_t>( 1, plc.size() ) * sizeof(CoveragePlacement) ), "coverage_extensions: buffers" );
  RS_TRY_DRAIN( st, W.h_in.ensure( std::max<size_t>( 1, plc.size() ) * sizeof(CoveragePlacement) ), "coverage_extensions: buffers" );
  RS_TRY_DRAIN( st, W.h_out.ensure( out_ints * 4 + 8 + std::max<size_t>( 1, n_cand ) * sizeof(ArrOverflow) ), "coverage_extensions: buffers" );
  RS_TRY_DRAIN( st, hipMemsetAsync( W.base.p, 0, plane_bytes, st ), "coverage_extensions: clear" );          // ONE plane per call (:1089)
  RS_TRY_DRAIN( st, hipMemsetAsync( W.out.p, 0, 8, st ), "coverage_extensions: clear" );
  if( !plc.empty() )
  {
    std::memcpy( W.h_in.p, plc.data(), plc.size() * sizeof(CoveragePlacement) );
    RS_TRY_DRAIN( st, hipMemcpyAsync( W.plc.p, W.h_in.p, plc.size() * sizeof(CoveragePlacement), hipMemcpyHostToDevice, st ), "coverage_extensions: upload" );
  }
  int* d_out = (int*)W.out.p;
  ExtLaunch L{};
  L.grid = c->grid; L.scene_bits = c->d_bits; L.base_bits = (const uint32_t*)W.base.p;
  L.cand = (const CoveragePlacement*)W.plc.p + n_base_plc; L.lds_bytes = g_arr_lds_bytes.load();
  L.fresh = d_out + 2; L.n_overflow = d_out + 1; L.overflow = (ArrOverflow*)W.over.p;
  {
    ProfSpan span( "coverage" );
    if( n_base_plc )
    {
      CoverageLaunch B{};
      B.grid = c->grid; B.scene_bits = c->d_bits; B.arr_bits = (uint32_t*)W.base.p; B.n_words = c->n_words;
      B.plc = (const CoveragePlacement*)W.plc.p; B.n_plc = (int)n_base_plc; B.max_pts = base_max; B.agree = d_out;
      launch_coverage( B, st );
    }
    if( n_cand > 0 ) hipLaunchKernelGGL( k_extend<false>, dim3( (unsigned)n_cand ), dim3( ARR_BLOCK ), 0, st, L );
  }
  RS_TRY_DRAIN( st, hipGetLastError(), "coverage_extensions: launch" );
  int* h_out = (int*)W.h_out.p;
  RS_TRY_DRAIN( st, hipMemcpyAsync( h_out, d_out, out_ints * 4, hipMemcpyDeviceToHost, st ), "coverage_extensions: download" );
  RS_TRY_DRAIN( st, hipStreamSynchronize( st ), "coverage_extensions" );
  const int n_over = h_out[1];
  if( n_over < 0 || n_over > n_cand ) return fail( RS_HIP_E_RUNTIME, "coverage_extensions: overflow list out of range" );
  if( n_over > 0 )
  {
    ArrOverflow* ho = (ArrOverflow*)( h_out + out_ints + ( out_ints & 1 ) );
    RS_TRY_DRAIN( st, hipMemcpyAsync( ho, W.over.p, (size_t)n_over * sizeof(ArrOverflow), hipMemcpyDeviceToHost, st ), "coverage_extensions: download" );
    RS_TRY_DRAIN( st, hipStreamSynchronize( st ), "coverage_extensions" );
    std::sort( ho, ho + n_over, []( const ArrOverflow& a, const ArrOverflow& b ) { return a.cand < b.cand; } );       // (the list's order is the workgroups')
    std::vector<ArrSlabJob> jobs( n_over );
    std::vector<std::pair<int, int>> chunks;                       // launches of at most ARR_SLAB_BYTES of sub-boxes
    size_t slab_words = 0;
    for( int i = 0; i < n_over; )
    {
      size_t used = 0; int j = i;
      while( j < n_over && ( j == i || ( used + ho[j].words ) * 4 <= ARR_SLAB_BYTES ) )
      {
        if( ho[j].cand < 0 || ho[j].cand >= n_cand || ho[j].words > (unsigned long long)c->n_words ) return fail( RS_HIP_E_RUNTIME, "coverage_extensions: overflow entry out of range" );
        jobs[j] = ArrSlabJob{ ho[j].cand, 0, used, ho[j].words }; used += ho[j].words; ++j;
      }
      chunks.emplace_back( i, j ); slab_words = std::max( slab_words, used ); i = j;
    }
    RS_TRY_DRAIN( st, W.slab.ensure( slab_words * 4 ), "coverage_extensions: scratch slab" );
    RS_TRY_DRAIN( st, W.jobs.ensure( jobs.size() * sizeof(ArrSlabJob) ), "coverage_extensions: buffers" );
    RS_TRY_DRAIN( st, hipMemcpyAsync( W.jobs.p, jobs.data(), jobs.size() * sizeof(ArrSlabJob), hipMemcpyHostToDevice, st ), "coverage_extensions: upload" );
    L.slab = (uint32_t*)W.slab.p;
    {
      ProfSpan span( "coverage" );
      for( const auto& ch : chunks )
      {
        L.jobs = (const ArrSlabJob*)W.jobs.p + ch.first;
        hipLaunchKernelGGL( k_extend<true>, dim3( (unsigned)( ch.second - ch.first ) ), dim3( ARR_BLOCK ), 0, st, L );
      }
    }
    RS_TRY_DRAIN( st, hipGetLastError(), "coverage_extensions: launch" );
    RS_TRY_DRAIN( st, hipMemcpyAsync( h_out, d_out, out_ints * 4, hipMemcpyDeviceToHost, st ), "coverage_extensions: download" );
    RS_TRY_DRAIN( st, hipStreamSynchronize( st ), "coverage_extensions" );      // (also keeps `jobs` alive until the upload is done)
  }
  g_arr_lds_route += n_cand - n_over; g_arr_slab_route += n_over;
  const int base_cnt = h_out[0];
  for( int32_t k = 0; k < n_cand; ++k )
  {
    if( h_out[2 + k] < 0 ) return fail( RS_HIP_E_RUNTIME, "coverage_extensions: a sub-box changed between the two routes" );
    const int cnt = base_cnt + h_out[2 + k];
    float s = (float)cnt / (float)c->valid;                      // :366
    if( c->valid == 0 ) s = 0.0f;                                // :367
    scores[k] = s;
    if( agree ) agree[k] = cnt;
  }
  if( base_agree ) *base_agree = base_cnt;
  return RS_HIP_OK;
}

int32_t rs_hip_coverage_lds_budget( int32_t bytes )
{
  if( bytes < 0 ) return g_arr_lds_bytes.load();
  return g_arr_lds_bytes.exchange( std::min( bytes, (int32_t)ARR_LDS_BYTES ) );
}

int rs_hip_arrange_release( void )
{
  ArrWorkspace& W = g_arr_ws;
  bool any = false;
  for( const Buf* b : { &W.props, &W.bits, &W.pos, &W.cls, &W.quality, &W.base, &W.plc, &W.out, &W.over, &W.jobs, &W.slab, &W.fp_cells, &W.fp_tight, &W.h_in, &W.h_out } ) any = any || b->p;
  if( !any ) return RS_HIP_OK;                                   // (nothing held: no device is touched)
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  hipError_t e = hipStreamSynchronize( st );                     // (both calls return drained; a caller's own stream work may not be)
  const hipError_t f = W.release();
  if( e == hipSuccess ) e = f;
  return e == hipSuccess ? RS_HIP_OK : fail( RS_HIP_E_RUNTIME, "arrange_release", e );
}

void rs_hip_coverage_extension_routes( int64_t* lds, int64_t* slab, int32_t reset )
{
  if( lds ) *lds = reset ? g_arr_lds_route.exchange( 0 ) : g_arr_lds_route.load();
  if( slab ) *slab = reset ? g_arr_slab_route.exchange( 0 ) : g_arr_slab_route.load();
  if( reset && !lds ) g_arr_lds_route = 0;
  if( reset && !slab ) g_arr_slab_route = 0;
}

rs_hip_footprints_t* rs_hip_coverage_footprints( rs_hip_coverage_t* c, const rs_hip_cloud_t* const* objects, const float* poses,
                                                 const int32_t* is_static, int32_t n_placements )
{
  if( !c || n_placements < 0 || ( n_placements > 0 && ( !objects || !poses || !is_static ) ) )
  { fail( RS_HIP_E_ARG, "coverage_footprints: bad arguments" ); return nullptr; }
  for( int32_t k = 0; k < n_placements; ++k )
    if( !is_static[k] && !objects[k] )
    {
      char msg[128]; snprintf( msg, sizeof(msg), "coverage_footprints: placement %d has no object cloud", k );
      fail( RS_HIP_E_ARG, msg ); return nullptr;
    }
  hipStream_t st = nullptr;
  if( api_ready( &st ) ) return nullptr;                         // (no device: its error text stands; the handle is not read before)
  rs_hip_footprints_t* f = new rs_hip_footprints_t();
  f->n_cells = c->grid.n_cells; f->valid = c->valid;
  if( footprints_device( c, objects, poses, is_static, n_placements, f->offsets, f->cells ) ) { delete f; return nullptr; }
  f->index();
  return f;
}

rs_hip_footprints_t* rs_hip_footprints_from_arrays( int64_t n_cells, int64_t valid_cells, const int64_t* offsets, const int32_t* cells, int32_t n_placements )
{
  if( n_cells < 0 || valid_cells < 0 || valid_cells > n_cells || n_placements < 0 || !offsets || offsets[0] != 0 )
  { fail( RS_HIP_E_ARG, "footprints_from_arrays: bad arguments" ); return nullptr; }
  if( n_cells > 2000000000ll ) { fail( RS_HIP_E_CAPACITY, "footprints_from_arrays: the cells do not fit the reference's int32 cell index" ); return nullptr; }
  for( int32_t k = 0; k < n_placements; ++k )
    if( offsets[k + 1] < offsets[k] )
    {
      char msg[128]; snprintf( msg, sizeof(msg), "footprints_from_arrays: the offsets decrease at placement %d", k );
      fail( RS_HIP_E_ARG, msg ); return nullptr;
    }
  if( offsets[n_placements] > 0 && !cells ) { fail( RS_HIP_E_ARG, "footprints_from_arrays: bad arguments" ); return nullptr; }
  for( int32_t k = 0; k < n_placements; ++k )
    for( int64_t i = offsets[k]; i < offsets[k + 1]; ++i )
      if( cells[i] < 0 || cells[i] >= n_cells || ( i > offsets[k] && cells[i] <= cells[i - 1] ) )
      {
        char msg[160]; snprintf( msg, sizeof(msg), "footprints_from_arrays: placement %d: cell %d at %lld is outside the grid, or not above the cell before it", k, cells[i], (long long)i );
        fail( RS_HIP_E_ARG, msg ); return nullptr;
      }
  rs_hip_footprints_t* f = new rs_hip_footprints_t();
  f->n_cells = n_cells; f->valid = valid_cells;
  f->offsets.assign( offsets, offsets + n_placements + 1 );
  if( offsets[n_placements] > 0 ) f->cells.assign( cells, cells + offsets[n_placements] );
  f->index();
  return f;
}

void rs_hip_footprints_destroy( rs_hip_footprints_t* f ) { delete f; }

int rs_hip_footprints_info( const rs_hip_footprints_t* f, int32_t* n_placements, int64_t* n_cells, int64_t* valid_cells, int64_t* total_cells )
{
  if( !f ) return fail( RS_HIP_E_ARG, "footprints_info: null handle" );
  if( n_placements ) *n_placements = (int32_t)( f->offsets.size() - 1 );
  if( n_cells ) *n_cells = f->n_cells;
  if( valid_cells ) *valid_cells = f->valid;
  if( total_cells ) *total_cells = f->offsets.back();
  return RS_HIP_OK;
}

int rs_hip_footprints_arrays( const rs_hip_footprints_t* f, int64_t* offsets, int32_t* cells )
{
  if( !f || !offsets || ( !cells && !f->cells.empty() ) ) return fail( RS_HIP_E_ARG, "footprints_arrays: bad arguments" );
  std::memcpy( offsets, f->offsets.data(), f->offsets.size() * sizeof(int64_t) );
  if( !f->cells.empty() ) std::memcpy( cells, f->cells.data(), f->cells.size() * sizeof(int32_t) );
  return RS_HIP_OK;
}

int rs_hip_footprints_scores( rs_hip_footprints_t* f, const int32_t* members, const int32_t* first, int32_t n_arrangements, float* scores, int32_t* agree )
{
  if( !f || n_arrangements < 0 || ( n_arrangements > 0 && ( !first || !scores ) ) ) return fail( RS_HIP_E_ARG, "footprints_scores: bad arguments" );
  if( n_arrangements == 0 ) return RS_HIP_OK;
  const int32_t n = (int32_t)( f->offsets.size() - 1 );
  if( first[0] < 0 || ( first[n_arrangements] > first[0] && !members ) ) return fail( RS_HIP_E_ARG, "footprints_scores: bad arguments" );
  for( int32_t a = 0; a < n_arrangements; ++a )
  {
    if( first[a + 1] < first[a] ) return fail( RS_HIP_E_ARG, "footprints_scores: the arrangements' first members decrease" );
    for( int32_t i = first[a]; i < first[a + 1]; ++i )
      if( members[i] < 0 || members[i] >= n )
      {
        char msg[128]; snprintf( msg, sizeof(msg), "footprints_scores: arrangement %d names member %d outside [0, %d)", a, members[i], n );
        return fail( RS_HIP_E_ARG, msg );
      }
  }
  const int32_t* dense = f->dense.data(); const int64_t* off = f->offsets.data(); uint32_t* stamp = f->stamp.data();
  for( int32_t a = 0; a < n_arrangements; ++a )
  {
    if( ++f->epoch == 0u ) { std::fill( f->stamp.begin(), f->stamp.end(), 0u ); f->epoch = 1u; }     // (once in 2^32 arrangements)
    const uint32_t e = f->epoch;
    int32_t cnt = 0;
    for( int32_t i = first[a]; i < first[a + 1]; ++i )
      for( int64_t j = off[members[i]], end = off[members[i] + 1]; j < end; ++j )
        if( stamp[dense[j]] != e ) { stamp[dense[j]] = e; ++cnt; }                     // a cell of several members, or of a repeated one, counts once
    float s = (float)cnt / (float)f->valid;                        // :366
    if( f->valid == 0 ) s = 0.0f;                                  // :367
    scores[a] = s;
    if( agree ) agree[a] = cnt;
  }
  return RS_HIP_OK;
}

void rs_hip_coverage_footprint_routes( int64_t* lds, int64_t* slab, int32_t reset )
{
  if( lds ) *lds = reset ? g_fp_lds_route.exchange( 0 ) : g_fp_lds_route.load();
  if( slab ) *slab = reset ? g_fp_slab_route.exchange( 0 ) : g_fp_slab_route.load();
  if( reset && !lds ) g_fp_lds_route = 0;
  if( reset && !slab ) g_fp_slab_route = 0;
}

} // extern "C"
