// librescan_hip k-nearest search (gfx950, wave64) — msh_hash_grid_knn_search (lib/msh/msh_hash_grid.h:1291-1447) on the device.
//
// The reference's k-NN is NOT an exact k-nearest search: it walks the bins of ITS OWN grid (geometry from the init radius, the
// bounding box grown by 1e-4, bins by truncation: :413-449,471-475) shell by shell around the query's bin, skips a bin whose lower
// bound is beyond the k-th distance held after the previous shell, and stops one shell after k points are held.  The shim's host
// restatement (KnnGrid, rs_dropin.cpp) pins those semantics; this file computes the same rows:
//   * rs_hip_knn_grid_create: the grid's geometry on the host from the cloud's box (a device min / max reduction — exact), then the
//     cloud's {x, y, z, index} records, already in HBM, ordered by bin with a counting sort (histogram -> scan -> scatter) plus a
//     w h d + 1 offset table.  Nothing is copied back to the host.
//   * k_knn: one wave per query.  The wave holds the 64 smallest keys (bits(dist²) << 32 | index) seen so far, one per lane,
//     ascending across the lanes; for dist² >= 0 the keys order exactly like (dist², index), so lanes 0..k-1 are the k rows.  Per
//     shell the lanes enumerate the shell's face bins 64 at a time, each lane applies the prune test against the previous shell's
//     k-th key, the surviving bins' point counts are prefix-summed over the lanes and their points streamed 64 at a time (every lane
//     finds its point's bin by a binary search over the lanes).  A batch's keys below the k-th are merged into the held set: by
//     single insertions when few, else by a bitonic sort of the batch and a bitonic merge (lane exchanges through DPP, ds_swizzle and
//     ds_bpermute).  Points inside a bin may be in any order: the answer is the k smallest keys over the visited bins.
//   Rows are ascending in (dist², index); a row holds min(k, points visited) entries.  Where the reference is undefined (a shell of
//   more than 128 bins, fewer than k points, a query outside the box) the answer is KnnGrid's: no bin cap, and the walk ends once
//   every bin has been visited.

#include "rs_buildplan.h"
#include "rs_host.h"
#include "rs_search.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

namespace rs {

// ------------------------------------------------------------------------------------------
// geometry (host) — KnnGrid::build's float / double mix, literally (msh_hash_grid.h:413-449)
// ------------------------------------------------------------------------------------------

struct KnnGeom
{
  float  min_pt[3];
  double cell, inv_cell;
  int64_t w, h, d;
};

// bins of the offset table at most (4 B each): a radius tiny against the box asks for an absurd table
constexpr double KNN_MAX_BINS = (double)( 1u << 26 );

// mn / mx: the points' own box (mn = 1e9, mx = -1e9 where there are no points, like the reference's starting values)
int knn_geometry( const float mn_in[3], const float mx_in[3], float radius, KnnGeom& g )
{
  float mn[3], mx[3];
  for( int a = 0; a < 3; ++a ) { mn[a] = mn_in[a]; mx[a] = mx_in[a]; }
  for( int a = 0; a < 3; ++a ) { mx[a] += 0.0001f; mn[a] -= 0.0001f; g.min_pt[a] = mn[a]; }        // :433-434
  const float dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
  const float max_dim = std::max( dx, std::max( dy, dz ) );
  if( radius > 0.0 ) g.cell = 2.0 * radius; else g.cell = max_dim / ( 32 * sqrtf( 3.0f ) );         // :443-444
  const double fw = dx / g.cell + 1.0, fh = dy / g.cell + 1.0, fd = dz / g.cell + 1.0;             // :446-448
  if( !( std::isfinite( fw ) && std::isfinite( fh ) && std::isfinite( fd ) ) || !( g.cell > 0.0 ) ) return RS_HIP_E_ARG;
  const double cw = std::max( fw, 1.0 ), ch = std::max( fh, 1.0 ), cd = std::max( fd, 1.0 );
  if( cw > INT_MAX || ch > INT_MAX || cd > INT_MAX || std::floor( cw ) * std::floor( ch ) * std::floor( cd ) > KNN_MAX_BINS ) return RS_HIP_E_CAPACITY;
  g.w = (int64_t)cw; g.h = (int64_t)ch; g.d = (int64_t)cd;
  g.inv_cell = 1.0f / g.cell;                                                                          // :449
  return RS_HIP_OK;
}

// ------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------

struct KnnView
{
  const float4*   rec;          // {x, y, z, bitcast(original index)}, bin order
  const uint32_t* start;        // w h d + 1
  float  minx, miny, minz;
  double inv_cell;
  float  cs;                    // (float)cell: the reference's `float cs = hg->cell_size` (:1312)
  int    w, h, d, last_layer;
  int    n;
};

#define KNN_BLOCK 256

__device__ __forceinline__ unsigned ordered_bits( float f )
{
  const unsigned u = __float_as_uint( f );
  return ( u & 0x80000000u ) ? ~u : ( u | 0x80000000u );
}

// out6: min x, y, z (ordered bits, start ~0), max x, y, z (start 0); NaN coordinates are ignored like the reference's compares do
__global__ __launch_bounds__( KNN_BLOCK ) void k_knn_bounds( const float4* rec, int n, unsigned* out6 )
{
  float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
  for( int i = blockIdx.x * KNN_BLOCK + threadIdx.x; i < n; i += gridDim.x * KNN_BLOCK )
  {
    const float4 p = rec[i];
    const float v[3] = { p.x, p.y, p.z };
    for( int a = 0; a < 3; ++a ) { lo[a] = fminf( lo[a], v[a] ); hi[a] = fmaxf( hi[a], v[a] ); }
  }
  for( int a = 0; a < 3; ++a )
  {
    const float l = wave_min( lo[a] ), h = wave_max( hi[a] );
    if( ( threadIdx.x & ( WAVE - 1 ) ) == 0 ) { atomicMin( &out6[a], ordered_bits( l ) ); atomicMax( &out6[3 + a], ordered_bits( h ) ); }
  }
}

// KnnGrid::build's bin of a point (:471-473): (p - min) in float, times inv_cell in double, truncated
__device__ __forceinline__ int knn_point_bin( float v, float mn, double inv, int dim )
{
  const double t = (double)( v - mn ) * inv;
  if( !( t >= 1.0 ) ) return 0;
  if( t >= (double)( dim - 1 ) ) return dim - 1;
  return (int)t;
}

__global__ __launch_bounds__( KNN_BLOCK ) void k_knn_count( const float4* rec, int n, KnnView g, uint32_t* bin_of, uint32_t* rank, uint32_t* counts )
{
  const int i = blockIdx.x * KNN_BLOCK + threadIdx.x;
  if( i >= n ) return;
  const float4 p = rec[i];
  const uint32_t b = (uint32_t)( ( knn_point_bin( p.z, g.minz, g.inv_cell, g.d ) * g.h + knn_point_bin( p.y, g.miny, g.inv_cell, g.h ) ) * g.w
                                 + knn_point_bin( p.x, g.minx, g.inv_cell, g.w ) );
  bin_of[i] = b;
  rank[i] = atomicAdd( &counts[b], 1u );
}

__global__ __launch_bounds__( KNN_BLOCK ) void k_knn_scatter( const float4* rec, int n, const uint32_t* bin_of, const uint32_t* rank, const uint32_t* start, float4* out )
{
  const int i = blockIdx.x * KNN_BLOCK + threadIdx.x;
  if( i >= n ) return;
  out[start[bin_of[i]] + rank[i]] = rec[i];
}

// ---- lane exchanges of 64-bit keys --------------------------------------------------------

typedef unsigned long long u64;

template <int X> __device__ __forceinline__ u64 xor_key( u64 v )
{
  if( X == 1 ) return dpp_u64<RS_DPP_QUAD_XOR1, 0xf>( v );
  if( X == 2 ) return dpp_u64<RS_DPP_QUAD_XOR2, 0xf>( v );
  if( X == 32 ) return __shfl_xor( v, 32 );
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_swizzle( (int)(uint32_t)v, ( X << 10 ) | 0x1f );       // bit-mask mode: lane ^ X within 32
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_swizzle( (int)(uint32_t)( v >> 32 ), ( X << 10 ) | 0x1f );
  return ( (u64)hi << 32 ) | lo;
}
__device__ __forceinline__ u64 lane_key( u64 v, int src )
{
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane( (int)(uint32_t)v, src ), hi = (uint32_t)__builtin_amdgcn_readlane( (int)(uint32_t)( v >> 32 ), src );
  return ( (u64)hi << 32 ) | lo;
}
// one compare-exchange step of a bitonic network: the lower lane of each pair keeps the min when `up`
template <int X> __device__ __forceinline__ u64 cmpx( u64 v, int lane, bool up )
{
  const u64 p = xor_key<X>( v );
  const bool keep_min = ( ( lane & X ) == 0 ) == up;
  return keep_min ? ( v < p ? v : p ) : ( v < p ? p : v );
}
template <int SIZE> __device__ __forceinline__ u64 bitonic_stage( u64 v, int lane )
{
  const bool up = ( lane & SIZE ) == 0;          // (SIZE = 64: every lane ascending)
  if( SIZE >= 64 ) v = cmpx<32>( v, lane, up );
  if( SIZE >= 32 ) v = cmpx<16>( v, lane, up );
  if( SIZE >= 16 ) v = cmpx<8>( v, lane, up );
  if( SIZE >= 8 )  v = cmpx<4>( v, lane, up );
  if( SIZE >= 4 )  v = cmpx<2>( v, lane, up );
  v = cmpx<1>( v, lane, up );
  return v;
}
__device__ __forceinline__ u64 sort64( u64 v, int lane )
{
  v = bitonic_stage<2>( v, lane ); v = bitonic_stage<4>( v, lane ); v = bitonic_stage<8>( v, lane );
  v = bitonic_stage<16>( v, lane ); v = bitonic_stage<32>( v, lane ); v = bitonic_stage<64>( v, lane );
  return v;
}
// held (ascending) := the 64 smallest of held and batch: min against the reversed sorted batch is bitonic, one merge sorts it
__device__ __forceinline__ u64 merge64( u64 held, u64 batch, int lane )
{
  batch = sort64( batch, lane );
  const u64 rev = __shfl_xor( batch, 63 );
  return bitonic_stage<64>( held < rev ? held : rev, lane );
}

// the lower bound of a bin along one axis (:1378-1380, 1388-1390, 1400-1402)
__device__ __forceinline__ float knn_gap( float p, int c, int o, float cs )
{
  if( o < 0 ) return p - (float)( c + 1 ) * cs;
  if( o > 0 ) return (float)c * cs - p;
  return 0.0f;
}
// the query's bin (:1363-1365; clamped into the grid, as KnnGrid does for a query outside the box)
__device__ __forceinline__ int knn_query_bin( float p, double inv, int dim )
{
  double t = (double)p * inv;
  if( !( t >= 0.0 ) ) t = 0.0;
  if( t > (double)( dim - 1 ) ) t = (double)( dim - 1 );
  return (int)t;
}

// below this many candidates in a batch, single insertions; from it on, sort + merge
#ifndef RS_KNN_INSERT_BELOW
#define RS_KNN_INSERT_BELOW 8
#endif

__global__ __launch_bounds__( KNN_BLOCK ) void k_knn( KnnView g, const float* q3, int nq, int k, float* out_d2, int* out_idx, int* out_n )
{
  const int lane = threadIdx.x & ( WAVE - 1 );
  const int qi = blockIdx.x * ( KNN_BLOCK / WAVE ) + threadIdx.x / WAVE;
  if( qi >= nq ) return;                                               // (whole waves)
  const float qx = q3[3 * (size_t)qi], qy = q3[3 * (size_t)qi + 1], qz = q3[3 * (size_t)qi + 2];
  const float px = qx - g.minx, py = qy - g.miny, pz = qz - g.minz;   // pt_prime (:1350-1361)
  const int ix = knn_query_bin( px, g.inv_cell, g.w ), iy = knn_query_bin( py, g.inv_cell, g.h ), iz = knn_query_bin( pz, g.inv_cell, g.d );
  // beyond this shell no bin of the grid is left
  const int reach = max( max( max( ix, g.w - 1 - ix ), max( iy, g.h - 1 - iy ) ), max( iz, g.d - 1 - iz ) );
  const float cs = g.cs;
  u64 held = ~0ull;                  // lane l: the l-th smallest key visited (~0: none)
  int visited = 0;                   // min(k, points visited)
  bool should_break = false;
  for( int L = 0; L <= g.last_layer && L <= reach; ++L )
  {
    const bool prune = visited >= k;
    const float kth = __uint_as_float( (uint32_t)( lane_key( held, k - 1 ) >> 32 ) );    // the previous shell's k-th distance
    const int x0 = max( -L, -ix ), x1 = min( L, g.w - 1 - ix ), y0 = max( -L, -iy ), y1 = min( L, g.h - 1 - iy ), z0 = max( -L, -iz ), z1 = min( L, g.d - 1 - iz );
    const int nx = x1 - x0 + 1, ny = y1 - y0 + 1, nxy = nx * ny;
    const int cube = nxy * ( z1 - z0 + 1 );
    for( int c0 = 0; c0 < cube; c0 += WAVE )
    {
      // this lane's bin of the clipped cube: on the shell's faces (the inc_x rule, :1392-1393), not pruned (:1404-1407)
      const int t = c0 + lane;
      const int oz = z0 + t / nxy, r = t - ( t / nxy ) * nxy, oy = y0 + r / nx, ox = x0 + r - ( r / nx ) * nx;
      uint32_t s0 = 0, cnt = 0;
      if( t < cube && ( abs( ox ) == L || abs( oy ) == L || abs( oz ) == L ) )
      {
        const int cx = ix + ox, cy = iy + oy, cz = iz + oz;
        const float ddz = knn_gap( pz, cz, oz, cs ), ddy = knn_gap( py, cy, oy, cs ), ddx = knn_gap( px, cx, ox, cs );
        const float dist_sq = ddz * ddz + ddy * ddy + ddx * ddx;                             // :1404
        if( !( prune && dist_sq > kth ) )
        {
          const size_t b = ( (size_t)cz * g.h + cy ) * g.w + cx;
          s0 = g.start[b]; cnt = g.start[b + 1] - s0;
        }
      }
      if( !wave_any( cnt != 0 ) ) continue;
      const uint32_t incl = wave_scan( cnt, lane );
      const int tot = (int)__builtin_amdgcn_readlane( (int)incl, WAVE - 1 );
      for( int p0 = 0; p0 < tot; p0 += WAVE )
      {
        const int p = p0 + lane;
        // the first lane whose inclusive count exceeds p owns point p
        int j = 0;
#pragma unroll
        for( int s = 32; s > 0; s >>= 1 ) if( (int)__shfl( incl, j + s - 1 ) <= p ) j += s;
        const uint32_t js = (uint32_t)min( j, WAVE - 1 );
        const uint32_t own_s0 = __shfl( s0, js ), own_end = __shfl( incl, js ), own_cnt = __shfl( cnt, js );
        u64 key = ~0ull;
        if( p < tot )
        {
          const float4 q = g.rec[own_s0 + ( (uint32_t)p - ( own_end - own_cnt ) )];
          const float vx = q.x - qx, vy = q.y - qy, vz = q.z - qz;                             // :1278-1287
          const float d2 = vx * vx + vy * vy + vz * vz;
          key = ( (u64)__float_as_uint( d2 ) << 32 ) | __float_as_uint( q.w );
        }
        visited = min( k, visited + min( WAVE, tot - p0 ) );
        const u64 kth_key = lane_key( held, k - 1 );
        const bool cand = key < kth_key;
        u64 mask = __builtin_amdgcn_ballot_w64( cand );
        if( !mask ) continue;
        if( __popcll( mask ) < RS_KNN_INSERT_BELOW )
        {
          while( mask )
          {
            const int src = __builtin_ctzll( mask ); mask &= mask - 1;
            const u64 x = lane_key( key, src );
            const int pos = __popcll( __builtin_amdgcn_ballot_w64( held < x ) );
            const u64 up = __shfl_up( held, 1 );
            held = lane < pos ? held : ( lane == pos ? x : up );
          }
        }
        else held = merge64( held, cand ? key : ~0ull, lane );
      }
    }
    if( should_break ) break;                                          // :1428-1429: one more shell after k were held
    if( visited >= k ) should_break = true;
  }
  if( lane < visited )
  {
    out_d2[(size_t)qi * k + lane] = __uint_as_float( (uint32_t)( held >> 32 ) );
    out_idx[(size_t)qi * k + lane] = (int)(uint32_t)held;
  }
  if( lane == 0 ) out_n[qi] = visited;
}

} // namespace rs

using namespace rs;

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------

struct rs_hip_knn_grid
{
  KnnGeom geom{};
  KnnView view{};
  float4* d_rec = nullptr;
  uint32_t* d_start = nullptr;
};

namespace {

struct KnnWorkspace { Buf q, rows, h_q{ nullptr, 0, true }, h_rows{ nullptr, 0, true }; };
thread_local KnnWorkspace g_knn_ws;

void host_box( const float* pos, int64_t n, int32_t dim, float mn[3], float mx[3] )
{
  for( int a = 0; a < 3; ++a ) { mn[a] = 1e9f; mx[a] = -1e9f; }                                        // :413-414
  for( int64_t i = 0; i < n; ++i )
    for( int a = 0; a < 3; ++a )
    {
      const float v = ( a == 2 && dim == 2 ) ? 0.0f : pos[3 * i + a];
      mn[a] = ( mn[a] > v ) ? v : mn[a]; mx[a] = ( mx[a] < v ) ? v : mx[a];
    }
}

int build_grid( rs_hip_knn_grid* G, const GridView& c, float radius, int32_t dim, hipStream_t st )
{
  const int n = c.n;
  unsigned box[6] = { ~0u, ~0u, ~0u, 0u, 0u, 0u };
  float mn[3] = { 1e9f, 1e9f, 1e9f }, mx[3] = { -1e9f, -1e9f, -1e9f };
  if( n > 0 )
  {
    unsigned* d_box = nullptr;
    RS_TRY( hipMalloc( (void**)&d_box, 24 ), "knn grid: bounds" );
    hipError_t e = hipMemcpyAsync( d_box, box, 24, hipMemcpyHostToDevice, st );
    if( e == hipSuccess ) { hipLaunchKernelGGL( k_knn_bounds, dim3( std::min( 1024u, blocks_for( n, KNN_BLOCK ) ) ), dim3( KNN_BLOCK ), 0, st, c.pos, n, d_box ); e = hipGetLastError(); }
    if( e == hipSuccess ) e = hipMemcpyAsync( box, d_box, 24, hipMemcpyDeviceToHost, st );
    if( e == hipSuccess ) e = hipStreamSynchronize( st );
    (void)hipFree( d_box );
    if( e != hipSuccess ) return fail( RS_HIP_E_RUNTIME, "knn grid: bounds", e );
    for( int a = 0; a < 3; ++a )
    {
      if( box[a] == ~0u ) continue;                                    // (every coordinate NaN)
      const float lo = bp_bounds_decode( box[a] ), hi = bp_bounds_decode( box[3 + a] );
      mn[a] = ( mn[a] > lo ) ? lo : mn[a]; mx[a] = ( mx[a] < hi ) ? hi : mx[a];      // against the reference's starting values
    }
    if( dim == 2 ) { mn[2] = 0.0f; mx[2] = 0.0f; }
  }
  KnnGeom& g = G->geom;
  if( n > 0 )
  {
    const int rc = knn_geometry( mn, mx, radius, g );
    if( rc == RS_HIP_E_CAPACITY ) return fail( rc, "knn grid: w*h*d bins exceed the offset table's limit (2^26): radius too small for the box" );
    if( rc ) return fail( rc, "knn grid: no finite geometry for this box and radius" );
  }
  else { for( int a = 0; a < 3; ++a ) g.min_pt[a] = 0.0f; g.cell = 1.0; g.inv_cell = 1.0; g.w = g.h = g.d = 1; }
  const size_t n_bins = (size_t)( g.w * g.h * g.d );
  KnnView& v = G->view;
  v.minx = g.min_pt[0]; v.miny = g.min_pt[1]; v.minz = g.min_pt[2];
  v.inv_cell = g.inv_cell; v.cs = (float)g.cell;
  v.w = (int)g.w; v.h = (int)g.h; v.d = (int)g.d; v.last_layer = (int)std::max( g.w, std::max( g.h, g.d ) ); v.n = n;
  RS_TRY( hipMalloc( (void**)&G->d_start, ( n_bins + 1 ) * 4 ), "knn grid: offset table" );
  RS_TRY( hipMalloc( (void**)&G->d_rec, (size_t)std::max( n, 1 ) * 16 ), "knn grid: records" );
  v.rec = G->d_rec; v.start = G->d_start;
  // counting sort: histogram (each point's rank inside its bin from the same atomic) -> exclusive scan -> scatter
  uint32_t *counts = nullptr, *bin_of = nullptr, *rank = nullptr; void* tmp = nullptr;
  const size_t tmp_bytes = build_scan_temp_bytes( n_bins + 1 );
  hipError_t e = hipMalloc( (void**)&counts, ( n_bins + 1 ) * 4 );
  if( e == hipSuccess ) e = hipMalloc( (void**)&bin_of, (size_t)std::max( n, 1 ) * 4 );
  if( e == hipSuccess ) e = hipMalloc( (void**)&rank, (size_t)std::max( n, 1 ) * 4 );
  if( e == hipSuccess ) e = hipMalloc( &tmp, tmp_bytes + 256 );
  if( e == hipSuccess ) e = hipMemsetAsync( counts, 0, ( n_bins + 1 ) * 4, st );
  if( e == hipSuccess && n > 0 )
  {
    hipLaunchKernelGGL( k_knn_count, dim3( blocks_for( n, KNN_BLOCK ) ), dim3( KNN_BLOCK ), 0, st, c.pos, n, v, bin_of, rank, counts );
    e = hipGetLastError();
  }
  if( e == hipSuccess && build_exclusive_scan( tmp, tmp_bytes, counts, G->d_start, n_bins + 1, st ) ) e = hipErrorUnknown;
  if( e == hipSuccess && n > 0 )
  {
    hipLaunchKernelGGL( k_knn_scatter, dim3( blocks_for( n, KNN_BLOCK ) ), dim3( KNN_BLOCK ), 0, st, c.pos, n, bin_of, rank, G->d_start, G->d_rec );
    e = hipGetLastError();
  }
  if( e == hipSuccess ) e = hipStreamSynchronize( st );
  for( void* p : { (void*)counts, (void*)bin_of, (void*)rank, tmp } ) if( p ) (void)hipFree( p );
  if( e != hipSuccess ) return fail( RS_HIP_E_RUNTIME, "knn grid: counting sort", e );
  return RS_HIP_OK;
}

} // namespace

extern "C" {

int rs_hip_knn_geometry( const float* pos, int64_t n, float radius, int32_t dim, int64_t dims[3], double* cell, float min_pt[3] )
{
  if( ( !pos && n > 0 ) || n <= 0 || ( dim != 2 && dim != 3 ) || !dims ) { api_set_err( "knn_geometry: bad arguments" ); return RS_HIP_E_ARG; }
  float mn[3], mx[3];
  host_box( pos, n, dim, mn, mx );
  KnnGeom g;
  const int rc = knn_geometry( mn, mx, radius, g );
  if( rc ) { api_set_err( rc == RS_HIP_E_CAPACITY ? "knn_geometry: too many bins" : "knn_geometry: no finite geometry" ); return rc; }
  dims[0] = g.w; dims[1] = g.h; dims[2] = g.d;
  if( cell ) *cell = g.cell;
  if( min_pt ) for( int a = 0; a < 3; ++a ) min_pt[a] = g.min_pt[a];
  return RS_HIP_OK;
}

rs_hip_knn_grid_t* rs_hip_knn_grid_create( const rs_hip_cloud_t* cloud, float radius, int32_t dim )
{
  hipStream_t st = nullptr;
  if( api_ready( &st ) ) return nullptr;
  const GridView* c = api_cloud_view( cloud );
  if( !c || ( dim != 2 && dim != 3 ) ) { api_set_err( "knn_grid_create: bad arguments" ); return nullptr; }
  rs_hip_knn_grid* G = new rs_hip_knn_grid();
  if( build_grid( G, *c, radius, dim, st ) ) { rs_hip_knn_grid_destroy( G ); return nullptr; }
  return G;
}

void rs_hip_knn_grid_destroy( rs_hip_knn_grid_t* g )
{
  if( !g ) return;
  if( g->d_rec ) (void)hipFree( g->d_rec );
  if( g->d_start ) (void)hipFree( g->d_start );
  delete g;
}

int rs_hip_knn_grid_geometry( const rs_hip_knn_grid_t* g, int64_t dims[3], double* cell, float min_pt[3] )
{
  if( !g || !dims ) { api_set_err( "knn_grid_geometry: bad arguments" ); return RS_HIP_E_ARG; }
  dims[0] = g->geom.w; dims[1] = g->geom.h; dims[2] = g->geom.d;
  if( cell ) *cell = g->geom.cell;
  if( min_pt ) for( int a = 0; a < 3; ++a ) min_pt[a] = g->geom.min_pt[a];
  return RS_HIP_OK;
}

int rs_hip_knn_search( const rs_hip_knn_grid_t* grid, const float* query, int64_t n_query, int32_t k,
                       float* distances_sq, int32_t* indices, size_t* n_neighbors, uint64_t* total )
{
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  if( !grid || ( !query && n_query > 0 ) || ( n_query > 0 && ( !distances_sq || !indices ) ) || n_query < 0 || k <= 0 )
  { api_set_err( "knn_search: bad arguments" ); return RS_HIP_E_ARG; }
  if( k > RS_HIP_KNN_MAX_K ) { api_set_err( "knn_search: k above RS_HIP_KNN_MAX_K" ); return RS_HIP_E_CAPACITY; }
  if( total ) *total = 0;
  if( n_query == 0 ) return RS_HIP_OK;
  if( grid->view.n == 0 )
  {
    if( n_neighbors ) for( int64_t i = 0; i < n_query; ++i ) n_neighbors[i] = 0;
    return RS_HIP_OK;
  }
  // chunks of at most ~32 MB of rows: any n_query fits
  const int64_t chunk = std::max<int64_t>( 1024, ( (int64_t)32 << 20 ) / ( (int64_t)k * 8 ) );
  KnnWorkspace& W = g_knn_ws;
  const int64_t first = std::min( chunk, n_query );
  const size_t row_words = (size_t)first * k * 2 + (size_t)first;
  RS_TRY( W.q.ensure( (size_t)first * 12 ), "knn_search: buffers" );
  RS_TRY( W.rows.ensure( row_words * 4 ), "knn_search: buffers" );
  RS_TRY( W.h_q.ensure( (size_t)first * 12 ), "knn_search: buffers" );
  RS_TRY( W.h_rows.ensure( row_words * 4 ), "knn_search: buffers" );
  uint64_t tot = 0;
  for( int64_t q0 = 0; q0 < n_query; q0 += chunk )
  {
    const int nc = (int)std::min( chunk, n_query - q0 );
    const size_t nk = (size_t)nc * k;
    std::memcpy( W.h_q.p, query + 3 * q0, (size_t)nc * 12 );
    float* d_d2 = (float*)W.rows.p; int* d_idx = (int*)W.rows.p + nk; int* d_n = (int*)W.rows.p + 2 * nk;
    RS_TRY( hipMemcpyAsync( W.q.p, W.h_q.p, (size_t)nc * 12, hipMemcpyHostToDevice, st ), "knn_search: upload" );
    hipLaunchKernelGGL( k_knn, dim3( ( nc + KNN_BLOCK / WAVE - 1 ) / ( KNN_BLOCK / WAVE ) ), dim3( KNN_BLOCK ), 0, st,
                        grid->view, (const float*)W.q.p, nc, (int)k, d_d2, d_idx, d_n );
    RS_TRY( hipGetLastError(), "knn_search: launch" );
    RS_TRY( hipMemcpyAsync( W.h_rows.p, W.rows.p, ( 2 * nk + nc ) * 4, hipMemcpyDeviceToHost, st ), "knn_search: download" );
    RS_TRY( hipStreamSynchronize( st ), "knn_search" );
    // rows are handed over up to their counts only (the caller's arrays keep whatever else they held, like the reference's);
    // runs of full rows in one copy each
    const float* hd = (const float*)W.h_rows.p; const int* hi = (const int*)W.h_rows.p + nk; const int* hn = (const int*)W.h_rows.p + 2 * nk;
    float* od = distances_sq + (size_t)q0 * k; int32_t* oi = indices + (size_t)q0 * k;
    for( int i = 0; i < nc; )
    {
      if( hn[i] == k )
      {
        int j = i; while( j < nc && hn[j] == k ) ++j;
        std::memcpy( od + (size_t)i * k, hd + (size_t)i * k, (size_t)( j - i ) * k * 4 );
        std::memcpy( oi + (size_t)i * k, hi + (size_t)i * k, (size_t)( j - i ) * k * 4 );
        i = j;
      }
      else
      {
        std::memcpy( od + (size_t)i * k, hd + (size_t)i * k, (size_t)hn[i] * 4 );
        std::memcpy( oi + (size_t)i * k, hi + (size_t)i * k, (size_t)hn[i] * 4 );
        ++i;
      }
    }
    for( int i = 0; i < nc; ++i ) { tot += (uint64_t)hn[i]; if( n_neighbors ) n_neighbors[q0 + i] = (size_t)hn[i]; }
  }
  if( total ) *total = tot;
  return RS_HIP_OK;
}

} // extern "C"
