// Device-side construction of a cloud's two layouts (the MI355X counterpart of msh_hash_grid_init_3d,
// lib/msh/msh_hash_grid.h:388-541): bounds, the density-derived cell size, the cell-sorted target
// layout with its dense offset table, and the Hilbert-ordered, tiled query layout — from the caller's
// raw AoS arrays, uploaded once.  Sorting and scanning use hipCUB (rocPRIM) device primitives; the
// kernels around them are below.  Orchestration (buffers, launches) is in rs_cloud_api.hip, the few
// host decisions between the kernels in rs_buildplan.h (CloudPlan).
//
// Nothing here decides a search result: results depend on neither the cell size, nor the order of
// points inside a cell, nor the tiling.  The one expression that must agree with the search kernels is
// the cell coordinate of a stored point (cell_of_dev; rs_search.h: axis_range covers it with a 0.01-cell margin).
#include "rs_device.h"
#include "rs_buildplan.h"
#include <hipcub/hipcub.hpp>
#include <cfloat>
#include <algorithm>

namespace rs {

#define B_BLOCK 256

// order-preserving float <-> unsigned encoding for atomicMin/atomicMax
__device__ __forceinline__ unsigned enc( float f ) { unsigned u = __float_as_uint( f ); return ( u & 0x80000000u ) ? ~u : ( u | 0x80000000u ); }

// out[0..2] = min xyz, out[3..5] = max xyz (encoded), out[6] = max |normal|² (plain bits; non-negative floats order as uints)
__global__ __launch_bounds__( B_BLOCK ) void k_build_bounds( const float* pos, const float* nor, int n, unsigned* out )
{
  float lo[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, hi[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX }, n2 = 0.0f;
  for( int i = blockIdx.x * B_BLOCK + threadIdx.x; i < n; i += gridDim.x * B_BLOCK )
  {
#pragma unroll
    for( int a = 0; a < 3; ++a ) bp_bounds_take( pos[3 * (size_t)i + a], lo[a], hi[a] );   // over the finite coordinates: neither NaN nor ±Inf wins
    if( nor ) { const float x = nor[3 * (size_t)i], y = nor[3 * (size_t)i + 1], z = nor[3 * (size_t)i + 2]; const float l = x * x + y * y + z * z; if( !( l <= n2 ) ) n2 = l; }   // NaN/inf propagate: certificates then stay off
  }
  for( int o = 32; o > 0; o >>= 1 )
  {
#pragma unroll
    for( int a = 0; a < 3; ++a ) { lo[a] = fminf( lo[a], __shfl_down( lo[a], o ) ); hi[a] = fmaxf( hi[a], __shfl_down( hi[a], o ) ); }
    const float other = __shfl_down( n2, o ); if( !( other <= n2 ) ) n2 = other;
  }
  if( ( threadIdx.x & 63 ) == 0 )
  {
#pragma unroll
    for( int a = 0; a < 3; ++a ) { atomicMin( out + a, enc( lo[a] ) ); atomicMax( out + 3 + a, enc( hi[a] ) ); }
    if( n2 == n2 ) atomicMax( out + 6, __float_as_uint( n2 ) ); else out[7] = 1u;      // [7]: a NaN normal was seen
  }
}

// occupancy of a trial grid: one bit per cell (rs_buildplan.h: every point's cell is inside the grid, whatever its coordinates)
__global__ __launch_bounds__( B_BLOCK ) void k_build_mark( const float* pos, int n, float mx, float my, float mz, float inv, float tx, float ty, float tz,
                                                           unsigned long long db, unsigned long long dc, uint32_t* bits )
{
  const int i = blockIdx.x * B_BLOCK + threadIdx.x;
  if( i >= n ) return;
  const unsigned long long id = bp_trial_cell( pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2], mx, my, mz, inv, tx, ty, tz, db, dc );
  atomicOr( bits + ( id >> 5 ), 1u << ( id & 31 ) );
}

// (cell_of_dev, the cell coordinate of a stored point along one axis: rs_buildplan.h)
__global__ __launch_bounds__( B_BLOCK ) void k_build_cellids( const float* pos, int n, float mx, float my, float mz, float inv_cell, int w, int h, int d,
                                                              uint32_t* cid, uint32_t* iota, uint32_t* counts )
{
  const int i = blockIdx.x * B_BLOCK + threadIdx.x;
  if( i >= n ) return;
  const int cx = cell_of_dev( pos[3 * (size_t)i], mx, inv_cell, w ), cy = cell_of_dev( pos[3 * (size_t)i + 1], my, inv_cell, h ), cz = cell_of_dev( pos[3 * (size_t)i + 2], mz, inv_cell, d );
  const uint32_t id = bp_cell_id( cx, cy, cz, w, h );
  cid[i] = id; iota[i] = (uint32_t)i;
  atomicAdd( counts + id, 1u );
}

__global__ __launch_bounds__( B_BLOCK ) void k_build_gather( const float* pos, const float* nor, const uint32_t* order, int n, float4* spos, float4* snor )
{
  const int s = blockIdx.x * B_BLOCK + threadIdx.x;
  if( s >= n ) return;
  const uint32_t i = order[s];
  spos[s] = make_float4( pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2], __uint_as_float( i ) );
  if( nor ) snor[s] = make_float4( nor[3 * (size_t)i], nor[3 * (size_t)i + 1], nor[3 * (size_t)i + 2], 0.0f );
}

__global__ __launch_bounds__( B_BLOCK ) void k_build_count_runs( const uint32_t* sorted, int n, int* out )
{
  const int s = blockIdx.x * B_BLOCK + threadIdx.x;
  int c = ( s < n && ( s == 0 || sorted[s] != sorted[s - 1] ) ) ? 1 : 0;
  for( int o = 32; o > 0; o >>= 1 ) c += __shfl_down( c, o );
  if( ( threadIdx.x & 63 ) == 0 && c ) atomicAdd( out, c );
}

// (hilbert3_dev, Skilling's transpose form, and a coordinate's Hilbert cell: rs_buildplan.h)
__global__ __launch_bounds__( B_BLOCK ) void k_build_hilbert( const float* pos, int n, float mx, float my, float mz, float scale, uint32_t* key, uint32_t* iota )
{
  const int i = blockIdx.x * B_BLOCK + threadIdx.x;
  if( i >= n ) return;
  const float mn[3] = { mx, my, mz };
  uint32_t c[3];
#pragma unroll
  for( int a = 0; a < 3; ++a ) c[a] = bp_hilbert_axis( pos[3 * (size_t)i + a], mn[a], scale );
  key[i] = hilbert3_dev( c[0], c[1], c[2], 10 );
  iota[i] = (uint32_t)i;
}

// Tiling of the Hilbert sequence, greedy from the front: a tile ends after 64 points or when adding the next
// point would stretch its bounding box beyond max_extent on any axis (the curve crosses empty space there).
// Sequential as stated; in parallel: next[s] = where the tile that STARTS at s would end (independent for every
// s), then the tile starts are the nodes reachable from 0 along next[], marked by pointer doubling.
__global__ __launch_bounds__( 64 ) void k_build_tile_next( const float4* qpos, int n, float max_extent, uint32_t* next )
{
  __shared__ float px[128], py[128], pz[128];
  const int lane = threadIdx.x, base = blockIdx.x * 64;
  for( int k = lane; k < 128; k += 64 )
  {
    const int s = base + k;
    const float4 p = s < n ? qpos[s] : make_float4( 0, 0, 0, 0 );
    px[k] = p.x; py[k] = p.y; pz[k] = p.z;
  }
  __syncthreads();
  const int s = base + lane;
  if( s >= n ) return;
  float lx = px[lane], hx = lx, ly = py[lane], hy = ly, lz = pz[lane], hz = lz;
  int len = 1;
  const int most = min( 64, n - s );
  for( ; len < most; ++len )
  {
    const float x = px[lane + len], y = py[lane + len], z = pz[lane + len];
    const float nlx = fminf( lx, x ), nhx = fmaxf( hx, x ), nly = fminf( ly, y ), nhy = fmaxf( hy, y ), nlz = fminf( lz, z ), nhz = fmaxf( hz, z );
    if( ( nhx - nlx > max_extent ) | ( nhy - nly > max_extent ) | ( nhz - nlz > max_extent ) ) break;
    lx = nlx; hx = nhx; ly = nly; hy = nhy; lz = nlz; hz = nhz;
  }
  next[s] = (uint32_t)( s + len );        // == n for the last tile
}

// one doubling round: everything one jump from a marked node gets marked; the jumps double (out-of-place)
__global__ __launch_bounds__( B_BLOCK ) void k_build_tile_round( const uint32_t* jump, uint32_t* jump_out, uint32_t* mark, int n )
{
  const int s = blockIdx.x * B_BLOCK + threadIdx.x;
  if( s >= n ) return;
  const uint32_t j = jump[s];
  if( mark[s] && j < (uint32_t)n ) mark[j] = 1u;
  jump_out[s] = j < (uint32_t)n ? jump[j] : (uint32_t)n;
}

__global__ __launch_bounds__( B_BLOCK ) void k_build_tile_scatter( const uint32_t* flags, const uint32_t* scanned, int n, uint32_t* tiles )
{
  const int s = blockIdx.x * B_BLOCK + threadIdx.x;
  if( s < n && flags[s] ) tiles[scanned[s]] = (uint32_t)s;
}

static inline unsigned blocks_for( long long n ) { return (unsigned)std::max<long long>( 1, ( n + B_BLOCK - 1 ) / B_BLOCK ); }

void launch_build_bounds( const float* pos3, const float* nor3, int n, unsigned* out8, hipStream_t st )
{
  hipLaunchKernelGGL( k_build_bounds, dim3( std::min( 1024u, blocks_for( n ) ) ), dim3( B_BLOCK ), 0, st, pos3, nor3, n, out8 );
}
void launch_build_mark( const float* pos3, int n, const float mn[3], float inv, const float top[3], unsigned long long db, unsigned long long dc, uint32_t* bits, hipStream_t st )
{
  hipLaunchKernelGGL( k_build_mark, dim3( blocks_for( n ) ), dim3( B_BLOCK ), 0, st, pos3, n, mn[0], mn[1], mn[2], inv, top[0], top[1], top[2], db, dc, bits );
}
void launch_build_cellids( const float* pos3, int n, const float mn[3], float inv_cell, const int dims[3], uint32_t* cid, uint32_t* iota, uint32_t* counts, hipStream_t st )
{
  hipLaunchKernelGGL( k_build_cellids, dim3( blocks_for( n ) ), dim3( B_BLOCK ), 0, st, pos3, n, mn[0], mn[1], mn[2], inv_cell, dims[0], dims[1], dims[2], cid, iota, counts );
}
void launch_build_gather( const float* pos3, const float* nor3, const uint32_t* order, int n, float4* spos, float4* snor, hipStream_t st )
{
  hipLaunchKernelGGL( k_build_gather, dim3( blocks_for( n ) ), dim3( B_BLOCK ), 0, st, pos3, nor3, order, n, spos, snor );
}
void launch_build_count_runs( const uint32_t* sorted, int n, int* out, hipStream_t st )
{
  hipLaunchKernelGGL( k_build_count_runs, dim3( blocks_for( n ) ), dim3( B_BLOCK ), 0, st, sorted, n, out );
}
void launch_build_hilbert( const float* pos3, int n, const float mn[3], float scale, uint32_t* key, uint32_t* iota, hipStream_t st )
{
  hipLaunchKernelGGL( k_build_hilbert, dim3( blocks_for( n ) ), dim3( B_BLOCK ), 0, st, pos3, n, mn[0], mn[1], mn[2], scale, key, iota );
}
// flags[0..n) = 1 where a tile starts; jump_a / jump_b: two scratch arrays of n words
void launch_build_tile_flags( const float4* qpos, int n, float max_extent, uint32_t* flags, uint32_t* jump_a, uint32_t* jump_b, hipStream_t st )
{
  hipLaunchKernelGGL( k_build_tile_next, dim3( ( n + 63 ) / 64 ), dim3( 64 ), 0, st, qpos, n, max_extent, jump_a );
  (void)hipMemsetAsync( flags, 0, (size_t)n * 4, st );
  const uint32_t one = 1u;
  (void)hipMemcpyAsync( flags, &one, 4, hipMemcpyHostToDevice, st );
  // a marked node at distance d from 0 is reached after ceil(log2(d+1)) rounds; the chain has at most n nodes
  // (concurrent marks inside a round only ever ADD nodes of the chain: mark[] is closed under next[] by then or later)
  for( long long reach = 1; reach < (long long)n; reach <<= 1 )
  {
    hipLaunchKernelGGL( k_build_tile_round, dim3( blocks_for( n ) ), dim3( B_BLOCK ), 0, st, jump_a, jump_b, flags, n );
    std::swap( jump_a, jump_b );
  }
}
void launch_build_tile_scatter( const uint32_t* flags, const uint32_t* scanned, int n, uint32_t* tiles, hipStream_t st )
{
  hipLaunchKernelGGL( k_build_tile_scatter, dim3( blocks_for( n ) ), dim3( B_BLOCK ), 0, st, flags, scanned, n, tiles );
}

// by_orig[original index] = query slot (the inverse of the Hilbert permutation kept in qpos[s].w)
__global__ __launch_bounds__( B_BLOCK ) void k_build_inverse( const float4* qpos, int n, int* by_orig )
{
  const int s = blockIdx.x * B_BLOCK + threadIdx.x;
  if( s < n ) by_orig[__float_as_int( qpos[s].w )] = s;
}
void launch_build_inverse( const float4* qpos, int n, int* by_orig, hipStream_t st )
{
  hipLaunchKernelGGL( k_build_inverse, dim3( blocks_for( n ) ), dim3( B_BLOCK ), 0, st, qpos, n, by_orig );
}

size_t build_sort_temp_bytes( int n, int bits )
{
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs( nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, bits );
  return b;
}
int build_sort_pairs( void* tmp, size_t bytes, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout, int n, int bits, hipStream_t st )
{
  return (int)hipcub::DeviceRadixSort::SortPairs( tmp, bytes, kin, kout, vin, vout, n, 0, bits, st );     // stable
}
size_t build_scan_temp_bytes( size_t n )
{
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum( nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n );
  return b;
}
int build_exclusive_scan( void* tmp, size_t bytes, const uint32_t* in, uint32_t* out, size_t n, hipStream_t st )
{
  return (int)hipcub::DeviceScan::ExclusiveSum( tmp, bytes, in, out, (int)n, st );
}

// ---- the build of many clouds at once ----------------------------------------------------------------------
// Segmented forms of the stages above: flat launches over the concatenated points of a group (never a grid row per cloud: a batch
// may be thousands of clouds of a handful of points), a lane reads its cloud from segid[] and the cloud's row of the segment
// table.  Each stage gives every cloud what the single build gives it: min / max / or / add atomics on integers do not depend on
// their order, the two sorts are stable and their keys carry the cloud above bit 32, so a cloud's points keep the relative order of
// a sort of its own, and the tiling walks never look past a cloud's last point.  A launch covers the points [first, first + count)
// of the group: a group whose offset tables pass their budget is finished in several such ranges.

// segid[i] = the cloud of point i: the last one whose offset is <= i (empty clouds own no point)
__global__ __launch_bounds__( B_BLOCK ) void k_many_segids( const int* off, int m, int n, int* segid )
{
  const int i = blockIdx.x * B_BLOCK + threadIdx.x;
  if( i >= n ) return;
  int lo = 0, hi = m;                   // off[lo] <= i < off[hi]
  while( hi - lo > 1 ) { const int mid = ( lo + hi ) >> 1; if( off[mid] <= i ) lo = mid; else hi = mid; }
  segid[i] = lo;
}

// out[s] += c for every lane with c != 0: one atomic for the wave when those lanes are all in one cloud.  Called by whole waves.
__device__ __forceinline__ void wave_seg_add( int s, int c, int* out )
{
  const unsigned long long has = __ballot( c != 0 );
  if( !has ) return;
  const int s0 = __shfl( s, __ffsll( (long long)has ) - 1 );
  if( __all( c == 0 || s == s0 ) )
  {
    for( int o = 32; o > 0; o >>= 1 ) c += __shfl_down( c, o );
    if( ( threadIdx.x & 63 ) == 0 ) atomicAdd( out + s0, c );
  }
  else if( c ) atomicAdd( out + s, c );
}

// k_build_bounds per cloud: out[8 s ..] as its out[0..8).  One point per lane; a wave inside one cloud reduces first.  (A NaN
// normal always sets the cloud's flag here; the single build's grid-stride maximum can lose one behind a later finite normal.)
__global__ __launch_bounds__( B_BLOCK ) void k_many_bounds( const float* pos, const float* nor, const int* segid, const ManySeg* segs, int n, unsigned* out )
{
  const int i = blockIdx.x * B_BLOCK + threadIdx.x;
  const bool live = i < n;
  float lo[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, hi[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX }, n2 = 0.0f;
  int s = -1, nan = 0, with_nor = 0;
  if( live )
  {
    s = segid[i];
#pragma unroll
    for( int a = 0; a < 3; ++a ) bp_bounds_take( pos[3 * (size_t)i + a], lo[a], hi[a] );
    with_nor = segs[s].has_nor;
    if( with_nor )
    {
      const float x = nor[3 * (size_t)i], y = nor[3 * (size_t)i + 1], z = nor[3 * (size_t)i + 2];
      const float l = x * x + y * y + z * z;
      if( l != l ) nan = 1; else n2 = l;
    }
  }
  const int s0 = __shfl( s, 0 );        // (lane 0 has the wave's smallest index: it is live if any lane is)
  if( __all( !live || s == s0 ) )
  {
    for( int o = 32; o > 0; o >>= 1 )
    {
#pragma unroll
      for( int a = 0; a < 3; ++a ) { lo[a] = fminf( lo[a], __shfl_down( lo[a], o ) ); hi[a] = fmaxf( hi[a], __shfl_down( hi[a], o ) ); }
      n2 = fmaxf( n2, __shfl_down( n2, o ) );
    }
    nan = __any( nan );
    if( ( threadIdx.x & 63 ) != 0 || s0 < 0 ) return;
  }
  else if( !live ) return;
  unsigned* o8 = out + 8 * (size_t)s;
#pragma unroll
  for( int a = 0; a < 3; ++a ) { atomicMin( o8 + a, enc( lo[a] ) ); atomicMax( o8 + 3 + a, enc( hi[a] ) ); }
  if( with_nor ) { atomicMax( o8 + 6, __float_as_uint( n2 ) ); if( nan ) o8[7] = 1u; }
}

__global__ __launch_bounds__( B_BLOCK ) void k_many_mark( const float* pos, const int* segid, const ManyTrial* trial, int first, int count, uint32_t* bits )
{
  const int r = blockIdx.x * B_BLOCK + threadIdx.x;
  if( r >= count ) return;
  const int i = first + r;
  const ManyTrial& T = trial[segid[i]];
  if( !T.active ) return;
  const unsigned long long id = bp_trial_cell( pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2], T.mn[0], T.mn[1], T.mn[2], T.inv, T.top[0], T.top[1], T.top[2], T.db, T.dc );
  atomicOr( bits + ( T.word + ( id >> 5 ) ), 1u << ( id & 31 ) );
}

// set bits per table: the tables lie side by side from table_start[t] (ascending, table_start[n_tables] = n_words), table t is cloud table_seg[t]'s
__global__ __launch_bounds__( B_BLOCK ) void k_many_popcount( const uint32_t* bits, unsigned long long n_words, const unsigned long long* table_start,
                                                              const int* table_seg, int n_tables, int* occupied )
{
  const unsigned long long stride = (unsigned long long)gridDim.x * B_BLOCK;
  for( unsigned long long w0 = (unsigned long long)blockIdx.x * B_BLOCK; w0 < n_words; w0 += stride )      // (w0 is the block's: whole waves stay together)
  {
    const unsigned long long w = w0 + threadIdx.x;
    const int c = w < n_words ? __popc( bits[w] ) : 0;
    int s = -1;
    if( c )
    {
      int lo = 0, hi = n_tables;          // table_start[lo] <= w < table_start[hi]
      while( hi - lo > 1 ) { const int mid = ( lo + hi ) >> 1; if( table_start[mid] <= w ) lo = mid; else hi = mid; }
      s = table_seg[lo];
    }
    wave_seg_add( s, c, occupied );
  }
}

// k_build_cellids: the key carries the cloud above the cell id, the value is the point's index inside its cloud, the count goes to the
// cloud's own table.  A table of n_cells + 1 words is followed by one word more, which the cloud's first point sets to -n: the one
// scan over all tables (unsigned, modulo 2^32) then starts every table at 0, as a scan of its own would.
__global__ __launch_bounds__( B_BLOCK ) void k_many_cellids( const float* pos, const int* segid, const ManySeg* segs, int first, int count,
                                                             unsigned long long* key, uint32_t* local, uint32_t* tables )
{
  const int r = blockIdx.x * B_BLOCK + threadIdx.x;
  if( r >= count ) return;
  const int i = first + r, s = segid[i];
  const ManySeg& S = segs[s];
  const int cx = cell_of_dev( pos[3 * (size_t)i], S.mn[0], S.inv_cell, S.dims[0] ), cy = cell_of_dev( pos[3 * (size_t)i + 1], S.mn[1], S.inv_cell, S.dims[1] ),
            cz = cell_of_dev( pos[3 * (size_t)i + 2], S.mn[2], S.inv_cell, S.dims[2] );
  const uint32_t id = bp_cell_id( cx, cy, cz, S.dims[0], S.dims[1] );
  key[i] = ( (unsigned long long)s << 32 ) | id; local[i] = (uint32_t)( i - S.base );
  atomicAdd( tables + ( S.cell_word + id ), 1u );
  if( i == S.base ) tables[S.cell_word + (unsigned long long)S.dims[0] * S.dims[1] * S.dims[2] + 1] = 0u - (uint32_t)S.n;
}

// k_build_gather into the cloud's own records (slot j of the sorted sequence is a slot of the cloud of point j: the clouds keep
// their sizes and their order); the query layout also gets k_build_inverse's by_orig
__global__ __launch_bounds__( B_BLOCK ) void k_many_gather( const float* pos, const float* nor, const int* segid, const ManySeg* segs, const uint32_t* order,
                                                            int first, int count, int query_layout )
{
  const int r = blockIdx.x * B_BLOCK + threadIdx.x;
  if( r >= count ) return;
  const int j = first + r;
  const ManySeg& S = segs[segid[j]];
  const uint32_t i = order[j];
  const size_t src = (size_t)S.base + i;
  const int slot = j - S.base;
  ( query_layout ? S.qpos : S.pos )[slot] = make_float4( pos[3 * src], pos[3 * src + 1], pos[3 * src + 2], __uint_as_float( i ) );
  if( S.has_nor ) ( query_layout ? S.qnor : S.nor )[slot] = make_float4( nor[3 * src], nor[3 * src + 1], nor[3 * src + 2], 0.0f );
  if( query_layout ) S.by_orig[i] = slot;
}

__global__ __launch_bounds__( B_BLOCK ) void k_many_count_runs( const unsigned long long* sorted, const int* segid, int first, int count, int* occupied )
{
  const int r = blockIdx.x * B_BLOCK + threadIdx.x;
  const bool live = r < count;
  const int j = first + r;
  const int c = ( live && ( r == 0 || sorted[j] != sorted[j - 1] ) ) ? 1 : 0;     // (the key carries the cloud: a cloud's first slot starts a run)
  wave_seg_add( live ? segid[j] : -1, c, occupied );
}

__global__ __launch_bounds__( B_BLOCK ) void k_many_hilbert( const float* pos, const int* segid, const ManySeg* segs, int first, int count,
                                                             unsigned long long* key, uint32_t* local )
{
  const int r = blockIdx.x * B_BLOCK + threadIdx.x;
  if( r >= count ) return;
  const int i = first + r, s = segid[i];
  const ManySeg& S = segs[s];
  uint32_t c[3];
#pragma unroll
  for( int a = 0; a < 3; ++a ) c[a] = bp_hilbert_axis( pos[3 * (size_t)i + a], S.mn[a], S.hscale );
  key[i] = ( (unsigned long long)s << 32 ) | hilbert3_dev( c[0], c[1], c[2], 10 );
  local[i] = (uint32_t)( i - S.base );
}

// k_build_tile_next over the concatenated Hilbert sequences: a tile ends with its cloud at the latest, so the last tile of a cloud
// points at the first point of the next cloud that has one, and the doubling from node 0 marks every cloud's first point.
// next[] holds indices relative to `first`.
__global__ __launch_bounds__( 64 ) void k_many_tile_next( const int* segid, const ManySeg* segs, int first, int count, uint32_t* next )
{
  __shared__ float px[128], py[128], pz[128];
  const int lane = threadIdx.x, base = blockIdx.x * 64;
  for( int k = lane; k < 128; k += 64 )
  {
    const int r = base + k;
    float4 p = make_float4( 0, 0, 0, 0 );
    if( r < count ) { const ManySeg& S = segs[segid[first + r]]; p = S.qpos[first + r - S.base]; }
    px[k] = p.x; py[k] = p.y; pz[k] = p.z;
  }
  __syncthreads();
  const int r = base + lane;
  if( r >= count ) return;
  const ManySeg& S = segs[segid[first + r]];
  const float max_extent = S.extent_limit;
  float lx = px[lane], hx = lx, ly = py[lane], hy = ly, lz = pz[lane], hz = lz;
  int len = 1;
  const int most = min( 64, S.base + S.n - ( first + r ) );       // never past the cloud's last point
  for( ; len < most; ++len )
  {
    const float x = px[lane + len], y = py[lane + len], z = pz[lane + len];
    const float nlx = fminf( lx, x ), nhx = fmaxf( hx, x ), nly = fminf( ly, y ), nhy = fmaxf( hy, y ), nlz = fminf( lz, z ), nhz = fmaxf( hz, z );
    if( ( nhx - nlx > max_extent ) | ( nhy - nly > max_extent ) | ( nhz - nlz > max_extent ) ) break;
    lx = nlx; hx = nhx; ly = nly; hy = nhy; lz = nlz; hz = nhz;
  }
  next[r] = (uint32_t)( r + len );
}

// tile starts into the clouds' own lists, relative to the cloud's first point and first tile; the lane of a cloud's first point
// (always a tile start) also closes the list with tiles[n_tiles] = n and reports n_tiles
__global__ __launch_bounds__( B_BLOCK ) void k_many_tile_scatter( const uint32_t* flags, const uint32_t* scanned, const int* segid, const ManySeg* segs,
                                                                  int first, int count, int* n_tiles )
{
  const int r = blockIdx.x * B_BLOCK + threadIdx.x;
  if( r >= count || !flags[r] ) return;
  const int s = segid[first + r];
  const ManySeg& S = segs[s];
  const int r0 = S.base - first;
  const uint32_t t0 = scanned[r0];
  S.tiles[scanned[r] - t0] = (uint32_t)( r - r0 );
  if( r == r0 ) { const uint32_t nt = scanned[r0 + S.n] - t0; S.tiles[nt] = (uint32_t)S.n; n_tiles[s] = (int)nt; }
}
// a cloud without points has the one closing entry
__global__ __launch_bounds__( B_BLOCK ) void k_many_tile_empty( const ManySeg* segs, int seg_first, int seg_count, int* n_tiles )
{
  const int k = blockIdx.x * B_BLOCK + threadIdx.x;
  if( k >= seg_count ) return;
  const ManySeg& S = segs[seg_first + k];
  if( S.n == 0 ) { S.tiles[0] = 0u; n_tiles[seg_first + k] = 0; }
}

void launch_many_segids( const int* offsets, int n_clouds, int n, int* segid, hipStream_t st )
{
  hipLaunchKernelGGL( k_many_segids, dim3( blocks_for( n ) ), dim3( B_BLOCK ), 0, st, offsets, n_clouds, n, segid );
}
void launch_many_bounds( const float* pos3, const float* nor3, const int* segid, const ManySeg* segs, int n, unsigned* out8, hipStream_t st )
{
  hipLaunchKernelGGL( k_many_bounds, dim3( blocks_for( n ) ), dim3( B_BLOCK ), 0, st, pos3, nor3, segid, segs, n, out8 );
}
void launch_many_mark( const float* pos3, const int* segid, const ManyTrial* trial, int first, int count, uint32_t* bits, hipStream_t st )
{
  hipLaunchKernelGGL( k_many_mark, dim3( blocks_for( count ) ), dim3( B_BLOCK ), 0, st, pos3, segid, trial, first, count, bits );
}
void launch_many_popcount( const uint32_t* bits, unsigned long long n_words, const unsigned long long* table_start, const int* table_seg, int n_tables,
                           int* occupied, hipStream_t st )
{
  const unsigned blocks = (unsigned)std::min<unsigned long long>( 16384ull, std::max<unsigned long long>( 1ull, ( n_words + B_BLOCK - 1 ) / B_BLOCK ) );
  hipLaunchKernelGGL( k_many_popcount, dim3( blocks ), dim3( B_BLOCK ), 0, st, bits, n_words, table_start, table_seg, n_tables, occupied );
}
void launch_many_cellids( const float* pos3, const int* segid, const ManySeg* segs, int first, int count, unsigned long long* key, uint32_t* local,
                          uint32_t* tables, hipStream_t st )
{
  hipLaunchKernelGGL( k_many_cellids, dim3( blocks_for( count ) ), dim3( B_BLOCK ), 0, st, pos3, segid, segs, first, count, key, local, tables );
}
void launch_many_gather( const float* pos3, const float* nor3, const int* segid, const ManySeg* segs, const uint32_t* order, int first, int count,
                         bool query_layout, hipStream_t st )
{
  hipLaunchKernelGGL( k_many_gather, dim3( blocks_for( count ) ), dim3( B_BLOCK ), 0, st, pos3, nor3, segid, segs, order, first, count, query_layout ? 1 : 0 );
}
void launch_many_count_runs( const unsigned long long* sorted, const int* segid, int first, int count, int* occupied, hipStream_t st )
{
  hipLaunchKernelGGL( k_many_count_runs, dim3( blocks_for( count ) ), dim3( B_BLOCK ), 0, st, sorted, segid, first, count, occupied );
}
void launch_many_hilbert( const float* pos3, const int* segid, const ManySeg* segs, int first, int count, unsigned long long* key, uint32_t* local, hipStream_t st )
{
  hipLaunchKernelGGL( k_many_hilbert, dim3( blocks_for( count ) ), dim3( B_BLOCK ), 0, st, pos3, segid, segs, first, count, key, local );
}
// flags[0 .. count] (relative to `first`; flags[count] = 0) = 1 where a tile starts; jump_a / jump_b: two scratch arrays of count words
void launch_many_tile_flags( const int* segid, const ManySeg* segs, int first, int count, uint32_t* flags, uint32_t* jump_a, uint32_t* jump_b, hipStream_t st )
{
  hipLaunchKernelGGL( k_many_tile_next, dim3( ( count + 63 ) / 64 ), dim3( 64 ), 0, st, segid, segs, first, count, jump_a );
  (void)hipMemsetAsync( flags, 0, ( (size_t)count + 1 ) * 4, st );
  (void)hipMemsetAsync( flags, 1, 1, st );                  // flags[0] = 1 (little endian), without a host word that must outlive the call
  for( long long reach = 1; reach < (long long)count; reach <<= 1 )
  {
    hipLaunchKernelGGL( k_build_tile_round, dim3( blocks_for( count ) ), dim3( B_BLOCK ), 0, st, jump_a, jump_b, flags, count );
    std::swap( jump_a, jump_b );
  }
}
void launch_many_tile_scatter( const uint32_t* flags, const uint32_t* scanned, const int* segid, const ManySeg* segs, int first, int count,
                               int seg_first, int seg_count, int* n_tiles, hipStream_t st )
{
  hipLaunchKernelGGL( k_many_tile_empty, dim3( blocks_for( seg_count ) ), dim3( B_BLOCK ), 0, st, segs, seg_first, seg_count, n_tiles );
  if( count > 0 ) hipLaunchKernelGGL( k_many_tile_scatter, dim3( blocks_for( count ) ), dim3( B_BLOCK ), 0, st, flags, scanned, segid, segs, first, count, n_tiles );
}
size_t build_sort64_temp_bytes( int n, int bits )
{
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs( nullptr, b, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, bits );
  return b;
}
int build_sort64_pairs( void* tmp, size_t bytes, const unsigned long long* kin, unsigned long long* kout, const uint32_t* vin, uint32_t* vout, int n,
                        int bits, hipStream_t st )
{
  return (int)hipcub::DeviceRadixSort::SortPairs( tmp, bytes, kin, kout, vin, vout, n, 0, bits, st );     // stable
}

} // namespace rs
