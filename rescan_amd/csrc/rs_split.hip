// The row that opens a sequence — seg2rsdb's pointcloud_to_rsdb (apps/seg2rsdb/main.cpp:80-136): a labelled scan cut into one
// object model per instance, every dynamic one moved so that its centroid sits over the origin: rs_hip_split_plan (host, rs_split.h),
// rs_hip_instance_table, rs_hip_split_by_instance, rs_hip_segment_centroids, rs_hip_scan_to_objects, rs_hip_cloud_split_objects.
//
// How a call runs:
//   1. k_split_table + k_split_compact      the distinct ids, their counts and first indices.  Ids are arbitrary int32, so the table is
//                                           open-addressed in global memory: 4 x MAX_INSTANCES slots of 64 bits, (1 << 32) | id, claimed
//                                           by a compare-and-swap of the empty word 0.  A wave first groups its 64 ids (they are mostly
//                                           equal): only a group's first lane claims the slot, lowers the slot's first index and adds the
//                                           group's size to its count.  A claim takes the next place of a dense list; a claim past
//                                           MAX_INSTANCES sets a flag and the call refuses.  Only that list (slot, id, first, count)
//                                           comes to the host, which orders it by first index — the reference's insertion order — and
//                                           hands every slot its rank back (k_split_ranks_to_slots).
//   2. the partition, one of two routes     LDS route (up to lds_ranks instances): a TILE is the 512 consecutive points of one wave.
//        k_split_hist                       rank[i] = the rank of ids[i] (a probe of the table); the wave counts its tile's points per
//                                           rank in LDS counters of its own, group by group, and writes them rank-major into a
//                                           [rank][tile] matrix.  One exclusive scan over the flattened matrix (hipCUB, rs_build.hip)
//                                           gives every (rank, tile) its first destination: all of rank r before any of rank r + 1, tile
//                                           by tile inside a rank.
//        k_split_scatter                    the wave loads its tile's destinations into the same LDS counters and walks its 8 rows of
//                                           64 points in order; within a row a point's slot is the counter of its rank plus the number
//                                           of lower lanes of the same rank (match by ballot, popcount below the lane), and the
//                                           group's first lane advances the counter by the group's size.  No global atomic; ids are
//                                           read once (k_split_hist), ranks once (k_split_scatter).
//        sort route                         above lds_ranks instances: a stable radix sort of (rank, index) pairs — the hipCUB call
//                                           rs_fuse.hip makes.  rs_hip_split_lds_ranks forces it, so that tests compare the two.
//   3. k_split_chain_blocks + _walk         the centroid sums: a summary per block of 512 points in parallel, then one wave per
//                                           (instance, axis) over the summaries in order, see below.
//   4. the host                             (float)( sum / n ), y = 0, msh_translate, msh_mat4_inverse for at most MAX_INSTANCES
//                                           objects (rs_split.h: finish_object, the code the plan runs).
//   5. k_split_apply                        one lane per output point: the scan point order[i], through msh_mat4_vec3_mul's operation
//                                           order when its instance is dynamic and as it is otherwise; written in output order.
//   6. the index builds                     rs_hip_cloud_split_objects: step 5 writes each segment where the index build of
//                                           rs_hip_cloud_create_level reads; one build per instance.
//
// THE CHAINS.  The reference adds a segment's coordinates one after the other into a double that starts at 0.0
// (rs_pointcloud.h:1326-1332).  A chain is cut into blocks of 512 addends (8 rows of 64, lane l of row j is addend 64 j + l), and for
// each block the walk tests whether the order of its additions can matter.  What the test needs of a block does not depend on the
// running sum — the smallest lowest-bit exponent, the largest magnitude, whether all addends are finite — so k_split_chain_blocks
// makes it for all blocks of all chains at once, one wave per block, together with the block's sum by a tree; k_split_chain_walk
// then meets the blocks of a chain in order with the running sum and takes a block's tree sum only where the condition holds (the
// condition bounds every partial sum of the tree too, so the tree sum was exact).  The gathers through `order`, which cost a lone
// wave walking its chain 8 us per block, are thereby spread over the whole device.
//
//   Condition.  Let S be the running sum, x_1 .. x_m the block's addends (floats widened to double, all finite), g the smallest
//   exponent of a lowest set bit over S and the x_i that are not zero (S and every x_i are integer multiples of 2^g),
//   A = m * max|x_i| (m a power of two, so A is exact and A >= sum|x_i|).  If S is finite and |S| + A < 2^(g+53), then the reference's
//   m sequential additions are all exact, and S + (x_1 + .. + x_m), the inner sum taken in ANY order in fp64, is the same double.
//
//   Proof.  Every partial result in question — a prefix S + x_1 + .. + x_k of the reference's chain, a partial sum of any subset of
//   the x_i inside a reduction tree, and S plus the block's sum — is an integer multiple of 2^g, because its terms are, and its
//   magnitude is at most |S| + sum|x_i| <= |S| + A < 2^(g+53).  An integer multiple q 2^g with |q| < 2^53 is a double (g >= -149 and
//   g + 53 <= 158 keep the exponent in range), so no addition in either evaluation rounds; both give the exact sum.  The test itself
//   is exact: 2^(g+53) - A is a multiple of 2^g below 2^(g+53), hence a double, so  A < 2^(g+53) && |S| < 2^(g+53) - A  decides
//   |S| + A < 2^(g+53) without rounding.  Zeros need no care: S is never -0.0 (it starts at +0.0, and x + (-x) is +0.0), so adding
//   +-0.0 leaves it as it is.
//
//   A block that fails the test is tried row by row (m = 64) with the same condition; a row that fails — and any row with an Inf
//   or NaN addend, or met with S not finite — is added one addend after the other in fp64, in the reference's order.
//   rs_hip_split_chains_sequential() reports how many addends of the last call went that way.
#include "rs_host.h"
#include "rs_split.h"

#include <chrono>
#include <climits>
#include <cstring>
#include <numeric>
#include <vector>

namespace rs {

constexpr int SPLIT_BLOCK = 256;
constexpr int SPLIT_WAVES = SPLIT_BLOCK / 64;
constexpr int SPLIT_ROWS = 8;
constexpr int SPLIT_TILE = 64 * SPLIT_ROWS;                  // the points of one wave: one column of the [rank][tile] matrix
constexpr uint32_t SPLIT_SLOT_BITS = 14;
constexpr uint32_t SPLIT_SLOTS = 1u << SPLIT_SLOT_BITS;      // 4 x MAX_INSTANCES: the probes stay short up to the refusal
constexpr int SPLIT_LDS_RANKS_MAX = 2048;                    // 4 waves x 2048 counters x 4 bytes = 32 KiB of LDS
constexpr int SPLIT_LDS_RANKS_DEFAULT = 1024;
constexpr size_t SPLIT_MATRIX_MAX = (size_t)1 << 26;         // entries of the [rank][tile] matrix beyond which the sort route runs
constexpr int CHAIN_ROWS = 8;
constexpr int CHAIN_BLOCK = 64 * CHAIN_ROWS;
static_assert( SPLIT_SLOTS >= 4u * (uint32_t)split::MAX_INSTANCES, "the table must stay sparse up to the refusal" );

// slot: SPLIT_SLOTS words (0: empty, else (1 << 32) | id); first / count: per slot; claimed: the slots in order of their claims;
// header[0]: claims, header[1]: overflow; slot_rank: per slot, the rank the host gave its id
struct SplitTable { unsigned long long* slot; uint32_t* first; uint32_t* count; uint32_t* claimed; uint32_t* header; int32_t* slot_rank; };

__device__ __forceinline__ uint32_t split_hash( int32_t key ) { return ( (uint32_t)key * 2654435761u ) >> ( 32 - SPLIT_SLOT_BITS ); }

__device__ void split_insert( const SplitTable& T, int32_t key, uint32_t index, uint32_t size )
{
  const unsigned long long want = ( 1ull << 32 ) | (unsigned long long)(uint32_t)key;
  uint32_t h = split_hash( key );
  for( uint32_t probe = 0; probe < SPLIT_SLOTS; ++probe, h = ( h + 1u ) & ( SPLIT_SLOTS - 1u ) )
  {
    unsigned long long cur = __hip_atomic_load( &T.slot[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
    if( cur == 0ull )
    {
      cur = atomicCAS( &T.slot[h], 0ull, want );
      if( cur == 0ull )
      {
        const uint32_t c = atomicAdd( &T.header[0], 1u );
        if( c < (uint32_t)split::MAX_INSTANCES ) T.claimed[c] = h; else T.header[1] = 1u;
        cur = want;
      }
    }
    if( cur == want ) { atomicMin( &T.first[h], index ); atomicAdd( &T.count[h], size ); return; }
  }
  T.header[1] = 1u;                                         // (a full table: only after the refusal is certain)
}
// the rank of an id the table holds
__device__ __forceinline__ uint32_t split_rank_of( const SplitTable& T, int32_t key )
{
  const unsigned long long want = ( 1ull << 32 ) | (unsigned long long)(uint32_t)key;
  uint32_t h = split_hash( key );
  for( uint32_t probe = 0; probe < SPLIT_SLOTS; ++probe, h = ( h + 1u ) & ( SPLIT_SLOTS - 1u ) )
    if( T.slot[h] == want ) return (uint32_t)T.slot_rank[h];
  return 0u;                                                // (never: every id of the scan was inserted)
}

// A wave's lanes grouped by key, one group per turn of the loop: `leader` is the group's first lane, `mask` its lanes.  f( mask ) runs
// on every lane of the group.  The loop is wave-uniform.
template <class F> __device__ __forceinline__ void split_groups( bool active, uint32_t key, F f )
{
  const int lane = threadIdx.x & 63;
  bool todo = active;
  for( ;; )
  {
    const unsigned long long rem = __ballot( todo );
    if( !rem ) break;
    const int leader = __ffsll( (long long)rem ) - 1;
    const uint32_t k = (uint32_t)__shfl( (int)key, leader );
    const bool mine = todo && key == k;
    const unsigned long long mask = __ballot( mine );
    if( mine ) { f( mask, lane == leader ); todo = false; }
  }
}

__global__ __launch_bounds__( SPLIT_BLOCK ) void k_split_table( const int32_t* ids, int n, SplitTable T )
{
  const int i = blockIdx.x * SPLIT_BLOCK + threadIdx.x;
  const bool active = i < n;
  const int32_t key = active ? ids[i] : 0;
  // (lanes are in index order: the group's first lane carries its smallest index)
  split_groups( active, (uint32_t)key, [&]( unsigned long long mask, bool leader ) {
    if( leader ) split_insert( T, key, (uint32_t)i, (uint32_t)__popcll( mask ) );
  } );
}
// entry c of the dense list: { slot, id, first, count }
__global__ __launch_bounds__( SPLIT_BLOCK ) void k_split_compact( SplitTable T, uint4* entries )
{
  const uint32_t c = blockIdx.x * SPLIT_BLOCK + threadIdx.x;
  if( c >= (uint32_t)split::MAX_INSTANCES || c >= T.header[0] ) return;
  const uint32_t h = T.claimed[c];
  entries[c] = make_uint4( h, (uint32_t)( T.slot[h] & 0xFFFFFFFFull ), T.first[h], T.count[h] );
}
__global__ __launch_bounds__( SPLIT_BLOCK ) void k_split_ranks_to_slots( SplitTable T, const int32_t* rank_of_claim, int n_claims )
{
  const int c = blockIdx.x * SPLIT_BLOCK + threadIdx.x;
  if( c < n_claims ) T.slot_rank[T.claimed[c]] = rank_of_claim[c];
}

// rank (n entries) for both routes; iota (may be null): the sort route's values; hist (may be null): the [rank][tile] matrix of the
// LDS route, n_ranks x n_tiles, every entry written.  Dynamic LDS: SPLIT_WAVES x n_ranks counters when hist is given.
__global__ __launch_bounds__( SPLIT_BLOCK ) void k_split_hist( const int32_t* ids, int n, SplitTable T, uint32_t* rank, uint32_t* iota, uint32_t* hist, int n_ranks, int n_tiles )
{
  extern __shared__ uint32_t s_cnt[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * SPLIT_WAVES + wave;
  uint32_t* cnt = s_cnt + (size_t)wave * n_ranks;
  if( hist ) for( int r = lane; r < n_ranks; r += 64 ) cnt[r] = 0u;
  __syncthreads();
  for( int j = 0; j < SPLIT_ROWS; ++j )
  {
    const long long i = (long long)tile * SPLIT_TILE + j * 64 + lane;
    const bool active = i < n;
    uint32_t r = 0u;
    if( active )
    {
      r = min( split_rank_of( T, ids[i] ), (uint32_t)( n_ranks - 1 ) );    // (the clamp is never taken: it keeps cnt[r] in bounds)
      rank[i] = r;
      if( iota ) iota[i] = (uint32_t)i;
    }
    if( hist )
      split_groups( active, r, [&]( unsigned long long mask, bool leader ) { if( leader ) cnt[r] += (uint32_t)__popcll( mask ); } );
  }
  __syncthreads();
  if( hist && tile < n_tiles ) for( int r = lane; r < n_ranks; r += 64 ) hist[(size_t)r * n_tiles + tile] = cnt[r];
}

// dest: the exclusive scan of hist.  order[dest] = i.
__global__ __launch_bounds__( SPLIT_BLOCK ) void k_split_scatter( const uint32_t* rank, int n, const uint32_t* dest, int n_ranks, int n_tiles, int32_t* order )
{
  extern __shared__ uint32_t s_cnt[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * SPLIT_WAVES + wave;
  uint32_t* cnt = s_cnt + (size_t)wave * n_ranks;
  if( tile < n_tiles ) for( int r = lane; r < n_ranks; r += 64 ) cnt[r] = dest[(size_t)r * n_tiles + tile];
  __syncthreads();
  const unsigned long long below = ( 1ull << lane ) - 1ull;
  for( int j = 0; j < SPLIT_ROWS; ++j )
  {
    const long long i = (long long)tile * SPLIT_TILE + j * 64 + lane;
    const bool active = i < n;
    const uint32_t r = active ? min( rank[i], (uint32_t)( n_ranks - 1 ) ) : 0u;
    split_groups( active, r, [&]( unsigned long long mask, bool leader ) {
      uint32_t base = 0u;
      if( leader ) { base = cnt[r]; cnt[r] = base + (uint32_t)__popcll( mask ); }
      base = (uint32_t)__shfl( (int)base, __ffsll( (long long)mask ) - 1 );
      const uint32_t at = base + (uint32_t)__popcll( mask & below );
      if( at < (uint32_t)n ) order[at] = (int32_t)i;        // (always: the destinations partition [0, n))
    } );
    __syncthreads();                                        // (uniform: every wave runs SPLIT_ROWS turns; orders the LDS updates of successive rows)
  }
}

// The scan's points for a reader: packed xyz arrays, or a cloud's query layout read through its original -> slot map.
// n: the number of points; an index outside [0, n) — none is ever made — reads point 0 instead of foreign memory.
struct SplitSrc { const float* pos3; const float* nor3; const float4* qpos; const float4* qnor; const int* by_orig; int n; };

__device__ __forceinline__ float split_coord( const SplitSrc& S, int o, int axis )
{
  if( (unsigned)o >= (unsigned)S.n ) o = 0;
  if( S.qpos ) { const float4 a = S.qpos[S.by_orig[o]]; return axis == 0 ? a.x : axis == 1 ? a.y : a.z; }
  return S.pos3[3 * (size_t)o + axis];
}

// the exponent of the lowest set bit of a finite, non-zero, normal double
__device__ __forceinline__ int chain_low_bit( double v )
{
  const unsigned long long b = (unsigned long long)__double_as_longlong( v );
  const unsigned long long m = ( b & 0xFFFFFFFFFFFFFull ) | ( 1ull << 52 );
  return (int)( ( b >> 52 ) & 0x7FFull ) - 1075 + ( __ffsll( (long long)m ) - 1 );
}
__device__ __forceinline__ double wave_sum( double v )   { for( int d = 32; d; d >>= 1 ) v += __shfl_xor( v, d ); return v; }
__device__ __forceinline__ double wave_max( double v )   { for( int d = 32; d; d >>= 1 ) v = fmax( v, __shfl_xor( v, d ) ); return v; }
__device__ __forceinline__ int    wave_min( int v )      { for( int d = 32; d; d >>= 1 ) v = min( v, __shfl_xor( v, d ) ); return v; }

// the condition of the header comment for m addends of largest magnitude amax and lowest bit g (amax > 0), wave-uniform arguments
__device__ __forceinline__ bool chain_order_free( double S, int g, double amax, double m )
{
  if( !( fabs( S ) < INFINITY ) ) return false;            // S finite (false for NaN too)
  if( S != 0.0 ) g = min( g, chain_low_bit( S ) );
  const double lim = ldexp( 1.0, g + 53 ), A = m * amax;
  return A < lim && fabs( S ) < lim - A;
}

// What k_split_chain_blocks leaves of one block of one axis: the block's sum by a tree (exact whenever the walk uses it, see the
// header comment), the largest magnitude, the smallest lowest-bit exponent over its non-zero addends, whether all are finite.
struct ChainSummary { double sum, amax; int g, fin; };

// One wave per block of CHAIN_BLOCK consecutive points of a segment, all three axes.  block_first[k]: the first block of instance k
// (n_instances + 1 entries).  out[3 block + axis].
__global__ __launch_bounds__( 64 ) void k_split_chain_blocks( SplitSrc S, const int32_t* order, const long long* offsets, const int* block_first, int n_instances, ChainSummary* out )
{
  const int bid = blockIdx.x, lane = threadIdx.x;
  int lo = 0, hi = n_instances;                                            // the last k with block_first[k] <= bid
  while( hi - lo > 1 ) { const int mid = ( lo + hi ) >> 1; if( block_first[mid] <= bid ) lo = mid; else hi = mid; }
  const int k = lo;
  const long long e = offsets[k + 1], at = offsets[k] + (long long)( bid - block_first[k] ) * CHAIN_BLOCK;
  double part[3] = { 0.0, 0.0, 0.0 }, amax[3] = { 0.0, 0.0, 0.0 };
  int g[3] = { INT_MAX, INT_MAX, INT_MAX };
  bool fin[3] = { true, true, true };
#pragma unroll
  for( int j = 0; j < CHAIN_ROWS; ++j )
  {
    const long long i = at + j * 64 + lane;
    if( i >= e ) continue;
    const int o = order[i];
#pragma unroll
    for( int a = 0; a < 3; ++a )
    {
      const double x = (double)split_coord( S, o, a ), ax = fabs( x );
      const bool f = ax < INFINITY;
      fin[a] = fin[a] && f;
      if( f ) { amax[a] = fmax( amax[a], ax ); if( x != 0.0 ) g[a] = min( g[a], chain_low_bit( x ) ); }
      part[a] += x;
    }
  }
#pragma unroll
  for( int a = 0; a < 3; ++a )
  {
    ChainSummary m;
    m.fin = __all( fin[a] ) ? 1 : 0; m.amax = wave_max( amax[a] ); m.g = wave_min( g[a] ); m.sum = wave_sum( part[a] );
    if( lane == 0 ) out[3 * (size_t)bid + a] = m;
  }
}

// The block at `at` of a chain whose block-wide test failed, row by row: a row of 64 addends is order-free under the same
// condition, or is added one addend after the other.
__device__ __forceinline__ void chain_rows( const SplitSrc& S, const int32_t* order, long long at, long long e, int axis, int lane, double& sum, unsigned long long& one_by_one )
{
  double cur[CHAIN_ROWS];
#pragma unroll
  for( int j = 0; j < CHAIN_ROWS; ++j )
  {
    const long long i = at + j * 64 + lane;
    cur[j] = i < e ? (double)split_coord( S, order[i], axis ) : 0.0;       // (padding: +0.0 changes no sum)
  }
#pragma unroll
  for( int j = 0; j < CHAIN_ROWS; ++j )
  {
    const double x = cur[j], ax = fabs( x );
    const bool f = ax < INFINITY;
    const bool row_fin = __all( f );
    const double a = wave_max( f ? ax : 0.0 ); const int gr = wave_min( ( f && x != 0.0 ) ? chain_low_bit( x ) : INT_MAX );
    if( row_fin && a == 0.0 ) continue;                                    // zeros only: the sum stays as it is
    if( row_fin && chain_order_free( sum, gr, a, 64.0 ) ) { sum += wave_sum( x ); continue; }
    const long long first = at + j * 64;
    const int m = (int)min( 64ll, e - first );
    for( int l = 0; l < m; ++l ) sum += __shfl( x, l );                    // the reference's order
    one_by_one += (unsigned long long)max( m, 0 );
  }
}

// One wave per (instance, axis): the chain over its blocks' summaries, in order.  sums[3 k + axis]; sequential: addends added one by
// one, summed over the chains.
__global__ __launch_bounds__( 64 ) void k_split_chain_walk( SplitSrc S, const int32_t* order, const long long* offsets, const int* block_first, const ChainSummary* summaries,
                                                            double* sums, unsigned long long* sequential )
{
  const int k = blockIdx.x / 3, axis = blockIdx.x % 3, lane = threadIdx.x;
  const long long b = offsets[k], e = offsets[k + 1];
  const int base = block_first[k], n_blocks = block_first[k + 1] - base;
  double sum = 0.0;
  unsigned long long one_by_one = 0ull;
  for( int c0 = 0; c0 < n_blocks; c0 += 64 )
  {
    const int cnt = min( 64, n_blocks - c0 );
    ChainSummary mine; mine.sum = 0.0; mine.amax = 0.0; mine.g = INT_MAX; mine.fin = 1;
    if( lane < cnt ) mine = summaries[3 * (size_t)( base + c0 + lane ) + axis];
    for( int l = 0; l < cnt; ++l )
    {
      const double block_sum = __shfl( mine.sum, l ), amax = __shfl( mine.amax, l );
      const int g = __shfl( mine.g, l ), fin = __shfl( mine.fin, l );
      if( fin && amax == 0.0 ) continue;                                   // zeros only
      if( fin && chain_order_free( sum, g, amax, (double)CHAIN_BLOCK ) ) { sum += block_sum; continue; }
      chain_rows( S, order, b + (long long)( c0 + l ) * CHAIN_BLOCK, e, axis, lane, sum, one_by_one );
    }
  }
  if( lane == 0 )
  {
    sums[blockIdx.x] = sum;
    if( one_by_one ) atomicAdd( sequential, one_by_one );
  }
}

// the same sums by a lone lane per chain adding in the reference's order: the form the block step is measured against
__global__ __launch_bounds__( 64 ) void k_split_chains_lone( SplitSrc S, const int32_t* order, const long long* offsets, int n_chains, double* sums )
{
  const int c = blockIdx.x * 64 + threadIdx.x;
  if( c >= n_chains ) return;
  const int k = c / 3, axis = c % 3;
  double sum = 0.0;
  for( long long i = offsets[k]; i < offsets[k + 1]; ++i ) sum += (double)split_coord( S, order[i], axis );
  sums[c] = sum;
}

// One lane per output point: point first + t of the instance-major order, written at t; its instance is found in offsets
// (n_instances + 1 entries).
struct SplitApplyArgs
{
  SplitSrc S; const int32_t* order; const long long* offsets; const float* xforms; const int32_t* is_static;
  int n_instances; long long first, count; float* out_pos; float* out_nor;
};

__global__ __launch_bounds__( SPLIT_BLOCK ) void k_split_apply( SplitApplyArgs A )
{
  const long long t = (long long)blockIdx.x * SPLIT_BLOCK + threadIdx.x;
  if( t >= A.count ) return;
  const long long i = A.first + t;
  int lo = 0, hi = A.n_instances;                                          // the last k with offsets[k] <= i
  while( hi - lo > 1 ) { const int mid = ( lo + hi ) >> 1; if( A.offsets[mid] <= i ) lo = mid; else hi = mid; }
  const int k = lo;
  int o = A.order[i];
  if( (unsigned)o >= (unsigned)A.S.n ) o = 0;
  float p[3], q[3] = { 0.0f, 0.0f, 0.0f };
  const bool with_nor = A.out_nor != nullptr;
  if( A.S.qpos )
  {
    const int s = A.S.by_orig[o];
    const float4 a = A.S.qpos[s]; p[0] = a.x; p[1] = a.y; p[2] = a.z;
    if( with_nor ) { const float4 c = A.S.qnor[s]; q[0] = c.x; q[1] = c.y; q[2] = c.z; }
  }
  else
  {
    const size_t s = 3 * (size_t)o;
    p[0] = A.S.pos3[s]; p[1] = A.S.pos3[s + 1]; p[2] = A.S.pos3[s + 2];
    if( with_nor ) { q[0] = A.S.nor3[s]; q[1] = A.S.nor3[s + 1]; q[2] = A.S.nor3[s + 2]; }
  }
  if( !A.is_static[k] )
  {
    float m[16];
#pragma unroll
    for( int c = 0; c < 16; ++c ) m[c] = A.xforms[16 * (size_t)k + c];
    float pp[3], qq[3];
    split::xform3( m, p, 1.0f, pp ); split::xform3( m, q, 0.0f, qq );
    p[0] = pp[0]; p[1] = pp[1]; p[2] = pp[2]; q[0] = qq[0]; q[1] = qq[1]; q[2] = qq[2];
  }
  const size_t d = 3 * (size_t)t;
  A.out_pos[d] = p[0]; A.out_pos[d + 1] = p[1]; A.out_pos[d + 2] = p[2];
  if( with_nor ) { A.out_nor[d] = q[0]; A.out_nor[d + 1] = q[1]; A.out_nor[d + 2] = q[2]; }
}

} // namespace rs

using namespace rs;

namespace {

struct SplitWorkspace { Buf table, entries, claim_rank, ids, rank, iota, skey, order, hist, dest, tmp, offsets, chain_first, chain_blocks, sums, xforms, is_static, pos, nor, out_pos, out_nor; };
thread_local SplitWorkspace g_split_ws;
thread_local int g_split_lds_ranks = SPLIT_LDS_RANKS_DEFAULT;
thread_local int64_t g_split_sequential = 0;
thread_local int g_split_chains_form = 0;                   // 0: the block step, 1: a lone lane per chain (rs_hip_split_chains_form)
// wall clock of the calling thread between the call's own synchronisations (rs_hip_split_seconds)
thread_local double g_split_s[5] = { 0, 0, 0, 0, 0 };
thread_local bool g_split_clock = false;

struct SplitClock
{
  hipStream_t st; std::chrono::steady_clock::time_point last;
  explicit SplitClock( hipStream_t s ) : st( s ), last( std::chrono::steady_clock::now() ) {}
  // (only with the clock on: a synchronisation the call would not need, so that the lap is the stage's own)
  void lap( int k )
  {
    if( !g_split_clock ) return;
    (void)hipStreamSynchronize( st );
    const auto now = std::chrono::steady_clock::now();
    g_split_s[k] += std::chrono::duration<double>( now - last ).count(); last = now;
  }
};

// the table's arrays inside one buffer
SplitTable split_table_view()
{
  SplitWorkspace& W = g_split_ws;
  char* p = (char*)W.table.p;
  SplitTable T;
  T.slot = (unsigned long long*)p;                           p += (size_t)SPLIT_SLOTS * 8;
  T.count = (uint32_t*)p;                                    p += (size_t)SPLIT_SLOTS * 4;
  T.header = (uint32_t*)p;                                   p += 256;
  T.first = (uint32_t*)p;                                    p += (size_t)SPLIT_SLOTS * 4;
  T.claimed = (uint32_t*)p;                                  p += (size_t)split::MAX_INSTANCES * 4;
  T.slot_rank = (int32_t*)p;
  return T;
}
constexpr size_t SPLIT_TABLE_ZERO = (size_t)SPLIT_SLOTS * 12 + 256;                                        // slot, count, header
constexpr size_t SPLIT_TABLE_BYTES = SPLIT_TABLE_ZERO + (size_t)SPLIT_SLOTS * 4 + (size_t)split::MAX_INSTANCES * 4 + (size_t)SPLIT_SLOTS * 4;

// The table of the n >= 1 ids in d_ids, ordered by first index, in T; the device keeps every slot's rank for the partition.
int split_table_device( const int32_t* d_ids, int n, split::Table& T, hipStream_t st )
{
  SplitWorkspace& W = g_split_ws;
  RS_TRY( W.table.ensure( SPLIT_TABLE_BYTES ), "split: buffers" );
  RS_TRY( W.entries.ensure( (size_t)split::MAX_INSTANCES * 16 ), "split: buffers" );
  RS_TRY( W.claim_rank.ensure( (size_t)split::MAX_INSTANCES * 4 ), "split: buffers" );
  const SplitTable D = split_table_view();
  RS_TRY( hipMemsetAsync( D.slot, 0, SPLIT_TABLE_ZERO, st ), "split: table reset" );
  RS_TRY( hipMemsetAsync( D.first, 0xFF, (size_t)SPLIT_SLOTS * 4, st ), "split: table reset" );
  {
    ProfSpan span( "split_table" );
    hipLaunchKernelGGL( k_split_table, dim3( blocks_for( n, SPLIT_BLOCK ) ), dim3( SPLIT_BLOCK ), 0, st, d_ids, n, D );
    hipLaunchKernelGGL( k_split_compact, dim3( blocks_for( split::MAX_INSTANCES, SPLIT_BLOCK ) ), dim3( SPLIT_BLOCK ), 0, st, D, W.entries.as<uint4>() );
  }
  RS_TRY( hipGetLastError(), "split: table launch" );
  uint32_t header[2] = { 0, 0 };
  RS_TRY_DRAIN( st, hipMemcpyAsync( header, D.header, 8, hipMemcpyDeviceToHost, st ), "split: download" );
  RS_TRY( hipStreamSynchronize( st ), "split: table" );
  if( header[1] || header[0] > (uint32_t)split::MAX_INSTANCES )
  {
    char msg[128]; snprintf( msg, sizeof(msg), "split: more than %d distinct instance ids", (int)split::MAX_INSTANCES );
    return fail( RS_HIP_E_CAPACITY, msg );
  }
  const int I = (int)header[0];
  std::vector<uint32_t> e( (size_t)I * 4 );
  RS_TRY_DRAIN( st, hipMemcpyAsync( e.data(), W.entries.p, (size_t)I * 16, hipMemcpyDeviceToHost, st ), "split: download" );
  RS_TRY( hipStreamSynchronize( st ), "split: table" );
  // the reference's insertion order: by first index (no two ids share one)
  std::vector<int32_t> by_first( (size_t)I ), rank_of_claim( (size_t)I );
  std::iota( by_first.begin(), by_first.end(), 0 );
  std::sort( by_first.begin(), by_first.end(), [&]( int32_t a, int32_t b ) { return e[4 * (size_t)a + 2] < e[4 * (size_t)b + 2]; } );
  T.ids.resize( (size_t)I ); T.counts.resize( (size_t)I ); T.first.resize( (size_t)I );
  for( int r = 0; r < I; ++r )
  {
    const size_t c = (size_t)by_first[(size_t)r];
    rank_of_claim[c] = r;
    T.ids[(size_t)r] = (int32_t)e[4 * c + 1]; T.first[(size_t)r] = (int64_t)e[4 * c + 2]; T.counts[(size_t)r] = (int64_t)e[4 * c + 3];
  }
  RS_TRY_DRAIN( st, hipMemcpyAsync( W.claim_rank.p, rank_of_claim.data(), (size_t)I * 4, hipMemcpyHostToDevice, st ), "split: upload" );
  hipLaunchKernelGGL( k_split_ranks_to_slots, dim3( blocks_for( I, SPLIT_BLOCK ) ), dim3( SPLIT_BLOCK ), 0, st, D, W.claim_rank.as<int32_t>(), I );
  RS_TRY_DRAIN( st, hipGetLastError(), "split: ranks launch" );
  RS_TRY( hipStreamSynchronize( st ), "split: ranks" );       // (rank_of_claim leaves scope)
  return RS_HIP_OK;
}

// the LDS route serves n_ranks instances of n points
bool split_lds_route( int n, int n_ranks )
{
  const size_t n_tiles = ( (size_t)n + SPLIT_TILE - 1 ) / SPLIT_TILE;
  return n_ranks <= g_split_lds_ranks && (size_t)n_ranks * n_tiles <= SPLIT_MATRIX_MAX;
}

// order (workspace, n entries): the stable multiway partition of the n >= 1 points by the ranks split_table_device left
int split_partition_device( const int32_t* d_ids, int n, int n_ranks, hipStream_t st )
{
  SplitWorkspace& W = g_split_ws;
  const SplitTable D = split_table_view();
  RS_TRY( W.rank.ensure( (size_t)n * 4 ), "split: buffers" ); RS_TRY( W.order.ensure( (size_t)n * 4 ), "split: buffers" );
  const int n_tiles = (int)( ( (size_t)n + SPLIT_TILE - 1 ) / SPLIT_TILE );
  const unsigned grid = blocks_for( n_tiles, SPLIT_WAVES );
  if( split_lds_route( n, n_ranks ) )
  {
    const size_t cells = (size_t)n_ranks * (size_t)n_tiles, lds = (size_t)SPLIT_WAVES * (size_t)n_ranks * 4;
    const size_t tmp_bytes = build_scan_temp_bytes( cells );
    RS_TRY( W.hist.ensure( cells * 4 ), "split: buffers" ); RS_TRY( W.dest.ensure( cells * 4 ), "split: buffers" );
    RS_TRY( W.tmp.ensure( tmp_bytes + 256 ), "split: buffers" );
    ProfSpan span( "split_partition" );
    hipLaunchKernelGGL( k_split_hist, dim3( grid ), dim3( SPLIT_BLOCK ), lds, st, d_ids, n, D, W.rank.as<uint32_t>(), (uint32_t*)nullptr, W.hist.as<uint32_t>(), n_ranks, n_tiles );
    if( build_exclusive_scan( W.tmp.p, tmp_bytes, W.hist.as<uint32_t>(), W.dest.as<uint32_t>(), cells, st ) )
      return fail( RS_HIP_E_RUNTIME, "split: device scan failed" );
    hipLaunchKernelGGL( k_split_scatter, dim3( grid ), dim3( SPLIT_BLOCK ), lds, st, W.rank.as<uint32_t>(), n, W.dest.as<uint32_t>(), n_ranks, n_tiles, W.order.as<int32_t>() );
  }
  else
  {
    int key_bits = 1; while( key_bits < 32 && ( 1ll << key_bits ) < (long long)n_ranks ) ++key_bits;
    const size_t tmp_bytes = build_sort_temp_bytes( n, key_bits );
    RS_TRY( W.iota.ensure( (size_t)n * 4 ), "split: buffers" ); RS_TRY( W.skey.ensure( (size_t)n * 4 ), "split: buffers" );
    RS_TRY( W.tmp.ensure( tmp_bytes + 256 ), "split: buffers" );
    ProfSpan span( "split_partition" );
    hipLaunchKernelGGL( k_split_hist, dim3( grid ), dim3( SPLIT_BLOCK ), 0, st, d_ids, n, D, W.rank.as<uint32_t>(), W.iota.as<uint32_t>(), (uint32_t*)nullptr, n_ranks, n_tiles );
    // stable, and the indices go in increasing: equal ranks keep their points in input order
    if( build_sort_pairs( W.tmp.p, tmp_bytes, W.rank.as<uint32_t>(), W.skey.as<uint32_t>(), W.iota.as<uint32_t>(), (uint32_t*)W.order.p, n, key_bits, st ) )
      return fail( RS_HIP_E_RUNTIME, "split: device sort failed" );
  }
  RS_TRY( hipGetLastError(), "split: partition launch" );
  return RS_HIP_OK;
}

// sums (host, 3 per instance) of the chains over the workspace's order; offsets (host, n_instances + 1) go to the device and stay there
int split_chains_device( const SplitSrc& S, const int64_t* offsets, int n_instances, double* sums, hipStream_t st )
{
  SplitWorkspace& W = g_split_ws;
  const int n_chains = 3 * n_instances;
  RS_TRY( W.offsets.ensure( ( (size_t)n_instances + 1 ) * 8 ), "split: buffers" );
  RS_TRY( W.sums.ensure( (size_t)n_chains * 8 + 8 ), "split: buffers" );
  unsigned long long* d_seq = (unsigned long long*)( W.sums.as<double>() + n_chains );
  RS_TRY( hipMemcpyAsync( W.offsets.p, offsets, ( (size_t)n_instances + 1 ) * 8, hipMemcpyHostToDevice, st ), "split: upload" );
  RS_TRY_DRAIN( st, hipMemsetAsync( d_seq, 0, 8, st ), "split: chains reset" );
  // the blocks of CHAIN_BLOCK points every segment is cut into
  std::vector<int> block_first( (size_t)n_instances + 1, 0 );
  for( int k = 0; k < n_instances; ++k )
    block_first[(size_t)k + 1] = block_first[(size_t)k] + (int)( ( offsets[k + 1] - offsets[k] + CHAIN_BLOCK - 1 ) / CHAIN_BLOCK );
  const int n_blocks = block_first[(size_t)n_instances];
  RS_TRY_DRAIN( st, W.chain_first.ensure( block_first.size() * 4 ), "split: buffers" );
  RS_TRY_DRAIN( st, W.chain_blocks.ensure( std::max<size_t>( 1, (size_t)n_blocks ) * 3 * sizeof(ChainSummary) ), "split: buffers" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( W.chain_first.p, block_first.data(), block_first.size() * 4, hipMemcpyHostToDevice, st ), "split: upload" );
  {
    ProfSpan span( "split_chains" );
    if( g_split_chains_form == 0 )
    {
      if( n_blocks > 0 )
        hipLaunchKernelGGL( k_split_chain_blocks, dim3( n_blocks ), dim3( 64 ), 0, st, S, W.order.as<int32_t>(), W.offsets.as<long long>(), W.chain_first.as<int>(), n_instances,
                            W.chain_blocks.as<ChainSummary>() );
      hipLaunchKernelGGL( k_split_chain_walk, dim3( n_chains ), dim3( 64 ), 0, st, S, W.order.as<int32_t>(), W.offsets.as<long long>(), W.chain_first.as<int>(),
                          W.chain_blocks.as<ChainSummary>(), W.sums.as<double>(), d_seq );
    }
    else
      hipLaunchKernelGGL( k_split_chains_lone, dim3( blocks_for( n_chains, 64 ) ), dim3( 64 ), 0, st, S, W.order.as<int32_t>(), W.offsets.as<long long>(), n_chains, W.sums.as<double>() );
  }
  RS_TRY_DRAIN( st, hipGetLastError(), "split: chains launch" );
  unsigned long long seq = 0;
  RS_TRY_DRAIN( st, hipMemcpyAsync( sums, W.sums.p, (size_t)n_chains * 8, hipMemcpyDeviceToHost, st ), "split: download" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( &seq, d_seq, 8, hipMemcpyDeviceToHost, st ), "split: download" );
  RS_TRY( hipStreamSynchronize( st ), "split: chains" );
  g_split_sequential = g_split_chains_form == 0 ? (int64_t)seq : offsets[n_instances] * 3;
  return RS_HIP_OK;
}

// what the host derives from the table and the sums, in the caller's arrays and in vectors for the apply step
struct SplitObjects { std::vector<int64_t> offsets; std::vector<int32_t> class_of, is_static; std::vector<double> sums; std::vector<float> centroids, xforms, poses; };

void split_write_outputs( const split::Table& T, const SplitObjects& O, const rs_hip_split_out_t* out )
{
  if( !out ) return;
  const size_t I = T.ids.size();
  if( out->n_instances ) *out->n_instances = (int32_t)I;
  if( out->inst_ids ) std::memcpy( out->inst_ids, T.ids.data(), I * 4 );
  if( out->counts ) std::memcpy( out->counts, T.counts.data(), I * 8 );
  if( out->first ) std::memcpy( out->first, T.first.data(), I * 8 );
  if( out->offsets ) std::memcpy( out->offsets, O.offsets.data(), ( I + 1 ) * 8 );
  if( out->class_of ) std::memcpy( out->class_of, O.class_of.data(), I * 4 );
  if( out->is_static ) std::memcpy( out->is_static, O.is_static.data(), I * 4 );
  if( out->sums ) std::memcpy( out->sums, O.sums.data(), I * 24 );
  if( out->centroids ) std::memcpy( out->centroids, O.centroids.data(), I * 12 );
  if( out->xforms ) std::memcpy( out->xforms, O.xforms.data(), I * 64 );
  if( out->poses ) std::memcpy( out->poses, O.poses.data(), I * 64 );
}

// Steps 1-4 for the n >= 1 points of S whose ids are in the workspace; xforms / is_static / offsets / order are on the device afterwards.
int split_objects_device( const SplitSrc& S, int n, const int32_t* class_ids, const int32_t* static_classes, int32_t n_static,
                          split::Table& T, SplitObjects& O, SplitClock& clk, hipStream_t st )
{
  SplitWorkspace& W = g_split_ws;
  int rc = split_table_device( W.ids.as<int32_t>(), n, T, st ); if( rc ) return rc;
  clk.lap( 0 );
  const int I = (int)T.ids.size();
  rc = split_partition_device( W.ids.as<int32_t>(), n, I, st ); if( rc ) return rc;
  clk.lap( 1 );
  O.offsets.assign( (size_t)I + 1, 0 );
  for( int k = 0; k < I; ++k ) O.offsets[(size_t)k + 1] = O.offsets[(size_t)k] + T.counts[(size_t)k];
  O.sums.assign( (size_t)I * 3, 0.0 );
  rc = split_chains_device( S, O.offsets.data(), I, O.sums.data(), st ); if( rc ) return rc;
  clk.lap( 2 );
  O.class_of.resize( (size_t)I ); O.is_static.resize( (size_t)I );
  O.centroids.resize( (size_t)I * 3 ); O.xforms.resize( (size_t)I * 16 ); O.poses.resize( (size_t)I * 16 );
  for( int k = 0; k < I; ++k )
  {
    const int32_t cls = class_ids[T.first[(size_t)k]];                     // main.cpp:114
    const bool stat = split::class_is_static( cls, static_classes, n_static );
    O.class_of[(size_t)k] = cls; O.is_static[(size_t)k] = stat ? 1 : 0;
    split::finish_object( &O.sums[3 * (size_t)k], T.counts[(size_t)k], stat, &O.centroids[3 * (size_t)k], &O.xforms[16 * (size_t)k], &O.poses[16 * (size_t)k] );
  }
  RS_TRY( W.xforms.ensure( (size_t)I * 64 ), "split: buffers" ); RS_TRY( W.is_static.ensure( (size_t)I * 4 ), "split: buffers" );
  RS_TRY( hipMemcpyAsync( W.xforms.p, O.xforms.data(), (size_t)I * 64, hipMemcpyHostToDevice, st ), "split: upload" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( W.is_static.p, O.is_static.data(), (size_t)I * 4, hipMemcpyHostToDevice, st ), "split: upload" );
  return RS_HIP_OK;
}

SplitApplyArgs split_apply_args( const SplitSrc& S, int n_instances )
{
  SplitWorkspace& W = g_split_ws;
  SplitApplyArgs A{};
  A.S = S; A.order = W.order.as<int32_t>(); A.offsets = W.offsets.as<long long>(); A.xforms = W.xforms.as<float>(); A.is_static = W.is_static.as<int32_t>();
  A.n_instances = n_instances;
  return A;
}

int split_check_out( const rs_hip_split_out_t* out, int64_t n )
{
  if( !out || !out->n_instances ) return fail( RS_HIP_E_ARG, "split: the output record and its n_instances are required" );
  (void)n;
  return RS_HIP_OK;
}

} // namespace

// (rs_split.h) steps 1 and 2 alone, for rs_fuse.hip's arrangement call
int rs::split::segments_device( const int32_t* instance_ids, int n, Table& T, std::vector<int64_t>& offsets, const int32_t** order, ihipStream_t* st )
{
  SplitWorkspace& W = g_split_ws;
  RS_TRY( W.ids.ensure( (size_t)n * 4 ), "split: buffers" );
  RS_TRY( hipMemcpyAsync( W.ids.p, instance_ids, (size_t)n * 4, hipMemcpyHostToDevice, st ), "split: upload" );
  int rc = split_table_device( W.ids.as<int32_t>(), n, T, st ); if( rc ) { (void)hipStreamSynchronize( st ); return rc; }
  const size_t I = T.ids.size();
  rc = split_partition_device( W.ids.as<int32_t>(), n, (int)I, st ); if( rc ) { (void)hipStreamSynchronize( st ); return rc; }
  offsets.assign( I + 1, 0 );
  for( size_t k = 0; k < I; ++k ) offsets[k + 1] = offsets[k] + T.counts[k];
  *order = W.order.as<int32_t>();
  return RS_HIP_OK;
}

extern "C" {

int rs_hip_split_plan( const float* pos, const float* nor, const int32_t* class_ids, const int32_t* instance_ids, int64_t n,
                       const int32_t* static_classes, int32_t n_static, const rs_hip_split_out_t* out )
{
  char err[256] = "";
  split::Plan P{};
  if( out )
  {
    P.n_instances = out->n_instances; P.inst_ids = out->inst_ids; P.counts = out->counts; P.first = out->first; P.offsets = out->offsets; P.order = out->order;
    P.class_of = out->class_of; P.is_static = out->is_static; P.sums = out->sums; P.centroids = out->centroids; P.xforms = out->xforms; P.poses = out->poses;
    P.out_pos = out->out_pos; P.out_nor = out->out_nor;
  }
  const int rc = split::plan( pos, nor, class_ids, instance_ids, n, static_classes, n_static, P, err, sizeof(err) );
  if( rc ) api_set_err( err );
  return rc;
}

void rs_hip_split_layout( int32_t* tile, int32_t* lds_ranks, int32_t* max_instances, int32_t* chain_block )
{
  if( tile ) *tile = SPLIT_TILE;
  if( lds_ranks ) *lds_ranks = g_split_lds_ranks;
  if( max_instances ) *max_instances = split::MAX_INSTANCES;
  if( chain_block ) *chain_block = CHAIN_BLOCK;
}

int32_t rs_hip_split_lds_ranks( int32_t ranks )
{
  const int32_t before = g_split_lds_ranks;
  if( ranks >= 0 ) g_split_lds_ranks = std::min<int32_t>( ranks, SPLIT_LDS_RANKS_MAX );
  return before;
}

int32_t rs_hip_split_chains_form( int32_t form )
{
  const int32_t before = g_split_chains_form;
  if( form >= 0 ) g_split_chains_form = form ? 1 : 0;
  return before;
}

int64_t rs_hip_split_chains_sequential( void ) { return g_split_sequential; }

void rs_hip_split_seconds( double out[5], int32_t enable )
{
  if( out ) for( int k = 0; k < 5; ++k ) out[k] = g_split_s[k];
  for( int k = 0; k < 5; ++k ) g_split_s[k] = 0.0;
  g_split_clock = enable != 0;
}

int rs_hip_instance_table( const int32_t* instance_ids, int64_t n, int32_t* inst_ids, int64_t* counts, int64_t* first, int32_t* n_instances )
{
  char err[256] = "";
  if( int rc = split::check_size( n, err, sizeof(err) ) ) return fail( rc, err );
  if( !n_instances || ( n > 0 && !instance_ids ) ) return fail( RS_HIP_E_ARG, "instance_table: the ids and n_instances are required" );
  if( n == 0 ) { *n_instances = 0; return RS_HIP_OK; }
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  SplitWorkspace& W = g_split_ws;
  RS_TRY( W.ids.ensure( (size_t)n * 4 ), "instance_table: buffers" );
  RS_TRY( hipMemcpyAsync( W.ids.p, instance_ids, (size_t)n * 4, hipMemcpyHostToDevice, st ), "instance_table: upload" );
  split::Table T;
  rc = split_table_device( W.ids.as<int32_t>(), (int)n, T, st ); if( rc ) return rc;
  const size_t I = T.ids.size();
  *n_instances = (int32_t)I;
  if( inst_ids ) std::memcpy( inst_ids, T.ids.data(), I * 4 );
  if( counts ) std::memcpy( counts, T.counts.data(), I * 8 );
  if( first ) std::memcpy( first, T.first.data(), I * 8 );
  return RS_HIP_OK;
}

int rs_hip_split_by_instance( const int32_t* instance_ids, int64_t n, int32_t* inst_ids, int64_t* offsets, int32_t* order, int32_t* n_instances )
{
  char err[256] = "";
  if( int rc = split::check_size( n, err, sizeof(err) ) ) return fail( rc, err );
  if( !n_instances || ( n > 0 && ( !instance_ids || !order ) ) ) return fail( RS_HIP_E_ARG, "split_by_instance: the ids, order and n_instances are required" );
  if( n == 0 ) { *n_instances = 0; if( offsets ) offsets[0] = 0; return RS_HIP_OK; }
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  SplitWorkspace& W = g_split_ws;
  RS_TRY( W.ids.ensure( (size_t)n * 4 ), "split_by_instance: buffers" );
  RS_TRY( hipMemcpyAsync( W.ids.p, instance_ids, (size_t)n * 4, hipMemcpyHostToDevice, st ), "split_by_instance: upload" );
  split::Table T;
  rc = split_table_device( W.ids.as<int32_t>(), (int)n, T, st ); if( rc ) return rc;
  const size_t I = T.ids.size();
  rc = split_partition_device( W.ids.as<int32_t>(), (int)n, (int)I, st ); if( rc ) return rc;
  RS_TRY_DRAIN( st, hipMemcpyAsync( order, W.order.p, (size_t)n * 4, hipMemcpyDeviceToHost, st ), "split_by_instance: download" );
  RS_TRY( hipStreamSynchronize( st ), "split_by_instance: kernels" );
  *n_instances = (int32_t)I;
  if( inst_ids ) std::memcpy( inst_ids, T.ids.data(), I * 4 );
  if( offsets ) { offsets[0] = 0; for( size_t k = 0; k < I; ++k ) offsets[k + 1] = offsets[k] + T.counts[k]; }
  return RS_HIP_OK;
}

int rs_hip_segment_centroids( const float* pos, int64_t n, const int32_t* order, const int64_t* offsets, int32_t n_instances, double* sums, float* centroids )
{
  char err[256] = "";
  if( int rc = split::check_size( n, err, sizeof(err) ) ) return fail( rc, err );
  if( n_instances < 0 || n_instances > split::MAX_INSTANCES ) return fail( n_instances < 0 ? RS_HIP_E_ARG : RS_HIP_E_CAPACITY, "segment_centroids: a negative instance count, or more than max_instances" );
  if( n_instances == 0 ) return RS_HIP_OK;
  if( !offsets || !sums ) return fail( RS_HIP_E_ARG, "segment_centroids: offsets and sums are required" );
  // the kernel reads order[offsets[k] .. offsets[k + 1]) and pos[3 order[.]]: both are judged here
  if( offsets[0] != 0 ) return fail( RS_HIP_E_ARG, "segment_centroids: offsets must start at 0" );
  for( int32_t k = 0; k < n_instances; ++k ) if( offsets[k + 1] < offsets[k] ) return fail( RS_HIP_E_ARG, "segment_centroids: offsets must not decrease" );
  const int64_t m = offsets[n_instances];
  if( m > split::MAX_POINTS ) return fail( RS_HIP_E_CAPACITY, "segment_centroids: more ordered points than an int32 index can name" );
  if( m > 0 && ( !pos || !order ) ) return fail( RS_HIP_E_ARG, "segment_centroids: pos and order are required" );
  for( int64_t j = 0; j < m; ++j ) if( order[j] < 0 || order[j] >= n ) return fail( RS_HIP_E_ARG, "segment_centroids: an entry of order names no point" );
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  SplitWorkspace& W = g_split_ws;
  RS_TRY( W.pos.ensure( std::max<size_t>( (size_t)n * 12, 12 ) ), "segment_centroids: buffers" ); RS_TRY( W.order.ensure( std::max<size_t>( (size_t)m * 4, 4 ) ), "segment_centroids: buffers" );
  if( n > 0 ) RS_TRY( hipMemcpyAsync( W.pos.p, pos, (size_t)n * 12, hipMemcpyHostToDevice, st ), "segment_centroids: upload" );
  if( m > 0 ) RS_TRY_DRAIN( st, hipMemcpyAsync( W.order.p, order, (size_t)m * 4, hipMemcpyHostToDevice, st ), "segment_centroids: upload" );
  SplitSrc S{}; S.pos3 = W.pos.as<float>(); S.n = (int)n;
  std::vector<double> s( (size_t)n_instances * 3 );
  rc = split_chains_device( S, offsets, n_instances, s.data(), st ); if( rc ) return rc;
  std::memcpy( sums, s.data(), s.size() * 8 );
  if( centroids )
    for( int32_t k = 0; k < n_instances; ++k )
      for( int a = 0; a < 3; ++a ) { double v = s[3 * (size_t)k + a]; v /= (double)( offsets[k + 1] - offsets[k] ); centroids[3 * (size_t)k + a] = (float)v; }
  return RS_HIP_OK;
}

int rs_hip_scan_to_objects( const float* pos, const float* nor, const int32_t* class_ids, const int32_t* instance_ids, int64_t n,
                            const int32_t* static_classes, int32_t n_static, const rs_hip_split_out_t* out )
{
  char err[256] = "";
  if( int rc = split::check_size( n, err, sizeof(err) ) ) return fail( rc, err );
  if( int rc = split::check_static( static_classes, n_static, err, sizeof(err) ) ) return fail( rc, err );
  if( int rc = split_check_out( out, n ) ) return rc;
  if( n > 0 && ( !pos || !class_ids || !instance_ids ) ) return fail( RS_HIP_E_ARG, "scan_to_objects: positions, class ids and instance ids are required" );
  if( n > 0 && out->out_nor && !nor ) return fail( RS_HIP_E_ARG, "scan_to_objects: normals asked for, none given" );
  if( n == 0 ) { *out->n_instances = 0; if( out->offsets ) out->offsets[0] = 0; return RS_HIP_OK; }
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  SplitWorkspace& W = g_split_ws;
  SplitClock clk( st );
  const bool with_nor = out->out_nor != nullptr, with_pts = out->out_pos || with_nor;
  RS_TRY( W.ids.ensure( (size_t)n * 4 ), "scan_to_objects: buffers" ); RS_TRY( W.pos.ensure( (size_t)n * 12 ), "scan_to_objects: buffers" );
  if( with_nor ) RS_TRY( W.nor.ensure( (size_t)n * 12 ), "scan_to_objects: buffers" );
  RS_TRY( hipMemcpyAsync( W.ids.p, instance_ids, (size_t)n * 4, hipMemcpyHostToDevice, st ), "scan_to_objects: upload" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( W.pos.p, pos, (size_t)n * 12, hipMemcpyHostToDevice, st ), "scan_to_objects: upload" );
  if( with_nor ) RS_TRY_DRAIN( st, hipMemcpyAsync( W.nor.p, nor, (size_t)n * 12, hipMemcpyHostToDevice, st ), "scan_to_objects: upload" );
  SplitSrc S{}; S.pos3 = W.pos.as<float>(); S.nor3 = with_nor ? W.nor.as<float>() : nullptr; S.n = (int)n;
  split::Table T; SplitObjects O;
  rc = split_objects_device( S, (int)n, class_ids, static_classes, n_static, T, O, clk, st );
  if( rc ) { (void)hipStreamSynchronize( st ); return rc; }
  if( with_pts )
  {
    RS_TRY_DRAIN( st, W.out_pos.ensure( (size_t)n * 12 ), "scan_to_objects: buffers" );
    if( with_nor ) RS_TRY_DRAIN( st, W.out_nor.ensure( (size_t)n * 12 ), "scan_to_objects: buffers" );
    SplitApplyArgs A = split_apply_args( S, (int)T.ids.size() );
    A.first = 0; A.count = n; A.out_pos = W.out_pos.as<float>(); A.out_nor = with_nor ? W.out_nor.as<float>() : nullptr;
    {
      ProfSpan span( "split_apply" );
      hipLaunchKernelGGL( k_split_apply, dim3( blocks_for( n, SPLIT_BLOCK ) ), dim3( SPLIT_BLOCK ), 0, st, A );
    }
    RS_TRY_DRAIN( st, hipGetLastError(), "scan_to_objects: apply launch" );
    if( out->out_pos ) RS_TRY_DRAIN( st, hipMemcpyAsync( out->out_pos, W.out_pos.p, (size_t)n * 12, hipMemcpyDeviceToHost, st ), "scan_to_objects: download" );
    if( with_nor ) RS_TRY_DRAIN( st, hipMemcpyAsync( out->out_nor, W.out_nor.p, (size_t)n * 12, hipMemcpyDeviceToHost, st ), "scan_to_objects: download" );
  }
  if( out->order ) RS_TRY_DRAIN( st, hipMemcpyAsync( out->order, W.order.p, (size_t)n * 4, hipMemcpyDeviceToHost, st ), "scan_to_objects: download" );
  RS_TRY( hipStreamSynchronize( st ), "scan_to_objects: kernels" );
  clk.lap( 3 );
  split_write_outputs( T, O, out );
  return RS_HIP_OK;
}

int rs_hip_cloud_split_objects( const rs_hip_cloud_t* scan, const int32_t* class_ids, const int32_t* instance_ids,
                                const int32_t* static_classes, int32_t n_static, float cell_size,
                                rs_hip_cloud_t** objects, const rs_hip_split_out_t* out )
{
  char err[256] = "";
  if( !scan || !objects ) return fail( RS_HIP_E_ARG, "cloud_split_objects: the scan and the array of objects are required" );
  if( int rc = split::check_static( static_classes, n_static, err, sizeof(err) ) ) return fail( rc, err );
  if( int rc = split_check_out( out, 0 ) ) return rc;
  if( out->out_pos || out->out_nor ) return fail( RS_HIP_E_ARG, "cloud_split_objects: the points stay on the device (rs_hip_cloud_points hands them out)" );
  const CloudPoints C = api_cloud_points( scan );
  if( !C.qnor ) return fail( RS_HIP_E_ARG, "cloud_split_objects: the scan needs normals" );
  const int n = C.n;
  if( n > 0 && ( !class_ids || !instance_ids ) ) return fail( RS_HIP_E_ARG, "cloud_split_objects: class ids and instance ids are required" );
  if( n <= 0 ) { *out->n_instances = 0; if( out->offsets ) out->offsets[0] = 0; return RS_HIP_OK; }
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  SplitWorkspace& W = g_split_ws;
  SplitClock clk( st );
  RS_TRY( W.ids.ensure( (size_t)n * 4 ), "cloud_split_objects: buffers" );
  RS_TRY( hipMemcpyAsync( W.ids.p, instance_ids, (size_t)n * 4, hipMemcpyHostToDevice, st ), "cloud_split_objects: upload" );
  SplitSrc S{}; S.qpos = C.qpos; S.qnor = C.qnor; S.by_orig = C.by_orig; S.n = n;
  split::Table T; SplitObjects O;
  rc = split_objects_device( S, n, class_ids, static_classes, n_static, T, O, clk, st );
  if( rc ) { (void)hipStreamSynchronize( st ); return rc; }
  std::vector<int32_t> order;
  if( out->order )
  {
    // (into a vector first: a failure below must leave the caller's arrays as they were)
    order.resize( (size_t)n );
    RS_TRY_DRAIN( st, hipMemcpyAsync( order.data(), W.order.p, (size_t)n * 4, hipMemcpyDeviceToHost, st ), "cloud_split_objects: download" );
    RS_TRY( hipStreamSynchronize( st ), "cloud_split_objects: download" );
  }
  // every instance into one workspace, instance after instance, in one launch; then one batched index build over its segments
  const int I = (int)T.ids.size();
  std::vector<rs_hip_cloud_t*> made( (size_t)I, nullptr );
  SplitApplyArgs A = split_apply_args( S, I );
  A.first = 0; A.count = n;
  if( api_level_workspace( (size_t)n, true, &A.out_pos, &A.out_nor ) ) { (void)hipStreamSynchronize( st ); return RS_HIP_E_RUNTIME; }
  {
    ProfSpan span( "split_apply" );
    hipLaunchKernelGGL( k_split_apply, dim3( blocks_for( n, SPLIT_BLOCK ) ), dim3( SPLIT_BLOCK ), 0, st, A );
  }
  RS_TRY_DRAIN( st, hipGetLastError(), "cloud_split_objects: apply launch" );
  clk.lap( 3 );
  rc = api_clouds_from_device( A.out_pos, A.out_nor, O.offsets.data(), T.counts.data(), I, cell_size, made.data() );      // (all or nothing)
  clk.lap( 4 );
  if( rc ) { (void)hipStreamSynchronize( st ); return rc; }
  for( int k = 0; k < I; ++k ) objects[k] = made[(size_t)k];
  if( out->order ) std::memcpy( out->order, order.data(), (size_t)n * 4 );
  split_write_outputs( T, O, out );
  return RS_HIP_OK;
}

} // extern "C"
