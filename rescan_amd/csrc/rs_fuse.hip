// The row that closes a timestep — rsdu_augment_database (apps/segment_transfer/database_update.cpp:22-91) for one placement:
// rs_hip_shuffle_plan, rs_hip_shuffle_permutation, rs_hip_select_by_ids, rs_hip_merge_shuffled, rs_hip_cloud_create_fused.
//
// The reference cuts the points with the placement's instance id out of the scan (rs_pointcloud_copy_by_ids,
// lib/rs/rs_pointcloud.h:239-297), aligns them to the object's model with icp_align from inverse( pose ) unless the object is
// static, moves them into the model's frame (rs_pointcloud_transform, :1367-1378), appends the model and shuffles the lot with a
// Fisher-Yates pass (rs_pointcloud_merge, :383-446).
//
// How a call runs:
//   1. k_fuse_flag + scan + k_fuse_scatter   a stable compaction: flag[i] = point_ids[i] in ids, an exclusive scan of the flags
//                                            (hipCUB, rs_build.hip), index[rank] = i — the order :272-289 emits.
//   2. ICP                                   the library's one host loop (rs_hip_icp_align), extracted points as source.
//   3. the permutation                       the shuffle is a chain of n-1 dependent swaps, but its permutation depends on n and the
//                                            seed alone and resolves in parallel.  Step i (i = n-1 .. 1) uses draw n-1-i of the
//                                            stream; k_fuse_draw jumps the generator to each draw (rs_fuse.h: JumpTable) and writes
//                                            j_i.  Position i is final after step i, so the element that ends at t >= 1 is what
//                                            position j_t held just before step t, and the one that ends at 0 is what position 0
//                                            holds after all steps.  "What position p held just before step t" is: the smallest
//                                            step s > t with j_s = p decides — if there is none, the original element p; otherwise
//                                            what position s held just before step s, i.e. the same question for (s, s).  A stable
//                                            radix sort of (key j_s, value s) lists the steps that target each position in
//                                            increasing s; k_fuse_walk answers every t with one binary search per hop.  s grows
//                                            with every hop, so the walk ends; on the CPU the chains had mean length 1 and a
//                                            longest of 21 at n = 200 000.
//   4. k_fuse_merge                          one lane per output element: src = perm[i]; an extracted point is read from the scan
//                                            and transformed (msh_mat4_vec3_mul's operation order, msh_vec_math.h:1554-1561, no
//                                            renormalisation), a model point is copied; positions and normals land where the index
//                                            build reads them.  Transform, concatenation and shuffle are never separate passes.
//   5. the index build                       rs_hip_cloud_create_level's.
//
// Above 16 384 extracted points the library's ICP is within 1e-4 of the reference's pose, not bit-identical to it, and
// the merged positions of such an object inherit that difference; everything else here is bit for bit.
//
// The whole loop over an arrangement in one call: rs_hip_shuffle_permutations, rs_hip_merge_shuffled_multi,
// rs_hip_cloud_fuse_arrangement.  Step 1 becomes one table and one stable partition of the scan's ids for all placements
// (rs_split.hip through rs::split::segments_device; segment k of its order is what step 1 returns for that id); the placements run in
// rounds by the depth of their model_from chains (a placement whose model is the shape an earlier one leaves runs a round after it; an
// ordinary arrangement is one round); a round runs step 2 per dynamic placement, then steps 3 and 4 ONCE for all its placements
// (k_fuse_draw_seg, one sort, k_fuse_walk_seg, k_fuse_merge_seg over the concatenation, the per-placement transform and sides in a
// table in global memory), then copies every placement's slice to where step 5 reads and builds its index.  The single-placement
// entry points and kernels above are not routed through any of it.
#include "rs_host.h"
#include "rs_fuse.h"
#include "rs_split.h"

#include <chrono>
#include <cstring>
#include <unordered_map>
#include <vector>

namespace rs {

constexpr int FUSE_BLOCK = 256;

struct FuseDrawArgs { fuse::JumpTable jump; int m; int n_bits; uint32_t* key; uint32_t* step; };

// lane t: step i = t + 1 of the shuffle over n = m + 1 elements; its draw is number m - 1 - t of the stream
__global__ __launch_bounds__( FUSE_BLOCK ) void k_fuse_draw( FuseDrawArgs A )
{
  const int t = blockIdx.x * FUSE_BLOCK + threadIdx.x;
  if( t >= A.m ) return;
  const uint32_t d = (uint32_t)( A.m - 1 - t );
  uint64_t s = A.jump.state;
  for( int k = 0; k < A.n_bits; ++k )
    if( ( d >> k ) & 1u ) s = s * A.jump.mul[k] + A.jump.add[k];
  // msh_rand_next (msh_std.h:1447-1455) of the state before the draw
  const uint32_t xorshifted = (uint32_t)( ( ( s >> 18 ) ^ s ) >> 27 );
  const uint32_t rot = (uint32_t)( s >> 59 );
  const uint32_t u = ( xorshifted >> rot ) | ( xorshifted << ( ( 0u - rot ) & 31u ) );
  const float f = __uint_as_float( 0x3F800000u | ( u >> 9 ) ) - 1.0f;
  const int i = t + 1;
  int j = (int)( f * (float)i );                 // rs_pointcloud.h:432
  j = min( j, i - 1 );                           // never taken for n <= 2^24 (rs_fuse.h); keeps every later index in bounds
  A.key[t] = (uint32_t)j;
  A.step[t] = (uint32_t)i;
}

// key[t - 1] = j_t as drawn; (skey, sstep): the same pairs sorted by (j, step).  perm[t] for every t in [0, n).
__global__ __launch_bounds__( FUSE_BLOCK ) void k_fuse_walk( const uint32_t* key, const uint32_t* skey, const uint32_t* sstep, int n, int32_t* perm )
{
  const int t = blockIdx.x * FUSE_BLOCK + threadIdx.x;
  if( t >= n ) return;
  const int m = n - 1;
  uint32_t p = t == 0 ? 0u : key[t - 1], after = (uint32_t)t;
  for( ;; )
  {
    // the first pair that is > (p, after) in (j, step) order
    int lo = 0, hi = m;
    while( lo < hi )
    {
      const int mid = ( lo + hi ) >> 1;
      const uint32_t k = skey[mid];
      if( k < p || ( k == p && sstep[mid] <= after ) ) lo = mid + 1; else hi = mid;
    }
    if( lo >= m || skey[lo] != p ) break;        // no later step targets p: it still holds what it held
    p = after = sstep[lo];                       // step s put there what position s held just before step s
  }
  perm[t] = (int32_t)p;
}

__global__ __launch_bounds__( FUSE_BLOCK ) void k_fuse_flag( const int32_t* point_ids, int n, const int32_t* ids, int n_ids, uint32_t* flags /* n + 1 */ )
{
  const int i = blockIdx.x * FUSE_BLOCK + threadIdx.x;
  if( i > n ) return;
  uint32_t f = 0u;
  if( i < n )
  {
    const int32_t v = point_ids[i];
    for( int k = 0; k < n_ids; ++k ) f |= ( ids[k] == v ) ? 1u : 0u;
  }
  flags[i] = f;
}
__global__ __launch_bounds__( FUSE_BLOCK ) void k_fuse_scatter( const uint32_t* flags, const uint32_t* rank, int n, int32_t* index )
{
  const int i = blockIdx.x * FUSE_BLOCK + threadIdx.x;
  if( i < n && flags[i] ) index[rank[i]] = i;
}

// One side of a merge: packed xyz arrays, or a cloud's query layout read through its original -> slot map; index (may be null)
// names the side's k-th point among those.
struct FuseSide { const float* pos3; const float* nor3; const float4* qpos; const float4* qnor; const int* by_orig; const int32_t* index; };

__device__ __forceinline__ void fuse_load( const FuseSide& S, int k, float p[3], float q[3] )
{
  if( S.index ) k = S.index[k];
  if( S.qpos )
  {
    const int s = S.by_orig[k];
    const float4 a = S.qpos[s], b = S.qnor[s];
    p[0] = a.x; p[1] = a.y; p[2] = a.z; q[0] = b.x; q[1] = b.y; q[2] = b.z;
  }
  else
  {
    const size_t o = 3 * (size_t)k;
    p[0] = S.pos3[o]; p[1] = S.pos3[o + 1]; p[2] = S.pos3[o + 2]; q[0] = S.nor3[o]; q[1] = S.nor3[o + 1]; q[2] = S.nor3[o + 2];
  }
}
// msh_mat4_vec3_mul (msh_vec_math.h:1554-1561): three products added left to right, then (float)is_point times the translation
__device__ __forceinline__ void fuse_xform( const Xform& M, const float v[3], float w, float o[3] )
{
  o[0] = M.m[0] * v[0] + M.m[4] * v[1] + M.m[ 8] * v[2] + w * M.m[12];
  o[1] = M.m[1] * v[0] + M.m[5] * v[1] + M.m[ 9] * v[2] + w * M.m[13];
  o[2] = M.m[2] * v[0] + M.m[6] * v[1] + M.m[10] * v[2] + w * M.m[14];
}

struct FuseMergeArgs { FuseSide a, b; int n_a, n; Xform x; const int32_t* perm; float* out_pos; float* out_nor; };

__global__ __launch_bounds__( FUSE_BLOCK ) void k_fuse_merge( FuseMergeArgs A )
{
  const int i = blockIdx.x * FUSE_BLOCK + threadIdx.x;
  if( i >= A.n ) return;
  const int src = A.perm[i];
  float p[3], q[3];
  if( src < A.n_a )
  {
    float pa[3], qa[3];
    fuse_load( A.a, src, pa, qa );
    fuse_xform( A.x, pa, 1.0f, p );
    fuse_xform( A.x, qa, 0.0f, q );
  }
  else fuse_load( A.b, src - A.n_a, p, q );
  const size_t o = 3 * (size_t)i;
  A.out_pos[o] = p[0]; A.out_pos[o + 1] = p[1]; A.out_pos[o + 2] = p[2];
  A.out_nor[o] = q[0]; A.out_nor[o + 1] = q[1]; A.out_nor[o + 2] = q[2];
}

// the side's points as they are, packed: the ICP source
__global__ __launch_bounds__( FUSE_BLOCK ) void k_fuse_gather( FuseSide S, int n, float* out_pos, float* out_nor )
{
  const int i = blockIdx.x * FUSE_BLOCK + threadIdx.x;
  if( i >= n ) return;
  float p[3], q[3];
  fuse_load( S, i, p, q );
  const size_t o = 3 * (size_t)i;
  out_pos[o] = p[0]; out_pos[o + 1] = p[1]; out_pos[o + 2] = p[2];
  out_nor[o] = q[0]; out_nor[o + 1] = q[1]; out_nor[o + 2] = q[2];
}

// ---- the segmented forms: all placements of a round in one draw, one sort, one walk and one merge -------------------------------
// Placement p owns the elements [off[p], off[p + 1]) of the concatenation and the pairs [poff[p], poff[p + 1]) of the pair arrays,
// poff[p + 1] - poff[p] = max( n_p - 1, 0 ): a placement of one element (or none) has no pair.  Keys and steps are GLOBAL positions
// (off[p] + local), so the keys of different placements lie in disjoint, increasing ranges and one stable sort of all pairs is the
// concatenation of the per-placement sorts: the sorted pairs of p are again [poff[p], poff[p + 1]).

// the last p in [0, P) with start[p] <= i (start has P + 1 non-decreasing entries, start[0] = 0 <= i < start[P]): empty placements
// share their successor's start and are passed over
__device__ __forceinline__ int fuse_segment_of( const int* start, int P, int i )
{
  int lo = 0, hi = P;
  while( hi - lo > 1 ) { const int mid = ( lo + hi ) >> 1; if( start[mid] <= i ) lo = mid; else hi = mid; }
  return lo;
}

struct FuseDrawSegArgs { fuse::JumpTable jump; const int* off; const int* poff; int P; int n_pairs; uint32_t* key; uint32_t* step; };

// lane t: pair t.  In its placement (m = n_p - 1 pairs) it is step i = t - poff[p] + 1, whose draw is number m - i of a stream that
// restarts for every placement (rs_pointcloud_merge seeds the generator itself).
__global__ __launch_bounds__( FUSE_BLOCK ) void k_fuse_draw_seg( FuseDrawSegArgs A )
{
  const long long tt = (long long)blockIdx.x * FUSE_BLOCK + threadIdx.x;
  if( tt >= A.n_pairs ) return;
  const int t = (int)tt;
  const int p = fuse_segment_of( A.poff, A.P, t );
  const int first = A.poff[p], m = A.poff[p + 1] - first, i = t - first + 1;
  const uint32_t d = (uint32_t)( m - i );
  uint64_t s = A.jump.state;
  for( int k = 0; k < fuse::JUMP_BITS && ( d >> k ); ++k )
    if( ( d >> k ) & 1u ) s = s * A.jump.mul[k] + A.jump.add[k];
  // msh_rand_next (msh_std.h:1447-1455) of the state before the draw
  const uint32_t xorshifted = (uint32_t)( ( ( s >> 18 ) ^ s ) >> 27 );
  const uint32_t rot = (uint32_t)( s >> 59 );
  const uint32_t u = ( xorshifted >> rot ) | ( xorshifted << ( ( 0u - rot ) & 31u ) );
  const float f = __uint_as_float( 0x3F800000u | ( u >> 9 ) ) - 1.0f;
  int j = (int)( f * (float)i );                 // rs_pointcloud.h:432
  j = min( j, i - 1 );                           // never taken for n_p <= 2^24 (rs_fuse.h); keeps every later index in bounds
  const uint32_t base = (uint32_t)A.off[p];
  A.key[t] = base + (uint32_t)j;
  A.step[t] = base + (uint32_t)i;
}

// k_fuse_walk for every global position t: the pairs searched are the placement's own, and perm[t] is LOCAL (an index into the
// placement's "A then B").  Local position 0 has no draw of its own: it starts from itself and never reads key[poff[p] - 1], the
// previous placement's last key.
__global__ __launch_bounds__( FUSE_BLOCK ) void k_fuse_walk_seg( const uint32_t* key, const uint32_t* skey, const uint32_t* sstep, const int* off, const int* poff, int P, int total, int32_t* perm )
{
  const long long tt = (long long)blockIdx.x * FUSE_BLOCK + threadIdx.x;
  if( tt >= total ) return;
  const int t = (int)tt;
  const int s = fuse_segment_of( off, P, t );
  const int base = off[s], first = poff[s], last = poff[s + 1], local = t - base;
  uint32_t p = local == 0 ? (uint32_t)base : key[first + local - 1], after = (uint32_t)t;
  for( ;; )
  {
    // the first pair of the placement that is > (p, after) in (j, step) order
    int lo = first, hi = last;
    while( lo < hi )
    {
      const int mid = ( lo + hi ) >> 1;
      const uint32_t k = skey[mid];
      if( k < p || ( k == p && sstep[mid] <= after ) ) lo = mid + 1; else hi = mid;
    }
    if( lo >= last || skey[lo] != p ) break;     // no later step targets p: it still holds what it held
    p = after = sstep[lo];                       // step s put there what position s held just before step s
  }
  perm[t] = (int32_t)( p - (uint32_t)base );
}

// what k_fuse_merge gets by value, per placement, in global memory
struct FuseSeg { FuseSide a, b; Xform x; int n_a, pad; };
struct FuseMergeSegArgs { const FuseSeg* seg; const int* off; int P; int total; const int32_t* perm; float* out_pos; float* out_nor; };

// one lane per element of the concatenation; from `src` on it is k_fuse_merge's body
__global__ __launch_bounds__( FUSE_BLOCK ) void k_fuse_merge_seg( FuseMergeSegArgs A )
{
  const long long ii = (long long)blockIdx.x * FUSE_BLOCK + threadIdx.x;
  if( ii >= A.total ) return;
  const int i = (int)ii;
  const FuseSeg& G = A.seg[fuse_segment_of( A.off, A.P, i )];
  const int n_a = G.n_a;
  const int src = A.perm[i];
  float p[3], q[3];
  if( src < n_a )
  {
    float pa[3], qa[3];
    fuse_load( G.a, src, pa, qa );
    fuse_xform( G.x, pa, 1.0f, p );
    fuse_xform( G.x, qa, 0.0f, q );
  }
  else fuse_load( G.b, src - n_a, p, q );
  const size_t o = 3 * (size_t)i;
  A.out_pos[o] = p[0]; A.out_pos[o + 1] = p[1]; A.out_pos[o + 2] = p[2];
  A.out_nor[o] = q[0]; A.out_nor[o + 1] = q[1]; A.out_nor[o + 2] = q[2];
}

} // namespace rs

using namespace rs;

namespace {

struct FuseWorkspace { Buf key, step, skey, sstep, perm, tmp, point_ids, ids, flags, rank, index, a_pos, a_nor, b_pos, b_nor, out_pos, out_nor, off, seg; };
thread_local FuseWorkspace g_fuse_ws;

// the permutation of n <= 2^24 elements in the workspace's perm buffer (n >= 1)
int fuse_permutation_device( int n, uint32_t seed, hipStream_t st )
{
  FuseWorkspace& W = g_fuse_ws;
  const int m = n - 1;
  RS_TRY( W.perm.ensure( (size_t)n * 4 ), "fuse: buffers" );
  const size_t mm = (size_t)std::max( m, 1 );
  int key_bits = 1; while( key_bits < 32 && ( (size_t)1 << key_bits ) < mm ) ++key_bits;      // keys are < m
  const size_t tmp_bytes = build_sort_temp_bytes( (int)mm, key_bits );
  RS_TRY( W.key.ensure( mm * 4 ), "fuse: buffers" ); RS_TRY( W.step.ensure( mm * 4 ), "fuse: buffers" );
  RS_TRY( W.skey.ensure( mm * 4 ), "fuse: buffers" ); RS_TRY( W.sstep.ensure( mm * 4 ), "fuse: buffers" );
  RS_TRY( W.tmp.ensure( tmp_bytes + 256 ), "fuse: buffers" );
  {
    ProfSpan span( "fuse_permutation" );
    if( m > 0 )
    {
      FuseDrawArgs D;
      D.jump = fuse::jump_table( seed ); D.m = m; D.key = W.key.as<uint32_t>(); D.step = W.step.as<uint32_t>();
      int bits = 1; while( bits < fuse::JUMP_BITS && ( (uint32_t)( m - 1 ) >> bits ) ) ++bits;
      D.n_bits = bits;
      hipLaunchKernelGGL( k_fuse_draw, dim3( blocks_for( m, FUSE_BLOCK ) ), dim3( FUSE_BLOCK ), 0, st, D );
      // stable, and the steps go in increasing: equal keys keep their steps in increasing order
      if( build_sort_pairs( W.tmp.p, tmp_bytes, W.key.as<uint32_t>(), W.skey.as<uint32_t>(), W.step.as<uint32_t>(), W.sstep.as<uint32_t>(), m, key_bits, st ) )
        return fail( RS_HIP_E_RUNTIME, "fuse: device sort failed" );
    }
    hipLaunchKernelGGL( k_fuse_walk, dim3( blocks_for( n, FUSE_BLOCK ) ), dim3( FUSE_BLOCK ), 0, st, W.key.as<uint32_t>(), W.skey.as<uint32_t>(), W.sstep.as<uint32_t>(), n, W.perm.as<int32_t>() );
  }
  RS_TRY( hipGetLastError(), "fuse: permutation launch" );
  return RS_HIP_OK;
}

// flags / rank / index of the n >= 1 ids in d_point_ids against the n_ids >= 1 entries of ids (host); *count is read back
int fuse_select_device( const int32_t* d_point_ids, int n, const int32_t* ids, int n_ids, int64_t* count, hipStream_t st )
{
  FuseWorkspace& W = g_fuse_ws;
  const size_t n1 = (size_t)n + 1;
  const size_t tmp_bytes = build_scan_temp_bytes( n1 );
  RS_TRY( W.ids.ensure( (size_t)n_ids * 4 ), "fuse: buffers" ); RS_TRY( W.flags.ensure( n1 * 4 ), "fuse: buffers" );
  RS_TRY( W.rank.ensure( n1 * 4 ), "fuse: buffers" ); RS_TRY( W.index.ensure( (size_t)n * 4 ), "fuse: buffers" );
  RS_TRY( W.tmp.ensure( tmp_bytes + 256 ), "fuse: buffers" );
  RS_TRY( hipMemcpyAsync( W.ids.p, ids, (size_t)n_ids * 4, hipMemcpyHostToDevice, st ), "fuse: upload" );
  {
    ProfSpan span( "fuse_select" );
    hipLaunchKernelGGL( k_fuse_flag, dim3( blocks_for( (long long)n1, FUSE_BLOCK ) ), dim3( FUSE_BLOCK ), 0, st, d_point_ids, n, W.ids.as<int32_t>(), n_ids, W.flags.as<uint32_t>() );
    if( build_exclusive_scan( W.tmp.p, tmp_bytes, W.flags.as<uint32_t>(), W.rank.as<uint32_t>(), n1, st ) )
      return fail( RS_HIP_E_RUNTIME, "fuse: device scan failed" );
    hipLaunchKernelGGL( k_fuse_scatter, dim3( blocks_for( n, FUSE_BLOCK ) ), dim3( FUSE_BLOCK ), 0, st, W.flags.as<uint32_t>(), W.rank.as<uint32_t>(), n, W.index.as<int32_t>() );
  }
  RS_TRY( hipGetLastError(), "fuse: select launch" );
  uint32_t got = 0;
  RS_TRY( hipMemcpyAsync( &got, W.rank.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, st ), "fuse: download" );
  RS_TRY( hipStreamSynchronize( st ), "fuse: select" );
  *count = (int64_t)got;
  return RS_HIP_OK;
}

int fuse_merge_launch( const FuseMergeArgs& A, hipStream_t st )
{
  {
    ProfSpan span( "fuse_merge" );
    hipLaunchKernelGGL( k_fuse_merge, dim3( blocks_for( A.n, FUSE_BLOCK ) ), dim3( FUSE_BLOCK ), 0, st, A );
  }
  RS_TRY( hipGetLastError(), "fuse: merge launch" );
  return RS_HIP_OK;
}

// the concatenation of P placements of n[p] elements: off / poff as the segmented kernels read them (P + 1 entries each)
struct FuseSegPlan { std::vector<int> off, poff; int total = 0, n_pairs = 0; };

// refusals of a list of sizes, judged the same way by every entry point: each n[p] as check_size judges it, their sum by what an
// int32 index names
int fuse_seg_plan( const int64_t* n, int P, FuseSegPlan& L, char* err, size_t err_cap )
{
  if( P < 0 ) return fuse::refuse( RS_HIP_E_ARG, err, err_cap, "fuse: %lld placements: a count cannot be negative", (long long)P );
  if( P > 0 && !n ) return fuse::refuse( RS_HIP_E_ARG, err, err_cap, "fuse: %lld placements without their sizes", (long long)P );
  int64_t total = 0, pairs = 0;
  L.off.assign( (size_t)P + 1, 0 ); L.poff.assign( (size_t)P + 1, 0 );
  for( int p = 0; p < P; ++p )
  {
    if( int rc = fuse::check_size( n[p], err, err_cap ) ) return rc;
    total += n[p]; pairs += std::max<int64_t>( n[p] - 1, 0 );
    if( total > fuse::MAX_TOTAL ) return fuse::refuse( RS_HIP_E_CAPACITY, err, err_cap, "fuse: %lld elements in all placements together: more than an int32 index can name", (long long)total );
    L.off[(size_t)p + 1] = (int)total; L.poff[(size_t)p + 1] = (int)pairs;
  }
  L.total = (int)total; L.n_pairs = (int)pairs;
  return RS_HIP_OK;
}

// the permutations of all placements of L (total >= 1), local indices, concatenated in the workspace's perm buffer; off / poff stay
// in the workspace's off buffer for the merge.  L must outlive the stream's next synchronisation.
int fuse_permutations_device( const FuseSegPlan& L, uint32_t seed, hipStream_t st )
{
  FuseWorkspace& W = g_fuse_ws;
  const int P = (int)L.off.size() - 1;
  const size_t row = (size_t)P + 1, mm = (size_t)std::max( L.n_pairs, 1 );
  int key_bits = 1; while( key_bits < 32 && ( (size_t)1 << key_bits ) < (size_t)L.total ) ++key_bits;       // keys are < total
  const size_t tmp_bytes = build_sort_temp_bytes( (int)mm, key_bits );
  RS_TRY( W.perm.ensure( (size_t)L.total * 4 ), "fuse: buffers" ); RS_TRY( W.off.ensure( 2 * row * 4 ), "fuse: buffers" );
  RS_TRY( W.key.ensure( mm * 4 ), "fuse: buffers" ); RS_TRY( W.step.ensure( mm * 4 ), "fuse: buffers" );
  RS_TRY( W.skey.ensure( mm * 4 ), "fuse: buffers" ); RS_TRY( W.sstep.ensure( mm * 4 ), "fuse: buffers" );
  RS_TRY( W.tmp.ensure( tmp_bytes + 256 ), "fuse: buffers" );
  int* d_off = W.off.as<int>(); int* d_poff = d_off + row;
  RS_TRY( hipMemcpyAsync( d_off, L.off.data(), row * 4, hipMemcpyHostToDevice, st ), "fuse: upload" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( d_poff, L.poff.data(), row * 4, hipMemcpyHostToDevice, st ), "fuse: upload" );
  {
    ProfSpan span( "fuse_permutation" );
    if( L.n_pairs > 0 )
    {
      FuseDrawSegArgs D;
      D.jump = fuse::jump_table( seed ); D.off = d_off; D.poff = d_poff; D.P = P; D.n_pairs = L.n_pairs; D.key = W.key.as<uint32_t>(); D.step = W.step.as<uint32_t>();
      hipLaunchKernelGGL( k_fuse_draw_seg, dim3( blocks_for( L.n_pairs, FUSE_BLOCK ) ), dim3( FUSE_BLOCK ), 0, st, D );
      // stable; inside a placement the steps go in increasing, and the placements' key ranges follow one another
      if( build_sort_pairs( W.tmp.p, tmp_bytes, W.key.as<uint32_t>(), W.skey.as<uint32_t>(), W.step.as<uint32_t>(), W.sstep.as<uint32_t>(), L.n_pairs, key_bits, st ) )
      { (void)hipStreamSynchronize( st ); return fail( RS_HIP_E_RUNTIME, "fuse: device sort failed" ); }
    }
    hipLaunchKernelGGL( k_fuse_walk_seg, dim3( blocks_for( L.total, FUSE_BLOCK ) ), dim3( FUSE_BLOCK ), 0, st, W.key.as<uint32_t>(), W.skey.as<uint32_t>(), W.sstep.as<uint32_t>(),
                        d_off, d_poff, P, L.total, W.perm.as<int32_t>() );
  }
  RS_TRY_DRAIN( st, hipGetLastError(), "fuse: permutation launch" );
  return RS_HIP_OK;
}

// one merge launch over the concatenation of L, after fuse_permutations_device( L ): seg (host, P records) goes to the workspace
int fuse_merge_seg_launch( const FuseSegPlan& L, const std::vector<FuseSeg>& seg, float* out_pos, float* out_nor, hipStream_t st )
{
  FuseWorkspace& W = g_fuse_ws;
  RS_TRY_DRAIN( st, W.seg.ensure( seg.size() * sizeof(FuseSeg) ), "fuse: buffers" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( W.seg.p, seg.data(), seg.size() * sizeof(FuseSeg), hipMemcpyHostToDevice, st ), "fuse: upload" );
  FuseMergeSegArgs A{};
  A.seg = W.seg.as<FuseSeg>(); A.off = W.off.as<int>(); A.P = (int)seg.size(); A.total = L.total; A.perm = W.perm.as<int32_t>(); A.out_pos = out_pos; A.out_nor = out_nor;
  {
    ProfSpan span( "fuse_merge" );
    hipLaunchKernelGGL( k_fuse_merge_seg, dim3( blocks_for( L.total, FUSE_BLOCK ) ), dim3( FUSE_BLOCK ), 0, st, A );
  }
  RS_TRY_DRAIN( st, hipGetLastError(), "fuse: merge launch" );
  return RS_HIP_OK;
}

} // namespace

extern "C" {

int rs_hip_shuffle_plan( int64_t n, uint32_t seed, int32_t* perm )
{
  char err[256] = "";
  const int rc = fuse::shuffle_plan( n, seed, perm, err, sizeof(err) );
  if( rc ) api_set_err( err );
  return rc;
}

int rs_hip_shuffle_permutation( int64_t n, uint32_t seed, int32_t* perm )
{
  char err[256] = "";
  if( int rc = fuse::check_size( n, err, sizeof(err) ) ) return fail( rc, err );
  if( n > 0 && !perm ) return fail( RS_HIP_E_ARG, "shuffle_permutation: no array for the permutation" );
  if( n == 0 ) return RS_HIP_OK;
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  rc = fuse_permutation_device( (int)n, seed, st ); if( rc ) return rc;
  RS_TRY( hipMemcpyAsync( perm, g_fuse_ws.perm.p, (size_t)n * 4, hipMemcpyDeviceToHost, st ), "shuffle_permutation: download" );
  RS_TRY( hipStreamSynchronize( st ), "shuffle_permutation: kernels" );
  return RS_HIP_OK;
}

int rs_hip_select_by_ids( const int32_t* point_ids, int64_t n, const int32_t* ids, int32_t n_ids, int32_t* index, int64_t* count )
{
  char err[256] = "";
  if( !count || n < 0 || ( n > 0 && ( !point_ids || !index ) ) ) return fail( RS_HIP_E_ARG, "select_by_ids: null arrays or a negative count" );
  if( n > 2147483646ll ) return fail( RS_HIP_E_CAPACITY, "select_by_ids: more points than an int32 index can name" );
  if( int rc = fuse::check_ids( ids, n_ids, err, sizeof(err) ) ) return fail( rc, err );
  *count = 0;
  if( n == 0 || n_ids == 0 ) return RS_HIP_OK;
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  FuseWorkspace& W = g_fuse_ws;
  RS_TRY( W.point_ids.ensure( (size_t)n * 4 ), "select_by_ids: buffers" );
  RS_TRY( hipMemcpyAsync( W.point_ids.p, point_ids, (size_t)n * 4, hipMemcpyHostToDevice, st ), "select_by_ids: upload" );
  int64_t got = 0;
  rc = fuse_select_device( W.point_ids.as<int32_t>(), (int)n, ids, n_ids, &got, st ); if( rc ) return rc;
  if( got > 0 )
  {
    RS_TRY( hipMemcpyAsync( index, W.index.p, (size_t)got * 4, hipMemcpyDeviceToHost, st ), "select_by_ids: download" );
    RS_TRY( hipStreamSynchronize( st ), "select_by_ids: download" );
  }
  *count = got;
  return RS_HIP_OK;
}

int rs_hip_merge_shuffled( const float* a_pos, const float* a_nor, int64_t n_a, const float xform[16],
                           const float* b_pos, const float* b_nor, int64_t n_b, uint32_t seed,
                           float* out_pos, float* out_nor, int32_t* source )
{
  char err[256] = "";
  if( n_a < 0 || n_b < 0 ) return fail( RS_HIP_E_ARG, "merge_shuffled: a negative count" );
  if( n_a > fuse::MAX_POINTS || n_b > fuse::MAX_POINTS ) return fail( RS_HIP_E_CAPACITY, "merge_shuffled: more than 2^24 points" );
  const int64_t n = n_a + n_b;
  if( int rc = fuse::check_size( n, err, sizeof(err) ) ) return fail( rc, err );
  if( !xform || ( n_a > 0 && ( !a_pos || !a_nor ) ) || ( n_b > 0 && ( !b_pos || !b_nor ) ) || ( n > 0 && ( !out_pos || !out_nor ) ) )
    return fail( RS_HIP_E_ARG, "merge_shuffled: null arrays (both clouds need normals)" );
  if( n == 0 ) return RS_HIP_OK;
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  FuseWorkspace& W = g_fuse_ws;
  const size_t ba = (size_t)n_a * 12, bb = (size_t)n_b * 12, bo = (size_t)n * 12;
  RS_TRY( W.a_pos.ensure( std::max<size_t>( ba, 12 ) ), "merge_shuffled: buffers" ); RS_TRY( W.a_nor.ensure( std::max<size_t>( ba, 12 ) ), "merge_shuffled: buffers" );
  RS_TRY( W.b_pos.ensure( std::max<size_t>( bb, 12 ) ), "merge_shuffled: buffers" ); RS_TRY( W.b_nor.ensure( std::max<size_t>( bb, 12 ) ), "merge_shuffled: buffers" );
  RS_TRY( W.out_pos.ensure( bo ), "merge_shuffled: buffers" ); RS_TRY( W.out_nor.ensure( bo ), "merge_shuffled: buffers" );
  if( n_a > 0 )
  {
    RS_TRY( hipMemcpyAsync( W.a_pos.p, a_pos, ba, hipMemcpyHostToDevice, st ), "merge_shuffled: upload" );
    RS_TRY( hipMemcpyAsync( W.a_nor.p, a_nor, ba, hipMemcpyHostToDevice, st ), "merge_shuffled: upload" );
  }
  if( n_b > 0 )
  {
    RS_TRY( hipMemcpyAsync( W.b_pos.p, b_pos, bb, hipMemcpyHostToDevice, st ), "merge_shuffled: upload" );
    RS_TRY( hipMemcpyAsync( W.b_nor.p, b_nor, bb, hipMemcpyHostToDevice, st ), "merge_shuffled: upload" );
  }
  rc = fuse_permutation_device( (int)n, seed, st ); if( rc ) return rc;
  FuseMergeArgs A{};
  A.a.pos3 = W.a_pos.as<float>(); A.a.nor3 = W.a_nor.as<float>(); A.b.pos3 = W.b_pos.as<float>(); A.b.nor3 = W.b_nor.as<float>();
  A.n_a = (int)n_a; A.n = (int)n; std::memcpy( A.x.m, xform, 64 );
  A.perm = W.perm.as<int32_t>(); A.out_pos = W.out_pos.as<float>(); A.out_nor = W.out_nor.as<float>();
  rc = fuse_merge_launch( A, st ); if( rc ) return rc;
  RS_TRY( hipMemcpyAsync( out_pos, W.out_pos.p, bo, hipMemcpyDeviceToHost, st ), "merge_shuffled: download" );
  RS_TRY( hipMemcpyAsync( out_nor, W.out_nor.p, bo, hipMemcpyDeviceToHost, st ), "merge_shuffled: download" );
  if( source ) RS_TRY( hipMemcpyAsync( source, W.perm.p, (size_t)n * 4, hipMemcpyDeviceToHost, st ), "merge_shuffled: download" );
  RS_TRY( hipStreamSynchronize( st ), "merge_shuffled: kernels" );
  return RS_HIP_OK;
}

// wall clock of the calling thread between the call's own synchronisations (rs_hip_fuse_seconds)
static thread_local double g_fuse_s[5] = { 0, 0, 0, 0, 0 };
static thread_local bool g_fuse_clock = false;

void rs_hip_fuse_seconds( double out[5], int32_t enable )
{
  if( out ) for( int k = 0; k < 5; ++k ) out[k] = g_fuse_s[k];
  for( int k = 0; k < 5; ++k ) g_fuse_s[k] = 0.0;
  g_fuse_clock = enable != 0;
}

rs_hip_cloud_t* rs_hip_cloud_create_fused( const rs_hip_cloud_t* scan, const int32_t* scan_instance_ids, int32_t uidx,
                                           const rs_hip_cloud_t* model, const float pose[16], int32_t refine,
                                           float max_dist, float max_angle, float cell_size,
                                           float xform_out[16], float* icp_err, int32_t* source, int32_t* scan_index, int64_t* n_extracted )
{
  auto refuse = []( int rc, const char* what ) { fail( rc, what ); return (rs_hip_cloud_t*)nullptr; };
  if( n_extracted ) *n_extracted = 0;
  if( !scan || !model || !pose ) return refuse( RS_HIP_E_ARG, "cloud_create_fused: scan, model and pose are required" );
  const CloudPoints S = api_cloud_points( scan ), M = api_cloud_points( model );
  if( !S.qnor || !M.qnor ) return refuse( RS_HIP_E_ARG, "cloud_create_fused: both clouds need normals" );
  if( S.n > 0 && !scan_instance_ids ) return refuse( RS_HIP_E_ARG, "cloud_create_fused: the scan's instance ids are required" );
  hipStream_t st = nullptr;
  if( api_ready( &st ) ) return nullptr;
  FuseWorkspace& W = g_fuse_ws;
  auto t_last = std::chrono::steady_clock::now();
  // (only with the clock on: a synchronisation the call would not need, so that the lap is the stage's own)
  auto lap = [&]( int k ) {
    if( !g_fuse_clock ) return;
    (void)hipStreamSynchronize( st );
    const auto now = std::chrono::steady_clock::now();
    g_fuse_s[k] += std::chrono::duration<double>( now - t_last ).count(); t_last = now;
  };
#define FUSED_TRY( expr, what ) do { hipError_t e_ = ( expr ); if( e_ != hipSuccess ) return refuse( RS_HIP_E_RUNTIME, what ); } while( 0 )

  // 1. the points that carry uidx, in the order the scan was given to its cloud
  int64_t n_a = 0;
  if( S.n > 0 )
  {
    FUSED_TRY( W.point_ids.ensure( (size_t)S.n * 4 ), "cloud_create_fused: buffers" );
    FUSED_TRY( hipMemcpyAsync( W.point_ids.p, scan_instance_ids, (size_t)S.n * 4, hipMemcpyHostToDevice, st ), "cloud_create_fused: upload" );
    if( fuse_select_device( W.point_ids.as<int32_t>(), S.n, &uidx, 1, &n_a, st ) ) return nullptr;
  }
  lap( 0 );
  if( n_a == 0 ) { api_set_err( "" ); return nullptr; }          // database_update.cpp:58: the model stays as it is
  const int64_t n = n_a + (int64_t)M.n;
  if( n > fuse::MAX_POINTS ) return refuse( RS_HIP_E_CAPACITY, "cloud_create_fused: more than 2^24 merged points: beyond it the reference's shuffle can draw j > i" );
  if( n_extracted ) *n_extracted = n_a;
  if( scan_index ) FUSED_TRY( hipMemcpyAsync( scan_index, W.index.p, (size_t)n_a * 4, hipMemcpyDeviceToHost, st ), "cloud_create_fused: download" );

  FuseSide A{}; A.qpos = S.qpos; A.qnor = S.qnor; A.by_orig = S.by_orig; A.index = W.index.as<int32_t>();
  FuseSide B{}; B.qpos = M.qpos; B.qnor = M.qnor; B.by_orig = M.by_orig;

  // 2. xform = inverse( pose ), refined by ICP against the model unless the object is static (database_update.cpp:62-68)
  float xform[16];
  rs_hip_mat4_inverse( pose, xform );
  float err = 0.0f;
  if( refine )
  {
    float *d_pos = nullptr, *d_nor = nullptr;
    if( api_level_workspace( (size_t)n_a, true, &d_pos, &d_nor ) ) return nullptr;
    hipLaunchKernelGGL( k_fuse_gather, dim3( blocks_for( n_a, FUSE_BLOCK ) ), dim3( FUSE_BLOCK ), 0, st, A, (int)n_a, d_pos, d_nor );
    FUSED_TRY( hipGetLastError(), "cloud_create_fused: gather launch" );
    rs_hip_cloud_t* src = api_cloud_from_level_workspace( true, (int32_t)n_a, -1.0f );
    if( !src ) return nullptr;
    const float identity[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1 };
    int32_t iters = 0;
    const int rc = rs_hip_icp_align( src, model, xform, identity, max_dist, max_angle, 100, 0, &err, &iters );
    rs_hip_cloud_destroy( src );
    if( rc ) return nullptr;
  }
  lap( 1 );
  if( xform_out ) std::memcpy( xform_out, xform, 64 );
  if( icp_err ) *icp_err = err;

  // 3. the permutation, 4. the merge into the index build's input
  if( fuse_permutation_device( (int)n, fuse::SEED_MERGE, st ) ) return nullptr;
  lap( 2 );
  FuseMergeArgs G{};
  G.a = A; G.b = B; G.n_a = (int)n_a; G.n = (int)n; std::memcpy( G.x.m, xform, 64 ); G.perm = W.perm.as<int32_t>();
  if( api_level_workspace( (size_t)n, true, &G.out_pos, &G.out_nor ) ) return nullptr;
  if( fuse_merge_launch( G, st ) ) return nullptr;
  if( source ) FUSED_TRY( hipMemcpyAsync( source, W.perm.p, (size_t)n * 4, hipMemcpyDeviceToHost, st ), "cloud_create_fused: download" );
  lap( 3 );
  // 5. (synchronises the stream: the caller's arrays are complete when it returns)
  rs_hip_cloud_t* out = api_cloud_from_level_workspace( true, (int32_t)n, cell_size );
  lap( 4 );
  return out;
#undef FUSED_TRY
}

int rs_hip_shuffle_permutations( const int64_t* n, int32_t n_placements, uint32_t seed, int32_t* perm )
{
  char err[256] = "";
  FuseSegPlan L;
  if( int rc = fuse_seg_plan( n, n_placements, L, err, sizeof(err) ) ) return fail( rc, err );
  if( L.total > 0 && !perm ) return fail( RS_HIP_E_ARG, "shuffle_permutations: no array for the permutations" );
  if( L.total == 0 ) return RS_HIP_OK;
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  rc = fuse_permutations_device( L, seed, st ); if( rc ) return rc;
  RS_TRY_DRAIN( st, hipMemcpyAsync( perm, g_fuse_ws.perm.p, (size_t)L.total * 4, hipMemcpyDeviceToHost, st ), "shuffle_permutations: download" );
  RS_TRY( hipStreamSynchronize( st ), "shuffle_permutations: kernels" );
  return RS_HIP_OK;
}

int rs_hip_merge_shuffled_multi( int32_t n_placements, const float* const* a_pos, const float* const* a_nor, const int64_t* n_a, const float* xforms,
                                 const float* const* b_pos, const float* const* b_nor, const int64_t* n_b, uint32_t seed,
                                 float* out_pos, float* out_nor, int32_t* source )
{
  char err[256] = "";
  const int P = n_placements;
  if( P < 0 ) return fail( RS_HIP_E_ARG, "merge_shuffled_multi: a negative number of placements" );
  if( P == 0 ) return RS_HIP_OK;
  if( !a_pos || !a_nor || !n_a || !xforms || !b_pos || !b_nor || !n_b ) return fail( RS_HIP_E_ARG, "merge_shuffled_multi: null arrays" );
  std::vector<int64_t> n( (size_t)P );
  int64_t sum_a = 0, sum_b = 0;
  for( int p = 0; p < P; ++p )
  {
    if( n_a[p] < 0 || n_b[p] < 0 ) return fail( RS_HIP_E_ARG, "merge_shuffled_multi: a negative count" );
    if( n_a[p] > fuse::MAX_POINTS || n_b[p] > fuse::MAX_POINTS ) return fail( RS_HIP_E_CAPACITY, "merge_shuffled_multi: more than 2^24 points" );
    if( ( n_a[p] > 0 && ( !a_pos[p] || !a_nor[p] ) ) || ( n_b[p] > 0 && ( !b_pos[p] || !b_nor[p] ) ) )
      return fail( RS_HIP_E_ARG, "merge_shuffled_multi: null arrays (both clouds need normals)" );
    n[(size_t)p] = n_a[p] + n_b[p]; sum_a += n_a[p]; sum_b += n_b[p];
  }
  FuseSegPlan L;
  if( int rc = fuse_seg_plan( n.data(), P, L, err, sizeof(err) ) ) return fail( rc, err );
  if( L.total > 0 && ( !out_pos || !out_nor ) ) return fail( RS_HIP_E_ARG, "merge_shuffled_multi: no arrays for the merged points" );
  if( L.total == 0 ) return RS_HIP_OK;
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  FuseWorkspace& W = g_fuse_ws;
  const size_t ba = std::max<size_t>( (size_t)sum_a * 12, 12 ), bb = std::max<size_t>( (size_t)sum_b * 12, 12 ), bo = (size_t)L.total * 12;
  RS_TRY( W.a_pos.ensure( ba ), "merge_shuffled_multi: buffers" ); RS_TRY( W.a_nor.ensure( ba ), "merge_shuffled_multi: buffers" );
  RS_TRY( W.b_pos.ensure( bb ), "merge_shuffled_multi: buffers" ); RS_TRY( W.b_nor.ensure( bb ), "merge_shuffled_multi: buffers" );
  RS_TRY( W.out_pos.ensure( bo ), "merge_shuffled_multi: buffers" ); RS_TRY( W.out_nor.ensure( bo ), "merge_shuffled_multi: buffers" );
  std::vector<FuseSeg> seg( (size_t)P );
  size_t at_a = 0, at_b = 0;
  for( int p = 0; p < P; ++p )
  {
    FuseSeg& G = seg[(size_t)p];
    G = FuseSeg{};
    G.a.pos3 = W.a_pos.as<float>() + 3 * at_a; G.a.nor3 = W.a_nor.as<float>() + 3 * at_a;
    G.b.pos3 = W.b_pos.as<float>() + 3 * at_b; G.b.nor3 = W.b_nor.as<float>() + 3 * at_b;
    G.n_a = (int)n_a[p]; std::memcpy( G.x.m, xforms + 16 * (size_t)p, 64 );
    if( n_a[p] > 0 )
    {
      RS_TRY_DRAIN( st, hipMemcpyAsync( (void*)G.a.pos3, a_pos[p], (size_t)n_a[p] * 12, hipMemcpyHostToDevice, st ), "merge_shuffled_multi: upload" );
      RS_TRY_DRAIN( st, hipMemcpyAsync( (void*)G.a.nor3, a_nor[p], (size_t)n_a[p] * 12, hipMemcpyHostToDevice, st ), "merge_shuffled_multi: upload" );
    }
    if( n_b[p] > 0 )
    {
      RS_TRY_DRAIN( st, hipMemcpyAsync( (void*)G.b.pos3, b_pos[p], (size_t)n_b[p] * 12, hipMemcpyHostToDevice, st ), "merge_shuffled_multi: upload" );
      RS_TRY_DRAIN( st, hipMemcpyAsync( (void*)G.b.nor3, b_nor[p], (size_t)n_b[p] * 12, hipMemcpyHostToDevice, st ), "merge_shuffled_multi: upload" );
    }
    at_a += (size_t)n_a[p]; at_b += (size_t)n_b[p];
  }
  rc = fuse_permutations_device( L, seed, st ); if( rc ) return rc;
  rc = fuse_merge_seg_launch( L, seg, W.out_pos.as<float>(), W.out_nor.as<float>(), st ); if( rc ) return rc;
  RS_TRY_DRAIN( st, hipMemcpyAsync( out_pos, W.out_pos.p, bo, hipMemcpyDeviceToHost, st ), "merge_shuffled_multi: download" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( out_nor, W.out_nor.p, bo, hipMemcpyDeviceToHost, st ), "merge_shuffled_multi: download" );
  if( source ) RS_TRY_DRAIN( st, hipMemcpyAsync( source, W.perm.p, (size_t)L.total * 4, hipMemcpyDeviceToHost, st ), "merge_shuffled_multi: download" );
  RS_TRY( hipStreamSynchronize( st ), "merge_shuffled_multi: kernels" );
  return RS_HIP_OK;
}

int rs_hip_cloud_fuse_arrangement( const rs_hip_cloud_t* scan, const int32_t* scan_instance_ids, const rs_hip_fuse_placement_t* placements, int32_t n_placements,
                                   float max_dist, float max_angle, float cell_size, rs_hip_fuse_result_t* results )
{
  char err[256] = "";
  const int P = n_placements;
  if( P < 0 ) return fail( RS_HIP_E_ARG, "cloud_fuse_arrangement: a negative number of placements" );
  if( P == 0 ) return RS_HIP_OK;
  if( !scan || !placements || !results ) return fail( RS_HIP_E_ARG, "cloud_fuse_arrangement: scan, placements and results are required" );
  for( int p = 0; p < P; ++p )
  {
    const int32_t from = placements[p].model_from;
    if( from < -1 || from >= p )
    { snprintf( err, sizeof(err), "cloud_fuse_arrangement: placement %d: model_from %d is outside [-1, %d)", p, (int)from, p ); return fail( RS_HIP_E_ARG, err ); }
    if( from == -1 && !placements[p].model )
    { snprintf( err, sizeof(err), "cloud_fuse_arrangement: placement %d: model_from is -1 and there is no model", p ); return fail( RS_HIP_E_ARG, err ); }
  }
  const CloudPoints S = api_cloud_points( scan );
  if( !S.qnor ) return fail( RS_HIP_E_ARG, "cloud_fuse_arrangement: the scan needs normals" );
  for( int p = 0; p < P; ++p )
    if( placements[p].model_from == -1 && !api_cloud_has_normals( placements[p].model ) )
    { snprintf( err, sizeof(err), "cloud_fuse_arrangement: placement %d: the model needs normals", p ); return fail( RS_HIP_E_ARG, err ); }
  if( S.n > 0 && !scan_instance_ids ) return fail( RS_HIP_E_ARG, "cloud_fuse_arrangement: the scan's instance ids are required" );
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  FuseWorkspace& W = g_fuse_ws;
  auto t_last = std::chrono::steady_clock::now();
  // (only with the clock on: a synchronisation the call would not need, so that the lap is the stage's own)
  auto lap = [&]( int k ) {
    if( !g_fuse_clock ) return;
    (void)hipStreamSynchronize( st );
    const auto now = std::chrono::steady_clock::now();
    g_fuse_s[k] += std::chrono::duration<double>( now - t_last ).count(); t_last = now;
  };

  // 1. one table and one stable partition of the scan's ids; every placement's points are a segment of `order`
  std::vector<int64_t> n_a( (size_t)P, 0 ), first( (size_t)P, 0 );
  const int32_t* d_order = nullptr;
  if( S.n > 0 )
  {
    split::Table T; std::vector<int64_t> offsets;
    rc = split::segments_device( scan_instance_ids, S.n, T, offsets, &d_order, st ); if( rc ) return rc;
    std::unordered_map<int32_t, size_t> at;
    for( size_t k = 0; k < T.ids.size(); ++k ) at.emplace( T.ids[k], k );
    for( int p = 0; p < P; ++p )
    {
      const auto it = at.find( placements[p].uidx );
      if( it != at.end() ) { n_a[(size_t)p] = T.counts[it->second]; first[(size_t)p] = offsets[it->second]; }
    }
  }
  lap( 0 );

  // what every placement merges, and in which round: a placement that takes the shape an earlier one leaves runs a round after it
  std::vector<int64_t> n_model( (size_t)P ), n_shape( (size_t)P );
  std::vector<int> depth( (size_t)P, 0 );
  int rounds = 0;
  for( int p = 0; p < P; ++p )
  {
    const int32_t from = placements[p].model_from;
    n_model[(size_t)p] = from < 0 ? (int64_t)api_cloud_points( placements[p].model ).n : n_shape[(size_t)from];
    depth[(size_t)p] = from < 0 ? 0 : depth[(size_t)from] + 1;
    const int64_t n = n_a[(size_t)p] + n_model[(size_t)p];
    n_shape[(size_t)p] = n_a[(size_t)p] > 0 ? n : n_model[(size_t)p];        // database_update.cpp:58: nothing extracted, the shape stays
    if( n_a[(size_t)p] > 0 && n > fuse::MAX_POINTS )
    { snprintf( err, sizeof(err), "cloud_fuse_arrangement: placement %d: more than 2^24 merged points: beyond it the reference's shuffle can draw j > i", p ); return fail( RS_HIP_E_CAPACITY, err ); }
    rounds = std::max( rounds, depth[(size_t)p] + 1 );
  }
  std::vector<std::vector<int>> in_round( (size_t)rounds );
  for( int p = 0; p < P; ++p ) if( n_a[(size_t)p] > 0 ) in_round[(size_t)depth[(size_t)p]].push_back( p );
  for( const std::vector<int>& list : in_round )
  {
    int64_t total = 0;
    for( int p : list ) total += n_a[(size_t)p] + n_model[(size_t)p];
    if( total > fuse::MAX_TOTAL ) return fail( RS_HIP_E_CAPACITY, "cloud_fuse_arrangement: the merged points of one round together are more than an int32 index can name" );
  }

  std::vector<rs_hip_cloud_t*> made( (size_t)P, nullptr );
  std::vector<const rs_hip_cloud_t*> shape( (size_t)P, nullptr );
  std::vector<float> xforms( (size_t)P * 16, 0.0f ), errs( (size_t)P, 0.0f );
  auto undo = [&]( int code ) { for( rs_hip_cloud_t* c : made ) if( c ) rs_hip_cloud_destroy( c ); (void)hipStreamSynchronize( st ); return code; };
#define ARR_TRY( expr, what ) do { hipError_t e_ = ( expr ); if( e_ != hipSuccess ) return undo( fail( RS_HIP_E_RUNTIME, what, e_ ) ); } while( 0 )
  for( int p = 0; p < P; ++p )
    if( n_a[(size_t)p] > 0 && results[p].scan_index )
      ARR_TRY( hipMemcpyAsync( results[p].scan_index, d_order + first[(size_t)p], (size_t)n_a[(size_t)p] * 4, hipMemcpyDeviceToHost, st ), "cloud_fuse_arrangement: download" );

  for( int r = 0; r < rounds; ++r )
  {
    // the shapes earlier rounds left are this round's models (resolved through placements that extracted nothing)
    for( int p = 0; p < P; ++p )
      if( depth[(size_t)p] == r && n_a[(size_t)p] == 0 )
        shape[(size_t)p] = placements[p].model_from < 0 ? placements[p].model : shape[(size_t)placements[p].model_from];
    const std::vector<int>& list = in_round[(size_t)r];
    if( list.empty() ) continue;
    const size_t Q = list.size();
    std::vector<FuseSeg> seg( Q );
    std::vector<int64_t> sizes( Q );
    std::vector<const rs_hip_cloud_t*> model( Q );
    // 2. xform = inverse( pose ), refined by ICP against the model unless the object is static (database_update.cpp:62-68)
    std::vector<int64_t> src_first, src_count;        // the refined placements' extracted points, side by side in the level workspace
    std::vector<size_t> refined;
    int64_t src_total = 0;
    for( size_t k = 0; k < Q; ++k )
    {
      const int p = list[k];
      const rs_hip_fuse_placement_t& pl = placements[p];
      model[k] = pl.model_from < 0 ? pl.model : shape[(size_t)pl.model_from];
      const CloudPoints M = api_cloud_points( model[k] );
      const int64_t na = n_a[(size_t)p];
      FuseSeg& G = seg[k];
      G = FuseSeg{};
      G.a.qpos = S.qpos; G.a.qnor = S.qnor; G.a.by_orig = S.by_orig; G.a.index = d_order + first[(size_t)p];
      G.b.qpos = M.qpos; G.b.qnor = M.qnor; G.b.by_orig = M.by_orig;
      G.n_a = (int)na;
      sizes[k] = na + (int64_t)M.n;
      rs_hip_mat4_inverse( pl.pose, &xforms[16 * (size_t)p] );
      if( pl.refine ) { refined.push_back( k ); src_first.push_back( src_total ); src_count.push_back( na ); src_total += na; }
    }
    if( !refined.empty() )        // (src_total is below the round's merged total, which an int32 index names)
    {
      // the ICP sources of the round: one gather per placement into its segment, one batched index build, one ICP per placement
      float *d_pos = nullptr, *d_nor = nullptr;
      if( api_level_workspace( (size_t)src_total, true, &d_pos, &d_nor ) ) return undo( RS_HIP_E_RUNTIME );
      for( size_t j = 0; j < refined.size(); ++j )
      {
        const int64_t na = src_count[j];
        hipLaunchKernelGGL( k_fuse_gather, dim3( blocks_for( na, FUSE_BLOCK ) ), dim3( FUSE_BLOCK ), 0, st, seg[refined[j]].a, (int)na,
                            d_pos + 3 * (size_t)src_first[j], d_nor + 3 * (size_t)src_first[j] );
      }
      ARR_TRY( hipGetLastError(), "cloud_fuse_arrangement: gather launch" );
      std::vector<rs_hip_cloud_t*> src( refined.size(), nullptr );
      if( int brc = api_clouds_from_device( d_pos, d_nor, src_first.data(), src_count.data(), (int32_t)refined.size(), -1.0f, src.data() ) ) return undo( brc );
      int irc = RS_HIP_OK;
      for( size_t j = 0; j < refined.size() && !irc; ++j )
      {
        const int p = list[refined[j]];
        const float identity[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1 };
        int32_t iters = 0;
        irc = rs_hip_icp_align( src[j], model[refined[j]], &xforms[16 * (size_t)p], identity, max_dist, max_angle, 100, 0, &errs[(size_t)p], &iters );
      }
      for( rs_hip_cloud_t* c : src ) rs_hip_cloud_destroy( c );
      if( irc ) return undo( irc );
    }
    for( size_t k = 0; k < Q; ++k ) std::memcpy( seg[k].x.m, &xforms[16 * (size_t)list[k]], 64 );
    lap( 1 );
    // 3. all permutations of the round, 4. one merge launch into the concatenation
    FuseSegPlan L;
    if( int prc = fuse_seg_plan( sizes.data(), (int)Q, L, err, sizeof(err) ) ) return undo( fail( prc, err ) );
    if( fuse_permutations_device( L, fuse::SEED_MERGE, st ) ) return undo( RS_HIP_E_RUNTIME );
    lap( 2 );
    ARR_TRY( W.out_pos.ensure( (size_t)L.total * 12 ), "cloud_fuse_arrangement: buffers" ); ARR_TRY( W.out_nor.ensure( (size_t)L.total * 12 ), "cloud_fuse_arrangement: buffers" );
    if( fuse_merge_seg_launch( L, seg, W.out_pos.as<float>(), W.out_nor.as<float>(), st ) ) return undo( RS_HIP_E_RUNTIME );
    for( size_t k = 0; k < Q; ++k )
      if( results[list[k]].source )
        ARR_TRY( hipMemcpyAsync( results[list[k]].source, W.perm.as<int32_t>() + L.off[k], (size_t)sizes[k] * 4, hipMemcpyDeviceToHost, st ), "cloud_fuse_arrangement: download" );
    lap( 3 );
    // 5. one batched index build for the round's merged clouds, read from the concatenation where the merge left them
    {
      std::vector<int64_t> at( Q );
      std::vector<rs_hip_cloud_t*> merged( Q, nullptr );
      for( size_t k = 0; k < Q; ++k ) at[k] = L.off[k];
      if( int brc = api_clouds_from_device( W.out_pos.as<float>(), W.out_nor.as<float>(), at.data(), sizes.data(), (int32_t)Q, cell_size, merged.data() ) ) return undo( brc );
      for( size_t k = 0; k < Q; ++k ) { made[(size_t)list[k]] = merged[k]; shape[(size_t)list[k]] = merged[k]; }
    }
    lap( 4 );
  }
  ARR_TRY( hipStreamSynchronize( st ), "cloud_fuse_arrangement: kernels" );
#undef ARR_TRY
  for( int p = 0; p < P; ++p )
  {
    results[p].cloud = made[(size_t)p]; results[p].n_extracted = n_a[(size_t)p];
    std::memcpy( results[p].xform, &xforms[16 * (size_t)p], 64 ); results[p].icp_err = errs[(size_t)p];
  }
  api_set_err( "" );
  return RS_HIP_OK;
}

} // extern "C"
