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
#include "rs_host.h"
#include "rs_fuse.h"

#include <chrono>
#include <cstring>
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

} // namespace rs

using namespace rs;

namespace {

struct FuseWorkspace { Buf key, step, skey, sstep, perm, tmp, point_ids, ids, flags, rank, index, a_pos, a_nor, b_pos, b_nor, out_pos, out_nor; };
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

} // extern "C"
