// Floor and wall planes — rspf__detect_floor, rspf__detect_walls, rspf__gather_model_inliers and rspf_relabel_walls_and_floors
// (lib/rs/rs_pointcloud_filters.cpp:116-323, 617-671): rs_hip_plane_hypotheses, rs_hip_plane_votes, rs_hip_detect_planes,
// rs_hip_gather_plane_inliers, rs_hip_relabel_walls_and_floors.
//
// The reference scores every hypothesis of a RANSAC round against every point, one after the other: 2 500 floor hypotheses, then
// 5 000 wall hypotheses per round for as many rounds as there are walls plus one.  The votes are integer counts over fp32
// arithmetic without reductions, so they are made equal to the reference's bit for bit and summed in any order.
//
// How a detection runs (round 0: the floor; rounds 1..: the walls):
//   k_plane_candidates   once: the cloud's points in the order it was created from (16-byte records) and the two candidate masks
//                        from the normals (:141-146, :209-214).
//   per round            the mask comes to the host (n bytes); rs_planes.h builds the alias table, draws the triples (the walls'
//                        redraws make the number of draws depend on the data: sequential) and computes centre and normal of each
//                        hypothesis and the walls' up test; those go to the device.
//   k_plane_flags + scan + k_plane_compact   the round's candidates' coordinates, compacted (order does not matter to a count).
//   k_plane_votes        one lane owns one hypothesis (six floats in registers, a private counter); a workgroup covers 256
//                        hypotheses x one tile of PLANE_TILE candidates and ends with one integer atomicAdd per lane.  The tile is
//                        staged in LDS and every lane of a wave reads the same address (a broadcast), or, form 1, the lanes read
//                        the tile through wave-uniform global loads.
//   k_plane_best         the lowest index among the maximal counts: the reference's strict > against a best of 0 (:181, :241).
//   k_plane_remove       remove_inliers (:96-114) on the mask, with the round's best model — or, kept as the reference has it, the
//                        previous one where the round detected nothing.
//   k_plane_gather_flags + scan + k_plane_scatter   one flag per (model, point), one exclusive scan over all of them, index and
//                        offsets from the ranks: stable, so each model's indices increase.
//   k_plane_relabel      one lane per point, the models in a loop: the relabel's gather and its writes fused, no index list.
#include "rs_host.h"
#include "rs_planes.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace rs {

constexpr int PLANE_BLOCK = 256;
constexpr int PLANE_TILE = 1024;         // candidates per workgroup of k_plane_votes: 16 KB of LDS

__device__ __forceinline__ float plane_abs( float x ) { return x < 0 ? -x : x; }           // msh_abs
// msh_vec3_dot( n, msh_vec3_sub( p, c ) )
__device__ __forceinline__ float plane_offset( const float n[3], const float c[3], float px, float py, float pz )
{
  return n[0] * ( px - c[0] ) + n[1] * ( py - c[1] ) + n[2] * ( pz - c[2] );
}

// lane i: original point i.  pts[i] = its position; the masks from its normal.
__global__ __launch_bounds__( PLANE_BLOCK ) void k_plane_candidates( const float4* qpos, const float4* qnor, const int* by_orig, int n,
                                                                      float dot_threshold, float4* pts, uint8_t* floor_mask, uint8_t* wall_mask )
{
  const int i = blockIdx.x * PLANE_BLOCK + threadIdx.x;
  if( i >= n ) return;
  const int s = by_orig[i];
  const float4 p = qpos[s], q = qnor[s];
  pts[i] = make_float4( p.x, p.y, p.z, 0.0f );
  const float dot = q.x * 0.0f + q.y * 1.0f + q.z * 0.0f;                                   // msh_vec3_dot( nrm, posy )
  floor_mask[i] = dot > dot_threshold ? 1 : 0;                                              // :212
  wall_mask[i] = plane_abs( dot ) < ( 1 - dot_threshold ) ? 1 : 0;                          // :144
}
// packed xyz (host arrays of rs_hip_plane_votes) to the 16-byte records
__global__ __launch_bounds__( PLANE_BLOCK ) void k_plane_pack( const float* pos3, int n, float4* pts )
{
  const int i = blockIdx.x * PLANE_BLOCK + threadIdx.x;
  if( i >= n ) return;
  const size_t o = 3 * (size_t)i;
  pts[i] = make_float4( pos3[o], pos3[o + 1], pos3[o + 2], 0.0f );
}
__global__ __launch_bounds__( PLANE_BLOCK ) void k_plane_flags( const uint8_t* mask, int n, uint32_t* flags /* n + 1 */ )
{
  const int i = blockIdx.x * PLANE_BLOCK + threadIdx.x;
  if( i > n ) return;
  flags[i] = ( i < n && mask[i] ) ? 1u : 0u;
}
__global__ __launch_bounds__( PLANE_BLOCK ) void k_plane_compact( const float4* pts, const uint32_t* flags, const uint32_t* rank, int n, float4* cand )
{
  const int i = blockIdx.x * PLANE_BLOCK + threadIdx.x;
  if( i < n && flags[i] ) cand[rank[i]] = pts[i];
}

// hyp: n_hyp records of two float4 (centre, normal).  blockIdx.x: 256 hypotheses, blockIdx.y: one tile of candidates.
template <bool LDS_TILE>
__global__ __launch_bounds__( PLANE_BLOCK ) void k_plane_votes( const float4* __restrict__ cand, int n_cand, const float4* __restrict__ hyp,
                                                                 const uint8_t* __restrict__ valid, int n_hyp, float dist_threshold, int32_t* counts )
{
  __shared__ float4 tile[LDS_TILE ? PLANE_TILE : 1];
  const int h = blockIdx.x * PLANE_BLOCK + threadIdx.x;
  const int base = blockIdx.y * PLANE_TILE;
  const int m = min( PLANE_TILE, n_cand - base );            // >= 1: the grid has ceil( n_cand / PLANE_TILE ) tiles
  if( LDS_TILE )
  {
    for( int k = threadIdx.x; k < m; k += PLANE_BLOCK ) tile[k] = cand[base + k];
    __syncthreads();
  }
  if( h >= n_hyp ) return;
  const float4 c4 = hyp[2 * (size_t)h], n4 = hyp[2 * (size_t)h + 1];
  const float c[3] = { c4.x, c4.y, c4.z }, nn[3] = { n4.x, n4.y, n4.z };
  int count = 0;
  for( int k = 0; k < m; ++k )
  {
    const float4 p = LDS_TILE ? tile[k] : cand[base + k];    // the same address in every lane
    const float dist = plane_abs( plane_offset( nn, c, p.x, p.y, p.z ) );
    count += dist < dist_threshold ? 1 : 0;
  }
  if( count && ( !valid || valid[h] ) ) atomicAdd( counts + h, count );
}

// One workgroup.  out[0] = the lowest index among the hypotheses with the maximal count, -1 if that count is 0; out[1] = the count.
__global__ __launch_bounds__( PLANE_BLOCK ) void k_plane_best( const int32_t* counts, int n_hyp, int32_t* out )
{
  __shared__ int32_t s_count[PLANE_BLOCK], s_idx[PLANE_BLOCK];
  int32_t best = 0, idx = -1;
  for( int h = threadIdx.x; h < n_hyp; h += PLANE_BLOCK )   // increasing h: strict > keeps the lowest index
  {
    const int32_t c = counts[h];
    if( c > best ) { best = c; idx = h; }
  }
  s_count[threadIdx.x] = best; s_idx[threadIdx.x] = idx;
  __syncthreads();
  for( int w = PLANE_BLOCK / 2; w > 0; w >>= 1 )
  {
    if( (int)threadIdx.x < w )
    {
      const int32_t c = s_count[threadIdx.x + w], i = s_idx[threadIdx.x + w];
      if( c > s_count[threadIdx.x] || ( c == s_count[threadIdx.x] && c > 0 && i < s_idx[threadIdx.x] ) ) { s_count[threadIdx.x] = c; s_idx[threadIdx.x] = i; }
    }
    __syncthreads();
  }
  if( threadIdx.x == 0 ) { out[0] = s_idx[0]; out[1] = s_count[0]; }
}

struct PlaneModel { float c[3], n[3]; };

__global__ __launch_bounds__( PLANE_BLOCK ) void k_plane_remove( const float4* pts, int n, PlaneModel M, float dist_threshold, uint8_t* mask )
{
  const int i = blockIdx.x * PLANE_BLOCK + threadIdx.x;
  if( i >= n || !mask[i] ) return;
  const float4 p = pts[i];
  if( plane_abs( plane_offset( M.n, M.c, p.x, p.y, p.z ) ) < dist_threshold ) mask[i] = 0;
}

// a model as the gather reads it
struct PlaneGatherModel { float c[3], n[3], poly[12]; float up_dot; int32_t valid; };

// rspf__is_point_within_convex_poly (:254-275) of the four-corner quad: i < n_verts - 1 covers three corners
__device__ __forceinline__ bool plane_within( const float* poly, float px, float py, float pz )
{
  for( int i = 0; i < 3; ++i )
  {
    const float* a = poly + 3 * i, *b = poly + 3 * ( i + 1 ), *c = poly + 3 * ( ( i + 2 ) % 4 );
    const float v1[3] = { b[0] - a[0], b[1] - a[1], b[2] - a[2] };
    const float v2[3] = { c[0] - b[0], c[1] - b[1], c[2] - b[2] };
    const float v3[3] = { px - b[0], py - b[1], pz - b[2] };
    const float n1[3] = { v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0] };
    const float n2[3] = { v1[1] * v3[2] - v1[2] * v3[1], v1[2] * v3[0] - v1[0] * v3[2], v1[0] * v3[1] - v1[1] * v3[0] };
    const float val = n1[0] * n2[0] + n1[1] * n2[1] + n1[2] * n2[2];
    if( val < 0 ) return false;
  }
  return true;
}
// :298-319 for one model and one point
__device__ __forceinline__ bool plane_inlier( const PlaneGatherModel& M, const float4 p, const float4 q, float dot_threshold, float dist_threshold,
                                              int check_validity, int check_extends )
{
  if( check_validity && !M.valid ) return false;
  const float dist = plane_abs( plane_offset( M.n, M.c, p.x, p.y, p.z ) );
  const float dot = plane_abs( q.x * M.n[0] + q.y * M.n[1] + q.z * M.n[2] );
  if( !( dot > dot_threshold && dist < dist_threshold ) ) return false;
  return check_extends ? plane_within( M.poly, p.x, p.y, p.z ) : true;
}

// lane t = m * n + i: flags[t] = point i (original order) is an inlier of model m; flags[n_models * n] = 0
__global__ __launch_bounds__( PLANE_BLOCK ) void k_plane_gather_flags( const float4* qpos, const float4* qnor, const int* by_orig, int n,
                                                                        const PlaneGatherModel* models, int n_models, float dot_threshold,
                                                                        float dist_threshold, int check_validity, int check_extends, uint32_t* flags )
{
  const long long t = (long long)blockIdx.x * PLANE_BLOCK + threadIdx.x;
  const long long total = (long long)n_models * n;
  if( t > total ) return;
  uint32_t f = 0u;
  if( t < total )
  {
    const int m = (int)( t / n ), i = (int)( t - (long long)m * n );
    const int s = by_orig[i];
    f = plane_inlier( models[m], qpos[s], qnor[s], dot_threshold, dist_threshold, check_validity, check_extends ) ? 1u : 0u;
  }
  flags[t] = f;
}
__global__ __launch_bounds__( PLANE_BLOCK ) void k_plane_scatter( const uint32_t* flags, const uint32_t* rank, int n, long long total, int32_t* index )
{
  const long long t = (long long)blockIdx.x * PLANE_BLOCK + threadIdx.x;
  if( t < total && flags[t] ) index[rank[t]] = (int32_t)( t % n );
}

// :646-667 per point: the models in order, each field decided by the first valid model that holds the point
__global__ __launch_bounds__( PLANE_BLOCK ) void k_plane_relabel( const float4* qpos, const float4* qnor, const int* by_orig, int n,
                                                                   const PlaneGatherModel* models, int n_models, int floor_idx, int wall_idx,
                                                                   int unlabelled_idx, int32_t* class_ids, int32_t* instance_ids )
{
  const int i = blockIdx.x * PLANE_BLOCK + threadIdx.x;
  if( i >= n ) return;
  const int s = by_orig[i];
  const float4 p = qpos[s], q = qnor[s];
  int32_t cls = class_ids[i], inst = instance_ids[i];
  for( int m = 0; m < n_models; ++m )
  {
    if( !plane_inlier( models[m], p, q, 0.0f, 0.05f, 1, 1 ) ) continue;
    const bool is_floor = models[m].up_dot > 0.8f;
    if( inst >= 1024 ) inst = is_floor ? 0 : 1;
    if( cls == unlabelled_idx ) cls = is_floor ? floor_idx : wall_idx;
  }
  class_ids[i] = cls; instance_ids[i] = inst;
}

} // namespace rs

using namespace rs;

namespace {

struct PlaneWorkspace { Buf pts, pos3, floor_mask, wall_mask, flags, rank, tmp, cand, hyp, valid, counts, best, models, index, cls, inst; };
thread_local PlaneWorkspace g_plane_ws;
int32_t g_plane_form = 0;

// The votes of n_hyp hypotheses (host arrays) over the points of W.pts that `mask` (device, n >= 1 bytes) keeps: compaction, votes
// and, where best is asked for, the best; counts land in W.counts, {index, count} in W.best.  *n_cand: the candidates.
int plane_round_device( int n, const uint8_t* d_mask, const float* center, const float* normal, const uint8_t* valid, int n_hyp,
                        float dist_threshold, bool with_best, int64_t* n_cand, hipStream_t st )
{
  PlaneWorkspace& W = g_plane_ws;
  const size_t n1 = (size_t)n + 1, hh = (size_t)std::max( n_hyp, 1 );
  const size_t tmp_bytes = build_scan_temp_bytes( n1 );
  RS_TRY( W.flags.ensure( n1 * 4 ), "planes: buffers" ); RS_TRY( W.rank.ensure( n1 * 4 ), "planes: buffers" );
  RS_TRY( W.tmp.ensure( tmp_bytes + 256 ), "planes: buffers" ); RS_TRY( W.cand.ensure( (size_t)n * 16 ), "planes: buffers" );
  RS_TRY( W.hyp.ensure( hh * 32 ), "planes: buffers" ); RS_TRY( W.valid.ensure( hh ), "planes: buffers" );
  RS_TRY( W.counts.ensure( hh * 4 ), "planes: buffers" ); RS_TRY( W.best.ensure( 8 ), "planes: buffers" );
  std::vector<float> packed( hh * 8, 0.0f );
  for( int h = 0; h < n_hyp; ++h )
  {
    std::memcpy( &packed[8 * (size_t)h], center + 3 * (size_t)h, 12 );
    std::memcpy( &packed[8 * (size_t)h + 4], normal + 3 * (size_t)h, 12 );
  }
  // (pageable memory: the copies have left the host arrays when the calls return)
  RS_TRY( hipMemcpyAsync( W.hyp.p, packed.data(), hh * 32, hipMemcpyHostToDevice, st ), "planes: upload" );
  if( valid && n_hyp > 0 ) RS_TRY( hipMemcpyAsync( W.valid.p, valid, (size_t)n_hyp, hipMemcpyHostToDevice, st ), "planes: upload" );
  RS_TRY( hipMemsetAsync( W.counts.p, 0, hh * 4, st ), "planes: clear" );
  {
    ProfSpan span( "plane_compact" );
    hipLaunchKernelGGL( k_plane_flags, dim3( blocks_for( (long long)n1, PLANE_BLOCK ) ), dim3( PLANE_BLOCK ), 0, st, d_mask, n, W.flags.as<uint32_t>() );
    if( build_exclusive_scan( W.tmp.p, tmp_bytes, W.flags.as<uint32_t>(), W.rank.as<uint32_t>(), n1, st ) )
      return fail( RS_HIP_E_RUNTIME, "planes: device scan failed" );
    hipLaunchKernelGGL( k_plane_compact, dim3( blocks_for( n, PLANE_BLOCK ) ), dim3( PLANE_BLOCK ), 0, st, W.pts.as<float4>(), W.flags.as<uint32_t>(), W.rank.as<uint32_t>(), n, W.cand.as<float4>() );
  }
  RS_TRY( hipGetLastError(), "planes: compaction launch" );
  uint32_t got = 0;
  RS_TRY( hipMemcpyAsync( &got, W.rank.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, st ), "planes: download" );
  RS_TRY( hipStreamSynchronize( st ), "planes: compaction" );
  *n_cand = (int64_t)got;
  {
    ProfSpan span( "plane_votes" );
    if( got > 0 && n_hyp > 0 )
    {
      const dim3 grid( blocks_for( n_hyp, PLANE_BLOCK ), ( got + PLANE_TILE - 1 ) / PLANE_TILE );
      const uint8_t* d_valid = valid ? W.valid.as<uint8_t>() : nullptr;
      if( g_plane_form == 0 )
        hipLaunchKernelGGL( k_plane_votes<true>, grid, dim3( PLANE_BLOCK ), 0, st, W.cand.as<float4>(), (int)got, W.hyp.as<float4>(), d_valid, n_hyp, dist_threshold, W.counts.as<int32_t>() );
      else
        hipLaunchKernelGGL( k_plane_votes<false>, grid, dim3( PLANE_BLOCK ), 0, st, W.cand.as<float4>(), (int)got, W.hyp.as<float4>(), d_valid, n_hyp, dist_threshold, W.counts.as<int32_t>() );
    }
  }
  if( with_best )
  {
    ProfSpan span( "plane_best" );
    hipLaunchKernelGGL( k_plane_best, dim3( 1 ), dim3( PLANE_BLOCK ), 0, st, W.counts.as<int32_t>(), n_hyp, W.best.as<int32_t>() );
  }
  RS_TRY( hipGetLastError(), "planes: votes launch" );
  return RS_HIP_OK;
}

// the models as the gather kernels read them, in W.models
int plane_upload_models( const float* centers, const float* normals, const float* axes, const float* extends, const int8_t* valid,
                         const float* up_dot, int n_models, bool with_quad, hipStream_t st )
{
  PlaneWorkspace& W = g_plane_ws;
  std::vector<PlaneGatherModel> M( (size_t)n_models );
  for( int m = 0; m < n_models; ++m )
  {
    PlaneGatherModel& G = M[(size_t)m];
    std::memset( &G, 0, sizeof(G) );
    std::memcpy( G.c, centers + 3 * (size_t)m, 12 ); std::memcpy( G.n, normals + 3 * (size_t)m, 12 );
    if( with_quad ) planes::quad( G.c, axes + 9 * (size_t)m, extends + 4 * (size_t)m, G.poly );
    G.up_dot = up_dot ? up_dot[m] : 0.0f;
    G.valid = valid ? ( valid[m] ? 1 : 0 ) : 1;
  }
  RS_TRY( W.models.ensure( M.size() * sizeof(PlaneGatherModel) ), "planes: buffers" );
  RS_TRY( hipMemcpyAsync( W.models.p, M.data(), M.size() * sizeof(PlaneGatherModel), hipMemcpyHostToDevice, st ), "planes: upload" );
  RS_TRY( hipStreamSynchronize( st ), "planes: upload" );     // M leaves scope
  return RS_HIP_OK;
}

} // namespace

extern "C" {

int32_t rs_hip_plane_votes_form( int32_t form )
{
  const int32_t was = g_plane_form;
  if( form >= 0 ) g_plane_form = form ? 1 : 0;
  return was;
}

int rs_hip_plane_hypotheses( const float* pos, int64_t n, const uint8_t* active, int32_t n_iter, int32_t distinct, uint32_t seed,
                             int32_t* idx, float* center, float* normal )
{
  char err[256] = "";
  const int rc = planes::hypotheses( pos, n, active, n_iter, distinct, seed, idx, center, normal, err, sizeof(err) );
  if( rc ) api_set_err( err );
  return rc;
}

int rs_hip_plane_votes( const float* pos, int64_t n, const uint8_t* active, const float* center, const float* normal,
                        const uint8_t* valid, int32_t n_hyp, float dist_threshold, int32_t* counts )
{
  if( n < 0 || n_hyp < 0 || ( n > 0 && ( !pos || !active ) ) || ( n_hyp > 0 && ( !center || !normal || !counts ) ) )
    return fail( RS_HIP_E_ARG, "plane_votes: null arrays or a negative count" );
  if( n > planes::MAX_POINTS ) return fail( RS_HIP_E_CAPACITY, "plane_votes: more than 2^24 points" );
  if( n_hyp == 0 ) return RS_HIP_OK;
  if( n == 0 ) { std::memset( counts, 0, (size_t)n_hyp * 4 ); return RS_HIP_OK; }
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  PlaneWorkspace& W = g_plane_ws;
  RS_TRY( W.pos3.ensure( (size_t)n * 12 ), "plane_votes: buffers" ); RS_TRY( W.pts.ensure( (size_t)n * 16 ), "plane_votes: buffers" );
  RS_TRY( W.wall_mask.ensure( (size_t)n ), "plane_votes: buffers" );
  RS_TRY( hipMemcpyAsync( W.pos3.p, pos, (size_t)n * 12, hipMemcpyHostToDevice, st ), "plane_votes: upload" );
  RS_TRY( hipMemcpyAsync( W.wall_mask.p, active, (size_t)n, hipMemcpyHostToDevice, st ), "plane_votes: upload" );
  hipLaunchKernelGGL( k_plane_pack, dim3( blocks_for( n, PLANE_BLOCK ) ), dim3( PLANE_BLOCK ), 0, st, W.pos3.as<float>(), (int)n, W.pts.as<float4>() );
  int64_t n_cand = 0;
  rc = plane_round_device( (int)n, W.wall_mask.as<uint8_t>(), center, normal, valid, n_hyp, dist_threshold, false, &n_cand, st ); if( rc ) return rc;
  RS_TRY( hipMemcpyAsync( counts, W.counts.p, (size_t)n_hyp * 4, hipMemcpyDeviceToHost, st ), "plane_votes: download" );
  RS_TRY( hipStreamSynchronize( st ), "plane_votes: kernels" );
  return RS_HIP_OK;
}

int rs_hip_detect_planes( const rs_hip_cloud_t* cloud, float dot_threshold, float dist_threshold, int64_t count_threshold,
                          int32_t floor_iters, int32_t wall_iters, int32_t capacity, float* centers, float* normals, int64_t* n_inliers,
                          int32_t* n_floors, int32_t* n_walls, int32_t* n_models, rs_hip_plane_trace_t* trace )
{
  if( !cloud || !n_floors || !n_walls || !n_models || capacity < 0 || floor_iters < 0 || wall_iters < 0 || count_threshold < 0 ||
      ( capacity > 0 && ( !centers || !normals || !n_inliers ) ) )
    return fail( RS_HIP_E_ARG, "detect_planes: null arrays or a negative count" );
  if( trace && ( trace->capacity_rounds < 0 || trace->max_iters < std::max( floor_iters, wall_iters ) ) )
    return fail( RS_HIP_E_ARG, "detect_planes: the trace's max_iters is below an iteration count, or its capacity is negative" );
  const CloudPoints S = api_cloud_points( cloud );
  if( !S.qnor ) return fail( RS_HIP_E_ARG, "detect_planes: the cloud needs normals" );
  if( S.n > planes::MAX_POINTS ) return fail( RS_HIP_E_CAPACITY, "detect_planes: more than 2^24 points: beyond it the reference's (float)n is inexact" );
  if( S.n <= 0 ) return fail( RS_HIP_E_ARG, "detect_planes: an empty cloud has no candidates: the reference's pdf would stay uninitialised" );
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  PlaneWorkspace& W = g_plane_ws;
  const int n = S.n;
  RS_TRY( W.pts.ensure( (size_t)n * 16 ), "detect_planes: buffers" );
  RS_TRY( W.floor_mask.ensure( (size_t)n ), "detect_planes: buffers" ); RS_TRY( W.wall_mask.ensure( (size_t)n ), "detect_planes: buffers" );
  hipLaunchKernelGGL( k_plane_candidates, dim3( blocks_for( n, PLANE_BLOCK ) ), dim3( PLANE_BLOCK ), 0, st, S.qpos, S.qnor, S.by_orig, n, dot_threshold,
                      W.pts.as<float4>(), W.floor_mask.as<uint8_t>(), W.wall_mask.as<uint8_t>() );
  RS_TRY( hipGetLastError(), "detect_planes: candidates launch" );
  // the planner reads positions on the host: three of them per hypothesis
  std::vector<float4> pts4( (size_t)n );
  RS_TRY( hipMemcpyAsync( pts4.data(), W.pts.p, (size_t)n * 16, hipMemcpyDeviceToHost, st ), "detect_planes: download" );
  RS_TRY( hipStreamSynchronize( st ), "detect_planes: candidates" );
  std::vector<float> pos( 3 * (size_t)n );
  for( int i = 0; i < n; ++i ) { pos[3 * (size_t)i] = pts4[(size_t)i].x; pos[3 * (size_t)i + 1] = pts4[(size_t)i].y; pos[3 * (size_t)i + 2] = pts4[(size_t)i].z; }
  std::vector<float4>().swap( pts4 );

  struct Model { float c[3], n[3]; int64_t count; };
  std::vector<Model> models;
  std::vector<uint8_t> mask( (size_t)n ), valid;
  std::vector<int32_t> idx, counts;
  std::vector<float> hc, hn;
  const float wall_limit = 1 - dot_threshold;               // :177, a float subtraction
  int round = 0;
  // one round: *best_idx = -1 where nothing was detected
  auto run_round = [&]( uint8_t* d_mask, int n_iter, int distinct, int32_t* best_idx, int32_t* best_count ) -> int
  {
    char err[256] = "";
    RS_TRY( hipMemcpyAsync( mask.data(), d_mask, (size_t)n, hipMemcpyDeviceToHost, st ), "detect_planes: download" );
    RS_TRY( hipStreamSynchronize( st ), "detect_planes: mask" );
    idx.assign( 3 * (size_t)n_iter, 0 ); hc.assign( 3 * (size_t)n_iter, 0.0f ); hn.assign( 3 * (size_t)n_iter, 0.0f ); valid.assign( (size_t)n_iter, 1 );
    if( int prc = planes::hypotheses( pos.data(), n, mask.data(), n_iter, distinct, planes::SEED, idx.data(), hc.data(), hn.data(), err, sizeof(err) ) )
      return fail( prc, err );
    if( distinct )
      for( int h = 0; h < n_iter; ++h ) valid[(size_t)h] = planes::abs_ref( planes::up_dot( &hn[3 * (size_t)h] ) ) < wall_limit ? 1 : 0;
    int64_t n_cand = 0;
    if( int drc = plane_round_device( n, d_mask, hc.data(), hn.data(), valid.data(), n_iter, dist_threshold, true, &n_cand, st ) ) return drc;
    int32_t best[2] = { -1, 0 };
    RS_TRY( hipMemcpyAsync( best, W.best.p, 8, hipMemcpyDeviceToHost, st ), "detect_planes: download" );
    const bool rec = trace && round < trace->capacity_rounds;
    if( rec && trace->counts && n_iter > 0 )
      RS_TRY( hipMemcpyAsync( trace->counts + (size_t)round * trace->max_iters, W.counts.p, (size_t)n_iter * 4, hipMemcpyDeviceToHost, st ), "detect_planes: download" );
    RS_TRY( hipStreamSynchronize( st ), "detect_planes: votes" );
    if( n_iter == 0 ) { best[0] = -1; best[1] = 0; }
    *best_idx = best[0]; *best_count = best[1];
    if( rec )
    {
      if( trace->idx ) std::memcpy( trace->idx + (size_t)round * 3 * trace->max_iters, idx.data(), idx.size() * 4 );
      if( trace->valid ) std::memcpy( trace->valid + (size_t)round * trace->max_iters, valid.data(), valid.size() );
      if( trace->best ) trace->best[round] = best[0];
      if( trace->n_iters ) trace->n_iters[round] = n_iter;
      if( trace->mask_before ) std::memcpy( trace->mask_before + (size_t)round * n, mask.data(), (size_t)n );
    }
    return RS_HIP_OK;
  };
  auto record_mask_after = [&]( const uint8_t* d_mask ) -> int
  {
    if( !( trace && round < trace->capacity_rounds && trace->mask_after ) ) return RS_HIP_OK;
    RS_TRY( hipMemcpyAsync( trace->mask_after + (size_t)round * n, d_mask, (size_t)n, hipMemcpyDeviceToHost, st ), "detect_planes: download" );
    RS_TRY( hipStreamSynchronize( st ), "detect_planes: mask" );
    return RS_HIP_OK;
  };

  // rspf__detect_floor (:204-252)
  int32_t bi = -1, bc = 0, floors = 0;
  rc = run_round( W.floor_mask.as<uint8_t>(), floor_iters, 0, &bi, &bc ); if( rc ) return rc;
  if( bi >= 0 )
  {
    Model m; std::memcpy( m.c, &hc[3 * (size_t)bi], 12 ); std::memcpy( m.n, &hn[3 * (size_t)bi], 12 ); m.count = bc;
    models.push_back( m ); floors = 1;
  }
  rc = record_mask_after( W.floor_mask.as<uint8_t>() ); if( rc ) return rc;
  ++round;

  // rspf__detect_walls (:136-202)
  Model best_wall; std::memset( &best_wall, 0, sizeof(best_wall) );      // best_wall_model = {0}
  int32_t walls = 0;
  do
  {
    best_wall.count = 0;                                                  // :157
    rc = run_round( W.wall_mask.as<uint8_t>(), wall_iters, 1, &bi, &bc ); if( rc ) return rc;
    if( bi >= 0 )
    {
      std::memcpy( best_wall.c, &hc[3 * (size_t)bi], 12 ); std::memcpy( best_wall.n, &hn[3 * (size_t)bi], 12 ); best_wall.count = bc;
      models.push_back( best_wall );
    }
    // :192: with the round's best, or — nothing detected — the model the last round left there
    PlaneModel R; std::memcpy( R.c, best_wall.c, 12 ); std::memcpy( R.n, best_wall.n, 12 );
    hipLaunchKernelGGL( k_plane_remove, dim3( blocks_for( n, PLANE_BLOCK ) ), dim3( PLANE_BLOCK ), 0, st, W.pts.as<float4>(), n, R, dist_threshold, W.wall_mask.as<uint8_t>() );
    RS_TRY( hipGetLastError(), "detect_planes: remove launch" );
    rc = record_mask_after( W.wall_mask.as<uint8_t>() ); if( rc ) return rc;
    ++round; ++walls;
  } while( best_wall.count > count_threshold );
  if( models.empty() ) return fail( RS_HIP_E_ARG, "detect_planes: no floor and no wall: the reference would pop an empty model array" );
  models.pop_back();                                                      // :197
  --walls;
  if( (int64_t)models.size() > capacity ) return fail( RS_HIP_E_CAPACITY, "detect_planes: more models than the caller's capacity" );
  for( size_t m = 0; m < models.size(); ++m )
  {
    std::memcpy( centers + 3 * m, models[m].c, 12 ); std::memcpy( normals + 3 * m, models[m].n, 12 ); n_inliers[m] = models[m].count;
  }
  *n_floors = floors; *n_walls = walls; *n_models = (int32_t)models.size();
  if( trace ) trace->n_rounds = round;
  return RS_HIP_OK;
}

int rs_hip_gather_plane_inliers( const rs_hip_cloud_t* cloud, const float* centers, const float* normals, const float* axes,
                                 const float* extends, const int8_t* valid, int32_t n_models, float dot_threshold,
                                 float dist_threshold, int32_t check_validity, int32_t check_extends,
                                 int32_t* index, int64_t capacity, int64_t* offsets )
{
  if( !cloud || !offsets || n_models < 0 || capacity < 0 || ( capacity > 0 && !index ) ||
      ( n_models > 0 && ( !centers || !normals || ( check_validity && !valid ) || ( check_extends && ( !axes || !extends ) ) ) ) )
    return fail( RS_HIP_E_ARG, "gather_plane_inliers: null arrays or a negative count" );
  const CloudPoints S = api_cloud_points( cloud );
  if( !S.qnor ) return fail( RS_HIP_E_ARG, "gather_plane_inliers: the cloud needs normals" );
  const long long total = (long long)n_models * std::max( S.n, 0 );
  if( total > 2147483646ll ) return fail( RS_HIP_E_CAPACITY, "gather_plane_inliers: models x points exceed what one scan of 2^31 flags holds" );
  if( total == 0 ) { for( int m = 0; m <= n_models; ++m ) offsets[m] = 0; return RS_HIP_OK; }
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  PlaneWorkspace& W = g_plane_ws;
  rc = plane_upload_models( centers, normals, axes, extends, check_validity ? valid : nullptr, nullptr, n_models, check_extends != 0, st ); if( rc ) return rc;
  const size_t n1 = (size_t)total + 1;
  const size_t tmp_bytes = build_scan_temp_bytes( n1 );
  RS_TRY( W.flags.ensure( n1 * 4 ), "gather_plane_inliers: buffers" ); RS_TRY( W.rank.ensure( n1 * 4 ), "gather_plane_inliers: buffers" );
  RS_TRY( W.tmp.ensure( tmp_bytes + 256 ), "gather_plane_inliers: buffers" );
  {
    ProfSpan span( "plane_gather_flags" );
    hipLaunchKernelGGL( k_plane_gather_flags, dim3( blocks_for( (long long)n1, PLANE_BLOCK ) ), dim3( PLANE_BLOCK ), 0, st, S.qpos, S.qnor, S.by_orig, S.n,
                        W.models.as<PlaneGatherModel>(), n_models, dot_threshold, dist_threshold, check_validity, check_extends, W.flags.as<uint32_t>() );
    if( build_exclusive_scan( W.tmp.p, tmp_bytes, W.flags.as<uint32_t>(), W.rank.as<uint32_t>(), n1, st ) )
      return fail( RS_HIP_E_RUNTIME, "gather_plane_inliers: device scan failed" );
  }
  RS_TRY( hipGetLastError(), "gather_plane_inliers: flags launch" );
  std::vector<uint32_t> off( (size_t)n_models + 1 );
  for( int m = 0; m <= n_models; ++m )
    RS_TRY( hipMemcpyAsync( &off[(size_t)m], W.rank.as<uint32_t>() + (size_t)m * S.n, 4, hipMemcpyDeviceToHost, st ), "gather_plane_inliers: download" );
  RS_TRY( hipStreamSynchronize( st ), "gather_plane_inliers: flags" );
  const uint32_t count = off[(size_t)n_models];
  if( (int64_t)count > capacity ) return fail( RS_HIP_E_CAPACITY, "gather_plane_inliers: more inliers than the caller's capacity" );
  if( count > 0 )
  {
    RS_TRY( W.index.ensure( (size_t)count * 4 ), "gather_plane_inliers: buffers" );
    {
      ProfSpan span( "plane_scatter" );
      hipLaunchKernelGGL( k_plane_scatter, dim3( blocks_for( total, PLANE_BLOCK ) ), dim3( PLANE_BLOCK ), 0, st, W.flags.as<uint32_t>(), W.rank.as<uint32_t>(), S.n, total, W.index.as<int32_t>() );
    }
    RS_TRY( hipGetLastError(), "gather_plane_inliers: scatter launch" );
    RS_TRY( hipMemcpyAsync( index, W.index.p, (size_t)count * 4, hipMemcpyDeviceToHost, st ), "gather_plane_inliers: download" );
    RS_TRY( hipStreamSynchronize( st ), "gather_plane_inliers: scatter" );
  }
  for( int m = 0; m <= n_models; ++m ) offsets[m] = (int64_t)off[(size_t)m];
  return RS_HIP_OK;
}

int rs_hip_relabel_walls_and_floors( const rs_hip_cloud_t* cloud, const float* centers, const float* normals, const float* axes,
                                     const float* extends, const int8_t* valid, const float* normal_up_dot, int32_t n_models,
                                     int32_t floor_idx, int32_t wall_idx, int32_t unlabelled_idx, int32_t* class_ids, int32_t* instance_ids )
{
  if( !cloud || n_models < 0 || ( n_models > 0 && ( !centers || !normals || !axes || !extends || !valid || !normal_up_dot ) ) )
    return fail( RS_HIP_E_ARG, "relabel_walls_and_floors: null arrays or a negative count" );
  const CloudPoints S = api_cloud_points( cloud );
  if( !S.qnor ) return fail( RS_HIP_E_ARG, "relabel_walls_and_floors: the cloud needs normals" );
  if( S.n > 0 && ( !class_ids || !instance_ids ) ) return fail( RS_HIP_E_ARG, "relabel_walls_and_floors: the class and instance ids are required" );
  if( S.n <= 0 || n_models == 0 ) return RS_HIP_OK;
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  PlaneWorkspace& W = g_plane_ws;
  rc = plane_upload_models( centers, normals, axes, extends, valid, normal_up_dot, n_models, true, st ); if( rc ) return rc;
  const size_t bytes = (size_t)S.n * 4;
  RS_TRY( W.cls.ensure( bytes ), "relabel_walls_and_floors: buffers" ); RS_TRY( W.inst.ensure( bytes ), "relabel_walls_and_floors: buffers" );
  RS_TRY( hipMemcpyAsync( W.cls.p, class_ids, bytes, hipMemcpyHostToDevice, st ), "relabel_walls_and_floors: upload" );
  RS_TRY( hipMemcpyAsync( W.inst.p, instance_ids, bytes, hipMemcpyHostToDevice, st ), "relabel_walls_and_floors: upload" );
  {
    ProfSpan span( "plane_relabel" );
    hipLaunchKernelGGL( k_plane_relabel, dim3( blocks_for( S.n, PLANE_BLOCK ) ), dim3( PLANE_BLOCK ), 0, st, S.qpos, S.qnor, S.by_orig, S.n,
                        W.models.as<PlaneGatherModel>(), n_models, floor_idx, wall_idx, unlabelled_idx, W.cls.as<int32_t>(), W.inst.as<int32_t>() );
  }
  RS_TRY( hipGetLastError(), "relabel_walls_and_floors: launch" );
  // into scratch first: a failed download leaves the caller's arrays as they were
  std::vector<int32_t> cls( (size_t)S.n ), inst( (size_t)S.n );
  RS_TRY( hipMemcpyAsync( cls.data(), W.cls.p, bytes, hipMemcpyDeviceToHost, st ), "relabel_walls_and_floors: download" );
  RS_TRY( hipMemcpyAsync( inst.data(), W.inst.p, bytes, hipMemcpyDeviceToHost, st ), "relabel_walls_and_floors: download" );
  RS_TRY( hipStreamSynchronize( st ), "relabel_walls_and_floors: kernel" );
  std::memcpy( class_ids, cls.data(), bytes ); std::memcpy( instance_ids, inst.data(), bytes );
  return RS_HIP_OK;
}

} // extern "C"
