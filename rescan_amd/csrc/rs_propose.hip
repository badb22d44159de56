// The multi-resolution pose search — mgs_propose_poses (apps/pose_proposal/pose_proposal.cpp:325-369) with
// mgs__initial_pose_proposals (:170-254) and mgs__pose_verification (:256-303): rs_hip_pose_grid_plan, rs_hip_propose_poses,
// rs_hip_cell_best, rs_hip_verify_marks, rs_hip_propose_release.
//
// The reference scores one pose after the other: every (cell x, cell z, yaw) of a grid over the scan's box at the coarsest level, the
// best rotation of each cell proposed where it beats the level's threshold, the proposals scored again at the finer levels.  Here the
// poses of a level are made, scored, judged and compacted on the device; the host plans the three tables (rs_propose.h), sizes the
// launches and, once per level, reads the objects' counts.  No pose and no score crosses the bus before the final lists.
//
// How a call runs, every object queued before the level's one wait:
//   level 0    k_pose_grid        one lane per (cell, yaw): yaw[k] with col[3] = ( origin.x + ox[i], height, origin.z + oz[j], 1 )
//                                 (:221-222), cells x-outer, z-inner (:213-215).  (An object level without points: k_fill, NaN.)
//              the score launches of rs_hip_alignment_scores on those device poses (rs_host.h: api_score_poses_device)
//              k_cell_best        one lane per cell: best from 0 by strict > in yaw order, flag = best > thresholds[0] (:217-238)
//              scan + k_keep      the flagged cells' pose and score into the object's proposal list, cell order kept (:240-241)
//   then, for the next level      k_list_flags + scan + k_list_gather: the proposals with score > 0.0f (:285), their poses compacted
//   level l    the score launches on the compacted poses; k_verify_marks: score > thresholds[l] ? score : -1.0f (:291-292)
//   the end    k_list_flags + scan + k_list_gather with fabsf( score ) > 0.000001f (:353): the final lists, the -1 entries among them
// The lists' lengths come from device counts (a launch is sized by a bound the host knows: the cells, later the proposals).
#include "rs_host.h"
#include "rs_propose.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

namespace rs {

constexpr int PROPOSE_BLOCK = 256;
constexpr int PROPOSE_MAX_LEVELS = 4;

// poses: n_x * n_z * n_yaw matrices of 16 floats (four 16-byte stores per lane)
__global__ __launch_bounds__( PROPOSE_BLOCK ) void k_pose_grid( const float* __restrict__ ox, const float* __restrict__ oz, const float4* __restrict__ yaw,
                                                                 int n_z, int n_yaw, int n_poses, float origin_x, float height, float origin_z, float4* poses )
{
  const int p = blockIdx.x * PROPOSE_BLOCK + threadIdx.x;
  if( p >= n_poses ) return;
  const int cell = p / n_yaw, k = p - cell * n_yaw;
  const int i = cell / n_z, j = cell - i * n_z;
  float4* o = poses + 4 * (size_t)p;
  o[0] = yaw[4 * k]; o[1] = yaw[4 * k + 1]; o[2] = yaw[4 * k + 2];
  o[3] = make_float4( origin_x + ox[i], height, origin_z + oz[j], 1.0f );                   // :222
}

__global__ __launch_bounds__( PROPOSE_BLOCK ) void k_fill( float* a, int n, float v )
{
  const int i = blockIdx.x * PROPOSE_BLOCK + threadIdx.x;
  if( i < n ) a[i] = v;
}

// lane c: cell c.  best_yaw = -1 where no score is > 0 (a NaN fails the compare).  flags has n_cells + 1 entries, the last one 0.
__global__ __launch_bounds__( PROPOSE_BLOCK ) void k_cell_best( const float* __restrict__ scores, int n_cells, int n_yaw, float threshold,
                                                                 int32_t* best_yaw, float* best_score, uint32_t* flags )
{
  const int c = blockIdx.x * PROPOSE_BLOCK + threadIdx.x;
  if( c > n_cells ) return;
  if( c == n_cells ) { flags[c] = 0u; return; }
  float best = 0.0f; int32_t arg = -1;                                                       // :217-218
  const float* s = scores + (size_t)c * n_yaw;
  for( int k = 0; k < n_yaw; ++k )
  {
    const float v = s[k];
    if( v > best ) { best = v; arg = k; }                                                    // :230-233
  }
  best_yaw[c] = arg; best_score[c] = best;
  flags[c] = best > threshold ? 1u : 0u;                                                     // :238
}

// The flagged cells, in cell order: pose (grid_poses may be null: none) and score to slot rank[c] of the list; slot (may be null)
// = that slot, -1 for a cell that proposes nothing; *count = the list's length.  A proposal without a winning rotation (possible
// only under a negative threshold) carries the reference's zero matrix (:218).
__global__ __launch_bounds__( PROPOSE_BLOCK ) void k_keep( const float4* __restrict__ grid_poses, const int32_t* __restrict__ best_yaw, const float* __restrict__ best_score,
                                                            const uint32_t* __restrict__ flags, const uint32_t* __restrict__ rank, int n_cells, int n_yaw,
                                                            float4* list_pose, float* list_score, int32_t* slot, int32_t* count )
{
  const int c = blockIdx.x * PROPOSE_BLOCK + threadIdx.x;
  if( c > n_cells ) return;
  if( c == n_cells ) { if( count ) *count = (int32_t)rank[c]; return; }
  const bool keep = flags[c] != 0u;
  if( slot ) slot[c] = keep ? (int32_t)rank[c] : -1;
  if( !keep ) return;
  const size_t r = rank[c];
  if( list_score ) list_score[r] = best_score[c];
  if( grid_poses )
  {
    const int k = best_yaw[c];
    const float4* src = grid_poses + 4 * ( (size_t)c * n_yaw + ( k < 0 ? 0 : k ) );
    const float4 m0 = src[0], m1 = src[1], m2 = src[2], m3 = src[3];
    list_pose[4 * r] = k < 0 ? make_float4( 0.0f, 0.0f, 0.0f, 0.0f ) : m0; list_pose[4 * r + 1] = k < 0 ? make_float4( 0.0f, 0.0f, 0.0f, 0.0f ) : m1;
    list_pose[4 * r + 2] = k < 0 ? make_float4( 0.0f, 0.0f, 0.0f, 0.0f ) : m2; list_pose[4 * r + 3] = k < 0 ? make_float4( 0.0f, 0.0f, 0.0f, 0.0f ) : m3;
  }
}

// flags[i] for the list's entries i < *m (i <= bound: the launch's size): MODE 0 score > 0.0f (:285), MODE 1 fabsf( score ) > 0.000001f (:353)
template <int MODE>
__global__ __launch_bounds__( PROPOSE_BLOCK ) void k_list_flags( const float* __restrict__ score, const int32_t* __restrict__ m, int bound, uint32_t* flags )
{
  const int i = blockIdx.x * PROPOSE_BLOCK + threadIdx.x;
  if( i > bound ) return;
  bool f = false;
  if( i < *m ) { const float s = score[i]; f = MODE == 0 ? s > 0.0f : fabsf( s ) > 0.000001f; }
  flags[i] = f ? 1u : 0u;
}
// the flagged entries in order: pose, and where asked for score and index; *count = how many
__global__ __launch_bounds__( PROPOSE_BLOCK ) void k_list_gather( const float4* __restrict__ pose, const float* __restrict__ score, const uint32_t* __restrict__ flags,
                                                                   const uint32_t* __restrict__ rank, int bound, float4* out_pose, float* out_score, int32_t* out_idx, int32_t* count )
{
  const int i = blockIdx.x * PROPOSE_BLOCK + threadIdx.x;
  if( i > bound ) return;
  if( i == bound ) *count = (int32_t)rank[i];
  if( !flags[i] ) return;
  const size_t r = rank[i];
  for( int q = 0; q < 4; ++q ) out_pose[4 * r + q] = pose[4 * (size_t)i + q];
  if( out_score ) out_score[r] = score[i];
  if( out_idx ) out_idx[r] = i;
}

// lane k: the k-th new score, of entry idx[k] (idx null: entry k).  An entry that was not > 0 keeps what it has (:294-297).
__global__ __launch_bounds__( PROPOSE_BLOCK ) void k_verify_marks( const float* old_score, const float* __restrict__ new_score, const int32_t* __restrict__ idx,
                                                                    const int32_t* __restrict__ n_dev, int n, float threshold, float* out )
{
  const int k = blockIdx.x * PROPOSE_BLOCK + threadIdx.x;
  if( k >= n || ( n_dev && k >= *n_dev ) ) return;
  const int i = idx ? idx[k] : k;
  const float o = old_score[i], s = new_score[k];
  out[i] = o > 0.0f ? ( s > threshold ? s : -1.0f ) : o;                                     // :285, :291-292
}

} // namespace rs

using namespace rs;

namespace {

struct ProposeWorkspace
{
  Buf tab, grid_pose, grid_score, best_yaw, best_score, flags, rank, tmp, slot;
  Buf list_pose, list_score, act_pose, act_idx, act_score, out_pose, out_score, counts;
  Buf h_counts{ nullptr, 0, true }, h_out{ nullptr, 0, true };
  Buf* all[19] = { &tab, &grid_pose, &grid_score, &best_yaw, &best_score, &flags, &rank, &tmp, &slot, &list_pose, &list_score,
                   &act_pose, &act_idx, &act_score, &out_pose, &out_score, &counts, &h_counts, &h_out };
};
thread_local ProposeWorkspace g_propose_ws;

// exclusive scan of W.flags[0 .. n] into W.rank
int propose_scan( size_t n1, hipStream_t st )
{
  ProposeWorkspace& W = g_propose_ws;
  const size_t tmp_bytes = build_scan_temp_bytes( n1 );
  RS_TRY_DRAIN( st, W.tmp.ensure( tmp_bytes + 256 ), "propose: buffers" );
  if( build_exclusive_scan( W.tmp.p, tmp_bytes, W.flags.as<uint32_t>(), W.rank.as<uint32_t>(), n1, st ) )
  { (void)hipStreamSynchronize( st ); return fail( RS_HIP_E_RUNTIME, "propose: device scan failed" ); }
  return RS_HIP_OK;
}

// Where the points of an object level can fall under every pose of the grid: its box under each yaw at the four extreme cells (a
// sum rounds monotonically, so the cells between lie between).  false: no box (a cloud without a grid of its own, or no points).
bool propose_query_box( const rs_hip_cloud_t* object, const std::vector<float>& ox, const std::vector<float>& oz, const std::vector<float>& yaw,
                        const float origin[3], float height, float box[6] )
{
  const GridView& og = *api_cloud_view( object );
  if( !( og.inv_cell > 0.0f ) ) return false;
  const float omin[3] = { og.minx, og.miny, og.minz }, omax[3] = { og.minx + og.w * og.cell, og.miny + og.h * og.cell, og.minz + og.d * og.cell };
  float qlo[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, qhi[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
  bool finite = true;
  for( size_t k = 0; k < yaw.size() / 16; ++k )
    for( int e = 0; e < 4; ++e )
    {
      const float* M = &yaw[16 * k];
      const float t[3] = { origin[0] + ( ( e & 1 ) ? ox.back() : ox.front() ), height, origin[2] + ( ( e & 2 ) ? oz.back() : oz.front() ) };
      for( int c = 0; c < 8; ++c )
      {
        const float x = ( c & 1 ) ? omax[0] : omin[0], y = ( c & 2 ) ? omax[1] : omin[1], z = ( c & 4 ) ? omax[2] : omin[2];
        for( int a = 0; a < 3; ++a )
        {
          const float v = M[a] * x + M[4 + a] * y + M[8 + a] * z + t[a];
          if( !std::isfinite( v ) ) finite = false;
          qlo[a] = std::min( qlo[a], v ); qhi[a] = std::max( qhi[a], v );
        }
      }
    }
  if( !finite ) return false;
  for( int a = 0; a < 3; ++a )
  {
    const float pad = 1e-3f + 1e-5f * std::max( std::fabs( qlo[a] ), std::fabs( qhi[a] ) );      // (rounding of the corner transforms; the box only groups)
    box[a] = qlo[a] - pad; box[3 + a] = qhi[a] + pad;
  }
  return true;
}

} // namespace

extern "C" {

int rs_hip_pose_grid_plan( const float bbox_min[3], const float bbox_max[3], float spacing, float angle_delta,
                           int32_t* n_x, int32_t* n_z, int32_t* n_yaw, float* ox, int32_t cap_x, float* oz, int32_t cap_z, float* yaw, int32_t cap_yaw )
{
  char err[256] = "";
  const int rc = propose::grid_plan( bbox_min, bbox_max, spacing, angle_delta, n_x, n_z, n_yaw, ox, cap_x, oz, cap_z, yaw, cap_yaw, err, sizeof(err) );
  if( rc ) api_set_err( err );
  return rc;
}

int rs_hip_cell_best( const float* scores, int32_t n_cells, int32_t n_yaw, float threshold, int32_t* best_yaw, float* best_score, int32_t* keep )
{
  if( n_cells < 0 || n_yaw < 0 || ( n_cells > 0 && ( !best_yaw || !best_score || !keep || ( n_yaw > 0 && !scores ) ) ) )
    return fail( RS_HIP_E_ARG, "cell_best: null arrays or a negative count" );
  if( (long long)n_cells * n_yaw > ( 1ll << 28 ) ) return fail( RS_HIP_E_CAPACITY, "cell_best: more than 2^28 scores" );
  if( n_cells == 0 ) return RS_HIP_OK;
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  ProposeWorkspace& W = g_propose_ws;
  const size_t nc = (size_t)n_cells, ns = std::max<size_t>( 1, nc * n_yaw );
  RS_TRY( W.grid_score.ensure( ns * 4 ), "cell_best: buffers" ); RS_TRY( W.best_yaw.ensure( nc * 4 ), "cell_best: buffers" );
  RS_TRY( W.best_score.ensure( nc * 4 ), "cell_best: buffers" ); RS_TRY( W.flags.ensure( ( nc + 1 ) * 4 ), "cell_best: buffers" );
  RS_TRY( W.rank.ensure( ( nc + 1 ) * 4 ), "cell_best: buffers" ); RS_TRY( W.slot.ensure( nc * 4 ), "cell_best: buffers" );
  if( n_yaw > 0 ) RS_TRY( hipMemcpyAsync( W.grid_score.p, scores, nc * n_yaw * 4, hipMemcpyHostToDevice, st ), "cell_best: upload" );
  {
    ProfSpan span( "pose_search" );
    hipLaunchKernelGGL( k_cell_best, dim3( blocks_for( (long long)nc + 1, PROPOSE_BLOCK ) ), dim3( PROPOSE_BLOCK ), 0, st, W.grid_score.as<float>(), n_cells, n_yaw, threshold,
                        W.best_yaw.as<int32_t>(), W.best_score.as<float>(), W.flags.as<uint32_t>() );
    if( ( rc = propose_scan( nc + 1, st ) ) ) return rc;
    hipLaunchKernelGGL( k_keep, dim3( blocks_for( (long long)nc + 1, PROPOSE_BLOCK ) ), dim3( PROPOSE_BLOCK ), 0, st, (const float4*)nullptr, W.best_yaw.as<int32_t>(), W.best_score.as<float>(),
                        W.flags.as<uint32_t>(), W.rank.as<uint32_t>(), n_cells, n_yaw, (float4*)nullptr, (float*)nullptr, W.slot.as<int32_t>(), (int32_t*)nullptr );
  }
  RS_TRY_DRAIN( st, hipGetLastError(), "cell_best: launch" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( best_yaw, W.best_yaw.p, nc * 4, hipMemcpyDeviceToHost, st ), "cell_best: download" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( best_score, W.best_score.p, nc * 4, hipMemcpyDeviceToHost, st ), "cell_best: download" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( keep, W.slot.p, nc * 4, hipMemcpyDeviceToHost, st ), "cell_best: download" );
  RS_TRY( hipStreamSynchronize( st ), "cell_best: kernels" );
  return RS_HIP_OK;
}

int rs_hip_verify_marks( const float* old_scores, const float* new_scores, int32_t n, float threshold, float* out )
{
  if( n < 0 || ( n > 0 && ( !old_scores || !new_scores || !out ) ) ) return fail( RS_HIP_E_ARG, "verify_marks: null arrays or a negative count" );
  if( n == 0 ) return RS_HIP_OK;
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  ProposeWorkspace& W = g_propose_ws;
  const size_t nn = (size_t)n;
  RS_TRY( W.list_score.ensure( nn * 4 ), "verify_marks: buffers" ); RS_TRY( W.act_score.ensure( nn * 4 ), "verify_marks: buffers" );
  RS_TRY( hipMemcpyAsync( W.list_score.p, old_scores, nn * 4, hipMemcpyHostToDevice, st ), "verify_marks: upload" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( W.act_score.p, new_scores, nn * 4, hipMemcpyHostToDevice, st ), "verify_marks: upload" );
  {
    ProfSpan span( "pose_search" );
    hipLaunchKernelGGL( k_verify_marks, dim3( blocks_for( n, PROPOSE_BLOCK ) ), dim3( PROPOSE_BLOCK ), 0, st, W.list_score.as<float>(), W.act_score.as<float>(),
                        (const int32_t*)nullptr, (const int32_t*)nullptr, n, threshold, W.list_score.as<float>() );
  }
  RS_TRY_DRAIN( st, hipGetLastError(), "verify_marks: launch" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( out, W.list_score.p, nn * 4, hipMemcpyDeviceToHost, st ), "verify_marks: download" );
  RS_TRY( hipStreamSynchronize( st ), "verify_marks: kernels" );
  return RS_HIP_OK;
}

int rs_hip_propose_poses( const rs_hip_cloud_t* const* objects, int32_t n_objects, int32_t n_levels, const rs_hip_cloud_t* scene,
                          const float bbox_min[3], const float bbox_max[3], float spacing, float angle_delta, float height,
                          const float* thresholds, float radius, int32_t max_n_neigh, int32_t capacity,
                          int32_t* counts, float* poses, float* scores, rs_hip_propose_trace_t* trace )
{
  if( n_objects < 0 || n_levels < 1 || n_levels > PROPOSE_MAX_LEVELS || !scene || !thresholds || capacity < 0 || max_n_neigh <= 0 ||
      ( n_objects > 0 && ( !objects || !counts || ( capacity > 0 && ( !poses || !scores ) ) ) ) )
    return fail( RS_HIP_E_ARG, "propose_poses: null arrays, a negative count or n_levels outside 1..4" );
  if( !api_cloud_has_normals( scene ) ) return fail( RS_HIP_E_ARG, "propose_poses: the scene has no normals" );
  for( int64_t k = 0; k < (int64_t)n_objects * n_levels; ++k )
    if( !objects[k] || !api_cloud_has_normals( objects[k] ) ) return fail( RS_HIP_E_ARG, "propose_poses: an object level is null or has no normals" );
  // the tables (rs_propose.h); refusals of the planner are this call's
  int32_t n_x = 0, n_z = 0, n_yaw = 0;
  char err[256] = "";
  int rc = propose::grid_plan( bbox_min, bbox_max, spacing, angle_delta, &n_x, &n_z, &n_yaw, nullptr, 0, nullptr, 0, nullptr, 0, err, sizeof(err) );
  if( rc ) return fail( rc, err );
  if( !std::isfinite( height ) ) return fail( RS_HIP_E_ARG, "propose_poses: height is not finite" );
  if( n_objects == 0 ) return RS_HIP_OK;
  const long long n_cells_ll = (long long)n_x * n_z, n_grid_ll = n_cells_ll * n_yaw;
  if( n_grid_ll > ( 1ll << 24 ) ) return fail( RS_HIP_E_CAPACITY, "propose_poses: more than 2^24 poses in the grid" );
  if( n_grid_ll == 0 )                            // (a box turned inside out: the reference's loops do not run)
  {
    for( int32_t o = 0; o < n_objects; ++o )
    {
      counts[o] = 0;
      if( trace && trace->n_proposed ) trace->n_proposed[o] = 0;
      for( int l = 0; l < n_levels; ++l )
      {
        if( trace && trace->n_scored ) trace->n_scored[(size_t)o * n_levels + l] = 0;
        if( trace && trace->n_kept ) trace->n_kept[(size_t)o * n_levels + l] = 0;
      }
    }
    return RS_HIP_OK;
  }
  const int n_cells = (int)n_cells_ll, n_grid = (int)n_grid_ll;
  std::vector<float> ox( (size_t)n_x ), oz( (size_t)n_z ), yaw( (size_t)n_yaw * 16 );
  rc = propose::grid_plan( bbox_min, bbox_max, spacing, angle_delta, &n_x, &n_z, &n_yaw, ox.data(), n_x, oz.data(), n_z, yaw.data(), n_yaw, err, sizeof(err) );
  if( rc ) return fail( rc, err );

  hipStream_t st = nullptr;
  rc = api_ready( &st ); if( rc ) return rc;
  ProposeWorkspace& W = g_propose_ws;
  const size_t nc = (size_t)n_cells, no = (size_t)n_objects;
  const size_t tab_floats = ( ( ox.size() + oz.size() + 3 ) / 4 ) * 4;       // the matrices after them stay 16-byte aligned
  RS_TRY( W.tab.ensure( ( tab_floats + yaw.size() ) * 4 ), "propose: buffers" );
  RS_TRY( W.grid_pose.ensure( (size_t)n_grid * 64 ), "propose: buffers" ); RS_TRY( W.grid_score.ensure( (size_t)n_grid * 4 ), "propose: buffers" );
  RS_TRY( W.best_yaw.ensure( nc * 4 ), "propose: buffers" ); RS_TRY( W.best_score.ensure( nc * 4 ), "propose: buffers" );
  RS_TRY( W.flags.ensure( ( nc + 1 ) * 4 ), "propose: buffers" ); RS_TRY( W.rank.ensure( ( nc + 1 ) * 4 ), "propose: buffers" );
  RS_TRY( W.list_pose.ensure( no * nc * 64 ), "propose: buffers" ); RS_TRY( W.list_score.ensure( no * nc * 4 ), "propose: buffers" );
  RS_TRY( W.act_pose.ensure( no * nc * 64 ), "propose: buffers" ); RS_TRY( W.act_idx.ensure( no * nc * 4 ), "propose: buffers" );
  RS_TRY( W.act_score.ensure( nc * 4 ), "propose: buffers" );
  RS_TRY( W.out_pose.ensure( no * nc * 64 ), "propose: buffers" ); RS_TRY( W.out_score.ensure( no * nc * 4 ), "propose: buffers" );
  // per object: [0] proposals, [1] of them > 0 (the next level's batch), [2] the final list's length
  RS_TRY( W.counts.ensure( no * 3 * 4 ), "propose: buffers" ); RS_TRY( W.h_counts.ensure( no * 3 * 4 ), "propose: buffers" );
  float* d_ox = W.tab.as<float>(); float* d_oz = d_ox + ox.size(); float* d_yaw = d_ox + tab_floats;
  // (pageable memory: the copies have left the host vectors when the calls return)
  RS_TRY( hipMemcpyAsync( d_ox, ox.data(), ox.size() * 4, hipMemcpyHostToDevice, st ), "propose: upload" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( d_oz, oz.data(), oz.size() * 4, hipMemcpyHostToDevice, st ), "propose: upload" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( d_yaw, yaw.data(), yaw.size() * 4, hipMemcpyHostToDevice, st ), "propose: upload" );
  RS_TRY_DRAIN( st, hipMemsetAsync( W.counts.p, 0, no * 3 * 4, st ), "propose: clear" );

  int32_t* d_counts = W.counts.as<int32_t>();
  int32_t* h_counts = W.h_counts.as<int32_t>();
  std::vector<int32_t> n_list( no, 0 ), n_active( no, 0 );
  auto cloud_of = [&]( size_t o, int l ) { return objects[o * (size_t)n_levels + (size_t)l]; };
  auto list_pose = [&]( size_t o ) { return W.list_pose.as<float4>() + 4 * o * nc; };
  auto list_score = [&]( size_t o ) { return W.list_score.as<float>() + o * nc; };
  auto act_pose = [&]( size_t o ) { return W.act_pose.as<float4>() + 4 * o * nc; };
  auto act_idx = [&]( size_t o ) { return W.act_idx.as<int32_t>() + o * nc; };
  // the proposals of object o that the next level scores (:285), bound = a length the list cannot exceed
  auto queue_next = [&]( size_t o, int bound ) -> int
  {
    ProfSpan span( "pose_search" );
    const dim3 grid( blocks_for( (long long)bound + 1, PROPOSE_BLOCK ) ), block( PROPOSE_BLOCK );
    hipLaunchKernelGGL( k_list_flags<0>, grid, block, 0, st, list_score( o ), d_counts + 3 * o, bound, W.flags.as<uint32_t>() );
    if( int r = propose_scan( (size_t)bound + 1, st ) ) return r;
    hipLaunchKernelGGL( k_list_gather, grid, block, 0, st, list_pose( o ), (const float*)nullptr, W.flags.as<uint32_t>(), W.rank.as<uint32_t>(), bound,
                        act_pose( o ), (float*)nullptr, act_idx( o ), d_counts + 3 * o + 1 );
    return RS_HIP_OK;
  };
  auto read_counts = [&]() -> int
  {
    RS_TRY_DRAIN( st, hipGetLastError(), "propose: launch" );
    RS_TRY_DRAIN( st, hipMemcpyAsync( h_counts, d_counts, no * 3 * 4, hipMemcpyDeviceToHost, st ), "propose: counts" );
    RS_TRY( hipStreamSynchronize( st ), "propose: kernels" );
    return RS_HIP_OK;
  };
  const bool want_kept = trace && trace->n_kept;

  // ---- level 0: the grid search (:188-250)
  for( size_t o = 0; o < no; ++o )
  {
    const rs_hip_cloud_t* obj = cloud_of( o, 0 );
    {
      ProfSpan span( "pose_search" );
      if( api_cloud_points( obj ).n == 0 )              // 0 / 0 for every pose (:156): nothing is > 0
        hipLaunchKernelGGL( k_fill, dim3( blocks_for( n_grid, PROPOSE_BLOCK ) ), dim3( PROPOSE_BLOCK ), 0, st, W.grid_score.as<float>(), n_grid, NAN );
      else
        hipLaunchKernelGGL( k_pose_grid, dim3( blocks_for( n_grid, PROPOSE_BLOCK ) ), dim3( PROPOSE_BLOCK ), 0, st, d_ox, d_oz, (const float4*)d_yaw, n_z, n_yaw, n_grid,
                            bbox_min[0], height, bbox_min[2], W.grid_pose.as<float4>() );
    }
    if( api_cloud_points( obj ).n > 0 )
    {
      float box[6];
      const bool have_box = propose_query_box( obj, ox, oz, yaw, bbox_min, height, box );
      rc = api_score_poses_device( obj, scene, W.grid_pose.as<float>(), have_box ? box : nullptr, n_grid, radius, max_n_neigh, W.grid_score.as<float>() );
      if( rc ) { (void)hipStreamSynchronize( st ); return rc; }
    }
    {
      ProfSpan span( "pose_search" );
      const dim3 grid( blocks_for( (long long)nc + 1, PROPOSE_BLOCK ) ), block( PROPOSE_BLOCK );
      hipLaunchKernelGGL( k_cell_best, grid, block, 0, st, W.grid_score.as<float>(), n_cells, n_yaw, thresholds[0], W.best_yaw.as<int32_t>(), W.best_score.as<float>(), W.flags.as<uint32_t>() );
      if( ( rc = propose_scan( nc + 1, st ) ) ) return rc;
      hipLaunchKernelGGL( k_keep, grid, block, 0, st, W.grid_pose.as<float4>(), W.best_yaw.as<int32_t>(), W.best_score.as<float>(), W.flags.as<uint32_t>(), W.rank.as<uint32_t>(),
                          n_cells, n_yaw, list_pose( o ), list_score( o ), (int32_t*)nullptr, d_counts + 3 * o );
    }
    if( ( n_levels > 1 || want_kept ) && ( rc = queue_next( o, n_cells ) ) ) return rc;
  }
  // (a single level needs no count on the host: its lists are bounded by the cells, and everything comes back with the final read)
  if( n_levels > 1 )
  {
    if( ( rc = read_counts() ) ) return rc;
    for( size_t o = 0; o < no; ++o ) { n_list[o] = h_counts[3 * o]; n_active[o] = h_counts[3 * o + 1]; }
  }
  else
    for( size_t o = 0; o < no; ++o ) n_list[o] = n_cells;
  for( size_t o = 0; o < no; ++o )
  {
    if( trace && trace->n_scored ) trace->n_scored[o * n_levels] = n_grid;
    if( trace && trace->n_kept && n_levels > 1 ) trace->n_kept[o * n_levels] = n_active[o];
  }

  // ---- levels 1 ..: the proposals that are still > 0, scored again (:266-302)
  for( int l = 1; l < n_levels; ++l )
  {
    const bool more = l + 1 < n_levels || want_kept;
    for( size_t o = 0; o < no; ++o )
    {
      const int na = n_active[o];
      if( na == 0 ) continue;
      const rs_hip_cloud_t* obj = cloud_of( o, l );
      if( api_cloud_points( obj ).n == 0 )
      {
        ProfSpan span( "pose_search" );
        hipLaunchKernelGGL( k_fill, dim3( blocks_for( na, PROPOSE_BLOCK ) ), dim3( PROPOSE_BLOCK ), 0, st, W.act_score.as<float>(), na, NAN );
      }
      else
      {
        float box[6];
        const bool have_box = propose_query_box( obj, ox, oz, yaw, bbox_min, height, box );
        rc = api_score_poses_device( obj, scene, (const float*)act_pose( o ), have_box ? box : nullptr, na, radius, max_n_neigh, W.act_score.as<float>() );
        if( rc ) { (void)hipStreamSynchronize( st ); return rc; }
      }
      {
        ProfSpan span( "pose_search" );
        hipLaunchKernelGGL( k_verify_marks, dim3( blocks_for( na, PROPOSE_BLOCK ) ), dim3( PROPOSE_BLOCK ), 0, st, list_score( o ), W.act_score.as<float>(), act_idx( o ),
                            d_counts + 3 * o + 1, na, thresholds[l], list_score( o ) );
      }
      if( more && ( rc = queue_next( o, n_list[o] ) ) ) return rc;
    }
    for( size_t o = 0; o < no; ++o ) if( trace && trace->n_scored ) trace->n_scored[o * n_levels + l] = n_active[o];
    if( more )
    {
      if( ( rc = read_counts() ) ) return rc;
      for( size_t o = 0; o < no; ++o ) n_active[o] = h_counts[3 * o + 1];
    }
    for( size_t o = 0; o < no; ++o ) if( trace && trace->n_kept ) trace->n_kept[o * n_levels + l] = n_active[o];
  }

  // ---- the final copy (:347-359) and the one read-back of poses and scores
  size_t total = 0;
  std::vector<size_t> first( no + 1, 0 );
  for( size_t o = 0; o < no; ++o ) { first[o] = total; total += (size_t)n_list[o]; }
  first[no] = total;
  RS_TRY( W.h_out.ensure( std::max<size_t>( 1, total ) * 68 ), "propose: buffers" );
  float* h_pose = W.h_out.as<float>(); float* h_score = h_pose + 16 * total;
  for( size_t o = 0; o < no; ++o )
  {
    const int bound = n_list[o];
    {
      ProfSpan span( "pose_search" );
      const dim3 grid( blocks_for( (long long)bound + 1, PROPOSE_BLOCK ) ), block( PROPOSE_BLOCK );
      hipLaunchKernelGGL( k_list_flags<1>, grid, block, 0, st, list_score( o ), d_counts + 3 * o, bound, W.flags.as<uint32_t>() );
      if( ( rc = propose_scan( (size_t)bound + 1, st ) ) ) return rc;
      hipLaunchKernelGGL( k_list_gather, grid, block, 0, st, list_pose( o ), list_score( o ), W.flags.as<uint32_t>(), W.rank.as<uint32_t>(), bound,
                          W.out_pose.as<float4>() + 4 * o * nc, W.out_score.as<float>() + o * nc, (int32_t*)nullptr, d_counts + 3 * o + 2 );
    }
    if( bound > 0 )
    {
      RS_TRY_DRAIN( st, hipMemcpyAsync( h_pose + 16 * first[o], W.out_pose.as<float>() + 16 * o * nc, (size_t)bound * 64, hipMemcpyDeviceToHost, st ), "propose: download" );
      RS_TRY_DRAIN( st, hipMemcpyAsync( h_score + first[o], W.out_score.as<float>() + o * nc, (size_t)bound * 4, hipMemcpyDeviceToHost, st ), "propose: download" );
    }
  }
  if( ( rc = read_counts() ) ) return rc;
  bool fits = true;
  for( size_t o = 0; o < no; ++o )
  {
    counts[o] = h_counts[3 * o + 2];
    if( counts[o] > capacity ) fits = false;
    if( trace && trace->n_proposed ) trace->n_proposed[o] = h_counts[3 * o];
    if( trace && trace->n_kept && n_levels == 1 ) trace->n_kept[o] = h_counts[3 * o + 1];
  }
  if( !fits ) return fail( RS_HIP_E_CAPACITY, "propose_poses: an object has more proposals than the capacity (counts hold what is needed)" );
  for( size_t o = 0; o < no; ++o )
  {
    std::memcpy( poses + 16 * o * (size_t)capacity, h_pose + 16 * first[o], (size_t)counts[o] * 64 );
    std::memcpy( scores + o * (size_t)capacity, h_score + first[o], (size_t)counts[o] * 4 );
  }
  return RS_HIP_OK;
}

int rs_hip_propose_release( void )
{
  hipError_t bad = hipSuccess;
  for( Buf* b : g_propose_ws.all ) { const hipError_t e = b->release(); if( e != hipSuccess ) bad = e; }
  return bad == hipSuccess ? RS_HIP_OK : fail( RS_HIP_E_RUNTIME, "propose_release", bad );
}

} // extern "C"
