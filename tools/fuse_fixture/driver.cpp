// FIXTURE GENERATION ONLY — not product code, not run by any test.
//
// A flat C interface over the reference's own functions, for tools/fuse_fixture/gen.py.  This file switches on the reference's
// single-header implementations, includes its headers by path and only CALLS its functions, in the order
// rsdu_augment_database does for one placement (apps/segment_transfer/database_update.cpp:35-85):
//   fx_augment   rs_pointcloud_copy_by_ids on the scan's level 1, msh_mat4_inverse, icp_align (unless static),
//                rs_pointcloud_transform, the two loops that set the instance ids to 0 and 1, rs_pointcloud_merge, and the
//                overwrite of the instance ids with the placement's uidx.  The clouds are assembled with rs_pointcloud_init /
//                rs_pointcloud__allocate_level.
//   fx_transform rs_pointcloud_transform of a level 0 assembled from positions and normals, for the hostile transforms.
//   fx_merge_ids rs_pointcloud_merge of two clouds whose instance ids carry the element's index in "A then B": the ids of the
//                result are the shuffle's permutation.
#define MSH_STD_IMPLEMENTATION
#define MSH_PLY_IMPLEMENTATION
#define MSH_ARGPARSE_IMPLEMENTATION
#define MSH_VEC_MATH_IMPLEMENTATION
#define MSH_GEOMETRY_IMPLEMENTATION
#define MSH_HASH_GRID_IMPLEMENTATION
#define RS_POINTCLOUD_IMPLEMENTATION
#define HASHTABLE_IMPLEMENTATION
#define ICP_IMPLEMENTATION

#include <cassert>
#include <cmath>
#include <cstring>
#include <cstdint>
#include <cstdarg>
#include <cstddef>
#include <cstdbool>
#include <cstdio>
#include <cstdlib>
#include <cfloat>
#include <cctype>

#include "msh/msh_std.h"
#include "msh/msh_argparse.h"
#include "msh/msh_vec_math.h"
#include "msh/msh_geometry.h"
#include "msh/msh_ply.h"
#include "msh/msh_hash_grid.h"
#include "mg/hashtable.h"
#include "icp.h"
#include "rs_pointcloud.h"

// the seven arrays of one level
struct fx_arrays { float* pos; float* nor; float* col; float* radii; float* qual; int32_t* cls; int32_t* inst; };

static rs_pointcloud_t* fx_cloud( const fx_arrays* a, int64_t n, int32_t level )
{
  rs_pointcloud_t* pc = rs_pointcloud_init( 1 );
  rs_pointcloud__allocate_level( pc, level, (int32_t)n );
  memcpy( pc->positions[level], a->pos, n * 12 );
  memcpy( pc->normals[level], a->nor, n * 12 );
  memcpy( pc->colors[level], a->col, n * 12 );
  memcpy( pc->radii[level], a->radii, n * 4 );
  memcpy( pc->qualities[level], a->qual, n * 4 );
  memcpy( pc->class_ids[level], a->cls, n * 4 );
  memcpy( pc->instance_ids[level], a->inst, n * 4 );
  return pc;
}
static void fx_read( const rs_pointcloud_t* pc, int32_t level, fx_arrays* a )
{
  const size_t n = pc->n_pts[level];
  memcpy( a->pos, pc->positions[level], n * 12 );
  memcpy( a->nor, pc->normals[level], n * 12 );
  memcpy( a->col, pc->colors[level], n * 12 );
  memcpy( a->radii, pc->radii[level], n * 4 );
  memcpy( a->qual, pc->qualities[level], n * 4 );
  memcpy( a->cls, pc->class_ids[level], n * 4 );
  memcpy( a->inst, pc->instance_ids[level], n * 4 );
}

extern "C" {

// One placement.  extracted: room for n_scan points, written as rs_pointcloud_copy_by_ids returned them (before the transform).
// Returns the merged cloud (fx_get copies its level 0 out, fx_free releases it), or NULL when nothing was extracted.
// seconds[0]: copy_by_ids .. transform without the ICP, [1]: the ICP, [2]: rs_pointcloud_merge (its level build included).
void* fx_augment( const fx_arrays* scan, int64_t n_scan, const fx_arrays* model, int64_t n_model, const float* pose, int32_t uidx,
                  int32_t is_static, fx_arrays* extracted, int64_t* n_extracted, float* xform_out, float* icp_err,
                  int64_t* n_merged, int64_t* level_counts, double* seconds )
{
  rs_pointcloud_t* input_scan = fx_cloud( scan, n_scan, 1 );
  rs_pointcloud_t* cur_shape = fx_cloud( model, n_model, 0 );
  msh_mat4_t placement_pose; memcpy( placement_pose.data, pose, 64 );
  *n_extracted = 0; *n_merged = 0; *icp_err = 0.0f;
  uint64_t t0 = msh_time_now();
  rs_pointcloud_t* extracted_shape = rs_pointcloud_copy_by_ids( input_scan, 1, RS_PT_INSTANCE_ID, &uidx, 1, 0 );
  rs_pointcloud_t* merged_shape = NULL;
  if( extracted_shape )
  {
    *n_extracted = (int64_t)extracted_shape->n_pts[0];
    fx_read( extracted_shape, 0, extracted );
    msh_mat4_t xform = msh_mat4_inverse( placement_pose );
    seconds[0] = msh_time_diff_ms( msh_time_now(), t0 ) * 1e-3;
    t0 = msh_time_now();
    if( !is_static )
    {
      *icp_err = icp_align( extracted_shape->positions[0], extracted_shape->normals[0], extracted_shape->n_pts[0],
                            cur_shape->positions[0], cur_shape->normals[0], cur_shape->n_pts[0],
                            &xform, msh_mat4_identity(), 0.05, msh_deg2rad(10.0f), 0 );
    }
    seconds[1] = msh_time_diff_ms( msh_time_now(), t0 ) * 1e-3;
    t0 = msh_time_now();
    rs_pointcloud_transform( extracted_shape, xform, 0 );
    for( size_t i = 0; i < extracted_shape->n_pts[0]; ++i ) extracted_shape->instance_ids[0][i] = 0;
    for( size_t i = 0; i < cur_shape->n_pts[0]; ++i ) cur_shape->instance_ids[0][i] = 1;
    seconds[0] += msh_time_diff_ms( msh_time_now(), t0 ) * 1e-3;
    t0 = msh_time_now();
    merged_shape = rs_pointcloud_merge( extracted_shape, cur_shape, 0 );
    seconds[2] = msh_time_diff_ms( msh_time_now(), t0 ) * 1e-3;
    for( size_t lvl = 0; lvl < RSPC_N_LEVELS; ++lvl )
    {
      for( size_t i = 0; i < merged_shape->n_pts[lvl]; ++i ) merged_shape->instance_ids[lvl][i] = uidx;
      level_counts[lvl] = (int64_t)merged_shape->n_pts[lvl];
    }
    memcpy( xform_out, xform.data, 64 );
    *n_merged = (int64_t)merged_shape->n_pts[0];
    rs_pointcloud_free( extracted_shape, 1 );
  }
  rs_pointcloud_free( cur_shape, 1 );
  rs_pointcloud_free( input_scan, 1 );
  return merged_shape;
}

// rs_pointcloud_transform alone (no level build): pos and nor (n points each) are rewritten in place
void fx_transform( float* pos, float* nor, int64_t n, const float* xform )
{
  rs_pointcloud_t* pc = rs_pointcloud_init( 1 );
  rs_pointcloud__allocate_level( pc, 0, (int32_t)n );
  memcpy( pc->positions[0], pos, n * 12 );
  memcpy( pc->normals[0], nor, n * 12 );
  msh_mat4_t m; memcpy( m.data, xform, 64 );
  rs_pointcloud_transform( pc, m, 0 );
  memcpy( pos, pc->positions[0], n * 12 );
  memcpy( nor, pc->normals[0], n * 12 );
  rs_pointcloud_free( pc, 1 );
}

void fx_get( void* h, fx_arrays* out ) { fx_read( (rs_pointcloud_t*)h, 0, out ); }
void fx_free( void* h ) { rs_pointcloud_free( (rs_pointcloud_t*)h, 1 ); }

// perm (n_a + n_b entries): the instance ids of rs_pointcloud_merge( A, B ) where A's ids are 0 .. n_a-1 and B's n_a .. n_a+n_b-1
void fx_merge_ids( const fx_arrays* a, int64_t n_a, const fx_arrays* b, int64_t n_b, int32_t* perm )
{
  rs_pointcloud_t* pa = fx_cloud( a, n_a, 0 );
  rs_pointcloud_t* pb = fx_cloud( b, n_b, 0 );
  for( int64_t i = 0; i < n_a; ++i ) pa->instance_ids[0][i] = (int32_t)i;
  for( int64_t i = 0; i < n_b; ++i ) pb->instance_ids[0][i] = (int32_t)( n_a + i );
  rs_pointcloud_t* m = rs_pointcloud_merge( pa, pb, 0 );
  assert( m && (int64_t)m->n_pts[0] == n_a + n_b );
  memcpy( perm, m->instance_ids[0], ( n_a + n_b ) * 4 );
  rs_pointcloud_free( m, 1 );
  rs_pointcloud_free( pa, 1 );
  rs_pointcloud_free( pb, 1 );
}

} // extern "C"
