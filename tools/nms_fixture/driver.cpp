// FIXTURE GENERATION ONLY — not product code, not run by any test.
//
// A flat C interface over the reference's own isect_get_overlap_factor (lib/rs/intersect.h) and
// mgs_non_maxima_suppresion (apps/pose_proposal/pose_proposal.cpp), for tools/nms_fixture/gen.py.  This file switches on
// the reference's single-header implementations, includes its headers by path and only CALLS its functions; the second
// translation unit of the library is the reference's pose_proposal.cpp, compiled where it lies (gen.py).  Asserts stay on.
#define MSH_STD_IMPLEMENTATION
#define MSH_PLY_IMPLEMENTATION
#define MSH_ARGPARSE_IMPLEMENTATION
#define MSH_VEC_MATH_IMPLEMENTATION
#define MSH_GEOMETRY_IMPLEMENTATION
#define MSH_HASH_GRID_IMPLEMENTATION
#define RS_POINTCLOUD_IMPLEMENTATION
#define RS_DISTANCE_FUNCTION_IMPLEMENTATION
#define RS_DATABASE_IMPLEMENTATION
#define FILEPATH_HELPERS_IMPLEMENTATION
#define HASHTABLE_IMPLEMENTATION

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
#include "filepath_helpers.h"
#include "rs_pointcloud.h"
#include "rs_database.h"
#include "rs_distance_function.h"
#include "intersect.h"
#include "pose_proposal.h"

// the msh_array instantiations pose_proposal.cpp uses (apps/pose_proposal/main.cpp instantiates them for the app)
template int* msh_array__grow<int>(int* arr, unsigned long long new_len, unsigned long long elem_size );
template rs_object_placement* msh_array__grow<rs_object_placement>(rs_object_placement* arr, unsigned long long new_len, unsigned long long elem_size );
template pose_proposal* msh_array__grow<pose_proposal>(pose_proposal* arr, unsigned long long new_len, unsigned long long elem_size );
template pose_proposal** msh_array__grow<pose_proposal*>(pose_proposal** arr, unsigned long long new_len, unsigned long long elem_size );
template mark* msh_array__grow<mark>(mark* arr, unsigned long long new_len, unsigned long long elem_size );

static msh_mat4_t mat_of( const float* m ) { msh_mat4_t o; memcpy( o.data, m, 64 ); return o; }

extern "C" {

// A shape from level-0 points: levels 1..3 by the reference's own level builder (rs_pointcloud.h:984-1106).
void* fx_shape_create( const float* pos, const float* nor, int32_t n )
{
  rs_pointcloud_t* pc = rs_pointcloud_init( 1 );
  rs_pointcloud__allocate_level( pc, 0, n );
  memcpy( pc->positions[0], pos, (size_t)n * sizeof(msh_vec3_t) );
  memcpy( pc->normals[0], nor, (size_t)n * sizeof(msh_vec3_t) );
  memset( pc->colors[0], 0, (size_t)n * sizeof(msh_vec3_t) );
  memset( pc->radii[0], 0, (size_t)n * 4 ); memset( pc->qualities[0], 0, (size_t)n * 4 );
  memset( pc->class_ids[0], 0, (size_t)n * 4 ); memset( pc->instance_ids[0], 0, (size_t)n * 4 );
  for( int32_t lvl = 1; lvl <= 3; ++lvl ) rs_pointcloud__compute_level( pc, lvl );
  return pc;
}

// A shape whose levels 1 and 3 are GIVEN (scaled / hand-made clouds); level 0 = level 1 (the centroid's level).
void* fx_shape_from_levels( const float* l1, int32_t n1, const float* l3, int32_t n3 )
{
  rs_pointcloud_t* pc = rs_pointcloud_init( 1 );
  rs_pointcloud__allocate_level( pc, 0, n1 ); memcpy( pc->positions[0], l1, (size_t)n1 * sizeof(msh_vec3_t) );
  rs_pointcloud__allocate_level( pc, 1, n1 ); memcpy( pc->positions[1], l1, (size_t)n1 * sizeof(msh_vec3_t) );
  rs_pointcloud__allocate_level( pc, 3, n3 ); memcpy( pc->positions[3], l3, (size_t)n3 * sizeof(msh_vec3_t) );
  return pc;
}

int32_t fx_level( void* shape, int32_t lvl, float* out )
{
  rs_pointcloud_t* pc = (rs_pointcloud_t*)shape;
  if( out ) memcpy( out, pc->positions[lvl], pc->n_pts[lvl] * sizeof(msh_vec3_t) );
  return (int32_t)pc->n_pts[lvl];
}

void fx_centroid( void* shape, float out[3] )
{
  const msh_vec3_t c = rs_pointcloud_centroid( (rs_pointcloud_t*)shape, 0 );
  out[0] = c.x; out[1] = c.y; out[2] = c.z;
}

// isect_get_overlap_factor itself; counts = {count_a, count_b, both} from the same public helpers it calls, in its order
// (0, 0, 0 where the boxes do not intersect)
float fx_overlap( void* shape_a, const float* pose_a, void* shape_b, const float* pose_b, float voxel, int32_t inside, int32_t by_smaller,
                  int32_t counts[3] )
{
  rs_pointcloud_t* a = (rs_pointcloud_t*)shape_a; rs_pointcloud_t* b = (rs_pointcloud_t*)shape_b;
  const msh_mat4_t pa = mat_of( pose_a ), pb = mat_of( pose_b );
  counts[0] = counts[1] = counts[2] = 0;
  msh_bbox_t ba = isect_get_transformed_aabbox( a, pa ), bb = isect_get_transformed_aabbox( b, pb );
  if( mshgeo_bbox_intersect( &ba, &bb ) )
  {
    msh_bbox_t bc = mshgeo_bbox_init();
    mshgeo_bbox_union( &bc, ba.min_p ); mshgeo_bbox_union( &bc, ba.max_p ); mshgeo_bbox_union( &bc, bb.min_p ); mshgeo_bbox_union( &bc, bb.max_p );
    isect_grid3d_t ga = {0}, gb = {0}, gc = {0};
    isect_grid3d_init( &ga, &bc, voxel ); isect_grid3d_init( &gb, &bc, voxel ); isect_grid3d_init( &gc, &bc, voxel );
    counts[0] = inside ? isect_compute_occupancy_grid( a, pa, &ga ) : isect_compute_boundary_grid( a, pa, &ga );
    counts[1] = inside ? isect_compute_occupancy_grid( b, pb, &gb ) : isect_compute_boundary_grid( b, pb, &gb );
    counts[2] = isect_compute_overlap_grid( &ga, &gb, &gc );
    isect_grid3d_term( &ga ); isect_grid3d_term( &gb ); isect_grid3d_term( &gc );
  }
  return isect_get_overlap_factor( a, pa, b, pb, voxel, inside, by_smaller );
}

// mgs_non_maxima_suppresion on one object's list; the kept proposals come back (poses, scores), their number is returned
int32_t fx_nms( void* shape, const float* poses, const float* scores, int32_t n, float dist_threshold, float* kept_poses, float* kept_scores )
{
  static rsdb_t* rsdb = NULL;
  if( !rsdb )
  {
    rsdb = rsdb_init();
    rsdb_add_class( rsdb, strdup( "object" ), 1 );
    rs_object_t o = rsdb_object_init();
    o.uidx = 0; o.class_idx = 0;
    rsdb_add_object( rsdb, &o );
  }
  rsdb->objects[0].shape = (rs_pointcloud_t*)shape;
  msh_array(pose_proposal_t) list = NULL;
  for( int32_t i = 0; i < n; ++i )
  {
    pose_proposal_t p; p.xform = mat_of( poses + 16 * (size_t)i ); p.score = scores[i];
    msh_array_push( list, p );
  }
  msh_array(msh_array(pose_proposal_t)) lists = NULL;
  msh_array_push( lists, list );
  mgs_non_maxima_suppresion( rsdb, &lists, 0, dist_threshold );
  const int32_t n_keep = (int32_t)msh_array_len( lists[0] );
  for( int32_t i = 0; i < n_keep; ++i ) { memcpy( kept_poses + 16 * (size_t)i, lists[0][i].xform.data, 64 ); kept_scores[i] = lists[0][i].score; }
  msh_array_free( lists[0] ); msh_array_free( lists );
  return n_keep;
}

} // extern "C"
