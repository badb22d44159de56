// FIXTURE GENERATION ONLY — not product code, not run by any test.
//
// A flat C interface over the reference's own rsao_compute_scene_saliency, rsao_rasterize_scene_to_grid and
// rsao__compute_scene_coverage_score (apps/segment_transfer/arrangement_optimization.cpp), for tools/arrange_fixture/gen.py.
// This file switches on the reference's single-header implementations, includes its headers by path and only CALLS its
// functions on a database assembled with the reference's own rsdb_init / rsdb_add_class / rsdb_add_object / rsdb_add_scene; the
// second translation unit of the library is the reference's arrangement_optimization.cpp, compiled where it lies (gen.py).
// What is not a call is interface glue the reference's headers demand of whoever includes them: the implementation macros and the two
// explicit msh_array__grow instantiations below are what apps/segment_transfer/main.cpp itself states in order to link.
// Asserts stay on.  One class table per process: the reference caches class ids in statics (rs_database.h:260-271).
//
// The implementation macros below are the ones apps/segment_transfer/main.cpp:6-17 defines, minus the two that
// arrangement_optimization.cpp:1-2 defines itself.
#define MSH_STD_IMPLEMENTATION
#define MSH_ARGPARSE_IMPLEMENTATION
#define MSH_VEC_MATH_IMPLEMENTATION
#define MSH_PLY_IMPLEMENTATION
#define MSH_HASH_GRID_IMPLEMENTATION
#define RS_DATABASE_IMPLEMENTATION
#define RS_POINTCLOUD_IMPLEMENTATION
#define RS_DISTANCE_FUNCTION_IMPLEMENTATION
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
#include "rs_distance_function.h"
#include "rs_database.h"
#include "intersect.h"
#include "arrangement_optimization.h"

// the msh_array instantiations arrangement_optimization.cpp uses (apps/segment_transfer/main.cpp instantiates them for the app)
template int* msh_array__grow<int>(int* arr, unsigned long long new_len, unsigned long long elem_size );
template rs_object_placement* msh_array__grow<rs_object_placement>(rs_object_placement* arr, unsigned long long new_len, unsigned long long elem_size );

// defined in arrangement_optimization.cpp
float rsao__compute_scene_coverage_score( rsdb_t* rsdb, msh_array(rs_obj_plcmnt_t) arrangement, rsao_opts_t* opts, int32_t verbose );

typedef struct fx
{
  rsdb_t* rsdb;
  rs_pointcloud_t scene_pc;
  isect_grid3d_t sal_grd, scn_grd, arr_grd;
  rsao_opts_t opts;
} fx_t;

extern "C" {

void* fx_create( const char** class_names, const int32_t* class_ids, int32_t n_classes )
{
  fx_t* h = (fx_t*)calloc( 1, sizeof(fx_t) );
  h->rsdb = rsdb_init();
  for( int32_t i = 0; i < n_classes; ++i ) rsdb_add_class( h->rsdb, strdup( class_names[i] ), class_ids[i] );
  rsao_init_opts( &h->opts );
  return h;
}

int32_t fx_class_idx( void* hp, const char* name ) { return rsdb_get_class_idx( ((fx_t*)hp)->rsdb, name ); }

// level-2 cloud of one database object (the caller keeps `pos` alive); returns its object index
int32_t fx_add_object( void* hp, float* pos, int64_t n, int32_t class_idx, int32_t uidx )
{
  fx_t* h = (fx_t*)hp;
  rs_pointcloud_t* pc = (rs_pointcloud_t*)calloc( 1, sizeof(rs_pointcloud_t) );
  pc->positions[2] = (msh_vec3_t*)pos; pc->n_pts[2] = (size_t)n;
  rs_object_t o = rsdb_object_init();
  o.uidx = uidx; o.class_idx = class_idx; o.shape = pc;
  return rsdb_add_object( h->rsdb, &o );
}

int32_t fx_is_static( void* hp, int32_t object_idx ) { return rsdb_is_object_static( ((fx_t*)hp)->rsdb, object_idx ); }

// The one scene: level 0 (positions, class ids, qualities — the saliency's output) and level 2 (positions, qualities — the
// scene grid's input); the caller keeps the arrays alive.  Call after every object was added: the scene's proposal lists
// (rsdb->proposed_poses[0]) get one entry per object.
void fx_set_scene( void* hp, float* pos0, int32_t* class0, float* quality0, int64_t n0, float* pos2, float* quality2, int64_t n2,
                   const float* bbox_min, const float* bbox_max )
{
  fx_t* h = (fx_t*)hp;
  h->scene_pc.positions[0] = (msh_vec3_t*)pos0; h->scene_pc.class_ids[0] = class0; h->scene_pc.qualities[0] = quality0; h->scene_pc.n_pts[0] = (size_t)n0;
  h->scene_pc.positions[2] = (msh_vec3_t*)pos2; h->scene_pc.qualities[2] = quality2; h->scene_pc.n_pts[2] = (size_t)n2;
  h->scene_pc.bbox.min_p = msh_vec3( bbox_min[0], bbox_min[1], bbox_min[2] );
  h->scene_pc.bbox.max_p = msh_vec3( bbox_max[0], bbox_max[1], bbox_max[2] );
  rs_scene_t scn; memset( &scn, 0, sizeof(scn) );
  scn.uidx = 0; scn.shape = &h->scene_pc;
  rsdb_add_scene( h->rsdb, &scn );
  msh_array( msh_array( msh_mat4_t ) ) per_object = NULL;
  for( size_t i = 0; i < msh_array_len( h->rsdb->objects ); ++i ) msh_array_push( per_object, (msh_array(msh_mat4_t))NULL );
  msh_array_push( h->rsdb->proposed_poses, per_object );
}

void fx_add_proposal( void* hp, int32_t object_idx, const float* pose )
{
  fx_t* h = (fx_t*)hp;
  msh_mat4_t m; memcpy( m.data, pose, 64 );
  msh_array_push( h->rsdb->proposed_poses[0][object_idx], m );
}

// isect_grid3d_init + rsao_compute_scene_saliency (apps/segment_transfer/main.cpp:327, 337).  res / origin / the grid's bytes come
// back; the qualities are in the caller's quality0 array.  Returns the number of cells.  grid may be NULL (sizing call: the
// saliency is NOT computed then).
int64_t fx_saliency( void* hp, float voxel_size, int32_t res[3], float origin[3], uint8_t* grid )
{
  fx_t* h = (fx_t*)hp;
  if( h->sal_grd.data ) isect_grid3d_term( &h->sal_grd );
  isect_grid3d_init( &h->sal_grd, &h->scene_pc.bbox, voxel_size );
  res[0] = h->sal_grd.x_res; res[1] = h->sal_grd.y_res; res[2] = h->sal_grd.z_res;
  origin[0] = h->sal_grd.bbox.min_p.x; origin[1] = h->sal_grd.bbox.min_p.y; origin[2] = h->sal_grd.bbox.min_p.z;
  if( !grid ) return h->sal_grd.n_cells;
  h->opts.saliency_grd = &h->sal_grd;
  rsao_compute_scene_saliency( h->rsdb, 0, &h->opts );
  memcpy( grid, h->sal_grd.data, (size_t)h->sal_grd.n_cells );
  return h->sal_grd.n_cells;
}

// isect_grid3d_init x 2 + rsao_rasterize_scene_to_grid (main.cpp:323-325, 339) from the scene's level 2.  grid may be NULL (sizing).
int64_t fx_scene_grid( void* hp, float voxel_size, float quality_threshold, int32_t res[3], uint8_t* grid )
{
  fx_t* h = (fx_t*)hp;
  if( h->scn_grd.data ) { isect_grid3d_term( &h->scn_grd ); isect_grid3d_term( &h->arr_grd ); }
  isect_grid3d_init( &h->scn_grd, &h->scene_pc.bbox, voxel_size );
  isect_grid3d_init( &h->arr_grd, &h->scene_pc.bbox, voxel_size );
  res[0] = h->scn_grd.x_res; res[1] = h->scn_grd.y_res; res[2] = h->scn_grd.z_res;
  rsao_rasterize_scene_to_grid( &h->rsdb->scenes[0], &h->scn_grd, quality_threshold );
  h->opts.scn_grd = &h->scn_grd; h->opts.arrangement_grd = &h->arr_grd;
  if( grid ) memcpy( grid, h->scn_grd.data, (size_t)h->scn_grd.n_cells );
  return h->scn_grd.n_cells;
}

// rsao__compute_scene_coverage_score for one arrangement; *agree = the cells its loop counted (:364), read off the two grids it leaves
float fx_coverage( void* hp, const int32_t* object_idx, const float* poses, int32_t n_plc, int32_t* agree )
{
  fx_t* h = (fx_t*)hp;
  msh_array(rs_obj_plcmnt_t) arr = 0;
  for( int32_t i = 0; i < n_plc; ++i )
  {
    rs_obj_plcmnt_t p; memset( &p, 0, sizeof(p) );
    p.object_idx = object_idx[i]; p.uidx = h->rsdb->objects[object_idx[i]].uidx;
    memcpy( p.pose.data, poses + 16 * i, 64 );
    msh_array_push( arr, p );
  }
  const float s = rsao__compute_scene_coverage_score( h->rsdb, arr, &h->opts, 0 );
  msh_array_free( arr );
  int32_t both = 0;
  for( int32_t i = 0; i < h->scn_grd.n_cells; ++i ) both += ( h->scn_grd.data[i] > 0 && h->arr_grd.data[i] > 0 ) ? 1 : 0;
  *agree = both;
  return s;
}

} // extern "C"
