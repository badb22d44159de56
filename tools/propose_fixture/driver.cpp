// FIXTURE GENERATION ONLY — not product code, not run by any test.
//
// A flat C interface over the reference's own mgs__propose_poses_at_level and mgs_propose_poses
// (apps/pose_proposal/pose_proposal.cpp:305-369), for tools/propose_fixture/gen.py.  This file switches on
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

// defined in pose_proposal.cpp, not declared in its header
void mgs__propose_poses_at_level( rsdb_t* rsdb, rs_pointcloud_t* input_scan, rs_df_t* df_input_scan, int32_t lvl,
                                  msh_array(msh_array(pose_proposal_t)) *proposed_poses, const mgs_opts_t* opts );

// what the last fx_run left: stages 0..2 = the proposal storage after levels 4, 3, 2; stage 3 = mgs_propose_poses' lists
static msh_array(msh_array(pose_proposal_t)) g_stage[4];

static msh_array(msh_array(pose_proposal_t)) copy_lists( msh_array(msh_array(pose_proposal_t)) in )
{
  msh_array(msh_array(pose_proposal_t)) out = NULL;
  for( size_t i = 0; i < msh_array_len( in ); ++i )
  {
    msh_array(pose_proposal_t) l = NULL;
    for( size_t j = 0; j < msh_array_len( in[i] ); ++j ) msh_array_push( l, in[i][j] );
    msh_array_push( out, l );
  }
  return out;
}

extern "C" {

// A cloud from level-0 points: bounding box, levels 1..4 by the reference's own level builder and the search grids
// (rs_pointcloud_compute_levels, lib/rs/rs_pointcloud.h:1306-1316).
void* fx_cloud( const float* pos, const float* nor, int32_t n )
{
  rs_pointcloud_t* pc = rs_pointcloud_init( 1 );
  rs_pointcloud__allocate_level( pc, 0, n );
  memcpy( pc->positions[0], pos, (size_t)n * sizeof(msh_vec3_t) );
  memcpy( pc->normals[0], nor, (size_t)n * sizeof(msh_vec3_t) );
  memset( pc->colors[0], 0, (size_t)n * sizeof(msh_vec3_t) );
  memset( pc->radii[0], 0, (size_t)n * 4 ); memset( pc->qualities[0], 0, (size_t)n * 4 );
  memset( pc->class_ids[0], 0, (size_t)n * 4 ); memset( pc->instance_ids[0], 0, (size_t)n * 4 );
  rs_pointcloud_compute_levels( pc );
  return pc;
}

int32_t fx_level( void* cloud, int32_t lvl, float* pos, float* nor )
{
  rs_pointcloud_t* pc = (rs_pointcloud_t*)cloud;
  if( pos ) memcpy( pos, pc->positions[lvl], pc->n_pts[lvl] * sizeof(msh_vec3_t) );
  if( nor ) memcpy( nor, pc->normals[lvl], pc->n_pts[lvl] * sizeof(msh_vec3_t) );
  return (int32_t)pc->n_pts[lvl];
}

void fx_bbox( void* cloud, float out[6] )
{
  rs_pointcloud_t* pc = (rs_pointcloud_t*)cloud;
  out[0] = pc->bbox.min_p.x; out[1] = pc->bbox.min_p.y; out[2] = pc->bbox.min_p.z;
  out[3] = pc->bbox.max_p.x; out[4] = pc->bbox.max_p.y; out[5] = pc->bbox.max_p.z;
}
// the box is the caller's datum (an app reads it off the scan); a case may set the one it wants searched
void fx_set_bbox( void* cloud, const float in[6] )
{
  rs_pointcloud_t* pc = (rs_pointcloud_t*)cloud;
  pc->bbox.min_p = msh_vec3( in[0], in[1], in[2] ); pc->bbox.max_p = msh_vec3( in[3], in[4], in[5] );
}

void* fx_db( void ) { return rsdb_init(); }
void fx_add_class( void* db, const char* name, int32_t idx ) { rsdb_add_class( (rsdb_t*)db, strdup( name ), idx ); }
int32_t fx_add_object( void* db, void* cloud, int32_t class_idx, int32_t uidx )
{
  rs_object_t o = rsdb_object_init();
  o.uidx = uidx; o.class_idx = class_idx; o.shape = (rs_pointcloud_t*)cloud;
  rsdb_add_object( (rsdb_t*)db, &o );
  return (int32_t)msh_array_len( ((rsdb_t*)db)->objects ) - 1;
}
int32_t fx_is_static( void* db, int32_t object_idx ) { return rsdb_is_object_static( (rsdb_t*)db, object_idx ); }

// mgs__propose_poses_at_level for levels 4, 3, 2 with the storage recorded after each, then mgs_propose_poses itself.
// Returns 1 where the whole function's lists equal the final copy (:347-359) of the staged run's storage, bit for bit.
int32_t fx_run( void* dbp, void* scene, float spacing, float angle_delta )
{
  rsdb_t* db = (rsdb_t*)dbp; rs_pointcloud_t* scan = (rs_pointcloud_t*)scene;
  mgs_opts_t opts; mgs_init_opts( &opts );
  opts.search_grid_spacing = spacing; opts.search_grid_angle_delta = angle_delta;
  msh_array(msh_array(pose_proposal_t)) storage = NULL;
  int32_t s = 0;
  for( int32_t lvl = RSPC_N_LEVELS - 1; lvl > RSPC_N_LEVELS - 4; lvl--, ++s )
  {
    mgs__propose_poses_at_level( db, scan, NULL, lvl, &storage, &opts );
    g_stage[s] = copy_lists( storage );
  }
  msh_array(msh_array(pose_proposal_t)) whole = NULL;
  mgs_propose_poses( db, scan, &whole, &opts, 0 );
  g_stage[3] = whole;
  int32_t same = msh_array_len( whole ) == msh_array_len( storage );
  for( size_t i = 0; same && i < msh_array_len( storage ); ++i )
  {
    size_t k = 0;
    for( size_t j = 0; j < msh_array_len( storage[i] ); ++j )
    {
      if( !( fabsf( storage[i][j].score ) > 0.000001f ) ) continue;
      if( k >= msh_array_len( whole[i] ) || memcmp( &whole[i][k], &storage[i][j], sizeof(pose_proposal_t) ) ) { same = 0; break; }
      ++k;
    }
    if( k != msh_array_len( whole[i] ) ) same = 0;
  }
  return same;
}

int32_t fx_stage_count( int32_t stage, int32_t object_idx ) { return (int32_t)msh_array_len( g_stage[stage][object_idx] ); }
void fx_stage_get( int32_t stage, int32_t object_idx, float* poses, float* scores )
{
  msh_array(pose_proposal_t) l = g_stage[stage][object_idx];
  for( size_t j = 0; j < msh_array_len( l ); ++j ) { memcpy( poses + 16 * j, l[j].xform.data, 64 ); scores[j] = l[j].score; }
}

} // extern "C"
