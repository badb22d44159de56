// FIXTURE GENERATION ONLY — not product code, not run by any test.
//
// A flat C interface over the reference's own plane functions, for tools/plane_fixture/gen.py.  rspf_detector_params_t and the
// functions that take it are defined inside lib/rs/rs_pointcloud_filters.cpp, so gen.py compiles ONE scratch translation unit
// in a temporary directory: that file's lines 1-14 and 16-879 (everything but the include of the un-vendored gco header and
// rspf_smooth_labels, its one user — the recipe the test infrastructure's Makefile uses for its filters library), followed by this file.  The
// reference's text above has declared its single-header libraries; the macros below make the second inclusion emit their
// implementations (the ones apps/segment_transfer/main.cpp:6-17 defines).
//
// This file only CALLS the reference: rspf__detect_floor, rspf__detect_walls, evaluate_plane_model, remove_inliers,
// rspf__gather_model_inliers, rspf_relabel_walls_and_floors, msh_discrete_distribution_init / _sample / _free and the msh_vec3
// functions.  The per-round recordings are made by gen.py from these calls and checked there against what the two detect
// functions return.

#define MSH_STD_IMPLEMENTATION
#define MSH_ARGPARSE_IMPLEMENTATION
#define MSH_VEC_MATH_IMPLEMENTATION
#define MSH_GEOMETRY_IMPLEMENTATION
#define MSH_PLY_IMPLEMENTATION
#define MSH_HASH_GRID_IMPLEMENTATION
#define RS_DATABASE_IMPLEMENTATION
#define RS_POINTCLOUD_IMPLEMENTATION
#define RS_DISTANCE_FUNCTION_IMPLEMENTATION
#define FILEPATH_HELPERS_IMPLEMENTATION
#define HASHTABLE_IMPLEMENTATION

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

// the msh_array instantiations the filters text uses (apps/segment_transfer/main.cpp:51-55 instantiates them for the app)
template int32_t* msh_array__grow<int32_t>( int32_t* arr, unsigned long long new_len, unsigned long long elem_size );
template rs_object_placement* msh_array__grow<rs_object_placement>( rs_object_placement* arr, unsigned long long new_len, unsigned long long elem_size );
template rspf_plane_model* msh_array__grow<rspf_plane_model>( rspf_plane_model* arr, unsigned long long new_len, unsigned long long elem_size );
template rspf_edge* msh_array__grow<rspf_edge>( rspf_edge* arr, unsigned long long new_len, unsigned long long elem_size );
template rs_pointcloud_t** msh_array__grow<rs_pointcloud_t*>( rs_pointcloud_t** arr, unsigned long long new_len, unsigned long long elem_size );

// plane models as plain arrays: center[3], normal[3], axes[9] column-major, extends[4], valid, normal_up_dot per model
struct fx_models { float* center; float* normal; float* axes; float* extends; int8_t* valid; float* up_dot; int64_t* n_inliers; };

static msh_array( rspf_plane_model_t ) fx_models_in( const fx_models* m, int32_t n_models )
{
  msh_array( rspf_plane_model_t ) a = {0};
  for( int32_t i = 0; i < n_models; ++i )
  {
    rspf_plane_model_t p; memset( &p, 0, sizeof(p) );
    memcpy( &p.plane.center, m->center + 3 * i, 12 );
    memcpy( &p.plane.normal, m->normal + 3 * i, 12 );
    if( m->axes ) memcpy( p.axes.data, m->axes + 9 * i, 36 );
    if( m->extends ) memcpy( p.extends.data, m->extends + 4 * i, 16 );
    if( m->valid ) p.valid = m->valid[i];
    if( m->up_dot ) p.features.normal_up_dot = m->up_dot[i];
    msh_array_push( a, p );
  }
  return a;
}

extern "C" {

// rspf__detect_floor then rspf__detect_walls as rspf_detect_planes calls them (:498-507).  out: room for 64 models.
void fx_detect( float* pos, float* nor, int64_t n, float dot_threshold, float dist_threshold, int64_t count_threshold,
                fx_models* out, int32_t* n_floors, int32_t* n_walls, int32_t* n_models, double* seconds )
{
  rspf_detector_params_t params = {0};
  params.pts = (msh_vec3_t*)pos; params.nrmls = (msh_vec3_t*)nor; params.n_pts = (size_t)n;
  params.dot_threshold = dot_threshold; params.dist_threshold = dist_threshold; params.count_threshold = (size_t)count_threshold;
  msh_array( rspf_plane_model_t ) models = {0};
  uint64_t t0 = msh_time_now();
  *n_floors = rspf__detect_floor( &params, &models );
  *n_walls = rspf__detect_walls( &params, &models );
  if( seconds ) *seconds = msh_time_diff_ms( msh_time_now(), t0 ) * 1e-3;
  *n_models = (int32_t)msh_array_len( models );
  for( int32_t i = 0; i < *n_models && i < 64; ++i )
  {
    memcpy( out->center + 3 * i, &models[i].plane.center, 12 );
    memcpy( out->normal + 3 * i, &models[i].plane.normal, 12 );
    out->n_inliers[i] = (int64_t)models[i].n_inliers;
  }
  msh_array_free( models );
}

// n_iter triples from msh_discrete_distribution_init( weights, n, 12346 ) and _sample; distinct: the walls' redraws (:162-164)
void fx_sample( double* weights, int64_t n, int32_t n_iter, int32_t distinct, int32_t* idx )
{
  msh_discrete_distrib_t dist = {0};
  msh_discrete_distribution_init( &dist, weights, (size_t)n, 12346ULL );
  for( int32_t i = 0; i < n_iter; ++i )
  {
    int32_t a, b, c;
    a = msh_discrete_distribution_sample( &dist );
    if( distinct )
    {
      do { b = msh_discrete_distribution_sample( &dist ); } while( a == b );
      do { c = msh_discrete_distribution_sample( &dist ); } while( b == c );
    }
    else { b = msh_discrete_distribution_sample( &dist ); c = msh_discrete_distribution_sample( &dist ); }
    idx[3 * i] = a; idx[3 * i + 1] = b; idx[3 * i + 2] = c;
  }
  msh_discrete_distribution_free( &dist );
}

// per triple: centre, normal (msh_vec3_sub / _cross / _normalize), the walls' up test against 1 - dot_threshold, and the
// votes of evaluate_plane_model
void fx_score( float* pos, int64_t n, double* weights, const int32_t* idx, int32_t n_iter, float dot_threshold, float dist_threshold,
               float* center, float* normal, uint8_t* valid, int32_t* counts )
{
  msh_vec3_t* pts = (msh_vec3_t*)pos;
  msh_vec3_t up = msh_vec3_posy();
  for( int32_t i = 0; i < n_iter; ++i )
  {
    msh_vec3_t p_a = pts[idx[3 * i]], p_b = pts[idx[3 * i + 1]], p_c = pts[idx[3 * i + 2]];
    msh_vec3_t nn = msh_vec3_normalize( msh_vec3_cross( msh_vec3_sub( p_b, p_a ), msh_vec3_sub( p_c, p_a ) ) );
    rspf_plane_model_t model; memset( &model, 0, sizeof(model) );
    model.plane.center = p_a; model.plane.normal = nn;
    evaluate_plane_model( &model, weights, pts, (size_t)n, dist_threshold );
    memcpy( center + 3 * i, &p_a, 12 ); memcpy( normal + 3 * i, &nn, 12 );
    valid[i] = msh_abs( msh_vec3_dot( nn, up ) ) < ( 1 - dot_threshold ) ? 1 : 0;
    counts[i] = (int32_t)model.n_inliers;
  }
}

// evaluate_plane_model for hypotheses given as centre and normal (the hostile fixture's planes come from no triple)
void fx_votes( float* pos, int64_t n, double* weights, const float* center, const float* normal, int32_t n_hyp, float dist_threshold,
               int32_t* counts )
{
  for( int32_t i = 0; i < n_hyp; ++i )
  {
    rspf_plane_model_t model; memset( &model, 0, sizeof(model) );
    memcpy( &model.plane.center, center + 3 * i, 12 ); memcpy( &model.plane.normal, normal + 3 * i, 12 );
    evaluate_plane_model( &model, weights, (msh_vec3_t*)pos, (size_t)n, dist_threshold );
    counts[i] = (int32_t)model.n_inliers;
  }
}

void fx_remove( float* pos, int64_t n, double* weights, const float* center, const float* normal, float dist_threshold )
{
  rspf_plane_model_t model; memset( &model, 0, sizeof(model) );
  memcpy( &model.plane.center, center, 12 ); memcpy( &model.plane.normal, normal, 12 );
  remove_inliers( &model, weights, (msh_vec3_t*)pos, (size_t)n, dist_threshold );
}

// rspf__gather_model_inliers: index (room for n_models * n) and n_models + 1 offsets
void fx_gather( float* pos, float* nor, int64_t n, const fx_models* m, int32_t n_models, float dot_threshold, float dist_threshold,
                int32_t check_validity, int32_t check_extends, int32_t* index, int64_t* offsets )
{
  rspf_detector_params_t params = {0};
  params.pts = (msh_vec3_t*)pos; params.nrmls = (msh_vec3_t*)nor; params.n_pts = (size_t)n;
  params.dot_threshold = dot_threshold; params.dist_threshold = dist_threshold;
  params.check_validity = check_validity != 0; params.check_extends = check_extends != 0;
  msh_array( rspf_plane_model_t ) models = fx_models_in( m, n_models );
  rspf__gather_model_inliers( &params, &models );
  int64_t at = 0;
  for( int32_t i = 0; i < n_models; ++i )
  {
    offsets[i] = at;
    const size_t k = msh_array_len( models[i].inlier_ind );
    if( k ) memcpy( index + at, models[i].inlier_ind, k * 4 );
    at += (int64_t)k;
    msh_array_free( models[i].inlier_ind );
  }
  offsets[n_models] = at;
  msh_array_free( models );
}

// rspf_relabel_walls_and_floors on a cloud whose level 1 is the caller's arrays; class_ids / instance_ids rewritten in place
void fx_relabel( float* pos, float* nor, int64_t n, const fx_models* m, int32_t n_models, int32_t floor_idx, int32_t wall_idx,
                 int32_t unlabelled_idx, int32_t* class_ids, int32_t* instance_ids )
{
  rsdb_t* rsdb = rsdb_init();
  rsdb_add_class( rsdb, strdup( "floor" ), floor_idx );
  rsdb_add_class( rsdb, strdup( "wall" ), wall_idx );
  rsdb_add_class( rsdb, strdup( "unlabelled" ), unlabelled_idx );
  rs_pointcloud_t* pc = (rs_pointcloud_t*)calloc( 1, sizeof(rs_pointcloud_t) );
  pc->positions[1] = (msh_vec3_t*)pos; pc->normals[1] = (msh_vec3_t*)nor; pc->n_pts[1] = (size_t)n;
  pc->class_ids[1] = class_ids; pc->instance_ids[1] = instance_ids;
  msh_array( rspf_plane_model_t ) models = fx_models_in( m, n_models );
  rspf_relabel_walls_and_floors( rsdb, pc, &models );
  for( int32_t i = 0; i < n_models; ++i ) msh_array_free( models[i].inlier_ind );
  msh_array_free( models );
  free( pc );        // the rsdb's tables are left to process exit (rsdb_free expects file-loaded clouds)
}

} // extern "C"
