// FIXTURE GENERATION ONLY — not product code, not run by any test.
//
// A flat C interface over the reference's own rs_pointcloud_uniform_resample (lib/rs/rs_pointcloud.h:1132-1227) and
// msh_discrete_distribution_init (lib/msh/msh_std.h:1917-1925), for tools/resample_fixture/gen.py.  This file switches on the
// reference's single-header implementations, includes its headers by path and only CALLS its functions:
//   fx_resample   rs_pointcloud_uniform_resample on a mesh assembled with rs_pointcloud_init / rs_pointcloud__allocate_level
//   fx_alias      msh_discrete_distribution_init on the same areas (taken with msh_vec3_sub / msh_vec3_cross / msh_vec3_norm as
//                 :1143-1154 takes them) and seed, to expose prob / alias — and, because the resampler does not hand out the face
//                 it sampled, msh_discrete_distribution_sample n times on that context: the sequence the resampler's own context
//                 (same weights, same seed) went through.
// The reference leaves the alias entry of a column whose prob is 1.0 unwritten (malloc'ed, msh_std.h:1899-1910,1923).  fx_alias
// finds those by calling msh_discrete_distribution_update — the table-filling half of the initialisation — again over a context
// whose alias array it has filled with a marker; gen.py stores the column's own index there.
#define MSH_STD_IMPLEMENTATION
#define MSH_PLY_IMPLEMENTATION
#define MSH_ARGPARSE_IMPLEMENTATION
#define MSH_VEC_MATH_IMPLEMENTATION
#define MSH_GEOMETRY_IMPLEMENTATION
#define MSH_HASH_GRID_IMPLEMENTATION
#define RS_POINTCLOUD_IMPLEMENTATION
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
#include "rs_pointcloud.h"

extern "C" {

// Runs the reference's resampler; returns the output cloud (fx_get copies it out, fx_free releases it) and its size in *n.
void* fx_resample( const float* pos, const float* nor, const float* col, const float* radii, const int32_t* cls, const int32_t* inst,
                   int64_t n_vertices, const int32_t* faces, int64_t n_faces, int64_t* n, double* seconds )
{
  rs_pointcloud_t* in = rs_pointcloud_init( 1 );
  rs_pointcloud__allocate_level( in, 0, (int32_t)n_vertices );
  memcpy( in->positions[0], pos, n_vertices * 12 );
  memcpy( in->normals[0], nor, n_vertices * 12 );
  memcpy( in->colors[0], col, n_vertices * 12 );
  memcpy( in->radii[0], radii, n_vertices * 4 );
  memcpy( in->class_ids[0], cls, n_vertices * 4 );
  memcpy( in->instance_ids[0], inst, n_vertices * 4 );
  in->faces_ind = (int32_t*)malloc( n_faces * 12 );
  memcpy( in->faces_ind, faces, n_faces * 12 );
  in->n_faces = (size_t)n_faces;
  rs_pointcloud_t* out = rs_pointcloud_init( 1 );
  const uint64_t t0 = msh_time_now();
  rs_pointcloud_uniform_resample( in, out );
  if( seconds ) *seconds = msh_time_diff_ms( msh_time_now(), t0 ) * 1e-3;
  rs_pointcloud_free( in, 1 );
  *n = (int64_t)out->n_pts[0];
  return out;
}

void fx_get( void* h, float* pos, float* nor, float* col, float* radii, int32_t* cls, int32_t* inst )
{
  rs_pointcloud_t* out = (rs_pointcloud_t*)h;
  const size_t n = out->n_pts[0];
  memcpy( pos, out->positions[0], n * 12 );
  memcpy( nor, out->normals[0], n * 12 );
  memcpy( col, out->colors[0], n * 12 );
  memcpy( radii, out->radii[0], n * 4 );
  memcpy( cls, out->class_ids[0], n * 4 );
  memcpy( inst, out->instance_ids[0], n * 4 );
}

void fx_free( void* h ) { rs_pointcloud_free( (rs_pointcloud_t*)h, 1 ); }

// prob / alias / written (n_faces each), the double total of the areas, and the first n_seq faces the sampler draws.
void fx_alias( const float* pos, const int32_t* faces, int64_t n_faces, double* prob, int32_t* alias, uint8_t* written,
               double* total_area, int32_t* face_seq, int64_t n_seq )
{
  const msh_vec3_t* p = (const msh_vec3_t*)pos;
  double* areas = (double*)malloc( n_faces * sizeof(double) );
  double total = 0;
  for( int64_t i = 0; i < n_faces; ++i )
  {
    msh_vec3_t a = p[faces[3 * i]], b = p[faces[3 * i + 1]], c = p[faces[3 * i + 2]];
    double cur = msh_vec3_norm( msh_vec3_cross( msh_vec3_sub( b, a ), msh_vec3_sub( c, a ) ) );
    total += cur;
    areas[i] = cur;
  }
  *total_area = total;
  msh_discrete_distrib_t ctx = {0};
  msh_discrete_distribution_init( &ctx, areas, (size_t)n_faces, 64321ULL );
  for( int64_t i = 0; i < n_faces; ++i ) { prob[i] = ctx.prob[i]; alias[i] = ctx.alias[i]; }
  // which alias entries did it write?  The table again, twice, over two different fillings of the context's own array
  // (msh_discrete_distribution_update is the part of the initialisation that fills the table, msh_std.h:1924)
  for( int64_t i = 0; i < n_faces; ++i ) ctx.alias[i] = -1;
  msh_discrete_distribution_update( &ctx, areas, (size_t)n_faces );
  for( int64_t i = 0; i < n_faces; ++i ) written[i] = ctx.alias[i] != -1;
  for( int64_t i = 0; i < n_faces; ++i ) ctx.alias[i] = -2;
  msh_discrete_distribution_update( &ctx, areas, (size_t)n_faces );
  for( int64_t i = 0; i < n_faces; ++i ) { assert( written[i] == ( ctx.alias[i] != -2 ) ); assert( !written[i] || ctx.alias[i] == alias[i] ); assert( ctx.prob[i] == prob[i] ); }
  for( int64_t i = 0; i < n_seq; ++i ) face_seq[i] = msh_discrete_distribution_sample( &ctx );
  msh_discrete_distribution_free( &ctx );
  free( areas );
}

} // extern "C"
