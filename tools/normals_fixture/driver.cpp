// FIXTURE GENERATION ONLY — not product code, not run by any test.
//
// A flat C interface over the reference's own rs_pointcloud__compute_normals (lib/rs/rs_pointcloud.h:556-596), for
// tools/normals_fixture/gen.py.  This file switches on the reference's single-header implementations, includes its headers by path
// and only CALLS its functions:
//   fx_normals   rs_pointcloud__compute_normals on a cloud assembled with rs_pointcloud_init / rs_pointcloud__allocate_level; where
//                asked, the loader's pass over the result, taken with msh_vec3_normalize / msh_isnan / msh_vec3_zeros as
//                rs_pointcloud__load_ply takes it (:745-751).
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

// out_nor: 3 * n_vertices floats.  seconds (may be null): the time of the reference's call alone.
void fx_normals( const float* pos, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t loader_pass, float* out_nor,
                 double* seconds )
{
  rs_pointcloud_t* pc = rs_pointcloud_init( 1 );
  rs_pointcloud__allocate_level( pc, 0, (int32_t)n_vertices );
  memcpy( pc->positions[0], pos, n_vertices * 12 );
  int32_t* ind = (int32_t*)malloc( n_faces * 12 );
  memcpy( ind, faces, n_faces * 12 );
  const uint64_t t0 = msh_time_now();
  rs_pointcloud__compute_normals( pc, ind, (int32_t)n_faces );
  if( seconds ) *seconds = msh_time_diff_ms( msh_time_now(), t0 ) * 1e-3;
  if( loader_pass )
    for( int64_t i = 0; i < n_vertices; ++i )
    {
      pc->normals[0][i] = msh_vec3_normalize( pc->normals[0][i] );
      if( msh_isnan( pc->normals[0][i].x ) || msh_isnan( pc->normals[0][i].y ) || msh_isnan( pc->normals[0][i].z ) ) pc->normals[0][i] = msh_vec3_zeros();
    }
  memcpy( out_nor, pc->normals[0], n_vertices * 12 );
  free( ind );
  rs_pointcloud_free( pc, 1 );
}

} // extern "C"
