// The reference's voxel grid (lib/rs/intersect.h:59-109) as the coverage code and the arrangement code (rs_rows.hip,
// rs_arrange.hip, rs_rows_api.hip) share it: the grid of a box, the cell of a point, the coverage object.
#pragma once
#include "rs_device.h"

#include <cmath>

// One bit per voxel of the scene grid (rs_hip_coverage_create), bit c & 31 of word c >> 5 for the reference's cell c.
struct rs_hip_coverage
{
  rs::VoxGrid grid{};
  float voxel_size = 0.0f, origin[3] = { 0, 0, 0 };
  int n_words = 0;
  long long valid = 0;
  uint32_t* d_bits = nullptr;
};

namespace rs {

// isect_grid3d_init (lib/rs/intersect.h:59-75), same float operations: the box fattened by 0.3, ceilf( extent / voxel ) + 1
// cells per axis.  False (nothing written) when the cell count is not positive or does not fit the reference's int32 index;
// *cells_out (may be null) receives the count either way.
inline bool vox_grid_init( const float bbox_min[3], const float bbox_max[3], float voxel_size, VoxGrid& g, double* cells_out )
{
  const float fat = 0.3f;
  float mn[3], mx[3];
  for( int a = 0; a < 3; ++a ) { mn[a] = bbox_min[a] - fat; mx[a] = bbox_max[a] + fat; }
  const double cells = ( (double)std::ceil( ( mx[0] - mn[0] ) / voxel_size ) + 1 ) * ( (double)std::ceil( ( mx[1] - mn[1] ) / voxel_size ) + 1 ) *
                       ( (double)std::ceil( ( mx[2] - mn[2] ) / voxel_size ) + 1 );
  if( cells_out ) *cells_out = cells;
  if( !( cells > 0 ) || cells > 2.0e9 ) return false;
  g.x_res = (int)std::ceil( ( mx[0] - mn[0] ) / voxel_size ) + 1;
  g.y_res = (int)std::ceil( ( mx[1] - mn[1] ) / voxel_size ) + 1;
  g.z_res = (int)std::ceil( ( mx[2] - mn[2] ) / voxel_size ) + 1;
  g.n_cells = g.x_res * g.y_res * g.z_res;
  g.ox = mn[0]; g.oy = mn[1]; g.oz = mn[2];
  g.inv_voxel = 1.0f / voxel_size;                              // :100
  return true;
}

#ifdef __HIPCC__
// isect_grid3d_cell_from_world_space (:97-109): the cell's index in the reference's byte array, -1 outside the grid.  The range
// test is made on the floored floats BEFORE the conversion: a NaN, an infinity or a value no int32 holds fails it, as the
// reference's conversion to INT_MIN does on its x86 build (a device conversion would make cell 0 of a NaN).  Every finite input
// keeps its cell while the resolutions are below 2^24, where (float)res is exact, as in isect_rasterise (rs_isect.hip); past
// 2^24 cells along one axis fp32 coordinates no longer tell neighbouring cells apart.
__device__ __forceinline__ int voxel_of( const VoxGrid& g, float x, float y, float z )
{
  const float fx = floorf( ( x - g.ox ) * g.inv_voxel );        // intersect.h:101-103
  const float fy = floorf( ( y - g.oy ) * g.inv_voxel );
  const float fz = floorf( ( z - g.oz ) * g.inv_voxel );
  if( !( fx >= 0.0f && fx < (float)g.x_res && fy >= 0.0f && fy < (float)g.y_res && fz >= 0.0f && fz < (float)g.z_res ) ) return -1;
  return (int)fy * g.x_res * g.z_res + (int)fz * g.x_res + (int)fx;      // :108
}
#endif

} // namespace rs
