// Host planner of the pose search (mgs__initial_pose_proposals, apps/pose_proposal/pose_proposal.cpp:203-222): the three tables the
// grid search enumerates — cell offsets along x and z and one rotation per yaw step.  Plain C++, no HIP: rs_propose.hip includes it
// for rs_hip_pose_grid_plan and rs_hip_propose_poses, and a stand-alone program can include it alone.
//
// The reference's loops are kept as written, with their accidents: the cell offsets are fp32 counters accumulated by += and compared
// in fp32 against length + spacing (:213, :215), so a length of 3.2 at spacing 0.1 gives 35 steps where the real numbers give 34; the
// yaw counter is fp32 too but compared against MSH_TWO_PI, the DOUBLE literal 6.2831853072 (:219, lib/msh/msh_std.h:619).
#pragma once
#include "rs_math.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

namespace rs {
namespace propose {

constexpr int32_t MAX_STEPS = 1 << 20;        // per table: beyond it the call is refused
constexpr int RC_OK = 0, RC_ARG = -2, RC_CAPACITY = -4;     // RS_HIP_OK, RS_HIP_E_ARG, RS_HIP_E_CAPACITY (include/rescan_hip.h)

// for( float o = -spacing; o < length + spacing; o += spacing ): the steps, written to out where it is not null.
// -1: the counter stopped advancing (the reference would never end); -2: more than MAX_STEPS
inline int32_t offsets( float length, float spacing, float* out )
{
  int32_t n = 0;
  const float bound = length + spacing;
  for( float o = -spacing; o < bound; )
  {
    if( n >= MAX_STEPS ) return -2;
    if( out ) out[n] = o;
    ++n;
    const float next = o + spacing;
    if( !( next > o ) ) return -1;
    o = next;
  }
  return n;
}

// for( float y_angle = 0.0f; y_angle < MSH_TWO_PI; y_angle += y_angle_inc ): the angles
inline int32_t yaw_angles( float angle_delta, float* out )
{
  int32_t n = 0;
  for( float a = 0.0f; (double)a < 6.2831853072; )
  {
    if( n >= MAX_STEPS ) return -2;
    if( out ) out[n] = a;
    ++n;
    const float next = a + angle_delta;
    if( !( next > a ) ) return -1;
    a = next;
  }
  return n;
}

// Two passes, like rs_hip_resample_plan: the counts always; a table only where it is not null, and then all of them or none.
// yaw: n_yaw column-major matrices, msh_rotate( msh_mat4_identity(), y_angle, (0, 1, 0) ) (:221) with the host libm's sinf / cosf.
inline int grid_plan( const float bbox_min[3], const float bbox_max[3], float spacing, float angle_delta,
                      int32_t* n_x, int32_t* n_z, int32_t* n_yaw, float* ox, int32_t cap_x, float* oz, int32_t cap_z, float* yaw, int32_t cap_yaw,
                      char* err, size_t err_len )
{
  if( !bbox_min || !bbox_max || !n_x || !n_z || !n_yaw ) { snprintf( err, err_len, "pose_grid_plan: null box or counts" ); return RC_ARG; }
  for( int a = 0; a < 3; ++a )
    if( !std::isfinite( bbox_min[a] ) || !std::isfinite( bbox_max[a] ) ) { snprintf( err, err_len, "pose_grid_plan: the box is not finite" ); return RC_ARG; }
  if( !( spacing > 0.0f ) || !std::isfinite( spacing ) || !( angle_delta > 0.0f ) || !std::isfinite( angle_delta ) )
  { snprintf( err, err_len, "pose_grid_plan: spacing and angle_delta must be positive and finite (the reference's loops would not end)" ); return RC_ARG; }
  const float length_x = bbox_max[0] - bbox_min[0], length_z = bbox_max[2] - bbox_min[2];     // :205-206
  if( !std::isfinite( length_x ) || !std::isfinite( length_z ) ) { snprintf( err, err_len, "pose_grid_plan: the box is not finite" ); return RC_ARG; }
  const int32_t nx = offsets( length_x, spacing, nullptr ), nz = offsets( length_z, spacing, nullptr ), ny = yaw_angles( angle_delta, nullptr );
  if( nx == -1 || nz == -1 || ny == -1 )
  { snprintf( err, err_len, "pose_grid_plan: a step too small to advance its fp32 counter (the reference's loop would not end)" ); return RC_ARG; }
  if( nx == -2 || nz == -2 || ny == -2 ) { snprintf( err, err_len, "pose_grid_plan: more than %d steps in a table", MAX_STEPS ); return RC_CAPACITY; }
  *n_x = nx; *n_z = nz; *n_yaw = ny;
  if( ( ox && cap_x < nx ) || ( oz && cap_z < nz ) || ( yaw && cap_yaw < ny ) )
  { snprintf( err, err_len, "pose_grid_plan: a table is too short (needed: %d, %d, %d)", nx, nz, ny ); return RC_CAPACITY; }
  if( ox ) offsets( length_x, spacing, ox );
  if( oz ) offsets( length_z, spacing, oz );
  if( yaw )
  {
    int32_t k = 0;
    for( float a = 0.0f; k < ny; a += angle_delta, ++k )
    {
      const Mat4 R = mat4_rotate_axis( mat4_identity(), a, 1 );
      for( int i = 0; i < 16; ++i ) yaw[16 * (size_t)k + i] = R.m[i];
    }
  }
  return RC_OK;
}

} // namespace propose
} // namespace rs
