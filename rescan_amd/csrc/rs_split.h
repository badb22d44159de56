// Host planner of the split that opens a sequence — seg2rsdb's pointcloud_to_rsdb (apps/seg2rsdb/main.cpp:80-136): the table of
// instance ids in order of first appearance (hashtable_keys returns insertion order, lib/mg/hashtable.h:535-577), the stable cut of
// the scan into one segment per instance (rs_pointcloud_copy_by_ids, lib/rs/rs_pointcloud.h:239-297), every segment's centroid
// (rs_pointcloud_centroid, :1318-1339), the transform that puts a dynamic object's centroid over the origin (msh_translate,
// rs_pointcloud_transform :1367-1378) and the pose inverse( xform ).  Plain C++, no HIP: rs_split.hip includes it for the device
// route, rs_dropin.cpp for the route without a device, and a stand-alone program can include it alone.
//
// The loops are the reference's, restated:
//   table     ids in order of first appearance; the reference's key is the int32 widened to 64 bits and read back through an
//             int32_t*, so the id is the int32 itself, negative values included
//   segment   the points with that id, in input order; the object's class is the class id of the segment's FIRST point (:114)
//   centroid  per axis  double c = 0; c += (double)p[i]  over the segment in order, c / (double)n, cast to float; then y = 0 (:119)
//   xform     identity for a class in the caller's static list (rsdb_is_class_static needs a class table; the caller has it);
//             otherwise msh_translate( identity, ( -cx, -0.0f, -cz ) ), and every position goes through msh_mat4_vec3_mul( xform, p, 1 ),
//             every normal through ( xform, n, 0 ): the general product, not a subtraction.  A static object's points are NOT
//             passed through the product
//   pose      msh_mat4_inverse( xform ), for the identity too
#pragma once

#include "../../include/rescan_hip.h"
#include "rs_math.h"

#include <cstdio>
#include <unordered_map>
#include <vector>

struct ihipStream_t;                             // (hipStream_t's target: this header needs no HIP)

namespace rs {
namespace split {

constexpr int32_t MAX_INSTANCES = 4096;          // the reference's own labels stop at 127 placements
constexpr int64_t MAX_POINTS = 2147483646ll;     // an int32 index names every point

inline int refuse( int rc, char* err, size_t err_cap, const char* what, long long v )
{
  if( err && err_cap ) snprintf( err, err_cap, what, v );
  return rc;
}
inline int check_size( int64_t n, char* err, size_t err_cap )
{
  if( n < 0 ) return refuse( RS_HIP_E_ARG, err, err_cap, "split: %lld points: a count cannot be negative", (long long)n );
  if( n > MAX_POINTS ) return refuse( RS_HIP_E_CAPACITY, err, err_cap, "split: %lld points: more than an int32 index can name", (long long)n );
  return RS_HIP_OK;
}
inline int check_static( const int32_t* static_classes, int32_t n_static, char* err, size_t err_cap )
{
  if( n_static < 0 || ( n_static > 0 && !static_classes ) )
    return refuse( RS_HIP_E_ARG, err, err_cap, "split: a list of %lld static classes without its array, or of negative length", (long long)n_static );
  return RS_HIP_OK;
}
inline bool class_is_static( int32_t cls, const int32_t* static_classes, int32_t n_static )
{
  for( int32_t k = 0; k < n_static; ++k ) if( static_classes[k] == cls ) return true;
  return false;
}

// msh_mat4_vec3_mul (msh_vec_math.h:1554-1561): three products added left to right, then (float)is_point times the translation
RS_HD inline void xform3( const float* m, const float v[3], float w, float o[3] )
{
  o[0] = m[0] * v[0] + m[4] * v[1] + m[ 8] * v[2] + w * m[12];
  o[1] = m[1] * v[0] + m[5] * v[1] + m[ 9] * v[2] + w * m[13];
  o[2] = m[2] * v[0] + m[6] * v[1] + m[10] * v[2] + w * m[14];
}

struct Table
{
  std::vector<int32_t> ids;
  std::vector<int64_t> counts, first;
};

// The table alone.  RS_HIP_E_CAPACITY above MAX_INSTANCES distinct ids.
inline int table( const int32_t* instance_ids, int64_t n, Table& T, char* err, size_t err_cap )
{
  std::unordered_map<int32_t, int32_t> rank;
  T.ids.clear(); T.counts.clear(); T.first.clear();
  for( int64_t i = 0; i < n; ++i )
  {
    const int32_t id = instance_ids[i];
    auto it = rank.find( id );
    if( it == rank.end() )
    {
      if( (int32_t)T.ids.size() == MAX_INSTANCES )
        return refuse( RS_HIP_E_CAPACITY, err, err_cap, "split: more than %lld distinct instance ids", (long long)MAX_INSTANCES );
      rank.emplace( id, (int32_t)T.ids.size() );
      T.ids.push_back( id ); T.counts.push_back( 1 ); T.first.push_back( i );
    }
    else T.counts[(size_t)it->second]++;
  }
  return RS_HIP_OK;
}

// (float)( sum / n ) per axis from the three doubles of one segment, and what the reference derives from it: the centroid with
// y = 0, xform and pose.  Shared by the plan and by the device route, which brings the sums back.
inline void finish_object( const double sum[3], int64_t count, bool is_static, float centroid[3], float xform[16], float pose[16] )
{
  float c[3];
  for( int a = 0; a < 3; ++a ) { double v = sum[a]; v /= (double)count; c[a] = (float)v; }
  c[1] = 0;                                                                       // main.cpp:119
  Mat4 X = mat4_identity();
  if( !is_static ) X = mat4_translate( mat4_identity(), -c[0], -c[1], -c[2] );    // msh_vec3_invert: -0.0f for y
  const Mat4 P = mat4_inverse( X );
  if( centroid ) std::memcpy( centroid, c, 12 );
  if( xform ) std::memcpy( xform, X.m, 64 );
  if( pose ) std::memcpy( pose, P.m, 64 );
}

struct Plan
{
  int32_t* n_instances; int32_t* inst_ids; int64_t* counts; int64_t* first; int64_t* offsets; int32_t* order;
  int32_t* class_of; int32_t* is_static; double* sums; float* centroids; float* xforms; float* poses; float* out_pos; float* out_nor;
};

// The whole of pointcloud_to_rsdb's loop on host arrays.  Every output of P may be null; nothing is written on a refusal.
inline int plan( const float* pos, const float* nor, const int32_t* class_ids, const int32_t* instance_ids, int64_t n,
                 const int32_t* static_classes, int32_t n_static, const Plan& P, char* err, size_t err_cap )
{
  if( int rc = check_size( n, err, err_cap ) ) return rc;
  if( int rc = check_static( static_classes, n_static, err, err_cap ) ) return rc;
  if( n > 0 && ( !pos || !class_ids || !instance_ids ) ) return refuse( RS_HIP_E_ARG, err, err_cap, "split: positions, class ids and instance ids are required (%lld points)", (long long)n );
  if( n > 0 && P.out_nor && !nor ) return refuse( RS_HIP_E_ARG, err, err_cap, "split: normals asked for, none given (%lld points)", (long long)n );
  Table T;
  if( int rc = table( instance_ids, n, T, err, err_cap ) ) return rc;
  const int32_t I = (int32_t)T.ids.size();
  std::vector<int64_t> off( (size_t)I + 1, 0 );
  for( int32_t k = 0; k < I; ++k ) off[(size_t)k + 1] = off[(size_t)k] + T.counts[(size_t)k];
  std::vector<int32_t> order( (size_t)n );
  {
    std::unordered_map<int32_t, int32_t> rank;
    for( int32_t k = 0; k < I; ++k ) rank.emplace( T.ids[(size_t)k], k );
    std::vector<int64_t> at( off.begin(), off.end() - 1 );
    for( int64_t i = 0; i < n; ++i ) order[(size_t)at[(size_t)rank[instance_ids[i]]]++] = (int32_t)i;
  }
  if( P.n_instances ) *P.n_instances = I;
  for( int32_t k = 0; k < I; ++k )
  {
    const int64_t b = off[(size_t)k], e = off[(size_t)k + 1];
    const int32_t cls = class_ids[T.first[(size_t)k]];                            // main.cpp:114
    const bool st = class_is_static( cls, static_classes, n_static );
    double c[3] = { 0, 0, 0 };                                                    // rs_pointcloud.h:1326-1332
    for( int64_t j = b; j < e; ++j )
    {
      const float* p = pos + 3 * (size_t)order[(size_t)j];
      c[0] += p[0]; c[1] += p[1]; c[2] += p[2];
    }
    float cen[3], X[16], Q[16];
    finish_object( c, e - b, st, cen, X, Q );
    if( P.inst_ids ) P.inst_ids[k] = T.ids[(size_t)k];
    if( P.counts ) P.counts[k] = T.counts[(size_t)k];
    if( P.first ) P.first[k] = T.first[(size_t)k];
    if( P.class_of ) P.class_of[k] = cls;
    if( P.is_static ) P.is_static[k] = st ? 1 : 0;
    if( P.sums ) std::memcpy( P.sums + 3 * (size_t)k, c, 24 );
    if( P.centroids ) std::memcpy( P.centroids + 3 * (size_t)k, cen, 12 );
    if( P.xforms ) std::memcpy( P.xforms + 16 * (size_t)k, X, 64 );
    if( P.poses ) std::memcpy( P.poses + 16 * (size_t)k, Q, 64 );
    for( int64_t j = b; j < e && ( P.out_pos || P.out_nor ); ++j )
    {
      const size_t s = 3 * (size_t)order[(size_t)j], d = 3 * (size_t)j;
      if( P.out_pos ) { if( st ) std::memcpy( P.out_pos + d, pos + s, 12 ); else xform3( X, pos + s, 1.0f, P.out_pos + d ); }
      if( P.out_nor ) { if( st ) std::memcpy( P.out_nor + d, nor + s, 12 ); else xform3( X, nor + s, 0.0f, P.out_nor + d ); }
    }
  }
  if( P.offsets ) for( int32_t k = 0; k <= I; ++k ) P.offsets[k] = off[(size_t)k];
  if( P.order && n > 0 ) std::memcpy( P.order, order.data(), (size_t)n * 4 );
  return RS_HIP_OK;
}

// The device route's table and stable partition for a caller in another unit (rs_fuse.hip: the arrangement call), defined in
// rs_split.hip: the n >= 1 ids (host) are uploaded once; T is the table in order of first appearance, offsets its n_instances + 1
// segment starts, and *order (device, n entries, the unit's workspace: valid until the thread's next split call) holds segment k at
// [offsets[k], offsets[k + 1]) — by contract what rs_hip_select_by_ids returns for T.ids[k].  RS_HIP_E_CAPACITY above MAX_INSTANCES.
int segments_device( const int32_t* instance_ids, int n, Table& T, std::vector<int64_t>& offsets, const int32_t** order, ihipStream_t* st );

} // namespace split
} // namespace rs
