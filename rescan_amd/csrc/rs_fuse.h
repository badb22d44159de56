// Host planner of the model fusion that closes a timestep (rsdu_augment_database, apps/segment_transfer/database_update.cpp:22-91):
// the permutation of rs_pointcloud_merge's shuffle (lib/rs/rs_pointcloud.h:427-442), the jump-ahead table that lets the device
// make the same permutation, and the refusals that are decided before a launch.  Plain C++, no HIP: rs_fuse.hip includes it for
// the device calls, and a stand-alone program can include it alone.
//
// The shuffle is a Fisher-Yates pass from the back: for i = n-1 .. 1, j = (int32_t)( msh_rand_nextf() * i ) — an fp32 product —
// and elements i and j change places.  Its permutation depends on n and the seed alone, never on the points.  Up to n = 2^24
// (float)i is exact and j < i for every draw (the largest value msh_rand_nextf can return is 1 - 2^-23); beyond it the
// reference's j can exceed i, so larger merges are refused.
//
// The generator is rs_mesh.h's PCG32; only the jump table is made here, because its add[] column depends on the seed.
#pragma once

#include "rs_mesh.h"

#include <algorithm>

namespace rs {
namespace fuse {

constexpr int64_t MAX_POINTS = 1ll << 24;
constexpr int64_t MAX_TOTAL = 2147483646ll;   // all placements of one segmented call together: an int32 index names every element
constexpr uint32_t SEED_MERGE = 12346u;       // rs_pointcloud.h:428
constexpr int JUMP_BITS = 24;                 // step i uses draw n-1-i <= 2^24 - 2

// 2^k steps of the seeded generator: s -> mul[k] s + add[k] (rs_mesh.h: jump-ahead)
struct JumpTable
{
  uint64_t mul[JUMP_BITS], add[JUMP_BITS];
  uint64_t state;                             // the state after seeding
};
inline JumpTable jump_table( uint32_t seed )
{
  JumpTable t;
  const mesh::Pcg g = mesh::pcg_seed( seed );
  uint64_t m = mesh::PCG_MUL, a = g.inc;
  for( int k = 0; k < JUMP_BITS; ++k ) { t.mul[k] = m; t.add[k] = a; a *= m + 1; m *= m; }
  t.state = g.state;
  return t;
}

inline float unit_float( uint32_t u )        // msh_rand__float_normalized_from_u32, msh_std.h:1412-1421
{
  const uint32_t b = ( 127u << 23 ) | ( u >> 9 );
  float f; std::memcpy( &f, &b, 4 );
  return f - 1.0f;
}

inline int refuse( int rc, char* err, size_t err_cap, const char* what, long long v )
{
  if( err && err_cap ) snprintf( err, err_cap, what, v );
  return rc;
}
// the size of a merge: judged the same way by every entry point
inline int check_size( int64_t n, char* err, size_t err_cap )
{
  if( n < 0 ) return refuse( RS_HIP_E_ARG, err, err_cap, "fuse: %lld points: a count cannot be negative", (long long)n );
  if( n > MAX_POINTS ) return refuse( RS_HIP_E_CAPACITY, err, err_cap, "fuse: %lld points: beyond 2^24 the reference's shuffle can draw j > i", (long long)n );
  return RS_HIP_OK;
}
// rs_pointcloud_copy_by_ids emits a point once per matching entry of ids (rs_pointcloud.h:273-289); a repeated id is refused
inline int check_ids( const int32_t* ids, int32_t n_ids, char* err, size_t err_cap )
{
  if( n_ids < 0 || ( n_ids > 0 && !ids ) ) return refuse( RS_HIP_E_ARG, err, err_cap, "fuse: a list of %lld ids without its array, or of negative length", (long long)n_ids );
  std::vector<int32_t> s( ids, ids + n_ids );
  std::sort( s.begin(), s.end() );
  for( size_t k = 1; k < s.size(); ++k )
    if( s[k] == s[k - 1] ) return refuse( RS_HIP_E_ARG, err, err_cap, "fuse: id %lld is listed twice (the reference would emit its points twice)", (long long)s[k] );
  return RS_HIP_OK;
}

// perm[i]: the index, in the concatenation "A then B", of the element the shuffle leaves at position i (n entries).
inline int shuffle_plan( int64_t n, uint32_t seed, int32_t* perm, char* err, size_t err_cap )
{
  if( int rc = check_size( n, err, err_cap ) ) return rc;
  if( n > 0 && !perm ) return refuse( RS_HIP_E_ARG, err, err_cap, "fuse: no array for the %lld entries of the permutation", (long long)n );
  for( int64_t i = 0; i < n; ++i ) perm[i] = (int32_t)i;
  mesh::Pcg g = mesh::pcg_seed( seed );
  for( int32_t i = (int32_t)n - 1; i > 0; i-- )
  {
    const int32_t j = (int32_t)( unit_float( mesh::pcg_next( g ) ) * (float)i );
    std::swap( perm[i], perm[j] );
  }
  return RS_HIP_OK;
}

} // namespace fuse
} // namespace rs
