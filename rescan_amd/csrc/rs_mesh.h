// Host planner of the uniform mesh resampler (rs_pointcloud_uniform_resample, lib/rs/rs_pointcloud.h:1132-1227).
//
// Everything of the reference's call that is sequential or decided before the first sample: the face areas and their
// double sum (:1143-1154), the sample count (:1157-1158), the alias table of msh_discrete_distribution_init
// (lib/msh/msh_std.h:1843-1849,1863-1925), the two PCG32 generators' seeding (msh_std.h:1423-1455) and the jump-ahead
// table that turns "the state before sample i" into a function of i.  Plain C++, no HIP: rs_mesh.hip includes it for the
// device call, and a stand-alone program can include it alone.
#pragma once

#include "../../include/rescan_hip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace rs {
namespace mesh {

constexpr int64_t MAX_FACES = 1ll << 24;      // (float)n_faces is exact up to here: the alias column stays below n_faces
constexpr uint32_t SEED_BARYCENTRIC = 12346u; // rs_pointcloud.h:1135-1137, seeds[0]
constexpr uint32_t SEED_ALIAS = 64321u;       // rs_pointcloud.h:1135,1160, seeds[1] (size_t -> uint32_t at msh_std.h:1920)
constexpr uint64_t PCG_MUL = 0x5851f42d4c957f2dULL;
constexpr int JUMP_BITS = 40;                 // 2 * i < 2^32 for i <= INT32_MAX; some room above

// ---- PCG32 (msh_std.h:1413-1470) ----------------------------------------------------------------------------------

struct Pcg { uint64_t state, inc; };

inline uint64_t murmur3_avalanche64( uint64_t h )      // msh_std.h:1423-1432
{
  h ^= h >> 33; h *= 0xff51afd7ed558ccdULL; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ULL; h ^= h >> 33;
  return h;
}
inline uint32_t pcg_next( Pcg& g )                      // msh_std.h:1447-1455
{
  const uint64_t old = g.state;
  g.state = old * PCG_MUL + g.inc;
  const uint32_t xorshifted = (uint32_t)( ( ( old >> 18 ) ^ old ) >> 27 );
  const uint32_t rot = (uint32_t)( old >> 59 );
  return ( xorshifted >> rot ) | ( xorshifted << ( ( 0u - rot ) & 31u ) );
}
inline Pcg pcg_seed( uint32_t seed )                    // msh_rand_init, msh_std.h:1434-1444
{
  uint64_t value = ( ( (uint64_t)seed ) << 1 ) | 1ULL;
  value = murmur3_avalanche64( value );
  Pcg g{ 0, ( value << 1 ) | 1ULL };
  pcg_next( g );
  g.state += murmur3_avalanche64( value );
  pcg_next( g );
  return g;
}

// Jump-ahead.  One step of the generator is the affine map s -> A s + c (mod 2^64); 2^k steps are s -> mul[k] s + add[k]
// with mul[k+1] = mul[k]^2 and add[k+1] = add[k] (mul[k] + 1).  All of these are powers of one map, so they commute: the
// state n steps on is the product over the set bits of n, in any order.  The sampler draws exactly two numbers per sample
// from each generator (rs_pointcloud.h:1118-1119, msh_std.h:1938-1939), so sample i starts 2 i steps after the seeding.
// Both generators share the multiplier; only the increments differ.
struct JumpTable
{
  uint64_t mul[JUMP_BITS];
  uint64_t add[2][JUMP_BITS];        // [0]: the alias sampler's generator, [1]: the barycentric one
  uint64_t state[2];                 // the states after seeding
};
inline JumpTable jump_table()
{
  JumpTable t;
  const Pcg g[2] = { pcg_seed( SEED_ALIAS ), pcg_seed( SEED_BARYCENTRIC ) };
  uint64_t m = PCG_MUL, a0 = g[0].inc, a1 = g[1].inc;
  for( int k = 0; k < JUMP_BITS; ++k )
  {
    t.mul[k] = m; t.add[0][k] = a0; t.add[1][k] = a1;
    a0 *= m + 1; a1 *= m + 1; m *= m;
  }
  t.state[0] = g[0].state; t.state[1] = g[1].state;
  return t;
}
inline uint64_t jump( const JumpTable& t, int which, uint64_t steps )
{
  uint64_t s = t.state[which];
  for( int k = 0; k < JUMP_BITS; ++k ) if( ( steps >> k ) & 1 ) s = s * t.mul[k] + t.add[which][k];
  return s;
}

// ---- areas, sample count, alias table ------------------------------------------------------------------------------

// The alias table of msh_discrete_distribution_update (msh_std.h:1871-1910) over a pdf of n entries, which it consumes.  An alias
// entry the reference never writes (prob = 1.0 leftovers, :1899-1910; malloc'ed and unread there) holds its own index.  Shared
// by the resampler's plan below and the plane detector's sampler (rs_planes.h).
inline void alias_table( double* pdf, size_t n, double* prob, int32_t* alias )
{
  const double avg = 1.0 / (double)n;
  // The two stacks together never hold more than n entries (every entry starts on one; a round pops two and pushes one),
  // so n slots each are enough.
  std::vector<int32_t> small( n ), large( n );
  size_t n_small = 0, n_large = 0;
  for( size_t i = 0; i < n; ++i )
  {
    alias[i] = (int32_t)i;
    if( pdf[i] >= avg ) large[n_large++] = (int32_t)i; else small[n_small++] = (int32_t)i;
  }
  while( n_small && n_large )
  {
    const int32_t l = small[--n_small], g = large[--n_large];
    prob[l] = pdf[l] * (double)n;
    alias[l] = g;
    pdf[g] = ( pdf[g] + pdf[l] ) - avg;
    if( pdf[g] >= avg ) large[n_large++] = g; else small[n_small++] = g;
  }
  while( n_small ) prob[small[--n_small]] = 1.0;
  while( n_large ) prob[large[--n_large]] = 1.0;
}

// n_samples, total_area and (where asked for: prob and alias may each be null) the alias table of the
// reference's call.  Returns RS_HIP_OK or the refusal's code with its text in err.
inline int plan( const float* pos, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                 int64_t* n_samples, double* total_area, double* prob, int32_t* alias, char* err, size_t err_cap )
{
#define RS_MESH_REFUSE( rc, ... ) do { if( err && err_cap ) snprintf( err, err_cap, __VA_ARGS__ ); return rc; } while( 0 )
  if( !pos || !faces || n_vertices < 0 ) RS_MESH_REFUSE( RS_HIP_E_ARG, "resample: null mesh arrays or a negative vertex count" );
  if( n_faces <= 0 ) RS_MESH_REFUSE( RS_HIP_E_ARG, "resample: %lld faces: a mesh needs at least one", (long long)n_faces );
  if( n_faces > MAX_FACES ) RS_MESH_REFUSE( RS_HIP_E_CAPACITY, "resample: %lld faces: beyond 2^24 the reference's (float)n_faces is inexact and its alias column can reach n_faces", (long long)n_faces );
  for( int64_t i = 0; i < 3 * n_faces; ++i )
    if( faces[i] < 0 || faces[i] >= n_vertices )
      RS_MESH_REFUSE( RS_HIP_E_ARG, "resample: face %lld names vertex %d, outside [0, %lld)", (long long)( i / 3 ), faces[i], (long long)n_vertices );

  // :1143-1154: fp32 edge vectors and cross product, norm as (float)sqrt( fp32 sum ), areas and their sum in double
  std::vector<double> areas( (size_t)n_faces );
  double total = 0;
  for( int64_t i = 0; i < n_faces; ++i )
  {
    const float* a = pos + 3 * (size_t)faces[3 * i], *b = pos + 3 * (size_t)faces[3 * i + 1], *c = pos + 3 * (size_t)faces[3 * i + 2];
    const float v1[3] = { b[0] - a[0], b[1] - a[1], b[2] - a[2] }, v2[3] = { c[0] - a[0], c[1] - a[1], c[2] - a[2] };
    const float x = v1[1] * v2[2] - v1[2] * v2[1], y = v1[2] * v2[0] - v1[0] * v2[2], z = v1[0] * v2[1] - v1[1] * v2[0];   // msh_vec_math.h:974
    const float sq = x * x + y * y + z * z;
    const double cur = (float)std::sqrt( (double)sq );                                                                 // msh_vec_math.h:988
    total += cur;
    areas[(size_t)i] = cur;
  }
  if( !std::isfinite( total ) ) RS_MESH_REFUSE( RS_HIP_E_ARG, "resample: the total area is not finite" );
  // msh_distrib2pdf (msh_std.h:1843-1849) normalises by msh_accumulated, which returns float: the same sequential double
  // sum, rounded to fp32 and widened again.  At or below 1e-8 it returns with the pdf unwritten and the reference samples
  // from uninitialised memory.
  const double sum = (double)(float)total;
  if( sum <= 0.00000001 ) RS_MESH_REFUSE( RS_HIP_E_ARG, "resample: the area sum %g is at or below 1e-8: the reference's pdf would stay uninitialised", sum );
  const double want = 0.5 * total * 12800.0;                               // :1157-1158
  if( want >= 2147483648.0 ) RS_MESH_REFUSE( RS_HIP_E_CAPACITY, "resample: %.0f samples exceed INT32_MAX", want );
  if( n_samples ) *n_samples = (int64_t)(size_t)want;
  if( total_area ) *total_area = total;
  if( !prob && !alias ) return RS_HIP_OK;

  // msh_discrete_distribution_update (msh_std.h:1863-1915)
  const size_t n = (size_t)n_faces;
  std::vector<double> pdf( n ), prob_own;
  std::vector<int32_t> alias_own;
  if( !prob ) { prob_own.resize( n ); prob = prob_own.data(); }
  if( !alias ) { alias_own.resize( n ); alias = alias_own.data(); }
  const double inv_sum = 1.0 / sum;
  for( size_t i = 0; i < n; ++i ) pdf[i] = areas[i] * inv_sum;
  alias_table( pdf.data(), n, prob, alias );
  return RS_HIP_OK;
#undef RS_MESH_REFUSE
}

} // namespace mesh
} // namespace rs
