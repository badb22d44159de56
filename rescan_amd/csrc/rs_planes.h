// Host planner of the plane detector (rspf__detect_floor / rspf__detect_walls, lib/rs/rs_pointcloud_filters.cpp:136-252): the
// sampler that draws a round's point triples and the arithmetic that turns a triple into a plane hypothesis.  Plain C++, no HIP:
// rs_planes.hip includes it for the device calls, and a stand-alone program can include it alone.
//
// The sampler is msh_discrete_distribution_init / _sample (lib/msh/msh_std.h:1863-1941) over weights that are 1.0 for a candidate
// point and 0.0 for every other: rs_mesh.h's alias table and PCG32, seeded anew for every round (:153-154, :216-217).  One sample
// takes two draws.  The floor takes three samples per hypothesis; the walls redraw b while b == a and c while c == b (:162-164), so
// how many draws a round takes depends on the data, and the loop is sequential.
#pragma once

#include "rs_mesh.h"

namespace rs {
namespace planes {

constexpr int64_t MAX_POINTS = 1ll << 24;     // (float)n is exact up to here: msh_rand_range's column stays below n
constexpr uint32_t SEED = 12346u;             // rs_pointcloud_filters.cpp:154,217

inline float unit_float( uint32_t u )        // msh_rand__float_normalized_from_u32, msh_std.h:1412-1421
{
  const uint32_t b = ( 127u << 23 ) | ( u >> 9 );
  float f; std::memcpy( &f, &b, 4 );
  return f - 1.0f;
}
inline float abs_ref( float x ) { return x < 0 ? -x : x; }                                  // msh_abs, msh_std.h:633
// msh_vec3_dot( v, msh_vec3_posy() ): the zero products stay, so that a NaN or infinite x or z gives NaN as it does there
inline float up_dot( const float v[3] ) { return v[0] * 0.0f + v[1] * 1.0f + v[2] * 0.0f; }

inline int refuse( int rc, char* err, size_t err_cap, const char* what, long long v )
{
  if( err && err_cap ) snprintf( err, err_cap, what, v );
  return rc;
}

struct Sampler
{
  std::vector<double> prob;
  std::vector<int32_t> alias;
  mesh::Pcg g;
  int32_t n;
  int64_t n_active;
};

// msh_discrete_distribution_init over weights[i] = active[i] ? 1.0 : 0.0
inline int sampler_init( Sampler& S, const uint8_t* active, int64_t n, uint32_t seed, char* err, size_t err_cap )
{
  if( n < 0 || ( n > 0 && !active ) ) return refuse( RS_HIP_E_ARG, err, err_cap, "planes: %lld points without a mask, or a negative count", (long long)n );
  if( n > MAX_POINTS ) return refuse( RS_HIP_E_CAPACITY, err, err_cap, "planes: %lld points: beyond 2^24 the reference's (float)n is inexact and its column can reach n", (long long)n );
  double total = 0;
  for( int64_t i = 0; i < n; ++i ) total += active[i] ? 1.0 : 0.0;
  // msh_distrib2pdf (msh_std.h:1843-1849): the sum comes back as a float; at or below 1e-8 the pdf stays unwritten
  const double sum = (double)(float)total;
  if( sum <= 0.00000001 ) return refuse( RS_HIP_E_ARG, err, err_cap, "planes: no candidate among %lld points: the reference's pdf would stay uninitialised", (long long)n );
  const double inv_sum = 1.0 / sum;
  std::vector<double> pdf( (size_t)n );
  for( int64_t i = 0; i < n; ++i ) pdf[(size_t)i] = ( active[i] ? 1.0 : 0.0 ) * inv_sum;
  S.prob.assign( (size_t)n, 0.0 ); S.alias.assign( (size_t)n, 0 );
  mesh::alias_table( pdf.data(), (size_t)n, S.prob.data(), S.alias.data() );
  S.g = mesh::pcg_seed( seed );
  S.n = (int32_t)n; S.n_active = (int64_t)total;
  return RS_HIP_OK;
}
// msh_discrete_distribution_sample (msh_std.h:1935-1941); msh_rand_range's product is fp32 (:1468)
inline int32_t sample( Sampler& S )
{
  const int32_t column = (int32_t)( unit_float( mesh::pcg_next( S.g ) ) * (float)S.n );
  const bool coin = (double)unit_float( mesh::pcg_next( S.g ) ) < S.prob[(size_t)column];
  return coin ? column : S.alias[(size_t)column];
}

// center = p_a, normal = normalize( cross( p_b - p_a, p_c - p_a ) ) (:166-175; msh_vec_math.h:868,974): fp32, no contraction.
// A degenerate triple gives NaN.
inline void hypothesis( const float* pos, const int32_t t[3], float center[3], float normal[3] )
{
  const float* a = pos + 3 * (size_t)t[0], *b = pos + 3 * (size_t)t[1], *c = pos + 3 * (size_t)t[2];
  const float va[3] = { b[0] - a[0], b[1] - a[1], b[2] - a[2] }, vb[3] = { c[0] - a[0], c[1] - a[1], c[2] - a[2] };
  const float x = va[1] * vb[2] - va[2] * vb[1], y = va[2] * vb[0] - va[0] * vb[2], z = va[0] * vb[1] - va[1] * vb[0];
  const float denom = 1.0f / sqrtf( x * x + y * y + z * z );
  center[0] = a[0]; center[1] = a[1]; center[2] = a[2];
  normal[0] = x * denom; normal[1] = y * denom; normal[2] = z * denom;
}

// One round's n_iter triples and (each where asked for) their centres and normals.  distinct: the walls' redraws.
inline int hypotheses( const float* pos, int64_t n, const uint8_t* active, int32_t n_iter, int32_t distinct, uint32_t seed,
                       int32_t* idx, float* center, float* normal, char* err, size_t err_cap )
{
  if( !pos || !active || n < 0 || n_iter < 0 || ( n_iter > 0 && !idx ) )
    return refuse( RS_HIP_E_ARG, err, err_cap, "planes: null arrays or a negative count (%lld points)", (long long)n );
  Sampler S;
  if( int rc = sampler_init( S, active, n, seed, err, err_cap ) ) return rc;
  if( distinct && S.n_active < 2 )
    return refuse( RS_HIP_E_ARG, err, err_cap, "planes: %lld wall candidate: the reference's redraw loop would never end", (long long)S.n_active );
  for( int32_t h = 0; h < n_iter; ++h )
  {
    int32_t* t = idx + 3 * (size_t)h;
    t[0] = sample( S );
    if( distinct )
    {
      do { t[1] = sample( S ); } while( t[0] == t[1] );
      do { t[2] = sample( S ); } while( t[1] == t[2] );
    }
    else { t[1] = sample( S ); t[2] = sample( S ); }
    float c[3], nn[3];
    hypothesis( pos, t, c, nn );
    if( center ) std::memcpy( center + 3 * (size_t)h, c, 12 );
    if( normal ) std::memcpy( normal + 3 * (size_t)h, nn, 12 );
  }
  return RS_HIP_OK;
}

// The quad of rspf__gather_model_inliers (:288-296) from a model's centre, column-major axes and extends
inline void quad( const float c[3], const float axes[9], const float ext[4], float poly[12] )
{
  float px[3], py[3], nx[3], ny[3];
  for( int k = 0; k < 3; ++k ) { px[k] = axes[k] * ext[0]; py[k] = axes[3 + k] * ext[1]; nx[k] = axes[k] * ext[2]; ny[k] = axes[3 + k] * ext[3]; }
  for( int k = 0; k < 3; ++k )
  {
    poly[k] = ( c[k] + px[k] ) + py[k];
    poly[3 + k] = ( c[k] + px[k] ) + ny[k];
    poly[6 + k] = ( c[k] + nx[k] ) + ny[k];
    poly[9 + k] = ( c[k] + nx[k] ) + py[k];
  }
}

} // namespace planes
} // namespace rs
