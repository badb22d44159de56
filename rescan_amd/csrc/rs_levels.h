// Host planner of the batched level builder (rs_levels.hip): all requested levels of many clouds decided side by side.  The reference
// samples every level from level 0 (lib/rs/rs_pointcloud.h:989-1011, :1305-1315), so level l of cloud c is a problem of its own on the
// points of cloud c: the lexicographically first maximal independent set of the "within radii[l]" graph (rs_rows.hip: k_level_*).
// Plain C++, no HIP: rs_levels.hip includes it for the device route, and a stand-alone program can include it alone.
//
// What the plan decides:
//   levels   sorted by radius, ascending and stable (equal radii keep the caller's order); radius_sq is the float of the double
//            product, as every search of the library takes it (msh_hash_grid.h:1104,1111 + :828).  order[s] is the caller's level
//            at sorted position s, rank[l] the sorted position of the caller's level l.
//   ids      the points of all clouds are numbered in one row, cloud after cloud in original order: pfirst[c] + original index.
//            Problem p = c * n_levels + l owns the global ids gfirst[p] + original index, gfirst[p] = rank[l] * n_points + pfirst[c]:
//            the ids of one sorted level lie together, and id / n_points is the level, id % n_points the point.
//   tiles    tile_first[c]: the first launch tile of cloud c, a prefix sum of the clouds' n_tiles; a wave of the neighbour sweep
//            finds its cloud by a search of this table.
//   refusals before any launch, see plan().
//   groups   after the counting pass: the clouds cut into consecutive groups whose adjacency entries fit ENTRY_BUDGET (groups()).
//   lanes    per sorted level, from its average row length, the lanes that walk one frontier item (lane_class()).
#pragma once

#include "../../include/rescan_hip.h"

#include <algorithm>
#include <cstdio>
#include <vector>

namespace rs {
namespace levels {

constexpr int32_t MAX_LEVELS = 8;                       // the reference has five levels, four of them sampled
constexpr int32_t MAX_PROBLEMS = 32768;                 // n_clouds * n_levels
// A frontier item is (global id << 1) | flag in an int, so ids stop at 2^30 - 1; a state word keeps LEVEL_COVERED = 2^30 above its
// count, which stays below a cloud's size.  Sum over the bases of (points x n_levels) may not pass this.
constexpr int64_t MAX_IDS = 1ll << 30;
// adjacency entries (4 bytes each) the unit holds for one group of clouds: 1 GiB.  Row offsets are 32-bit within a group.
constexpr int64_t ENTRY_BUDGET = 1ll << 28;
constexpr int64_t ENTRY_MAX = 4294967295ll;             // a cloud that alone passes the budget runs alone, up to what a uint32 offset names
// A base of more points than this takes rs_hip_level_samples' own path inside the call (the result is the same by contract).  The
// constant started at the index build's 499 999 (rs_hip_cloud_many_single_above) and is where the timing put it
// (profiles/r27/levels_many_timing.txt): at 1 000 000 points the batch beats the loop of single calls by 1-7 % for one base and by
// 9-13 % for two bases on levels (4, 3, 2), and trails it by 5-7 % for two bases on levels 1-4; routed to the single path (the same
// file, the library built with 499 999) those bases trailed it by 4-7 % in three of the four cases.  Nothing larger was measured,
// so nothing larger is batched: that also bounds the unit's workspace.
#ifndef RS_LEVELS_SINGLE_ABOVE          // (tools/variant.sh: a library with another constant, for tools/levels_many_timing.py)
#define RS_LEVELS_SINGLE_ABOVE 1000000
#endif
constexpr int32_t SINGLE_ABOVE = RS_LEVELS_SINGLE_ABOVE;

inline float radius_sq_of( float r ) { return (float)( (double)r * (double)r ); }

// lanes per frontier item from a level's average row length: the cuts rs_hip_level_samples takes per call
inline int lane_class( double avg_row ) { return avg_row >= 24.0 ? 64 : ( avg_row >= 3.0 ? 8 : 1 ); }

struct LevelsPlan
{
  int32_t n_clouds = 0, n_levels = 0;
  int32_t order[MAX_LEVELS] = {}, rank[MAX_LEVELS] = {}, cap[MAX_LEVELS] = {};       // order / cap by sorted position, rank by caller's level
  float   radius[MAX_LEVELS] = {}, radius_sq[MAX_LEVELS] = {};                       // by sorted position
  int64_t n_points = 0, n_ids = 0, n_tiles = 0;
  std::vector<int32_t> pfirst, tile_first;              // n_clouds + 1
  std::vector<int32_t> gfirst;                          // n_clouds * n_levels, problem c * n_levels + l (caller's l)
};

inline int refuse( int rc, char* err, size_t err_cap, const char* what, long long a = 0, long long b = 0 )
{
  if( err && err_cap ) snprintf( err, err_cap, what, a, b );
  return rc;
}

// sizes[c] < 0 stands for a NULL base.  Nothing of P is to be used after a refusal.
inline int plan( const int32_t* sizes, const int32_t* n_tiles, int32_t n_clouds, const float* radii, const int32_t* max_n_neigh, int32_t n_levels,
                 LevelsPlan& P, char* err, size_t err_cap )
{
  P = LevelsPlan();
  if( n_clouds < 0 || n_levels < 0 ) return refuse( RS_HIP_E_ARG, err, err_cap, "levels_many: %lld clouds, %lld levels: a count cannot be negative", n_clouds, n_levels );
  if( n_levels > MAX_LEVELS ) return refuse( RS_HIP_E_ARG, err, err_cap, "levels_many: %lld levels, at most %lld in one call", n_levels, MAX_LEVELS );
  if( (int64_t)n_clouds * n_levels > MAX_PROBLEMS ) return refuse( RS_HIP_E_ARG, err, err_cap, "levels_many: %lld problems, at most %lld in one call", (long long)n_clouds * n_levels, MAX_PROBLEMS );
  P.n_clouds = n_clouds; P.n_levels = n_levels;
  if( n_clouds == 0 || n_levels == 0 ) return RS_HIP_OK;
  if( !sizes || !n_tiles || !radii || !max_n_neigh ) return refuse( RS_HIP_E_ARG, err, err_cap, "levels_many: the bases, radii and caps are required" );
  for( int32_t l = 0; l < n_levels; ++l )
  {
    if( !( radii[l] > 0.0f ) ) return refuse( RS_HIP_E_ARG, err, err_cap, "levels_many: level %lld: the radius must be > 0", l );
    if( max_n_neigh[l] <= 0 ) return refuse( RS_HIP_E_ARG, err, err_cap, "levels_many: level %lld: max_n_neigh = %lld must be > 0", l, max_n_neigh[l] );
  }
  for( int32_t c = 0; c < n_clouds; ++c )
    if( sizes[c] < 0 ) return refuse( RS_HIP_E_ARG, err, err_cap, "levels_many: cloud %lld is NULL", c );
  for( int32_t l = 0; l < n_levels; ++l ) P.order[l] = l;
  std::stable_sort( P.order, P.order + n_levels, [&]( int32_t a, int32_t b ) { return radii[a] < radii[b]; } );
  for( int32_t s = 0; s < n_levels; ++s )
  {
    const int32_t l = P.order[s];
    P.rank[l] = s; P.radius[s] = radii[l]; P.radius_sq[s] = radius_sq_of( radii[l] ); P.cap[s] = max_n_neigh[l];
  }
  P.pfirst.assign( (size_t)n_clouds + 1, 0 ); P.tile_first.assign( (size_t)n_clouds + 1, 0 );
  int64_t points = 0, tiles = 0;
  for( int32_t c = 0; c < n_clouds; ++c )
  {
    points += sizes[c]; tiles += n_tiles[c];
    if( points * n_levels > MAX_IDS )
      return refuse( RS_HIP_E_CAPACITY, err, err_cap, "levels_many: %lld points x levels up to cloud %lld: more than the 2^30 ids a frontier item can name", points * n_levels, c );
    P.pfirst[(size_t)c + 1] = (int32_t)points; P.tile_first[(size_t)c + 1] = (int32_t)tiles;
  }
  P.n_points = points; P.n_ids = points * n_levels; P.n_tiles = tiles;
  P.gfirst.resize( (size_t)n_clouds * n_levels );
  for( int32_t c = 0; c < n_clouds; ++c )
    for( int32_t l = 0; l < n_levels; ++l )
      P.gfirst[(size_t)c * n_levels + l] = (int32_t)( (int64_t)P.rank[l] * points + P.pfirst[c] );
  return RS_HIP_OK;
}

// Consecutive units cut into groups whose totals together stay within the budget; a unit that alone passes it is a group of its own.
// gend[g]: one past the last unit of group g.  Returns the number of groups (0 for no units).
inline int groups( const int64_t* totals, int32_t n, int64_t budget, std::vector<int32_t>& gend )
{
  gend.clear();
  int64_t sum = 0; int32_t first = 0;
  for( int32_t k = 0; k < n; ++k )
  {
    if( k > first && sum + totals[k] > budget ) { gend.push_back( k ); first = k; sum = 0; }
    sum += totals[k];
  }
  if( n > 0 ) gend.push_back( n );
  return (int)gend.size();
}

} // namespace levels
} // namespace rs
