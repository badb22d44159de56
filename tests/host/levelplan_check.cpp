// Stand-alone host program over rescan_amd/csrc/rs_levels.h (no HIP, no device): prints the plan of the batched level builder for a
// list of batches, one line each with its inputs, so that tests/test_levels_many_cpu.py can recompute every line in numpy.  Built
// and run under the address and undefined-behaviour sanitizers by that test.
#include "rs_levels.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace rs::levels;

static uint32_t bits( float f ) { uint32_t u; std::memcpy( &u, &f, 4 ); return u; }
template <class T> static void list( const char* name, const T* v, size_t n )
{
  printf( " %s=", name );
  for( size_t i = 0; i < n; ++i ) printf( "%s%lld", i ? "," : "", (long long)v[i] );
}

static void plan_line( const std::vector<int32_t>& sizes, const std::vector<float>& radii, const std::vector<int32_t>& caps )
{
  std::vector<int32_t> tiles( sizes.size() );
  for( size_t c = 0; c < sizes.size(); ++c ) tiles[c] = sizes[c] > 0 ? ( sizes[c] + 63 ) / 64 : 0;
  std::vector<uint32_t> rbits( radii.size() );
  for( size_t l = 0; l < radii.size(); ++l ) rbits[l] = bits( radii[l] );
  LevelsPlan P; char err[256] = "";
  const int rc = plan( sizes.data(), tiles.data(), (int32_t)sizes.size(), radii.data(), caps.data(), (int32_t)radii.size(), P, err, sizeof(err) );
  printf( "plan" );
  list( "sizes", sizes.data(), sizes.size() ); list( "tiles", tiles.data(), tiles.size() ); list( "radii", rbits.data(), rbits.size() ); list( "caps", caps.data(), caps.size() );
  printf( " -> rc=%d", rc );
  if( rc == 0 && !sizes.empty() && !radii.empty() )
  {
    uint32_t rsq[MAX_LEVELS], rad[MAX_LEVELS];
    for( int s = 0; s < P.n_levels; ++s ) { rsq[s] = bits( P.radius_sq[s] ); rad[s] = bits( P.radius[s] ); }
    list( "order", P.order, (size_t)P.n_levels ); list( "rank", P.rank, (size_t)P.n_levels ); list( "cap", P.cap, (size_t)P.n_levels );
    list( "radius", rad, (size_t)P.n_levels ); list( "rsq", rsq, (size_t)P.n_levels );
    list( "pfirst", P.pfirst.data(), P.pfirst.size() ); list( "tile_first", P.tile_first.data(), P.tile_first.size() ); list( "gfirst", P.gfirst.data(), P.gfirst.size() );
    printf( " n_points=%lld n_ids=%lld n_tiles=%lld", (long long)P.n_points, (long long)P.n_ids, (long long)P.n_tiles );
  }
  else if( rc ) printf( " err=\"%s\"", err );
  printf( "\n" );
}

static void groups_line( const std::vector<int64_t>& totals, int64_t budget )
{
  std::vector<int32_t> gend;
  const int ng = groups( totals.data(), (int32_t)totals.size(), budget, gend );
  printf( "groups" ); list( "totals", totals.data(), totals.size() );
  printf( " budget=%lld -> n=%d", (long long)budget, ng ); list( "gend", gend.data(), gend.size() );
  printf( "\n" );
}

int main()
{
  const std::vector<float> four = { 0.08f, 0.01f, 0.04f, 0.02f };
  const std::vector<int32_t> caps4 = { 1024, 256, 768, 512 };
  // level order: unsorted, sorted, equal radii (stable), all equal
  plan_line( { 1000 }, four, caps4 );
  plan_line( { 1000, 50, 7 }, { 0.01f, 0.02f, 0.04f, 0.08f }, { 256, 512, 768, 1024 } );
  plan_line( { 10, 20 }, { 0.02f, 0.01f, 0.02f, 0.01f }, { 1, 2, 3, 4 } );
  plan_line( { 10 }, { 0.5f, 0.5f, 0.5f }, { 3, 2, 1 } );
  plan_line( { 10 }, { 0.1f }, { 1 } );
  // the tile table and gfirst around a tile and a block
  plan_line( { 0, 1, 63, 64, 65, 255, 256, 257 }, four, caps4 );
  plan_line( { 257, 0, 0, 64, 0 }, { 0.04f, 0.02f }, { 768, 512 } );
  plan_line( { 0, 0 }, four, caps4 );
  // nothing to do
  plan_line( {}, four, caps4 );
  plan_line( { 5 }, {}, {} );
  // refusals at their bounds and one inside
  plan_line( { 5 }, std::vector<float>( 8, 0.25f ), std::vector<int32_t>( 8, 9 ) );
  plan_line( { 5 }, std::vector<float>( 9, 0.25f ), std::vector<int32_t>( 9, 9 ) );
  plan_line( std::vector<int32_t>( 4096, 1 ), std::vector<float>( 8, 0.25f ), std::vector<int32_t>( 8, 9 ) );      // 32768 problems
  plan_line( std::vector<int32_t>( 4097, 1 ), std::vector<float>( 8, 0.25f ), std::vector<int32_t>( 8, 9 ) );
  plan_line( { 5 }, { 0.0f }, { 9 } );
  plan_line( { 5 }, { -1.0f }, { 9 } );
  plan_line( { 5 }, { std::numeric_limits<float>::quiet_NaN() }, { 9 } );
  plan_line( { 5 }, { std::numeric_limits<float>::denorm_min() }, { 9 } );
  plan_line( { 5 }, { 1.0f, 0.0f }, { 9, 9 } );
  plan_line( { 5 }, { 1.0f }, { 0 } );
  plan_line( { 5 }, { 1.0f }, { -3 } );
  plan_line( { 5 }, { 1.0f }, { 1 } );
  plan_line( { 5, -1, 5 }, { 1.0f }, { 1 } );                                                                 // a NULL base
  plan_line( { 1 << 29, 1 << 29 }, { 1.0f }, { 1 } );                                                          // 2^30 ids
  plan_line( { 1 << 29, ( 1 << 29 ) + 1 }, { 1.0f }, { 1 } );
  plan_line( { 1 << 29 }, { 1.0f, 2.0f }, { 1, 1 } );
  plan_line( { ( 1 << 29 ) + 1 }, { 1.0f, 2.0f }, { 1, 1 } );
  plan_line( { 1 << 27 }, std::vector<float>( 8, 0.25f ), std::vector<int32_t>( 8, 9 ) );
  plan_line( { 1 << 27, 1 }, std::vector<float>( 8, 0.25f ), std::vector<int32_t>( 8, 9 ) );
  // groups around the budget
  const int64_t B = ENTRY_BUDGET;
  groups_line( {}, B );
  groups_line( { 5 }, B );
  groups_line( { B / 2, B / 2 - 1 }, B );                  // just under
  groups_line( { B / 2, B / 2 }, B );                      // exactly at
  groups_line( { B / 2, B / 2 + 1 }, B );                  // just over
  groups_line( { 1, B + 7, 1, 1 }, B );                    // one that alone passes it
  groups_line( { B + 7 }, B );
  groups_line( { B, B, B }, B );
  groups_line( { 0, 0, B, 0, 1, B - 1, 0 }, B );
  groups_line( { 3, 3, 3, 3, 3, 3, 3 }, 7 );
  // lane classes on both sides of each cut
  const double avgs[] = { 0.0, 1.0, std::nextafter( 3.0, 0.0 ), 3.0, 3.5, std::nextafter( 24.0, 0.0 ), 24.0, 100.0 };
  printf( "lanes" );
  for( double a : avgs ) printf( " %a:%d", a, lane_class( a ) );
  printf( "\n" );
  printf( "consts MAX_LEVELS=%d MAX_PROBLEMS=%d MAX_IDS=%lld ENTRY_BUDGET=%lld ENTRY_MAX=%lld SINGLE_ABOVE=%d\n", (int)MAX_LEVELS, (int)MAX_PROBLEMS, (long long)MAX_IDS,
          (long long)ENTRY_BUDGET, (long long)ENTRY_MAX, (int)SINGLE_ABOVE );
  printf( "levelplan_check ok\n" );
  return 0;
}
