// Stand-alone check of rescan_amd/csrc/rs_xcdmap.h, the tile map of phase A's natural part (k_icp_corr): for chunk sizes 2^0 .. 2^10
// and the contiguous eighths (k < 0), for 1 and 4 tiles per natural block, for block counts at every edge of a chunk and of a round
// of eight chunks, the workgroups of the grid — each taking its block exactly as the kernel does — must hit every tile of the problem
// once and nothing else below its end, every workgroup a block of its own XCD class b & 7, ascending within the class, under the
// problem's own grid and under a larger problem's.  Built with -fsanitize=address,undefined and run by tests/test_xcd_map_cpu.py.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I rescan_amd/csrc tests/host/xcdmap_check.cpp -o xcdmap_check
#include "rs_xcdmap.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

using namespace rs;

static long long g_checked = 0;

#define REQUIRE( c, ... ) do { if( !( c ) ) { fprintf( stderr, "xcdmap_check: %s:%d: %s failed: ", __FILE__, __LINE__, #c ); fprintf( stderr, __VA_ARGS__ ); fprintf( stderr, "\n" ); exit( 1 ); } } while( 0 )

// the map of rounds 1 to 19, restated from k_icp_corr as it stood: INT_MAX beyond the problem's own eighths
static int parent_tile( int block, int n_tiles, int pa_waves, int wib )
{
  const int per = ( ( n_tiles + pa_waves - 1 ) / pa_waves + 7 ) / 8;
  if( ( block >> 3 ) >= per ) return INT_MAX;
  return ( ( block & 7 ) * per + ( block >> 3 ) ) * pa_waves + wib;
}
static int parent_class( int tile, int n_tiles, int pa_waves )
{
  const int per = ( ( n_tiles + pa_waves - 1 ) / pa_waves + 7 ) / 8, c = ( tile / pa_waves ) / per;
  return c < 7 ? c : 7;
}

// a problem of n_tiles tiles under the natural part of a grid sized for grid_tiles >= n_tiles tiles
static void check_problem( int n_tiles, int grid_tiles, int k, int pa_waves )
{
  const int nb = xm_blocks( n_tiles, pa_waves ), grid = xm_grid( xm_blocks( grid_tiles, pa_waves ), k );
  REQUIRE( nb * pa_waves >= n_tiles && ( nb - 1 ) * pa_waves < n_tiles, "n_tiles %d, %d waves: %d blocks", n_tiles, pa_waves, nb );
  REQUIRE( grid % 8 == 0 && grid >= nb && grid >= xm_grid( nb, k ), "k %d, %d blocks under %d tiles' grid: grid %d", k, nb, grid_tiles, grid );
  if( k >= 0 ) REQUIRE( grid % ( 8 << k ) == 0 && grid - xm_blocks( grid_tiles, pa_waves ) < ( 8 << k ), "k %d: grid %d is not the blocks rounded up to eight chunks", k, grid );
  // heap arrays of exactly the problem's size: the sanitizer sees any index past them
  std::vector<unsigned char> hit( (size_t)n_tiles, 0 );
  int last[8] = { -1, -1, -1, -1, -1, -1, -1, -1 };
  for( int b = 0; b < grid; ++b )
  {
    const bool beyond = xm_beyond( b, nb, k );
    const int block = beyond ? INT_MAX : xm_block( b, nb, k );
    REQUIRE( block >= 0, "k %d, nb %d: workgroup %d takes block %d", k, nb, b, block );
    if( k >= 0 ) REQUIRE( beyond == ( xm_block( b, nb, k ) >= nb ) && xm_block( b, nb, k ) < grid, "k %d, nb %d: workgroup %d, block %d of a grid of %d, beyond %d", k, nb, b, xm_block( b, nb, k ), grid, (int)beyond );
    for( int wib = 0; wib < pa_waves; ++wib )
    {
      // the kernel's natural_tile
      const int tile = beyond ? INT_MAX : block * pa_waves + wib;
      if( k < 0 ) REQUIRE( tile == parent_tile( b, n_tiles, pa_waves, wib ), "k %d, %d tiles: workgroup %d wave %d takes tile %d, the contiguous eighths give %d", k, n_tiles, b, wib, tile, parent_tile( b, n_tiles, pa_waves, wib ) );
      if( tile >= n_tiles ) { REQUIRE( block >= nb || block == nb - 1, "k %d, nb %d: workgroup %d's block %d is the problem's, its tile %d is not", k, nb, b, block, tile ); continue; }
      REQUIRE( block < nb, "k %d, nb %d: tile %d of block %d", k, nb, tile, block );
      REQUIRE( !hit[(size_t)tile], "k %d, %d tiles: tile %d taken twice (again by workgroup %d)", k, n_tiles, tile, b );
      hit[(size_t)tile] = 1;
      const int cls = xm_class( tile / pa_waves, nb, k );
      REQUIRE( cls == ( b & 7 ), "k %d, %d tiles: workgroup %d (class %d) takes tile %d of class %d", k, n_tiles, b, b & 7, tile, cls );
      if( k < 0 ) REQUIRE( cls == parent_class( tile, n_tiles, pa_waves ), "k %d, %d tiles: tile %d in class %d, the contiguous eighths say %d", k, n_tiles, tile, cls, parent_class( tile, n_tiles, pa_waves ) );
      ++g_checked;
    }
    if( block < nb )
    {
      REQUIRE( block > last[b & 7], "k %d, nb %d: class %d goes from block %d back to %d at workgroup %d", k, nb, b & 7, last[b & 7], block, b );
      last[b & 7] = block;
    }
  }
  for( int t = 0; t < n_tiles; ++t ) REQUIRE( hit[(size_t)t], "k %d, %d tiles (%d blocks) under a grid of %d: tile %d is nobody's", k, n_tiles, nb, grid, t );
}

int main()
{
  for( int pa_waves : { 1, 4 } )
    for( int k = -1; k <= 10; ++k )
    {
      const int C = k < 0 ? 1 : 1 << k;
      std::set<int> counts = { 0, 1, 7, 8, 9, C - 1, C, C + 1, 8 * C - 1, 8 * C, 8 * C + 1, 24 * C + 5, 15640, 1 << 20 };
      std::vector<int> tiles;
      for( int nb : counts )
      {
        // whole blocks, and a last block one tile short of full and one tile long
        tiles.push_back( nb * pa_waves );
        if( pa_waves > 1 && nb > 0 ) { tiles.push_back( nb * pa_waves - 1 ); tiles.push_back( ( nb - 1 ) * pa_waves + 1 ); }
      }
      for( int n : tiles ) check_problem( n, n, k, pa_waves );
      // two problems of different sizes under one grid: every smaller one under the grids of some larger ones
      for( size_t a = 0; a < tiles.size(); ++a )
        for( size_t b = 0; b < tiles.size(); ++b )
          if( tiles[a] < tiles[b] && tiles[b] <= ( 24 * C + 5 ) * pa_waves ) check_problem( tiles[a], tiles[b], k, pa_waves );
      check_problem( 15640 * pa_waves, ( 1 << 20 ) * pa_waves, k, pa_waves );
      check_problem( 8 * C + 1, 15640 * pa_waves, k, pa_waves );
    }
  // a negative k is a negative k
  for( int k : { -1, -2, -31 } ) for( int b = 0; b < 64; ++b ) REQUIRE( xm_block( b, 50, k ) == xm_block( b, 50, -1 ) && xm_beyond( b, 50, k ) == ( b >= 56 ) && xm_grid( 50, k ) == 56, "k %d", k );
  printf( "xcdmap_check ok: %lld tiles placed\n", g_checked );
  return 0;
}
