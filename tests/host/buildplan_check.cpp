// Stand-alone run of rescan_amd/csrc/rs_buildplan.h, the arithmetic of a cloud's index build, on one cloud of tests/hard_builds.py:
// the library's own decisions (CloudPlan and its functions, as cloud_create_impl and many_build_group of rs_cloud_api.hip drive them)
// with every kernel's indexing expression applied to every point, in the launches' place, on tables of exactly the size the library
// allocates — the bit table of every trial grid, the offset table, the 30-bit Hilbert key.
// Every index must be inside its table; the plan is printed (floats as their bits) and the per-point arrays are written to a file,
// for tests/test_hard_build_cpu.py to compare with tests/build_restate.py field for field.  Built with
// -fsanitize=address,undefined,float-cast-overflow: a conversion of a value outside its integer type ends the run.
//   c++ -std=c++17 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -I rescan_amd/csrc tests/host/buildplan_check.cpp -o buildplan_check
//   buildplan_check IN OUT      IN: int32 n, float cell_size, float auto_cell_scale, float tile_extent_max, n * 3 floats
//                               OUT: n uint32 cell ids, n uint32 Hilbert keys
#include "rs_buildplan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace rs;

#define REQUIRE( c, ... ) do { if( !( c ) ) { fprintf( stderr, "buildplan_check: %s:%d: %s failed: ", __FILE__, __LINE__, #c ); fprintf( stderr, __VA_ARGS__ ); fprintf( stderr, "\n" ); exit( 1 ); } } while( 0 )

static unsigned bits_of( float f ) { unsigned u; memcpy( &u, &f, 4 ); return u; }
// the bounds kernel's order-preserving word of a float (rs_build.hip: enc)
static unsigned enc( float f ) { const unsigned u = bits_of( f ); return ( u & 0x80000000u ) ? ~u : ( u | 0x80000000u ); }

int main( int argc, char** argv )
{
  REQUIRE( argc == 3, "usage: buildplan_check IN OUT" );
  FILE* in = fopen( argv[1], "rb" );
  REQUIRE( in, "cannot read %s", argv[1] );
  int32_t n = 0; float cell_size = 0, scale = 0, extent_max = 0;
  REQUIRE( fread( &n, 4, 1, in ) == 1 && fread( &cell_size, 4, 1, in ) == 1 && fread( &scale, 4, 1, in ) == 1 && fread( &extent_max, 4, 1, in ) == 1 && n >= 0, "header" );
  std::vector<float> pos( (size_t)3 * n );
  if( n ) REQUIRE( fread( pos.data(), 4, pos.size(), in ) == pos.size(), "points" );
  fclose( in );

  CloudPlan P;
  const float *mn = P.mn, *mx = P.mx; const int* dims = P.dims;

  // bounds: what k_build_bounds leaves (each lane's chain, their minimum), as its eight words, and the host's decoding and sanitising
  if( n > 0 )
  {
    float lo[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, hi[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
    for( int i = 0; i < n; ++i ) for( int a = 0; a < 3; ++a ) bp_bounds_take( pos[3 * (size_t)i + a], lo[a], hi[a] );
    unsigned got[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for( int a = 0; a < 3; ++a ) { got[a] = enc( lo[a] ); got[3 + a] = enc( hi[a] ); }
    bp_plan_bounds( P, got, n, false );
  }
  for( int a = 0; a < 3; ++a ) REQUIRE( bp_finite( mn[a] ) && bp_finite( mx[a] ) && mx[a] >= mn[a], "axis %d", a );
  printf( "mn %08x %08x %08x\nmx %08x %08x %08x\n", bits_of( mn[0] ), bits_of( mn[1] ), bits_of( mn[2] ), bits_of( mx[0] ), bits_of( mx[1] ), bits_of( mx[2] ) );

  const bool asked_auto = cell_size < 0.0f;
  bp_plan_cell_begin( P, cell_size, n );
  for( int attempt = 0; P.undecided; ++attempt )
  {
    const bool last = attempt == RS_BP_TRIAL_ATTEMPTS - 1;
    TrialGrid tg;
    if( !bp_plan_trial( P, last, tg ) ) continue;
    const float c0 = P.c0;                             // (of the grid to count)
    const size_t words = tg.words();
    std::vector<uint32_t> table( words );              // exactly what the library allocates and clears
    REQUIRE( (double)tg.td[0] * (double)tg.td[1] * (double)tg.td[2] == tg.cells, "td" );
    for( int a = 0; a < 3; ++a ) REQUIRE( tg.top[a] >= 0.0f && (double)tg.top[a] <= (double)( tg.td[a] - 1 ), "top of axis %d", a );
    unsigned long long sum = 0;
    for( int i = 0; i < n; ++i )
    {
      const unsigned long long id = bp_trial_cell( pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2], mn[0], mn[1], mn[2], tg.inv,
                                                   tg.top[0], tg.top[1], tg.top[2], tg.td[1], tg.td[2] );
      REQUIRE( (double)id < tg.cells && ( id >> 5 ) < words, "point %d: trial cell %llu of %.0f, word %llu of %zu", i, id, tg.cells, id >> 5, words );
      table[id >> 5] |= 1u << ( id & 31 );
      sum += id;
    }
    int occ = 0;
    for( size_t w = 0; w < words; ++w ) occ += __builtin_popcount( table[w] );
    printf( "trial %d c0 %08x td %llu %llu %llu top %08x %08x %08x words %zu occupied %d idsum %llu\n", attempt, bits_of( c0 ), tg.td[0], tg.td[1], tg.td[2],
            bits_of( tg.top[0] ), bits_of( tg.top[1] ), bits_of( tg.top[2] ), words, occ, sum );
    bp_plan_trial_counted( P, n, occ, last );
  }
  bp_plan_table( P, n, asked_auto, scale );
  const float inv_cell = P.inv_cell, cell = P.cell;
  printf( "cell_size %08x\n", bits_of( P.chosen ) );       // (as it went into the table; the table's own cell is on the next line)

  // the maximum's own cell is inside the table without the clamp: a query there starts its range at that cell
  if( inv_cell > 0.0f ) for( int a = 0; a < 3; ++a ) REQUIRE( floorf( ( mx[a] - mn[a] ) * inv_cell ) <= (float)( dims[a] - 1 ), "axis %d: the maximum's cell", a );
  for( int a = 0; a < 3; ++a ) REQUIRE( dims[a] >= 1 && dims[a] <= (int)RS_BP_TABLE_DIM_MAX && (int)(float)( dims[a] - 1 ) == dims[a] - 1, "dims[%d] = %d", a, dims[a] );
  const double cells_d = (double)dims[0] * dims[1] * dims[2];
  REQUIRE( cells_d <= RS_BP_TABLE_CELLS_MAX, "%.0f cells", cells_d );
  const size_t n_cells = (size_t)dims[0] * dims[1] * dims[2];
  REQUIRE( n_cells == P.n_cells, "n_cells %zu, the plan's %zu", n_cells, P.n_cells );
  printf( "cell %08x inv_cell %08x dims %d %d %d\n", bits_of( inv_cell > 0.0f ? cell : 0.0f ), bits_of( inv_cell ), dims[0], dims[1], dims[2] );

  std::vector<uint32_t> counts( n_cells + 1 ), ids( (size_t)n ), keys( (size_t)n );
  size_t occupied = 0;
  for( int i = 0; i < n; ++i )
  {
    const int cx = cell_of_dev( pos[3 * (size_t)i], mn[0], inv_cell, dims[0] ), cy = cell_of_dev( pos[3 * (size_t)i + 1], mn[1], inv_cell, dims[1] ),
              cz = cell_of_dev( pos[3 * (size_t)i + 2], mn[2], inv_cell, dims[2] );
    REQUIRE( cx >= 0 && cx < dims[0] && cy >= 0 && cy < dims[1] && cz >= 0 && cz < dims[2], "point %d: cell %d %d %d", i, cx, cy, cz );
    const uint32_t id = bp_cell_id( cx, cy, cz, dims[0], dims[1] );
    REQUIRE( id < n_cells, "point %d: cell id %u of %zu", i, id, n_cells );
    if( !counts[id]++ ) ++occupied;
    ids[i] = id;
  }
  bp_plan_query_layout( P, n, occupied, extent_max );
  printf( "occupied %zu limit %08x\n", P.occupied, bits_of( P.extent_limit ) );

  const float hs = P.hscale;
  for( int i = 0; i < n; ++i )
  {
    uint32_t c[3];
    for( int a = 0; a < 3; ++a ) { c[a] = bp_hilbert_axis( pos[3 * (size_t)i + a], mn[a], hs ); REQUIRE( c[a] < 1024u, "point %d axis %d: Hilbert cell %u", i, a, c[a] ); }
    keys[i] = hilbert3_dev( c[0], c[1], c[2], 10 );
    REQUIRE( keys[i] < ( 1u << 30 ), "point %d: key %u", i, keys[i] );
  }
  printf( "hilbert_scale %08x\n", bits_of( hs ) );

  FILE* out = fopen( argv[2], "wb" );
  REQUIRE( out, "cannot write %s", argv[2] );
  if( n ) REQUIRE( fwrite( ids.data(), 4, ids.size(), out ) == ids.size() && fwrite( keys.data(), 4, keys.size(), out ) == keys.size(), "arrays" );
  fclose( out );
  printf( "buildplan_check ok\n" );
  return 0;
}
