// Stand-alone check of rescan_amd/csrc/rs_rowtable.h, the index arithmetic of the cooperative sweep's row table, against a linear
// walk: for random and adversarial row tables, for 2, 4 and 8 waves, the chunks that the waves fetch — each wave walking its own
// share exactly as sweep_stream does — must be the linear stream, every candidate once, in stream order within every wave, chunk c
// at wave c mod NW, super-batch by super-batch.  Built with -fsanitize=address,undefined and run by tests/test_coop_stream_cpu.py.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I rescan_amd/csrc tests/host/rowtable_check.cpp -o rowtable_check
#include "rs_rowtable.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace rs;

struct Row { uint32_t sa, la, sb, lb; };
static long long g_checked = 0;

#define REQUIRE( c, ... ) do { if( !( c ) ) { fprintf( stderr, "rowtable_check: %s:%d: %s failed: ", __FILE__, __LINE__, #c ); fprintf( stderr, __VA_ARGS__ ); fprintf( stderr, "\n" ); exit( 1 ); } } while( 0 )

// One shell of rows.size() cell rows swept by NW waves.  The table's arrays live across the super-batches, as the kernel's do: an entry
// past the shell's last row is rewritten as empty, never left over from the super-batch before.
template <int NW>
static void check_shell( const std::vector<Row>& rows, const char* what )
{
  const int n_rows = (int)rows.size();
  const int n_sb = rt_super_batches( n_rows, NW );
  REQUIRE( ( n_sb * rt_table_rows( NW ) >= n_rows && ( n_sb - 1 ) * rt_table_rows( NW ) < n_rows ) || ( n_rows == 0 && n_sb == 0 ), "%s: %d rows, %d super-batches", what, n_rows, n_sb );
  // heap arrays of exactly the table's size: the sanitizer sees any index past them
  std::vector<uint32_t> seg_a( NW * RT_BLOCK, 0xdeadbeefu ), len_a( NW * RT_BLOCK, 0xdeadbeefu ), seg_b( NW * RT_BLOCK, 0xdeadbeefu ), pre( NW * RT_BLOCK, 0xdeadbeefu ), block_total( NW, 0xdeadbeefu );
  int rows_seen = 0;
  for( int sb = 0; sb < n_sb; ++sb )
  {
    // the table, as the lanes write it: every entry describes its own row only, every wave scans its own block
    std::vector<uint32_t> linear;                         // the stream: rows ascending, piece a then piece b
    for( int w = 0; w < NW; ++w )
    {
      uint32_t incl = 0;
      for( int l = 0; l < RT_BLOCK; ++l )
      {
        const int e = w * RT_BLOCK + l, r = rt_row_of_entry( sb, NW, e );
        REQUIRE( r == rows_seen + e, "%s: entry %d of super-batch %d is row %d", what, e, sb, r );
        Row x{ 0, 0, 0, 0 };
        if( r < n_rows ) x = rows[r];
        seg_a[e] = x.sa; len_a[e] = x.la; seg_b[e] = x.sb; pre[e] = incl;
        incl += x.la + x.lb;
        for( uint32_t k = 0; k < x.la; ++k ) linear.push_back( x.sa + k );
        for( uint32_t k = 0; k < x.lb; ++k ) linear.push_back( x.sb + k );
      }
      block_total[w] = incl;
    }
    rows_seen += rt_table_rows( NW );
    uint32_t blk[NW];
    const uint32_t total = rt_block_offsets<NW>( block_total.data(), blk );
    REQUIRE( total == linear.size(), "%s: super-batch %d holds %zu candidates, the offsets say %u", what, sb, linear.size(), total );
    for( int w = 0; w < NW; ++w ) { uint32_t s = 0; for( int v = 0; v < w; ++v ) s += block_total[v]; REQUIRE( blk[w] == s, "%s: block offset %d", what, w ); }
    // every wave's share, walked as sweep_stream walks it
    std::vector<int> times( linear.size(), 0 );
    uint32_t chunks_seen = 0;
    for( int w = 0; w < NW; ++w )
    {
      for( uint32_t c0 = rt_first( w ); c0 < total; c0 += rt_stride( NW ) )
      {
        REQUIRE( c0 % RT_BLOCK == 0 && rt_chunk_owner( c0 / RT_BLOCK, NW ) == w, "%s: chunk %u fetched by wave %d", what, c0 / RT_BLOCK, w );
        ++chunks_seen;
        for( uint32_t lane = 0; lane < RT_BLOCK; ++lane )
        {
          const uint32_t j = c0 + lane;
          if( j >= total ) continue;
          int e = -1;
          const uint32_t src = rt_source<NW>( blk, pre.data(), seg_a.data(), len_a.data(), seg_b.data(), j, &e );
          REQUIRE( src == linear[j], "%s: NW %d, super-batch %d, candidate %u of %u: cloud position %u, the linear walk has %u (entry %d)", what, NW, sb, j, total, src, linear[j], e );
          REQUIRE( e >= 0 && e < NW * RT_BLOCK && rt_row_of_entry( sb, NW, e ) < n_rows, "%s: candidate %u from entry %d", what, j, e );
          ++times[j]; ++g_checked;
        }
      }
    }
    REQUIRE( chunks_seen == ( total + RT_BLOCK - 1 ) / RT_BLOCK, "%s: %u chunks fetched of %u candidates (the last, partial one included)", what, chunks_seen, total );
    for( size_t j = 0; j < times.size(); ++j ) REQUIRE( times[j] == 1, "%s: candidate %zu fetched %d times", what, j, times[j] );
  }
}

static void check_all( const std::vector<Row>& rows, const char* what )
{
  check_shell<2>( rows, what ); check_shell<4>( rows, what ); check_shell<8>( rows, what );
}

// rows whose pieces are consecutive runs of a cloud, so that a wrong row shows as a wrong position
static std::vector<Row> make_rows( std::mt19937& rng, int n_rows, double p_empty, int max_len, double p_two )
{
  std::vector<Row> rows( n_rows );
  uint32_t at = 1000;
  std::uniform_real_distribution<double> u( 0.0, 1.0 );
  for( Row& r : rows )
  {
    r = Row{ at, 0, at, 0 };
    if( u( rng ) < p_empty ) { at += 3; continue; }
    r.la = (uint32_t)( rng() % (uint32_t)( max_len + 1 ) );
    at += r.la + ( rng() % 5 );                      // the cells of the inner box lie between the two pieces
    if( u( rng ) < p_two ) { r.sb = at; r.lb = (uint32_t)( rng() % (uint32_t)( max_len + 1 ) ); at += r.lb; }
    at += rng() % 7;
  }
  return rows;
}

int main()
{
  std::mt19937 rng( 1701 );
  // random tables: sizes around every table edge (NW x 64 - 1 / + 0 / + 1 for NW = 2, 4, 8), several super-batches, sparse and dense
  const int sizes[] = { 0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1100, 1537, 2500 };
  for( int n : sizes )
    for( double p_empty : { 0.0, 0.5, 0.95 } )
      for( int max_len : { 1, 7, 200 } )
        check_all( make_rows( rng, n, p_empty, max_len, 0.4 ), "random" );
  // adversarial tables
  for( int n : { 128, 256, 512, 600, 1030 } )
  {
    std::vector<Row> rows( n, Row{ 5, 0, 5, 0 } );
    check_all( rows, "all rows empty" );
    for( int at : { 0, 1, 63, 64, 65, 127, 128, 255, 256, 511, n - 1 } )      // the first row of a later wave's block, the table's last row, ...
    {
      if( at >= n ) continue;
      for( uint32_t len : { 1u, 63u, 64u, 65u, 129u } )
      {
        std::vector<Row> one = rows;
        one[at] = Row{ 77, len, 9000, 0 };
        check_all( one, "one occupied row, piece a" );
        one[at] = Row{ 77, 0, 9000, len };
        check_all( one, "one occupied row, piece b" );
        one[at] = Row{ 77, 1, 9000, len };
        check_all( one, "one occupied row, both pieces" );
      }
    }
    // runs of empty rows between occupied ones, every stride
    for( int every : { 2, 63, 64, 65, 200 } )
    {
      std::vector<Row> sparse = rows;
      uint32_t at = 0;
      for( int r = 0; r < n; r += every ) { sparse[r] = Row{ at, 3, at + 10, 2 }; at += 20; }
      check_all( sparse, "runs of empty rows" );
    }
    // streams of exactly NW x 64 x d - 1 / + 0 / + 1 candidates (d = 1, 2, 3 chunks in flight), spread over the rows
    for( int nw : { 2, 4, 8 } )
      for( int d : { 1, 2, 3 } )
        for( int delta : { -1, 0, 1 } )
        {
          const int want = nw * 64 * d + delta;
          std::vector<Row> full = rows;
          int left = want; uint32_t at = 0;
          for( int r = 0; r < n && left > 0; ++r ) { const int len = ( r == n - 1 || r == rt_table_rows( nw ) - 1 ) ? left : ( left < 3 ? left : 3 ); full[r] = Row{ at, (uint32_t)len, at, 0 }; at += len + 1; left -= len; }
          check_all( full, "stream of NW x 64 x d candidates" );
        }
  }
  printf( "rowtable_check ok: %lld candidates looked up\n", g_checked );
  return 0;
}
