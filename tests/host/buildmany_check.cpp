// The grouping rule of the batched cloud build (rescan_amd/csrc/rs_buildplan.h: bp_many_groups) on the batches where a greedy cut goes
// wrong: none, all-empty clouds, one cloud over each budget, totals one below, at and one above each budget, 4096 clouds.  For every case:
// each cloud is in exactly one group, the groups are in order, and a group is within both budgets unless it is a single cloud that passes
// one alone.  A plain host program (tests/test_many_build_cpu.py compiles it with the address and undefined-behaviour sanitizers).
#include "rs_buildplan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace rs;

static int g_cases = 0;

static void fail( const char* what, int k )
{
  std::printf( "buildmany_check FAILED: %s (case %d, at %d)\n", what, g_cases, k );
  std::exit( 1 );
}

// runs the rule on one batch with both costs, and with each cost alone (the build's three uses), and checks the cut
static void check( const std::vector<double>& a, const std::vector<double>& b, double budget_a, double budget_b, int want_groups = -1 )
{
  const int n = (int)a.size();
  for( int use = 0; use < 3; ++use )
  {
    ++g_cases;
    const double* ca = use != 2 ? a.data() : nullptr; const double* cb = use != 1 ? b.data() : nullptr;
    std::vector<int> end( (size_t)n + 1, -7 );        // (one word more than the rule may write: it stays -7)
    const int groups = bp_many_groups( ca, cb, n, budget_a, budget_b, end.data() );
    if( groups < 0 || groups > n ) fail( "number of groups", groups );
    if( ( n == 0 ) != ( groups == 0 ) ) fail( "a batch without clouds has no group, any other has one", groups );
    if( end[(size_t)groups] != -7 ) fail( "wrote past its groups", groups );
    int at = 0;
    for( int g = 0; g < groups; ++g )
    {
      if( end[g] <= at ) fail( "an empty group, or groups out of order", g );
      double sa = 0.0, sb = 0.0;
      for( int k = at; k < end[g]; ++k ) { sa += ca ? ca[k] : 0.0; sb += cb ? cb[k] : 0.0; }
      if( ( sa > budget_a || sb > budget_b ) && end[g] - at != 1 ) fail( "a group of several clouds over a budget", g );
      // greedy: the next cloud did not fit
      if( g + 1 < groups )
      {
        const double na = ca ? ca[end[g]] : 0.0, nb = cb ? cb[end[g]] : 0.0;
        if( !( sa + na > budget_a || sb + nb > budget_b ) ) fail( "cut although the next cloud fits", g );
      }
      at = end[g];
    }
    if( at != n ) fail( "clouds left out", at );
    if( use == 0 && want_groups >= 0 && groups != want_groups ) fail( "groups expected", groups );
  }
}

int main()
{
  const double P = RS_BP_MANY_POINTS_MAX, T = RS_BP_MANY_TRIAL_WORDS_MAX, W = RS_BP_MANY_CELL_WORDS_MAX;
  // the budgets hold what one cloud can need: a trial table (2^25 + 2 words), an offset table (48e6 + 2 words, rounded to 64)
  if( !( T >= RS_BP_TRIAL_CELLS_MAX / 32.0 + 2.0 ) || !( W >= RS_BP_TABLE_CELLS_MAX + 66.0 ) || !( P <= 2147483647.0 ) ) fail( "budgets", 0 );
  const double budgets[3][2] = { { P, T }, { P, W }, { 1000.0, 64.0 } };
  for( const auto& bb : budgets )
  {
    const double A = bb[0], B = bb[1];
    check( {}, {}, A, B, 0 );                                                   // no cloud
    check( std::vector<double>( 9, 0.0 ), std::vector<double>( 9, 0.0 ), A, B, 1 );   // all empty
    check( { 0.0 }, { 0.0 }, A, B, 1 );
    // one cloud over a budget: alone, first, in the middle, last
    check( { A + 1 }, { 1 }, A, B, 1 );
    check( { 1 }, { B + 1 }, A, B, 1 );
    check( { A + 1, 5, 5 }, { 1, 1, 1 }, A, B, 2 );
    check( { 5, A + 1, 5 }, { 1, 1, 1 }, A, B, 3 );
    check( { 5, 5, A + 1 }, { 1, 1, 1 }, A, B, 2 );
    check( { 5, 5, 5 }, { 1, B + 1, 1 }, A, B, 3 );
    check( { A + 1, A + 1 }, { B + 1, B + 1 }, A, B, 2 );
    // totals one below, at and one above a budget
    for( int d = -1; d <= 1; ++d )
    {
      const int want = d > 0 ? 2 : 1;
      check( { A - 10, 10.0 + d }, { 1, 1 }, A, B, want );
      check( { 1, 1 }, { B - 10, 10.0 + d }, A, B, want );
      check( { A - 10, 0, 10.0 + d, 0 }, { 0, 0, 0, 0 }, A, B, want );          // (empty clouds in between join whatever is open)
      check( { 3, A - 3 + d }, { B - 3 + d, 3 }, A, B, want );
      check( { A / 2, A / 2 + d, A / 2, A / 2 + d }, { 1, 1, 1, 1 }, A, B, d > 0 ? 4 : 2 );
    }
    // 4096 clouds: of a handful of points; of a seventh of a budget each; alternately empty and full
    std::vector<double> a( 4096 ), b( 4096 );
    for( int k = 0; k < 4096; ++k ) { a[k] = 1 + k % 5; b[k] = 3; }
    check( a, b, A, B );
    for( int k = 0; k < 4096; ++k ) { a[k] = A / 7.0; b[k] = B / 9.0; }
    check( a, b, A, B );
    for( int k = 0; k < 4096; ++k ) { a[k] = k % 2 ? A : 0.0; b[k] = k % 3 ? 0.0 : B; }
    check( a, b, A, B );
  }
  std::printf( "buildmany_check ok %d\n", g_cases );
  return 0;
}
