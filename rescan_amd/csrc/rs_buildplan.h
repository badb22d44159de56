// The arithmetic of a cloud's index build: every expression of rs_cloud_api.hip (cloud_create_impl, many_build_group) and
// rs_build.hip that produces an index or a size — the sanitised bounds, the trial grids of the density-derived cell and a point's
// cell in them, the cell size, the offset table's dimensions, a stored point's cell, its Hilbert cell and key, the tile extent
// limit — and the one statement of the host's decisions between the kernels (CloudPlan).  For the host and, under
// hipcc, for the device (RS_HD, like rs_math.h); nothing of HIP is needed when a host compiler reads it, so that
// tests/host/buildplan_check.cpp runs these very expressions under the sanitizers and tests/build_restate.py is held to them.
//
// Two rules hold throughout: a value becomes an integer only after it was clamped, as a float, into the range of its table; and
// sizes are formed and compared in double before any of them is cast.  A coordinate that is not finite (NaN, ±Inf) takes no part
// in the bounds; its point is stored like any other, in the clamped cell: NaN and -Inf in cell 0 of the axis, +Inf in the last.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#ifndef RS_HD
#if defined( __HIPCC__ )
#define RS_HD __host__ __device__
#else
#define RS_HD
#endif
#endif

namespace rs {

#define RS_BP_TRIAL_CELLS_MAX 1073741824.0      // a trial grid of more cells is too fine to count: one bit per cell, 128 MiB
#define RS_BP_TABLE_CELLS_MAX 48.0e6            // keeps the dense offset table below ~200 MB
#define RS_BP_TABLE_DIM_MAX 16777216.0          // 2^24: every cell coordinate of the table, and dim - 1, is then exact as a float
#define RS_BP_TRIAL_ATTEMPTS 8

// ---- bounds ----
RS_HD inline bool bp_finite( float v ) { return fabsf( v ) <= FLT_MAX; }      // false for NaN and ±Inf
// one coordinate into the running bounds of its axis (start: lo = FLT_MAX, hi = -FLT_MAX)
RS_HD inline void bp_bounds_take( float v, float& lo, float& hi )
{
  if( !bp_finite( v ) ) return;
  if( v < lo ) lo = v;
  if( v > hi ) hi = v;
}
// the float of a word of the bounds kernels, which take minima and maxima of floats as unsigned atomics on an order-preserving
// encoding (negative: every bit flipped, else the sign bit set)
inline float bp_bounds_decode( unsigned u ) { const unsigned b = ( u & 0x80000000u ) ? ( u ^ 0x80000000u ) : ~u; float f; std::memcpy( &f, &b, 4 ); return f; }
// an axis without a finite coordinate (lo > hi) gets [0, 0]
inline void bp_sanitise_bounds( float mn[3], float mx[3] )
{
  for( int a = 0; a < 3; ++a )
    if( !( mx[a] >= mn[a] ) || !bp_finite( mn[a] ) || !bp_finite( mx[a] ) ) { mn[a] = 0.0f; mx[a] = 0.0f; }
}

// ---- the trial grids of the density-derived cell ----
inline float bp_trial_first_cell( const float mn[3], const float mx[3] )
{
  const float e0 = mx[0] - mn[0], e1 = mx[1] - mn[1], e2 = mx[2] - mn[2];
  const float ext = e0 > ( e1 > e2 ? e1 : e2 ) ? e0 : ( e1 > e2 ? e1 : e2 );     // (may be +Inf: -FLT_MAX and FLT_MAX in one cloud)
  const float q = ext / 64.0f, lo = q > 1e-4f ? q : 1e-4f;
  return lo < 0.1f ? lo : 0.1f;
}
struct TrialGrid
{
  float inv;                      // 1 / cell
  double cells;                   // td[0] * td[1] * td[2], formed in double; td[] and top[] are valid only when countable()
  unsigned long long td[3];       // cells per axis: the extent's cell + 2
  float top[3];                   // the largest float that is not above td - 1: what a point's cell is clamped to before it is cast
  RS_HD bool countable() const { return cells <= RS_BP_TRIAL_CELLS_MAX; }
  size_t words() const { return (size_t)( cells / 32.0 ) + 2; }                  // of the bit table
};
inline TrialGrid bp_trial_grid( const float mn[3], const float mx[3], float c0 )
{
  TrialGrid g; g.inv = 1.0f / c0; g.cells = 1.0;
  double d[3];
  for( int a = 0; a < 3; ++a )
  {
    float f = floorf( ( mx[a] - mn[a] ) * g.inv );
    if( !( f >= 0.0f ) ) f = 0.0f;
    d[a] = (double)f + 2.0; g.cells *= d[a];        // (f = +Inf: cells = +Inf, not countable)
    g.td[a] = 0; g.top[a] = 0.0f;
  }
  if( g.countable() )
    for( int a = 0; a < 3; ++a )
    {
      g.td[a] = (unsigned long long)d[a];             // every factor is >= 2, so each is <= 2^28
      float t = (float)( g.td[a] - 1 );
      if( (double)t > d[a] - 1.0 ) t = nextafterf( t, 0.0f );
      g.top[a] = t;
    }
  return g;
}
// a coordinate's cell along one axis of a trial grid, in [0, td - 1]
RS_HD inline unsigned long long bp_trial_axis( float v, float gmin, float inv, float top )
{
  float c = floorf( ( v - gmin ) * inv );
  if( !( c >= 0.0f ) ) c = 0.0f;          // NaN, -Inf, below the box
  if( c > top ) c = top;                  // +Inf, and whatever the bounds did not count
  return (unsigned long long)c;
}
RS_HD inline unsigned long long bp_trial_cell( float x, float y, float z, float mx, float my, float mz, float inv, float tx, float ty, float tz,
                                               unsigned long long db, unsigned long long dc )
{
  return ( bp_trial_axis( x, mx, inv, tx ) * db + bp_trial_axis( y, my, inv, ty ) ) * dc + bp_trial_axis( z, mz, inv, tz );
}

// ---- the cell size ----
inline float bp_per_cell( int32_t n, int occupied ) { return (float)n / (float)( occupied > 1 ? occupied : 1 ); }
// about two sample spacings: a surface patch then holds ~4 points per cell.  A grid that could not be counted stands for 4 per cell.
#define RS_BP_PER_CELL_WANTED 4.0f
inline float bp_auto_cell_of( float per_cell, float c0 ) { return 2.0f * c0 / sqrtf( per_cell > 1.0f ? per_cell : 1.0f ); }
inline float bp_auto_cell( int32_t n, int occupied, float c0 ) { return bp_auto_cell_of( bp_per_cell( n, occupied ), c0 ); }
inline float bp_auto_cell_scaled( float cell, float scale )
{
  const float s = cell * scale, lo = s > 0.005f ? s : 0.005f;
  return lo < 2.0f ? lo : 2.0f;
}

// ---- the offset table ----
// dims of the table over [mn, mx] with cells of `cell` (> 0), the cell doubled until the table has at most RS_BP_TABLE_CELLS_MAX cells
// and at most RS_BP_TABLE_DIM_MAX along every axis (cell_of_dev and the searches' axis_range clamp in float, up to 2^24).  An axis has
// the cells of its extent, counted in double, and never fewer than the cell the kernels' own float expression gives the maximum:
// rounding may put that one cell further (always, once 0.01 cell is below the float's spacing), and a query there starts its range at
// that cell, so the table must have it.  false, dims untouched: no table — an extent that is not finite as a float (-FLT_MAX and
// FLT_MAX in one cloud) has no cell coordinates; the caller builds the brute layout.
inline bool bp_table_dims( const float mn[3], const float mx[3], float& cell, int dims[3] )
{
  for( int a = 0; a < 3; ++a ) if( !bp_finite( mx[a] - mn[a] ) ) return false;
  for( ;; )
  {
    const float inv = 1.0f / cell;
    if( !( inv > 0.0f ) ) return false;
    double d[3], cells = 1.0;
    for( int a = 0; a < 3; ++a )
    {
      d[a] = floor( ( (double)mx[a] - (double)mn[a] ) / (double)cell ) + 1.0;
      const double f = (double)floorf( ( mx[a] - mn[a] ) * inv ) + 1.0;
      if( f > d[a] ) d[a] = f;
      cells *= d[a];
    }
    if( cells <= RS_BP_TABLE_CELLS_MAX && d[0] <= RS_BP_TABLE_DIM_MAX && d[1] <= RS_BP_TABLE_DIM_MAX && d[2] <= RS_BP_TABLE_DIM_MAX )
    {
      for( int a = 0; a < 3; ++a ) dims[a] = (int)d[a];
      return true;
    }
    cell *= 2.0f;
  }
}
// cell coordinate of a stored point along one axis (the search kernels' axis_range covers this expression with a 0.01-cell margin)
RS_HD inline int cell_of_dev( float v, float gmin, float inv_cell, int dim )
{
  float c = floorf( ( v - gmin ) * inv_cell );
  if( !( c >= 0.0f ) ) c = 0.0f;
  if( c > (float)( dim - 1 ) ) c = (float)( dim - 1 );
  return (int)c;
}
RS_HD inline uint32_t bp_cell_id( int cx, int cy, int cz, int w, int h ) { return (uint32_t)( ( (size_t)cz * h + cy ) * w + cx ); }

// ---- the Hilbert order ----
// 10 bits per axis over the largest finite extent
inline float bp_hilbert_scale( const float mn[3], const float mx[3] )
{
  float ext = 0.0f;
  for( int a = 0; a < 3; ++a ) { const float e = mx[a] - mn[a]; if( bp_finite( e ) && e > ext ) ext = e; }
  return ext > 0.0f ? 1024.0f / ext : 0.0f;
}
RS_HD inline uint32_t bp_hilbert_axis( float v, float gmin, float scale )
{
  float f = ( v - gmin ) * scale;
  if( !( f >= 0.0f ) ) f = 0.0f;
  if( f > 1023.0f ) f = 1023.0f;
  return (uint32_t)f;
}
// Index of a cell on a 3-D Hilbert curve with `bits` bits per axis (Skilling's transpose form)
RS_HD inline uint32_t hilbert3_dev( uint32_t x, uint32_t y, uint32_t z, int bits )
{
  uint32_t X[3] = { x, y, z };
  const uint32_t M = 1u << ( bits - 1 );
  for( uint32_t Q = M; Q > 1; Q >>= 1 )
  {
    const uint32_t P = Q - 1;
#pragma unroll
    for( int i = 0; i < 3; ++i )
    {
      if( X[i] & Q ) X[0] ^= P;
      else { const uint32_t t = ( X[0] ^ X[i] ) & P; X[0] ^= t; X[i] ^= t; }
    }
  }
  X[1] ^= X[0]; X[2] ^= X[1];
  uint32_t t = 0;
  for( uint32_t Q = M; Q > 1; Q >>= 1 ) if( X[2] & Q ) t ^= Q - 1;
  X[0] ^= t; X[1] ^= t; X[2] ^= t;
  uint32_t h = 0;
  for( int b = bits - 1; b >= 0; --b )
#pragma unroll
    for( int i = 0; i < 3; ++i ) h = ( h << 1 ) | ( ( X[i] >> b ) & 1u );
  return h;
}

// ---- the tiles ----
// the brute layout has one cell: the occupancy of a 0.1 m grid is estimated from the box instead
inline size_t bp_brute_occupied( int32_t n, const float mn[3], const float mx[3] )
{
  double vol_cells = 1.0;
  for( int a = 0; a < 3; ++a ) vol_cells *= floor( ( (double)mx[a] - mn[a] ) / 0.1 ) + 1.0;
  const double e = pow( vol_cells, 2.0 / 3.0 ), m = (double)n < e ? (double)n : e;
  return (size_t)( m > 1.0 ? m : 1.0 );
}
// Tile extent limit from the cloud's own sampling density: a full tile of 64 surface samples spans about 8 sample spacings; allow
// half as much again, never less than 0.25 m and never more than extent_max (RS_HIP_TILE_EXTENT_MAX).
inline float query_extent_limit( int32_t n, size_t occupied_cells, float cell, float extent_max )
{
  if( n <= 0 || occupied_cells == 0 || !( cell > 0.0f ) ) return FLT_MAX;
  const float per_cell = (float)n / (float)occupied_cells;
  const float spacing = cell / sqrtf( per_cell > 1.0f ? per_cell : 1.0f );
  const float want = 12.0f * spacing, lo = want > 0.25f ? want : 0.25f;
  return extent_max < lo ? extent_max : lo;
}

// ---- the plan of one cloud ----
// What the host decides for one cloud, and the one statement of how: each function below covers what lies between two of a build's
// device synchronisations.  The single build (cloud_create_impl) and the batched one (many_build_group) of rs_cloud_api.hip drive them
// with their own launches around them, and tests/host/buildplan_check.cpp with loops over the points in the launches' place.
struct CloudPlan
{
  float mn[3] = { 0, 0, 0 }, mx[3] = { 0, 0, 0 };       // sanitised bounds
  float nor_max = 1.0f;                                 // max |normal|
  float cell_size = 0.0f;                               // as asked, then as chosen; 0: the brute layout
  float chosen = 0.0f;                                  // cell_size as it went into the table (given, or derived and scaled): the check's report
  float c0 = 0.0f; bool undecided = false;              // the trial grid's cell while the density-derived cell is being looked for
  float cell = 0.0f, inv_cell = 0.0f;                   // of the offset table (coarsened into its budget)
  int dims[3] = { 1, 1, 1 };
  size_t n_cells = 1, occupied = 0;
  float extent_limit = 0.0f, hscale = 0.0f;             // of the query layout: the tile extent limit, the Hilbert scale
};
// after the bounds kernel: its eight words (min and max per axis in the order-preserving encoding, the largest |normal|^2 as a
// float's bits, a flag for a normal that is not finite).  The kernel took the finite coordinates only; an axis without one: [0, 0].
inline void bp_plan_bounds( CloudPlan& p, const unsigned got[8], int32_t n, bool has_nor )
{
  if( n <= 0 ) return;
  for( int a = 0; a < 3; ++a ) { p.mn[a] = bp_bounds_decode( got[a] ); p.mx[a] = bp_bounds_decode( got[3 + a] ); }
  bp_sanitise_bounds( p.mn, p.mx );
  if( has_nor )
  {
    float n2; std::memcpy( &n2, &got[6], 4 );
    p.nor_max = ( got[7] || !std::isfinite( n2 ) ) ? INFINITY : std::sqrt( n2 ) * 1.00001f;
  }
}
// cell_size < 0: pick the cell from the cloud's own sampling density (about two sample spacings: a surface patch then holds ~4
// points per cell, the first search shell ~100-300), over at most RS_BP_TRIAL_ATTEMPTS trial grids
inline void bp_plan_cell_begin( CloudPlan& p, float cell_size, int32_t n )
{
  p.cell_size = cell_size;
  if( !( cell_size < 0.0f ) ) return;
  p.cell_size = 0.1f;
  if( n > 0 ) { p.undecided = true; p.c0 = bp_trial_first_cell( p.mn, p.mx ); }
}
// one attempt of an undecided cloud, before the device: true, tg: count the occupied cells of this grid and call bp_plan_trial_counted.
// false: the grid is too fine to count (huge, sparse extent): coarsened, or, at the last attempt, standing for the wanted density.
inline bool bp_plan_trial( CloudPlan& p, bool last, TrialGrid& tg )
{
  tg = bp_trial_grid( p.mn, p.mx, p.c0 );
  if( tg.countable() ) return true;
  if( !last ) p.c0 *= 2.0f;
  else { p.cell_size = bp_auto_cell_of( RS_BP_PER_CELL_WANTED, p.c0 ); p.undecided = false; }
  return false;
}
// ... and after the count
inline void bp_plan_trial_counted( CloudPlan& p, int32_t n, int occ, bool last )
{
  const float per_cell = bp_per_cell( n, occ );
  if( per_cell >= RS_BP_PER_CELL_WANTED || last ) { p.cell_size = bp_auto_cell_of( per_cell, p.c0 ); p.undecided = false; }
  else p.c0 *= 2.0f;
}
// the offset table (asked_auto: the caller's cell_size was < 0; auto_scale: RS_HIP_AUTO_CELL_SCALE)
inline void bp_plan_table( CloudPlan& p, int32_t n, bool asked_auto, float auto_scale )
{
  if( asked_auto && n > 0 ) p.cell_size = bp_auto_cell_scaled( p.cell_size, auto_scale );
  p.chosen = p.cell = p.cell_size;
  if( p.cell_size > 0.0f && n > 0 )
  {
    // (in double before any cast: an extent of any size is coarsened into the table; one that overflows a float gets the brute layout)
    if( bp_table_dims( p.mn, p.mx, p.cell, p.dims ) ) p.inv_cell = 1.0f / p.cell;
    else p.cell_size = p.cell = 0.0f;
  }
  p.n_cells = (size_t)p.dims[0] * p.dims[1] * p.dims[2];
}
// the query layout, after the cell index (counted: its occupied cells; extent_max: RS_HIP_TILE_EXTENT_MAX): Hilbert order, tiles of
// <= 64 points within the extent limit
inline void bp_plan_query_layout( CloudPlan& p, int32_t n, size_t counted, float extent_max )
{
  p.occupied = counted;
  const float lim_cell = p.cell_size > 0.0f ? p.cell : 0.1f;
  if( !( p.cell_size > 0.0f ) ) p.occupied = bp_brute_occupied( n, p.mn, p.mx );
  p.extent_limit = query_extent_limit( n, p.occupied, lim_cell, extent_max );
  p.hscale = n > 0 ? bp_hilbert_scale( p.mn, p.mx ) : 0.0f;
}
// rs_hip_cloud_bytes: the cell-sorted records (16 bytes each, at least one) and the offset table | the same records in Hilbert
// order, the tile list and the inverse of the order
inline int64_t bp_plan_bytes( int32_t n, bool has_nor, size_t n_cells, int n_tiles )
{
  const size_t pb = (size_t)( n > 1 ? n : 1 ) * 16;
  return (int64_t)( pb * ( has_nor ? 2 : 1 ) + ( n_cells + 1 ) * 4 ) + (int64_t)( pb * ( has_nor ? 2 : 1 ) + ( (size_t)n_tiles + 1 ) * 4 + (size_t)n * 4 );
}

// ---- the batched build (cloud_create_many_impl) ----
// A batch is cut into groups of consecutive clouds that are built together.  The budgets of a group:
#define RS_BP_MANY_POINTS_MAX 67108864.0        // 2^26 points: every index of a group's concatenated arrays fits an int32 with room to spare
#define RS_BP_MANY_TRIAL_WORDS_MAX 67108864.0   // 2^26 words (256 MiB) of trial bit tables side by side; one table is at most 2^25 + 2
#define RS_BP_MANY_CELL_WORDS_MAX 268435456.0   // 2^28 words (1 GiB) of offset tables: one scan (an int count) runs over all of them
// The grouping rule, greedy and in order: cloud k joins the open group unless one of the two totals would then pass its budget; then
// it opens the next.  cost_a / cost_b: what each cloud adds (points and words; either may be null: nothing).  group_end[g] = one
// past the last cloud of group g; returns the number of groups.  Every cloud is in exactly one group, the groups are in order, and a
// group is within both budgets unless it is ONE cloud that passes a budget alone (it is then built by itself).
inline int bp_many_groups( const double* cost_a, const double* cost_b, int n_clouds, double budget_a, double budget_b, int* group_end )
{
  int groups = 0, open = 0;           // open: clouds in the open group
  double a = 0.0, b = 0.0;
  for( int k = 0; k < n_clouds; ++k )
  {
    const double ca = cost_a ? cost_a[k] : 0.0, cb = cost_b ? cost_b[k] : 0.0;
    if( open && ( a + ca > budget_a || b + cb > budget_b ) ) { group_end[groups++] = k; open = 0; a = b = 0.0; }
    a += ca; b += cb; ++open;
  }
  if( open ) group_end[groups++] = n_clouds;
  return groups;
}

} // namespace rs
