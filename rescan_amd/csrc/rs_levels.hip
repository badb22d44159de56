// The level builder for many clouds and many levels at once: rs_hip_level_samples_many, rs_hip_cloud_create_levels_many.
//
// rs_pointcloud_compute_levels samples EVERY level from level 0 (lib/rs/rs_pointcloud.h:989-1011, :1305-1315), so the levels of a
// cloud are independent problems on the same points, as the clouds of a batch are independent of each other: n_clouds x n_levels
// lexicographically first maximal independent sets (rs_rows.hip: the statement above k_level_neighbours), decided side by side.
// The radii are nested, so ONE sweep of a cloud's neighbourhoods at the largest radius sees every pair any level needs.
//
// How a call runs (the plan: rs_levels.h):
//   1. k_levels_neighbours<false>   one launch over all tiles of all bases.  A wave finds its cloud in the tile table, sweeps the cell
//                                   box of the largest radius once (wave_bounds, cell_box, sweep_shell, dist2x4: k_level_neighbours'
//                                   own expressions) and classifies every candidate against the ascending radius_sq table with the
//                                   strict <.  Per (level, point): earlier (into the state word), later, and within against the
//                                   level's cap; an over-cap is an atomicMin of the problem index.  Per (cloud, level) the sum of the
//                                   later counts in 64 bits.
//   2. the first read-back          the over-cap word and the 64-bit totals.  Refusal, groups and lane classes are the host's.
//   per group of clouds (as a rule: one):
//   3. scan                         row offsets from the later counts of the LARGEST level: one row per point
//   4. k_levels_neighbours<true>    the same sweep writes each later neighbour's point id (pfirst + original index) into the row,
//                                   ordered by level class: the neighbours within the smallest radius first, then those the next
//                                   radius adds, ...  Level s reads the row up to its own later count: the adjacency costs what
//                                   the largest level alone costs.  Rows are indexed by point id, so no step needs a by_orig.
//   5. k_levels_init / _frontier    k_level_frontier's state words, items and step semantics on global ids (level * n_points +
//                                   point id): problems cannot touch each other's words.  One launch per step, 16 steps per
//                                   read-back.  Each lane class (1, 8 or 64 lanes per item, per level from its average row) has
//                                   frontier lists of its own; an item's pushes stay in its level, hence in its list.
//   6. k_levels_flags, scan, k_levels_bounds, the second read-back (per-problem sample counts), k_levels_gather (sample indices,
//      positions and normals of all problems packed into one workspace), one batched index build.
#include "rs_host.h"
#include "rs_levels.h"
#include "rs_search.h"

#include <climits>
#include <cstring>
#include <vector>

namespace rs {

using levels::MAX_LEVELS;
#define LEVELS_COVERED 0x40000000      // k_level_frontier's LEVEL_COVERED
constexpr int LEVELS_BATCH = 16;       // frontier steps per read-back
constexpr int LEVELS_CLASSES = 3;      // lanes per item: 1, 8, 64

struct LevelsCloud { GridView tgt; QueryView q; const float4* qnor; const int* by_orig; int pfirst; int n; };

struct LevelsSweep
{
  const LevelsCloud* clouds; const int* tile_first;
  int cloud0, cloud1;                  // the launch covers the tiles [tile0, tile0 + n_tiles) = all tiles of the clouds [cloud0, cloud1)
  int tile0, n_tiles;
  int n_levels, n_points;
  float radius_max, rsq[MAX_LEVELS];   // rsq beyond n_levels: -1, which no dist² is below
  int cap[MAX_LEVELS], caller[MAX_LEVELS];
  int* word;                           // [level * n_points + point]: earlier neighbours (the state word's first value)
  int* later;                          // [level * n_points + point]: later neighbours within the level's radius
  unsigned long long* totals;          // [cloud * n_levels + level]: sum of later
  int* over;                           // lowest problem index (cloud * n_levels + caller's level) with a point over its cap
  const unsigned* offset; int u0;      // row starts of the points u0 .. of this group
  int* adj;
};

template <bool WRITE>
__global__ __launch_bounds__( BLOCK ) void k_levels_neighbours( LevelsSweep L )
{
  __shared__ WaveLds lds[WAVES_PER_BLOCK];
  const int lane = threadIdx.x & ( WAVE - 1 );
  const int wib = threadIdx.x / WAVE;
  const int lt = blockIdx.x * WAVES_PER_BLOCK + wib;
  if( lt >= L.n_tiles ) return;
  const int gt = L.tile0 + lt;
  int lo = L.cloud0, hi = L.cloud1;                     // tile_first[lo] <= gt < tile_first[hi]
  while( hi - lo > 1 ) { const int mid = ( lo + hi ) >> 1; if( L.tile_first[mid] <= gt ) lo = mid; else hi = mid; }
  const int c = uni( lo );
  const GridView tgt = L.clouds[c].tgt;
  const QueryView Q = L.clouds[c].q;
  const int pfirst = L.clouds[c].pfirst;
  EvalScope eval_scope( tgt.evals, lds[wib], lane );
  const int tile = gt - L.tile_first[c];
  const int i = (int)Q.tiles[tile] + lane;
  const bool active = i < (int)Q.tiles[tile + 1];
  float4 q = make_float4( 0, 0, 0, 0 );
  if( active ) q = Q.pos[i];
  const int orig = __float_as_int( q.w );
  const int u = pfirst + orig;
  const TileBounds tb = wave_bounds( active, q.x, q.y, q.z );
  CellBox box = cell_box( tgt, tb, L.radius_max );
  int earlier[MAX_LEVELS], later[MAX_LEVELS], within[MAX_LEVELS], at[MAX_LEVELS];
#pragma unroll
  for( int s = 0; s < MAX_LEVELS; ++s ) { earlier[s] = later[s] = within[s] = 0; at[s] = 0; }
  int* row = nullptr;
  if( WRITE && active )
  {
    row = L.adj + L.offset[u - L.u0];
    // class s starts where the later neighbours of the smaller radii end
#pragma unroll
    for( int s = 1; s < MAX_LEVELS; ++s ) if( s < L.n_levels ) at[s] = L.later[(size_t)( s - 1 ) * L.n_points + u];
  }
  const float rsq_max = L.rsq[L.n_levels - 1];
  if( tb.any && !box_empty( box ) )
  {
    sweep_shell<false>( tgt, box, box, false, lds[wib], lane, 0, 1, [&]( const float4& X, const float4& Y, const float4& Z, int k4 )
    {
      float d[4];
      dist2x4( X, Y, Z, q.x, q.y, q.z, d[0], d[1], d[2], d[3] );
#pragma unroll
      for( int k = 0; k < 4; ++k )
      {
        if( active & ( d[k] < rsq_max ) )                              // strict, msh_hash_grid.h:857
        {
          const int idx = lds[wib].pidx[k4 + k];
          const bool before = idx < orig, after = idx > orig;
          bool inner = false;                                          // within a smaller level's radius already
#pragma unroll
          for( int s = 0; s < MAX_LEVELS; ++s )
          {
            const bool hit = d[k] < L.rsq[s];
            if( !WRITE ) { within[s] += hit; earlier[s] += hit & before; later[s] += hit & after; }
            else if( hit & after & !inner ) { row[at[s]] = pfirst + idx; at[s]++; }
            inner |= hit;
          }
        }
      }
    } );
  }
  if( !WRITE )
  {
#pragma unroll
    for( int s = 0; s < MAX_LEVELS; ++s )
    {
      if( s >= L.n_levels ) break;
      if( active )
      {
        const size_t g = (size_t)s * L.n_points + u;
        L.word[g] = earlier[s]; L.later[g] = later[s];
        if( within[s] > L.cap[s] ) atomicMin( L.over, c * L.n_levels + L.caller[s] );
      }
      unsigned long long t = active ? (unsigned long long)later[s] : 0ull;
#pragma unroll
      for( int o = WAVE / 2; o >= 1; o >>= 1 ) t += __shfl_xor( t, o );
      if( lane == 0 && t ) atomicAdd( L.totals + (size_t)c * L.n_levels + s, t );
    }
  }
}

struct LevelsRounds
{
  int n_points, n_levels;
  int u0, n_group;                     // the group's points
  const unsigned* offset; const int* adj; const int* later;
  int* word; int* state;
  int cls[MAX_LEVELS];                 // lane class of a level: 0, 1, 2
  const int* front_in[LEVELS_CLASSES]; int* front_out[LEVELS_CLASSES];
  const int* count_in; int* count_out; // LEVELS_CLASSES counters each
};

// word = number of earlier neighbours (written by the counting pass); the ids without any are samples and the first frontier
__global__ __launch_bounds__( BLOCK ) void k_levels_init( LevelsRounds R )
{
  const int t = blockIdx.x * BLOCK + threadIdx.x;
  const int s = blockIdx.y;
  if( t >= R.n_group ) return;
  const int g = s * R.n_points + R.u0 + t;
  const int ne = R.word[g];
  R.state[g] = ne == 0 ? 1 : 0;
  if( ne == 0 ) { const int k = R.cls[s]; R.front_out[k][atomicAdd( R.count_out + k, 1 )] = ( g << 1 ) | 1; }
}

// k_level_frontier's step for the list of one lane class
template <int G>
__device__ __forceinline__ void levels_step( const LevelsRounds& R, const int* front_in, int m, int* front_out, int* count_out )
{
  const int lane = threadIdx.x & ( WAVE - 1 );
  const int sub = threadIdx.x & ( G - 1 );
  const int n_groups = gridDim.x * ( BLOCK / G );
  // (every lane of a wave runs the same number of outer and inner iterations: the ballot below needs them all)
  const int m_pad = ( m + ( WAVE / G ) - 1 ) / ( WAVE / G ) * ( WAVE / G );
  for( int t = blockIdx.x * ( BLOCK / G ) + threadIdx.x / G; t < m_pad; t += n_groups )
  {
    bool sample = false; unsigned e0 = 0, e1 = 0; int lbase = 0;
    if( t < m )
    {
      const int item = front_in[t];
      const int g = item >> 1; sample = item & 1;
      const int s = g / R.n_points;
      lbase = s * R.n_points;
      e0 = R.offset[g - lbase - R.u0]; e1 = e0 + (unsigned)R.later[g];
    }
    unsigned len = e1 - e0;
#pragma unroll
    for( int o = WAVE / 2; o >= G; o >>= 1 ) len = max( len, (unsigned)__shfl_xor( (int)len, o ) );
    for( unsigned eb = 0; eb < len; eb += G )
    {
      const unsigned e = e0 + eb + (unsigned)sub;
      int push = -1;
      if( e < e1 )
      {
        const int k = lbase + R.adj[e];
        if( sample )
        {
          const int old = atomicOr( R.word + k, LEVELS_COVERED );
          if( !( old & LEVELS_COVERED ) ) push = k << 1;
        }
        else
        {
          const int now = atomicSub( R.word + k, 1 ) - 1;
          if( now == 0 ) { R.state[k] = 1; push = ( k << 1 ) | 1; }
        }
      }
      const unsigned long long mask = __ballot( push >= 0 );
      if( mask )
      {
        int base = 0;
        if( lane == 0 ) base = atomicAdd( count_out, (int)__popcll( mask ) );
        base = __builtin_amdgcn_readfirstlane( base );
        if( push >= 0 ) front_out[base + (int)__popcll( mask & ( ( 1ull << lane ) - 1ull ) )] = push;
      }
    }
  }
}

__global__ __launch_bounds__( BLOCK ) void k_levels_frontier( LevelsRounds R )
{
  const int m0 = R.count_in[0], m1 = R.count_in[1], m2 = R.count_in[2];
  if( m0 ) levels_step<1>( R, R.front_in[0], m0, R.front_out[0], R.count_out + 0 );
  if( m1 ) levels_step<8>( R, R.front_in[1], m1, R.front_out[1], R.count_out + 1 );
  if( m2 ) levels_step<64>( R, R.front_in[2], m2, R.front_out[2], R.count_out + 2 );
}

// flags over all ids and one more
__global__ __launch_bounds__( BLOCK ) void k_levels_flags( const int* state, int n_ids, unsigned* flags )
{
  const int g = blockIdx.x * BLOCK + threadIdx.x;
  if( g <= n_ids ) flags[g] = ( g < n_ids && state[g] == 1 ) ? 1u : 0u;
}
// bounds[p], p = level * n_clouds + cloud: the first packed sample of that problem; bounds[n_clouds * n_levels]: all samples
__global__ __launch_bounds__( BLOCK ) void k_levels_bounds( const unsigned* scan, const int* pfirst, int n_clouds, int n_levels, int n_points, unsigned* bounds )
{
  const int p = blockIdx.x * BLOCK + threadIdx.x;
  if( p > n_clouds * n_levels ) return;
  const int s = p / n_clouds, c = p - s * n_clouds;
  bounds[p] = p == n_clouds * n_levels ? scan[(size_t)n_levels * n_points] : scan[(size_t)s * n_points + pfirst[c]];
}
// every sample to its packed place (ids ascend with level, cloud, original index): its original index, position and normal
__global__ __launch_bounds__( BLOCK ) void k_levels_gather( const unsigned* flags, const unsigned* scan, const LevelsCloud* clouds, const int* pfirst, int n_clouds,
                                                            int n_points, int n_ids, int* samples, float* pos3, float* nor3 )
{
  const int g = blockIdx.x * BLOCK + threadIdx.x;
  if( g >= n_ids || !flags[g] ) return;
  const int u = g % n_points;
  int lo = 0, hi = n_clouds;                            // pfirst[lo] <= u < pfirst[hi]
  while( hi - lo > 1 ) { const int mid = ( lo + hi ) >> 1; if( pfirst[mid] <= u ) lo = mid; else hi = mid; }
  const LevelsCloud& C = clouds[lo];
  const int orig = u - C.pfirst;
  const size_t i = scan[g];
  samples[i] = orig;
  const int slot = C.by_orig[orig];
  const float4 p = C.q.pos[slot];
  pos3[3 * i] = p.x; pos3[3 * i + 1] = p.y; pos3[3 * i + 2] = p.z;
  if( C.qnor ) { const float4 m = C.qnor[slot]; nor3[3 * i] = m.x; nor3[3 * i + 1] = m.y; nor3[3 * i + 2] = m.z; }
}

namespace {

struct LevelsWorkspace { Buf clouds, tables, word, later, state, totals, misc, offset, adj, front, flags, scan, tmp, bounds, samples, pos, nor; };
thread_local LevelsWorkspace g_levels_ws;

// what the device route leaves for its two entry points: the samples of all problems packed in the workspace (level-major)
struct LevelsResult
{
  levels::LevelsPlan P;
  std::vector<unsigned> bounds;        // n_problems + 1, packed order: sorted level * n_clouds + cloud
  std::vector<char> has_nor;           // per cloud
  int rounds = 0;
  int over_cloud = -1, over_level = -1; // RS_HIP_E_CAPACITY: the lowest problem with a point over its cap (the batch's cloud index, caller's level)
  unsigned first_of( int c, int l ) const { return bounds[(size_t)P.rank[l] * P.n_clouds + c]; }
  unsigned count_of( int c, int l ) const { const size_t p = (size_t)P.rank[l] * P.n_clouds + c; return bounds[p + 1] - bounds[p]; }
};

int levels_device( const rs_hip_cloud_t* const* bases, int32_t n_clouds, const float* radii, const int32_t* max_n_neigh, int32_t n_levels,
                   LevelsResult& out, hipStream_t st )
{
  char err[256] = "";
  LevelsWorkspace& W = g_levels_ws;
  levels::LevelsPlan& P = out.P;
  std::vector<int32_t> sizes( (size_t)n_clouds ), tiles( (size_t)n_clouds );
  for( int c = 0; c < n_clouds; ++c )
  {
    sizes[c] = bases[c] ? rs_hip_cloud_size( bases[c] ) : -1;
    tiles[c] = bases[c] ? rs_hip_cloud_tiles( bases[c] ) : 0;
  }
  if( int rc = levels::plan( sizes.data(), tiles.data(), n_clouds, radii, max_n_neigh, n_levels, P, err, sizeof(err) ) ) return fail( rc, err );
  const int NP = (int)P.n_points, NI = (int)P.n_ids, NL = n_levels, NC = n_clouds, n_prob = NC * NL;
  out.bounds.assign( (size_t)n_prob + 1, 0u );
  out.has_nor.assign( (size_t)NC, 0 );
  for( int c = 0; c < NC; ++c ) out.has_nor[c] = api_cloud_has_normals( bases[c] ) ? 1 : 0;
  out.rounds = 0;
  // (room for one point at least: an empty level of a base with normals is told from one without by its normals' pointer)
  RS_TRY( W.samples.ensure( 4 ), "levels_many: buffers" );
  RS_TRY( W.pos.ensure( 12 ), "levels_many: buffers" );
  RS_TRY( W.nor.ensure( 12 ), "levels_many: buffers" );
  if( NP == 0 ) return RS_HIP_OK;

  // the tables: clouds | tile_first | pfirst
  std::vector<LevelsCloud> hc( (size_t)NC );
  for( int c = 0; c < NC; ++c )
  {
    const CloudPoints cp = api_cloud_points( bases[c] );
    hc[c].tgt = *api_cloud_view( bases[c] ); hc[c].q = *api_cloud_query( bases[c] ); hc[c].qnor = cp.qnor; hc[c].by_orig = cp.by_orig;
    hc[c].pfirst = P.pfirst[c]; hc[c].n = sizes[c];
  }
  const size_t n1 = (size_t)NI + 1;
  const size_t tmp_bytes = std::max( build_scan_temp_bytes( n1 ), build_scan_temp_bytes( (size_t)NP + 1 ) );
  RS_TRY( W.clouds.ensure( (size_t)NC * sizeof(LevelsCloud) ), "levels_many: buffers" );
  RS_TRY( W.tables.ensure( 2 * ( (size_t)NC + 1 ) * 4 ), "levels_many: buffers" );
  RS_TRY( W.word.ensure( n1 * 4 ), "levels_many: buffers" );
  RS_TRY( W.later.ensure( n1 * 4 ), "levels_many: buffers" );
  RS_TRY( W.state.ensure( n1 * 4 ), "levels_many: buffers" );
  RS_TRY( W.totals.ensure( (size_t)n_prob * 8 + 8 ), "levels_many: buffers" );
  RS_TRY( W.misc.ensure( ( LEVELS_BATCH + 1 ) * 4 * 4 ), "levels_many: buffers" );
  RS_TRY( W.tmp.ensure( tmp_bytes + 256 ), "levels_many: buffers" );
  RS_TRY( W.bounds.ensure( ( (size_t)n_prob + 1 ) * 4 ), "levels_many: buffers" );
  LevelsCloud* d_clouds = W.clouds.as<LevelsCloud>();
  int* d_tile_first = W.tables.as<int>(); int* d_pfirst = d_tile_first + NC + 1;
  unsigned long long* d_totals = W.totals.as<unsigned long long>(); int* d_over = (int*)( d_totals + n_prob );
  RS_TRY( hipMemcpyAsync( d_clouds, hc.data(), (size_t)NC * sizeof(LevelsCloud), hipMemcpyHostToDevice, st ), "levels_many: tables" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( d_tile_first, P.tile_first.data(), ( (size_t)NC + 1 ) * 4, hipMemcpyHostToDevice, st ), "levels_many: tables" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( d_pfirst, P.pfirst.data(), ( (size_t)NC + 1 ) * 4, hipMemcpyHostToDevice, st ), "levels_many: tables" );
  std::vector<unsigned long long> totals( (size_t)n_prob + 1, 0ull ), zeros( (size_t)n_prob + 1, 0ull );
  { int* o = (int*)&zeros[(size_t)n_prob]; o[0] = INT_MAX; o[1] = 0; }         // the over-cap word follows the totals
  RS_TRY_DRAIN( st, hipMemcpyAsync( d_totals, zeros.data(), ( (size_t)n_prob + 1 ) * 8, hipMemcpyHostToDevice, st ), "levels_many: tables" );

  // 1. the counting pass
  LevelsSweep S{};
  S.clouds = d_clouds; S.tile_first = d_tile_first; S.cloud0 = 0; S.cloud1 = NC; S.tile0 = 0; S.n_tiles = (int)P.n_tiles;
  S.n_levels = NL; S.n_points = NP; S.radius_max = P.radius[NL - 1];
  for( int s = 0; s < MAX_LEVELS; ++s ) { S.rsq[s] = s < NL ? P.radius_sq[s] : -1.0f; S.cap[s] = s < NL ? P.cap[s] : INT_MAX; S.caller[s] = s < NL ? P.order[s] : 0; }
  S.word = W.word.as<int>(); S.later = W.later.as<int>(); S.totals = d_totals; S.over = d_over;
  {
    ProfSpan span( "levels_neighbours" );
    hipLaunchKernelGGL( k_levels_neighbours<false>, dim3( blocks_for( S.n_tiles, WAVES_PER_BLOCK ) ), dim3( BLOCK ), 0, st, S );
  }
  RS_TRY_DRAIN( st, hipGetLastError(), "levels_many: counting launch" );
  // 2. the first read-back: totals and the over-cap word
  RS_TRY_DRAIN( st, hipMemcpyAsync( totals.data(), d_totals, ( (size_t)n_prob + 1 ) * 8, hipMemcpyDeviceToHost, st ), "levels_many: read-back" );
  RS_TRY( hipStreamSynchronize( st ), "levels_many: counting pass" );
  {
    const int over = *(const int*)&totals[(size_t)n_prob];
    if( over != INT_MAX )
    {
      out.over_cloud = over / NL; out.over_level = over % NL;
      return RS_HIP_E_CAPACITY;                          // (the caller words it: it knows the cloud's index in its own list)
    }
  }
  std::vector<int64_t> rows( (size_t)NC );
  for( int c = 0; c < NC; ++c )
  {
    rows[c] = (int64_t)totals[(size_t)c * NL + ( NL - 1 )];
    if( rows[c] > levels::ENTRY_MAX )
    {
      snprintf( err, sizeof(err), "levels_many: cloud %d: %lld adjacency entries, more than a 32-bit row offset names", c, (long long)rows[c] );
      return fail( RS_HIP_E_CAPACITY, err );
    }
  }
  LevelsRounds R{};
  R.n_points = NP; R.n_levels = NL; R.later = S.later; R.word = S.word; R.state = W.state.as<int>();
  int lanes[MAX_LEVELS] = {};
  for( int s = 0; s < NL; ++s )
  {
    double sum = 0.0;
    for( int c = 0; c < NC; ++c ) sum += (double)totals[(size_t)c * NL + s];
    lanes[s] = levels::lane_class( sum / (double)NP );
    R.cls[s] = lanes[s] >= 64 ? 2 : ( lanes[s] >= 8 ? 1 : 0 );
  }
  std::vector<int32_t> gend;
  const int ng = levels::groups( rows.data(), NC, levels::ENTRY_BUDGET, gend );
  int* misc = W.misc.as<int>();                         // [step of the batch][class]: frontier lengths
  for( int gi = 0; gi < ng; ++gi )
  {
    const int ca = gi ? gend[gi - 1] : 0, cb = gend[gi];
    const int u0 = P.pfirst[ca], ng_pts = P.pfirst[cb] - u0;
    if( ng_pts == 0 ) continue;
    int64_t entries = 0;
    for( int c = ca; c < cb; ++c ) entries += rows[c];
    // list capacities: a class holds the ids of its levels
    size_t cls_cap[LEVELS_CLASSES] = { 0, 0, 0 };
    for( int s = 0; s < NL; ++s ) cls_cap[R.cls[s]] += (size_t)ng_pts;
    const size_t front_ints = 2 * ( cls_cap[0] + cls_cap[1] + cls_cap[2] ) + 16;
    RS_TRY( W.offset.ensure( ( (size_t)ng_pts + 1 ) * 4 ), "levels_many: buffers" );
    RS_TRY( W.adj.ensure( (size_t)std::max<int64_t>( 1, entries ) * 4 ), "levels_many: buffers" );
    RS_TRY( W.front.ensure( front_ints * 4 ), "levels_many: buffers" );
    // 3. row offsets of the group's points
    if( build_exclusive_scan( W.tmp.p, tmp_bytes, (const uint32_t*)( S.later + (size_t)( NL - 1 ) * NP + u0 ), W.offset.as<uint32_t>(), (size_t)ng_pts + 1, st ) )
    { (void)hipStreamSynchronize( st ); return fail( RS_HIP_E_RUNTIME, "levels_many: device scan failed" ); }
    // 4. the write pass
    S.cloud0 = ca; S.cloud1 = cb; S.tile0 = P.tile_first[ca]; S.n_tiles = P.tile_first[cb] - P.tile_first[ca];
    S.offset = W.offset.as<unsigned>(); S.u0 = u0; S.adj = W.adj.as<int>();
    {
      ProfSpan span( "levels_neighbours" );
      hipLaunchKernelGGL( k_levels_neighbours<true>, dim3( blocks_for( S.n_tiles, WAVES_PER_BLOCK ) ), dim3( BLOCK ), 0, st, S );
    }
    // 5. rounds
    R.u0 = u0; R.n_group = ng_pts; R.offset = S.offset; R.adj = S.adj;
    int* fr[2][LEVELS_CLASSES];
    { int* f = W.front.as<int>(); for( int b = 0; b < 2; ++b ) for( int k = 0; k < LEVELS_CLASSES; ++k ) { fr[b][k] = f; f += cls_cap[k]; } }
    RS_TRY_DRAIN( st, hipMemsetAsync( misc, 0, ( LEVELS_BATCH + 1 ) * 16, st ), "levels_many: rounds" );
    for( int k = 0; k < LEVELS_CLASSES; ++k ) R.front_out[k] = fr[0][k];
    R.count_out = misc;
    hipLaunchKernelGGL( k_levels_init, dim3( blocks_for( ng_pts, BLOCK ), NL ), dim3( BLOCK ), 0, st, R );
    // a block takes 256, 32 or 4 items of a class at a time; the first frontier can hold every id
    const long long most = std::min<long long>( 16384, std::max<long long>( 1, std::max<long long>( ( (long long)cls_cap[0] + 255 ) / 256, std::max<long long>( ( (long long)cls_cap[1] + 31 ) / 32, ( (long long)cls_cap[2] + 3 ) / 4 ) ) ) );
    int rounds = 0, blocks = (int)most; bool done = false, first = true;
    while( !done )
    {
      if( rounds > ng_pts + LEVELS_BATCH ) { (void)hipStreamSynchronize( st ); return fail( RS_HIP_E_RUNTIME, "levels_many: no fixed point" ); }
      if( !first ) RS_TRY_DRAIN( st, hipMemcpyAsync( misc, misc + 4 * LEVELS_BATCH, 16, hipMemcpyDeviceToDevice, st ), "levels_many: rounds" );
      RS_TRY_DRAIN( st, hipMemsetAsync( misc + 4, 0, LEVELS_BATCH * 16, st ), "levels_many: rounds" );
      {
        ProfSpan span( "levels_rounds" );
        for( int b = 0; b < LEVELS_BATCH; ++b )
        {
          const int r = rounds + b;
          for( int k = 0; k < LEVELS_CLASSES; ++k ) { R.front_in[k] = fr[r & 1][k]; R.front_out[k] = fr[( r + 1 ) & 1][k]; }
          R.count_in = misc + 4 * b; R.count_out = misc + 4 * ( b + 1 );
          hipLaunchKernelGGL( k_levels_frontier, dim3( std::max( 1, blocks ) ), dim3( BLOCK ), 0, st, R );
        }
      }
      int len[( LEVELS_BATCH + 1 ) * 4];
      RS_TRY_DRAIN( st, hipMemcpyAsync( len, misc, sizeof(len), hipMemcpyDeviceToHost, st ), "levels_many: rounds" );
      RS_TRY( hipStreamSynchronize( st ), "levels_many: rounds" );
      long long need = 1;
      for( int b = 0; b <= LEVELS_BATCH && !done; ++b )
      {
        const int* l = len + 4 * b;
        if( l[0] == 0 && l[1] == 0 && l[2] == 0 ) done = true;
        else { if( b < LEVELS_BATCH ) rounds++; need = std::max<long long>( need, std::max<long long>( ( l[0] + 255 ) / 256, std::max<long long>( ( l[1] + 31 ) / 32, ( l[2] + 3 ) / 4 ) ) ); }
      }
      blocks = (int)std::min<long long>( most, std::max<long long>( 256, 2 * need ) );   // the next batch's frontiers are about as wide as this one's
      first = false;
    }
    out.rounds = std::max( out.rounds, rounds );
  }
  // 6. the samples of every problem, packed
  RS_TRY( W.flags.ensure( n1 * 4 ), "levels_many: buffers" );
  RS_TRY( W.scan.ensure( n1 * 4 ), "levels_many: buffers" );
  {
    ProfSpan span( "levels_samples" );
    hipLaunchKernelGGL( k_levels_flags, dim3( blocks_for( (long long)NI + 1, BLOCK ) ), dim3( BLOCK ), 0, st, R.state, NI, W.flags.as<unsigned>() );
    if( build_exclusive_scan( W.tmp.p, tmp_bytes, W.flags.as<uint32_t>(), W.scan.as<uint32_t>(), n1, st ) )
    { (void)hipStreamSynchronize( st ); return fail( RS_HIP_E_RUNTIME, "levels_many: device scan failed" ); }
    hipLaunchKernelGGL( k_levels_bounds, dim3( blocks_for( n_prob + 1, BLOCK ) ), dim3( BLOCK ), 0, st, W.scan.as<unsigned>(), d_pfirst, NC, NL, NP, W.bounds.as<unsigned>() );
  }
  RS_TRY_DRAIN( st, hipMemcpyAsync( out.bounds.data(), W.bounds.p, ( (size_t)n_prob + 1 ) * 4, hipMemcpyDeviceToHost, st ), "levels_many: read-back" );
  RS_TRY( hipStreamSynchronize( st ), "levels_many: samples" );
  const size_t total = std::max<size_t>( 1, out.bounds[(size_t)n_prob] );
  RS_TRY( W.samples.ensure( total * 4 ), "levels_many: buffers" );
  RS_TRY( W.pos.ensure( total * 12 ), "levels_many: buffers" );
  RS_TRY( W.nor.ensure( total * 12 ), "levels_many: buffers" );
  {
    ProfSpan span( "levels_samples" );
    hipLaunchKernelGGL( k_levels_gather, dim3( blocks_for( NI, BLOCK ) ), dim3( BLOCK ), 0, st, W.flags.as<unsigned>(), W.scan.as<unsigned>(), d_clouds, d_pfirst, NC, NP, NI,
                        W.samples.as<int>(), W.pos.as<float>(), W.nor.as<float>() );
  }
  RS_TRY_DRAIN( st, hipGetLastError(), "levels_many: gather launch" );
  return RS_HIP_OK;
}

// the packed sample indices to the host, in one copy
int levels_samples_host( const LevelsResult& Rz, std::vector<int32_t>& host, hipStream_t st )
{
  const size_t total = Rz.bounds.empty() ? 0 : Rz.bounds.back();
  host.resize( total );
  if( total )
  {
    RS_TRY_DRAIN( st, hipMemcpyAsync( host.data(), g_levels_ws.samples.p, total * 4, hipMemcpyDeviceToHost, st ), "levels_many: download" );
    RS_TRY( hipStreamSynchronize( st ), "levels_many: download" );
  }
  return RS_HIP_OK;
}

// What a call hands back, held until nothing can fail any more: per problem (caller's order) the samples and, if asked for, the cloud.
struct LevelsOut
{
  std::vector<std::vector<int32_t>> idx;
  std::vector<int32_t> count;
  std::vector<rs_hip_cloud_t*> clouds;
  int rounds = 0;
  void undo() { for( rs_hip_cloud_t*& c : clouds ) { rs_hip_cloud_destroy( c ); c = nullptr; } }
};

int levels_over_cap( const char* who, int c, int l, int cap )
{
  char err[256];
  snprintf( err, sizeof(err), "%s: cloud %d, level %d: a point has more than max_n_neigh = %d points within the radius (a reference search would be truncated)", who, c, l, cap );
  return fail( RS_HIP_E_CAPACITY, err );
}

// Both entry points.  Bases of at most levels::SINGLE_ABOVE points are decided together (levels_device); a larger one takes the
// single call's path level by level, to the same result.
int levels_run( const char* who, const rs_hip_cloud_t* const* bases, int32_t n_clouds, const float* radii, const int32_t* max_n_neigh, const float* cell_sizes,
                int32_t n_levels, bool want_clouds, bool want_idx, LevelsOut& O )
{
  char err[256];
  if( n_clouds < 0 || n_levels < 0 || ( n_clouds > 0 && n_levels > 0 && ( !bases || !radii || !max_n_neigh ) ) )
  { snprintf( err, sizeof(err), "%s: bad arguments", who ); return fail( RS_HIP_E_ARG, err ); }
  // the host refusals, for the whole list
  {
    std::vector<int32_t> sizes( (size_t)n_clouds ), tiles( (size_t)n_clouds, 0 );
    for( int c = 0; c < n_clouds; ++c ) sizes[c] = bases[c] ? ( rs_hip_cloud_size( bases[c] ) <= levels::SINGLE_ABOVE ? rs_hip_cloud_size( bases[c] ) : 0 ) : -1;
    levels::LevelsPlan P;
    if( int rc = levels::plan( sizes.data(), tiles.data(), n_clouds, radii, max_n_neigh, n_levels, P, err, sizeof(err) ) ) return fail( rc, err );
  }
  const int n_prob = n_clouds * n_levels;
  O.idx.assign( (size_t)n_prob, {} ); O.count.assign( (size_t)n_prob, 0 ); O.clouds.assign( (size_t)n_prob, nullptr ); O.rounds = 0;
  if( n_prob == 0 ) return RS_HIP_OK;
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  std::vector<const rs_hip_cloud_t*> batch; std::vector<int> batch_c, single_c;
  for( int c = 0; c < n_clouds; ++c )
    if( rs_hip_cloud_size( bases[c] ) <= levels::SINGLE_ABOVE ) { batch.push_back( bases[c] ); batch_c.push_back( c ); } else single_c.push_back( c );
  // a large base through the single call; an over-cap is reported by its place in the caller's list
  auto single = [&]( int c, int l ) -> int
  {
    const size_t p = (size_t)c * n_levels + l;
    const int n = rs_hip_cloud_size( bases[c] );
    O.idx[p].assign( (size_t)std::max( 1, n ), 0 );
    int32_t cnt = 0, rounds = 0; int r = RS_HIP_OK;
    if( want_clouds )
    {
      O.clouds[p] = rs_hip_cloud_create_level( bases[c], radii[l], max_n_neigh[l], cell_sizes ? cell_sizes[l] : -1.0f, O.idx[p].data(), &cnt );
      if( !O.clouds[p] ) r = RS_HIP_E_RUNTIME;
    }
    if( !want_clouds || r )      // (the single call's cloud form has no code: the samples alone tell an over-cap from a failure)
    {
      const int r2 = rs_hip_level_samples( bases[c], radii[l], max_n_neigh[l], O.idx[p].data(), &cnt, &rounds );
      if( r2 == RS_HIP_E_CAPACITY ) return levels_over_cap( who, c, l, max_n_neigh[l] );
      if( r2 ) return r2;
      if( r ) return r;
    }
    O.idx[p].resize( (size_t)cnt ); O.count[p] = cnt; O.rounds = std::max( O.rounds, (int)rounds );
    return RS_HIP_OK;
  };
  if( !batch.empty() )
  {
    LevelsResult Rz;
    rc = levels_device( batch.data(), (int32_t)batch.size(), radii, max_n_neigh, n_levels, Rz, st );
    if( rc == RS_HIP_E_CAPACITY && Rz.over_cloud >= 0 )
    {
      // the text names the lowest problem that is over: a large base before that cloud may be one
      const int cb = batch_c[(size_t)Rz.over_cloud];
      std::vector<int32_t> tmp;
      for( int c : single_c )
      {
        if( c > cb ) break;
        tmp.assign( (size_t)rs_hip_cloud_size( bases[c] ), 0 );
        for( int l = 0; l < n_levels; ++l )
        {
          int32_t cnt = 0;
          if( rs_hip_level_samples( bases[c], radii[l], max_n_neigh[l], tmp.data(), &cnt, nullptr ) == RS_HIP_E_CAPACITY ) return levels_over_cap( who, c, l, max_n_neigh[l] );
        }
      }
      return levels_over_cap( who, cb, Rz.over_level, max_n_neigh[Rz.over_level] );
    }
    if( rc ) return rc;
    O.rounds = Rz.rounds;
    const int nb = (int)batch.size();
    std::vector<int32_t> host;
    if( want_idx && ( rc = levels_samples_host( Rz, host, st ) ) ) return rc;
    for( int b = 0; b < nb; ++b )
      for( int l = 0; l < n_levels; ++l )
      {
        const size_t p = (size_t)batch_c[(size_t)b] * n_levels + l;
        O.count[p] = (int32_t)Rz.count_of( b, l );
        if( want_idx && O.count[p] ) O.idx[p].assign( host.begin() + Rz.first_of( b, l ), host.begin() + Rz.first_of( b, l ) + O.count[p] );
      }
    if( want_clouds )
    {
      // one batched index build over the packed segments
      const size_t m = (size_t)nb * n_levels;
      std::vector<int64_t> first( m ), count( m );
      std::vector<int32_t> has_nor( m );
      std::vector<float> cells( m );
      for( int b = 0; b < nb; ++b )
        for( int l = 0; l < n_levels; ++l )
        {
          const size_t k = (size_t)b * n_levels + l;
          first[k] = Rz.first_of( b, l ); count[k] = Rz.count_of( b, l ); has_nor[k] = Rz.has_nor[(size_t)b]; cells[k] = cell_sizes ? cell_sizes[l] : -1.0f;
        }
      std::vector<rs_hip_cloud_t*> made( m, nullptr );
      {
        ProfSpan span( "levels_build" );
        rc = api_clouds_from_device_each( g_levels_ws.pos.as<float>(), g_levels_ws.nor.as<float>(), first.data(), count.data(), has_nor.data(), cells.data(), (int32_t)m, made.data() );
      }
      if( rc ) { (void)hipStreamSynchronize( st ); return rc; }
      for( int b = 0; b < nb; ++b )
        for( int l = 0; l < n_levels; ++l ) O.clouds[(size_t)batch_c[(size_t)b] * n_levels + l] = made[(size_t)b * n_levels + l];
    }
  }
  for( int c : single_c )
    for( int l = 0; l < n_levels; ++l )
      if( ( rc = single( c, l ) ) ) { O.undo(); return rc; }
  return RS_HIP_OK;
}

} // namespace

} // namespace rs

using namespace rs;

extern "C" {

int rs_hip_level_samples_many( const rs_hip_cloud_t* const* bases, int32_t n_clouds, const float* radii, const int32_t* max_n_neigh, int32_t n_levels,
                               int32_t* const* sample_idx, int32_t* n_samples, int32_t* n_rounds )
{
  if( n_clouds > 0 && n_levels > 0 && ( !sample_idx || !n_samples ) ) return fail( RS_HIP_E_ARG, "level_samples_many: the sample arrays and their counts are required" );
  LevelsOut O;
  if( int rc = levels_run( "level_samples_many", bases, n_clouds, radii, max_n_neigh, nullptr, n_levels, false, true, O ) ) return rc;
  for( size_t p = 0; p < O.count.size(); ++p )
  {
    n_samples[p] = O.count[p];
    if( sample_idx[p] && O.count[p] ) std::memcpy( sample_idx[p], O.idx[p].data(), (size_t)O.count[p] * 4 );
  }
  if( n_rounds ) *n_rounds = O.rounds;
  return RS_HIP_OK;
}

int rs_hip_cloud_create_levels_many( const rs_hip_cloud_t* const* bases, int32_t n_clouds, const float* radii, const int32_t* max_n_neigh, const float* cell_sizes,
                                     int32_t n_levels, rs_hip_cloud_t** out, int32_t* const* sample_idx, int32_t* n_samples )
{
  if( n_clouds > 0 && n_levels > 0 && !out ) return fail( RS_HIP_E_ARG, "cloud_create_levels_many: the array of clouds is required" );
  LevelsOut O;
  if( int rc = levels_run( "cloud_create_levels_many", bases, n_clouds, radii, max_n_neigh, cell_sizes, n_levels, true, sample_idx != nullptr, O ) ) return rc;
  for( size_t p = 0; p < O.count.size(); ++p )
  {
    out[p] = O.clouds[p];
    if( n_samples ) n_samples[p] = O.count[p];
    if( sample_idx && sample_idx[p] && O.count[p] ) std::memcpy( sample_idx[p], O.idx[p].data(), (size_t)O.count[p] * 4 );
  }
  return RS_HIP_OK;
}

} // extern "C"
