// librescan_hip device code (gfx950, wave64) — ICP estimators: the reference's seven centroid sums as grid chains (scans) and lane chains (objects), and the plain step's fp64 moments (lib/rs/icp.h:136-148)
#define RS_TAIL_DBG_MOM 1    // (diagnostic builds: this unit holds k_plain_moments' stamps, rs_tail_dbg.h)
#include "rs_icp_estimate.h"

namespace rs {

// ------------------------------------------------------------------------------------------
// Grid chains: the reference's seven centroid sums (icp.h:136-148), bit for bit, at the cost of a reduction
//
// A sequential fp32 sum  s <- RN( s + x )  is an INTEGER sum while s stays inside one binade: with u = ulp( s ), s = M u,
// RN( s + x ) = ( M + rndne( x / u ) ) u  unless x / u sits exactly half way between two integers (then the parity of M decides) —
// and integer addition is associative.  So for a stretch of addends and an exponent E the whole effect on the chain is three
// integers: D = Σ rndne( x_i / u ) and the smallest / largest partial sum, which say for which start mantissas M the chain stays
// inside the binade all the way (a margin of one grid step at the ends keeps clear of the neighbouring binades' grids).  Such
// records compose (intervals intersect, advances add).  A tie is part of the record too (ChainFn below: what it adds depends on the
// parity of the start alone).  The only sequential part left is the handful of places where the chain really changes binade (~15
// times on the way from 0 to 2^21) or sign: there the addends of one segment are added one after the other in fp32.
//
//   the searches    leave one 48-byte record per source point at the point's ORIGINAL index (icp_emit);
//   k_chain_segrecs one record per (segment of 64 points, chain): the functions for the binades e-1, e, e+1 around a guess e of the
//                   running sum's exponent there, and what the segment adds (the guessed binade's own advance, i.e. the chain's sum
//                   with its rounding drift — what the walks forecast with);
//   k_chain_compose a block's 64 segment records composed (per chain and binade), the quarter blocks' sums;
//   k_chain_walk_and_moments   ONE launch for three things that do not need each other:
//       the walks   one workgroup per chain (chain_walk_row: forecasts, fetches, the walk proper — ~35 us for a 1 M-point scan);
//       the moments the fp64 moments of k_icp_moments, read from the records in the reference's order (a quarter block per workgroup);
//       the guesses for the NEXT iteration's records, from this iteration's sums (k_chain_guess's work, a block per workgroup);
//   k_icp_update_wide   finishes the iteration (icp.h:253-295,455-493), centred on the chains' centroids.
// The first iteration has no guesses yet: k_chain_moments (with the segments' fp64 sums) and k_chain_guess run before the records,
// k_chain_walk alone after them.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__( BLOCK ) void k_chain_moments( IcpLaunch L, ChainBufs B )
{
  RS_CHAIN_SETPRIO();
  __shared__ ChainMomLds S;
  const int prob = blockIdx.y;
  if( L.active[prob] == 0 ) return;
  chain_moments_block( L, B, prob, blockIdx.x, S, L.rec + (size_t)prob * L.src.n * REC_F4 );
}

// The plain step's moments WITHOUT records (round 10): what a plain iteration needs of a correspondence is its weight and the 35 addends,
// in no particular order — so its search writes no 48-byte record (L.rec == null: slot, dist² and dot only, 12 B per point, coalesced by
// query slot) and this kernel forms the addends from what the search leaves for everyone else: one wave per source tile, the source point
// under the current pose by icp_query's float operations, the match's position and normal gathered from the target.  The weight is
// chain_addends', the addends are moments_add's: every addend has the bits k_chain_moments gives it, only the order of the fp64
// additions differs — and that order is a function of the launch's shape alone (wave w of workgroup b takes the tiles
// plain_first + k * plain_stride of its range, lanes are added by wave_sums, the four waves in turn, the workgroups' partials by
// k_icp_update_wide): two runs give the same bits.
// The tiles are walked as the warm searches walk them (k_icp_corr<true>: natural_tile): workgroups are dealt round-robin over the 8 XCDs,
// and XCD class c = b mod 8 takes the c-th eighth of the source's (Hilbert) tile order, so the target lines an XCD gathers are the ones its
// L2 holds from the search.  (Behind the cold search, which deals the order out in chunks, they are not; this walk stays as it is all the
// same: which wave takes which tile IS the order of the fp64 additions.  FETCH_SIZE unchanged, profiles/r20.)  RS_PLAIN_XCD=0: plain
// striding (measurements).
#ifndef RS_PLAIN_XCD
#define RS_PLAIN_XCD 1
#endif
#ifndef RS_PLAIN_MAX_BLOCKS
#define RS_PLAIN_MAX_BLOCKS 512
#endif
constexpr int PLAIN_MAX_BLOCKS = RS_PLAIN_MAX_BLOCKS;     // workgroups per problem at most: two per CU (two waves per SIMD), 35 x 512 partials for k_icp_update_wide instead of 35 x n / 1 024.
// (With two waves on a SIMD the kernel is bound by its fp64 instructions — ~280 per tile and wave, 4 cycles each: while one wave waits for
//  its gathers the other adds.  Round 11 tried the loads as a pipeline ahead of the arithmetic — gathers one tile ahead, point words two,
//  counted waits — and 1 024 workgroups again: 14.5 against 14.8 us alone on the chip, nothing in the bench; 1 024: slower.  DESIGN §3.)
constexpr int PLAIN_TILES_PER_WAVE = 4;    // ... and no fewer tiles per wave than this while the grid is below that
int plain_moment_blocks( int n_tiles )
{
  const int b = ( std::max( n_tiles, 1 ) + WAVES_PER_BLOCK * PLAIN_TILES_PER_WAVE - 1 ) / ( WAVES_PER_BLOCK * PLAIN_TILES_PER_WAVE );
  return std::min( PLAIN_MAX_BLOCKS, ( b + 7 ) & ~7 );        // (a multiple of 8: every XCD class gets the same number of workgroups)
}
__global__ __launch_bounds__( BLOCK ) void k_plain_moments( IcpLaunch L )
{
  RS_CHAIN_SETPRIO();
  __shared__ double red[WAVES_PER_BLOCK][ICP_NMOM];
  __shared__ unsigned long long s_stat[WAVES_PER_BLOCK][3];
  const int prob = blockIdx.y;
  if( L.active[prob] == 0 ) return;
  icp_bind( L, prob );
  // (block 0 leaves n, mean, stddev and the queue's length in L.res for icp_update_tail, as chain_moments_block does)
  const float sd = chain_stats( L, prob, s_stat, ( blockIdx.x == 0 && threadIdx.x == 0 ) ? L.res + (size_t)prob * ICP_NRES + ICP_NMOM : nullptr );
  const bool use_sd = sd > 0.000001;
  const float cut = 2.5f * sd;
  Xform T1;
#pragma unroll
  for( int k = 0; k < 16; ++k ) T1.m[k] = L.T1[prob * 16 + k];
  const int lane = threadIdx.x & ( WAVE - 1 ), wib = uni( (int)threadIdx.x / WAVE );
  const int n_tiles = L.src.n_tiles;
#if RS_PLAIN_XCD
  const int per = ( n_tiles + 7 ) / 8, cls = (int)blockIdx.x & 7;
  const int t_end = min( n_tiles, ( cls + 1 ) * per ), stride = ( (int)gridDim.x >> 3 ) * WAVES_PER_BLOCK;
  int t = cls * per + ( (int)blockIdx.x >> 3 ) * WAVES_PER_BLOCK + wib;
#else
  const int t_end = n_tiles, stride = (int)gridDim.x * WAVES_PER_BLOCK;
  int t = (int)blockIdx.x * WAVES_PER_BLOCK + wib;
#endif

  double acc[ICP_NMOM];
#pragma unroll
  for( int k = 0; k < ICP_NMOM; ++k ) acc[k] = 0.0;
  // what a lane reads of its point by query slot (coalesced); the next tile's are on their way while this tile's gathers are
  struct Pt { int slot; float d2, dot; float4 p; };
  auto fetch = [&]( int tt ) -> Pt
  {
    Pt r; r.slot = -1; r.d2 = 0.0f; r.dot = 0.0f; r.p = make_float4( 0.0f, 0.0f, 0.0f, 0.0f );
    if( tt < t_end )
    {
      const int i = (int)L.src.tiles[tt] + lane;
      if( i < (int)L.src.tiles[tt + 1] )
      {
        const size_t o = (size_t)L.pt_off + i;
        r.slot = L.m_slot[o]; r.d2 = L.m_d2[o]; r.dot = L.m_dot[o]; r.p = L.src.pos[i];
      }
    }
    return r;
  };
#if RS_TAIL_DBG
  const int td_wave = (int)blockIdx.x * WAVES_PER_BLOCK + wib;
  unsigned long long* const dbg = ( prob == 0 && lane == 0 && td_wave < TD_WAVES ) ? d_mom_dbg[L.iter_index & ( TD_ITERS - 1 )][td_wave] : nullptr;
  int td_tile = 0;
#endif
  TD_STAMP( dbg, 0 );
  Pt cur = fetch( t );
  TD_STAMP( dbg, 1 );
  for( ; t < t_end; t += stride )
  {
    const Pt nxt = fetch( t + stride );
    if( cur.slot >= 0 )
    {
      const float4 q4 = L.tgt.pos[cur.slot], n4 = L.tgt.nor[cur.slot];
      float w = ( 1.0f - __fdiv_rn( cur.d2, L.radius ) ) * cur.dot;         // chain_addends' weight (icp.h:387,396-401)
      if( use_sd && cur.d2 > cut ) w = 0.0f;
      float tx, ty, tz, px, py, pz;
      xform3( T1, cur.p.x, cur.p.y, cur.p.z, 1.0f, tx, ty, tz );           // icp_query's float operations
      xform3( L.T2i, tx, ty, tz, 1.0f, px, py, pz );
      moments_add( acc, w, px, py, pz, q4, n4 );
    }
    cur = nxt;
#if RS_TAIL_DBG
    if( td_tile < TD_TILES ) TD_STAMP( dbg, 2 + td_tile );
    ++td_tile;
#endif
  }
  TD_STAMP( dbg, 13 );
  { const double v = wave_sums( acc, lane ); if( lane < ICP_NMOM ) red[wib][lane] = v; }
  __syncthreads();
  if( threadIdx.x < ICP_NMOM )
  {
    double v = 0.0;
    for( int w = 0; w < WAVES_PER_BLOCK; ++w ) v += red[w][threadIdx.x];
    L.mom_part[( (size_t)prob * ICP_NMOM + threadIdx.x ) * L.n_mom_blocks + blockIdx.x] = v;      // (moment-major, as k_chain_moments: L.n_mom_blocks == gridDim.x)
  }
#if RS_TAIL_DBG
  TD_STAMP( dbg, 14 );
  if( dbg ) dbg[15] = (unsigned long long)td_tile;
#endif
}

// (CH_M_LO, CH_M_HI, ChainFn, chain_never, chain_identity, chain_prefix: rs_icp_estimate.h)
__device__ __forceinline__ int chain_tau( int tau, int parity ) { return ( tau >> ( 2 * ( parity & 1 ) ) ) & 3; }
// the function of a record for the (biased) exponent E and sign bit sg of the running value
__device__ __forceinline__ ChainFn chain_select( const ChainRec& r, int E, int sg )
{
  const int c = E - ( r.e_sign & 255 ) + 1;
  ChainFn f = chain_never();
  if( ( ( r.e_sign >> 8 ) & 1 ) == sg )
  {
    int d = 0;
    if( c == 0 ) { f.lo = r.lo[0]; f.hi = r.hi[0]; d = r.D[0]; }
    if( c == 1 ) { f.lo = r.lo[1]; f.hi = r.hi[1]; d = r.D[1]; }
    if( c == 2 ) { f.lo = r.lo[2]; f.hi = r.hi[2]; d = r.D[2]; }
    f.D = d >> 4; f.tau = d & 15;
  }
  return f;
}
// ... for the binade of the value with the bits vb.  A value of exactly zero has no binade: it stays zero through a stretch whose
// addends are ALL zero (bit 16 of e_sign — the unmatched points a scan may well begin with; without it every such segment would be
// added up addend by addend), anything else from there is added one by one (as are denormals, inf and NaN).
#define CH_ALL_ZERO ( 1 << 16 )
__device__ __forceinline__ ChainFn chain_fn_for( const ChainRec& r, uint32_t vb )
{
  const int E = (int)( ( vb >> 23 ) & 255u ), sg = (int)( vb >> 31 );
  if( E == 0 ) return ( ( vb << 1 ) == 0u && ( r.e_sign & CH_ALL_ZERO ) ) ? chain_identity() : chain_never();
  if( E == 255 ) return chain_never();
  return chain_select( r, E, sg );
}

// The guesses (refresh iterations): every chain's fp64 prefix at each segment's start — the quarter blocks before from their sums,
// then a scan of the block's own 64 segment sums — kept as exponent | sign << 8 per (chain, segment).  One workgroup per block.
__device__ __forceinline__ void chain_guess_block( const IcpLaunch& L, const ChainBufs& B, int prob, int blk, int n_waves )
{
  const int lane = threadIdx.x & ( WAVE - 1 );
  for( int r = threadIdx.x / WAVE; r < CH_ROWS; r += n_waves )
  {
    const double* bsum = B.blksum + ( (size_t)prob * CH_ROWS + r ) * ( B.n_blk * CH_QUARTERS );
    double before = 0.0;
    for( int b = lane; b < blk * CH_QUARTERS; b += WAVE ) before += bsum[b];
    before = wave_sum( before );
    const int seg = blk * CH_BLK + lane;
    const double v = seg < B.n_seg ? B.segsum[( (size_t)prob * CH_ROWS + r ) * B.n_seg + seg] : 0.0;
    const double incl = wave_scan_f64( v, lane );
    const uint32_t gb = __float_as_uint( (float)( before + ( incl - v ) ) );
    if( seg < B.n_seg ) B.guess[( (size_t)prob * CH_ROWS + r ) * B.n_seg + seg] = (int)( ( ( gb >> 23 ) & 255u ) | ( ( gb >> 31 ) << 8 ) );
  }
}
__global__ __launch_bounds__( CH_ROWS * WAVE ) void k_chain_guess( IcpLaunch L, ChainBufs B )
{
  RS_CHAIN_SETPRIO();
  const int prob = blockIdx.y;
  if( L.active[prob] == 0 ) return;
  chain_guess_block( L, B, prob, blockIdx.x, CH_ROWS );
}

// The block records: a block's 64 segment records composed per chain and exponent (around the block's first guess), and the quarter
// blocks' sums of the segments' (the walks' forecasts, the next guesses).
__device__ __forceinline__ void chain_rec_copy_fwd( ChainRec& d, const ChainRec& r )
{
  d.e_sign = r.e_sign;
#pragma unroll
  for( int c = 0; c < 3; ++c ) { d.lo[c] = r.lo[c]; d.hi[c] = r.hi[c]; d.D[c] = r.D[c]; }
}
// One workgroup per (block, chain): three waves, one per binade; the first also sums the quarters.  (One workgroup per block with all
// seven chains — 21 scans over 8 waves, 18 KB staged — took 11 us per launch, nearly all of it the latency of that one workgroup's
// load -> scans -> store; 2 000 small ones take 7.)
__device__ __forceinline__ void chain_compose_block( const ChainBufs& B, int prob, int blk, int r )
{
  const int lane = threadIdx.x & ( WAVE - 1 ), c = uni( (int)threadIdx.x / WAVE );
  const int seg = blk * CH_BLK + lane;
  ChainRec mine; mine.e_sign = -1;
  const ChainRec* src = B.seg + ( (size_t)prob * CH_ROWS + r ) * B.n_seg;
  chain_rec_copy_fwd( mine, src[min( seg, B.n_seg - 1 )] );
  if( seg >= B.n_seg ) mine.e_sign = -1;                                  // (past the end of the cloud)
  if( c == 0 )
  {
    const double v = seg < B.n_seg ? B.segsum[( (size_t)prob * CH_ROWS + r ) * B.n_seg + seg] : 0.0;
    // the quarter blocks' sums: a row of 16 lanes each (fixed order: lane 0's quad tree)
    double q = v;
    q += dpp_d<RS_DPP_QUAD_XOR1, 0xf>( 0.0, q ); q += dpp_d<RS_DPP_QUAD_XOR2, 0xf>( 0.0, q );
    q += dpp_d<RS_DPP_HALF_MIRROR, 0xf>( 0.0, q ); q += dpp_d<RS_DPP_ROW_MIRROR, 0xf>( 0.0, q );
    if( ( lane & 15 ) == 0 ) B.blksum[( (size_t)prob * CH_ROWS + r ) * ( B.n_blk * CH_QUARTERS ) + blk * CH_QUARTERS + ( lane >> 4 )] = q;
  }
  const int first = __builtin_amdgcn_readlane( mine.e_sign, 0 );
  const int E = ( first & 255 ) - 1 + c, sg = ( first >> 8 ) & 1;
  const bool all_zero = RS_BALLOT( mine.e_sign != -1 && !( mine.e_sign & CH_ALL_ZERO ) ) == 0ull;
  const ChainFn f0 = mine.e_sign == -1 ? chain_identity() : chain_select( mine, E, sg );
  ChainFn f = chain_prefix( f0, lane );
  // the ties inside, in order: what the block adds for an even / an odd start (each record's tau picked by the parity of ITS start)
  unsigned long long tm = RS_BALLOT( f0.tau != 0 );
  const int ex = f.D - f0.D;
  int t0 = 0, t1 = 0, tmax = 0;
  while( tm != 0ull )
  {
    const int k = __builtin_ctzll( tm ); tm &= tm - 1ull;
    const int exk = __builtin_amdgcn_readlane( ex, k ), tk = __builtin_amdgcn_readlane( f0.tau, k );
    t0 += chain_tau( tk, exk + t0 ); t1 += chain_tau( tk, 1 + exk + t1 ); tmax += max( tk & 3, tk >> 2 );
  }
  if( lane == WAVE - 1 )
  {
    ChainRec* out = B.blk + ( (size_t)prob * CH_ROWS + r ) * B.n_blk + blk;
    if( c == 0 ) out->e_sign = ( first & 0x1ff ) | ( all_zero ? CH_ALL_ZERO : 0 );
    const int hi = f.hi - tmax;
    const bool ok = f.lo <= hi && t0 <= 3 && t1 <= 3;                   // (a never-record has lo > hi already)
    out->lo[c] = ok ? f.lo : CH_M_HI; out->hi[c] = ok ? hi : CH_M_LO; out->D[c] = ok ? f.D * 16 + t0 + 4 * t1 : 0;
  }
}

// The segment records: a wave stages THREE consecutive segments' addends in LDS (lane = point), then lane = (segment, exponent
// class, chain) runs down its segment's 64 addends in integers — no cross-lane traffic, 63 records at once.  The guesses are the
// kept ones (k_chain_guess): between two ICP iterations the sums move by a few per cent at most (the radius shrinks by 5 %, a per
// cent of the correspondences change), far less than the factor of two a record's three exponents cover.
#define CHAIN_REC_TASK 3          // segments per wave and round
#define CHAIN_REC_ROUNDS 1
__global__ __launch_bounds__( BLOCK ) void k_chain_segrecs( IcpLaunch L, ChainBufs B )
{
  RS_CHAIN_SETPRIO();
  // (rows of 65: lane = (segment, class, chain) reads row (segment, chain) at column j — with rows of 64 all 21 rows' column j sit in
  //  ONE bank, a 21-way conflict on every read of the loop below)
  __shared__ float s_x[WAVES_PER_BLOCK][CHAIN_REC_TASK][CH_ROWS][CH_SEG + 1];
  __shared__ int s_zero[WAVES_PER_BLOCK][CHAIN_REC_TASK][CH_ROWS];           // all 64 addends of (segment, chain) are zero
  __shared__ unsigned long long s_stat[WAVES_PER_BLOCK][3];
  const int prob = blockIdx.y;
  if( L.active[prob] == 0 ) return;
  const int lane = threadIdx.x & ( WAVE - 1 ), wib = threadIdx.x / WAVE;
  // (CHAIN_REC_ROUNDS tasks per wave, the loads of all first.  One: with two — the second's loads in flight while the first is worked on,
  //  half as many waves — the launch took 29 us instead of 25: the kernel is bound by its ~1 100 vector instructions per task, not by
  //  the loads.)
  const float4* R = L.rec + (size_t)prob * L.src.n * REC_F4;
  float4 A2[CHAIN_REC_ROUNDS][CHAIN_REC_TASK], Q2[CHAIN_REC_ROUNDS][CHAIN_REC_TASK];
#pragma unroll
  for( int t = 0; t < CHAIN_REC_ROUNDS; ++t )
#pragma unroll
    for( int q = 0; q < CHAIN_REC_TASK; ++q )               // (the loads first: the cut's reduction below runs while they are in flight)
    {
      const int sg = ( ( blockIdx.x * CHAIN_REC_ROUNDS + t ) * WAVES_PER_BLOCK + wib ) * CHAIN_REC_TASK + q, i = sg * CH_SEG + lane;
      const size_t ic = (size_t)min( i, L.src.n - 1 );
      A2[t][q] = R[ic * REC_F4]; Q2[t][q] = R[ic * REC_F4 + 1];
      if( sg >= B.n_seg || i >= L.src.n ) { A2[t][q] = make_float4( 0.0f, 0.0f, 0.0f, -1.0f ); Q2[t][q] = make_float4( 0.0f, 0.0f, 0.0f, 0.0f ); }
    }
  const float sd = chain_stats( L, prob, s_stat, nullptr );                  // (its own: in the iterations that keep their guesses this kernel runs BEFORE the moments)
  ChainPar P; P.use_sd = sd > 0.000001; P.cut = 2.5f * sd; P.max_dist = L.radius;
#pragma unroll
  for( int t = 0; t < CHAIN_REC_ROUNDS; ++t )
  {
  const int task = ( blockIdx.x * CHAIN_REC_ROUNDS + t ) * WAVES_PER_BLOCK + wib, seg0 = task * CHAIN_REC_TASK;
  if( t > 0 ) wave_lds_fence();                                              // (the round before has read its rows)
#pragma unroll
  for( int q = 0; q < CHAIN_REC_TASK; ++q )
  {
    float x[CH_ROWS], w;
    chain_addends( A2[t][q], Q2[t][q], P, x, w );
#pragma unroll
    for( int r = 0; r < CH_ROWS; ++r )
    {
      s_x[wib][q][r][lane] = x[r];
      const unsigned long long nz = RS_BALLOT( x[r] != 0.0f );
      if( lane == 0 ) s_zero[wib][q][r] = nz == 0ull ? CH_ALL_ZERO : 0;
    }
  }
  wave_lds_fence();
  const int q = lane / ( CH_ROWS * 3 ), combo = lane % ( CH_ROWS * 3 );
  const int r = combo % CH_ROWS, c = combo / CH_ROWS;
  const int seg = seg0 + q;
  if( q < CHAIN_REC_TASK && seg < B.n_seg )
  {
  const int es = B.guess[( (size_t)prob * CH_ROWS + r ) * B.n_seg + seg];
  const int eg = es & 255, sg = es >> 8;
  const int E = eg - 1 + c;                                            // s = M * 2^(E - 150), M in [2^23, 2^24)
  int Pj = 0, pmin = 0, pmax = 0;                                      // partial sums, the start included
  const bool bad_e = E < 1 || E > 254;
  bool odd = bad_e, big = bad_e, seen = false;
  int cpar = 0;
  const float* xs = &s_x[wib][q][r][0];
#pragma unroll 8
  for( int j = 0; j < CH_SEG; ++j )
  {
    const float xv = xs[j];
    const float y = ldexpf( sg ? -xv : xv, 150 - E );                  // x / ulp( s ): exact (a power of two), or 0 / inf at the ends; the chain of |s| for negative s
    const float rn = rintf( y );                                       // to nearest, ties to even
    odd |= (int)!( fabsf( y ) < 8388608.0f ) | (int)( fabsf( y - rn ) == 0.5f );  // too big for this binade (or NaN), or a tie: M's parity decides
    Pj += (int)rn;
    pmin = min( pmin, Pj ); pmax = max( pmax, Pj );
  }
  float fsum = 0.0f;
  if( odd )        // one segment in a few hundred: again, telling the two apart and taking the ties as they fall (see ChainFn)
  {
    Pj = 0; pmin = 0; pmax = 0;
    int Pfa = 0;
    for( int j = 0; j < CH_SEG; ++j )
    {
      const float xv = xs[j];
      const float y = ldexpf( sg ? -xv : xv, 150 - E );
      const float rn = rintf( y );
      big |= !( fabsf( y ) < 8388608.0f );
      if( fabsf( y - rn ) == 0.5f )                                    // to the even neighbour
      {
        const int kl = (int)floorf( y );
        if( !seen ) { seen = true; cpar = ( Pj + kl ) & 1; Pj += kl; Pfa = Pj; }      // M + Pj + ( ( M + cpar ) & 1 ): even from here on, = "M' + ( Pj - Pfa )"
        else Pj += kl + ( ( Pj - Pfa + kl ) & 1 );
      }
      else Pj += (int)rn;
      pmin = min( pmin, Pj ); pmax = max( pmax, Pj );
      fsum += xv;
    }
    pmax += seen ? 1 : 0;
  }
  const bool bad = big;
  // What the segment adds to the chain, for the walks' forecasts of where the chain changes binade (chain_walk_row) and for the
  // next iteration's guesses: the guessed binade's own advance — D grid steps, i.e. the CHAIN's sum, its rounding drift included —
  // or, where the addends do not fit that grid, their plain sum.
  if( c == 1 )
    B.segsum[( (size_t)prob * CH_ROWS + r ) * B.n_seg + seg] = big ? (double)fsum : ldexp( (double)( sg ? -Pj : Pj ), E - 150 );
  // every value on the way, the start included, at least one grid step inside the binade: the neighbouring binades' grids
  // (half / twice as fine) then play no part in any of the roundings
  long long lo = (long long)CH_M_LO + 1 - pmin, hi = (long long)CH_M_HI - 1 - pmax;
  lo = lo < CH_M_LO ? CH_M_LO : lo; hi = hi > CH_M_HI ? CH_M_HI : hi;
  const bool ok = !bad && lo <= hi;
  ChainRec* out = B.seg + ( (size_t)prob * CH_ROWS + r ) * B.n_seg + seg;
  if( c == 0 ) out->e_sign = es | s_zero[wib][q][r];
  out->lo[c] = ok ? (int)lo : CH_M_HI; out->hi[c] = ok ? (int)hi : CH_M_LO; out->D[c] = ok ? Pj * 16 + ( seen ? ( cpar ? 1 : 4 ) : 0 ) : 0;      // tau = { cpar, 1 - cpar }
  }
  }
}

// (One launch per block.  Having the k_chain_segrecs workgroup that completes a block compose it — a counter per block, the last of
//  its six or seven to arrive — was tried: correct, and 300 us per launch instead of 25 + 11, because the 1 500 workgroups' release
//  fences each write back their XCD's L2, which the search has just filled with dirty records.)
__global__ __launch_bounds__( 3 * WAVE ) void k_chain_compose( IcpLaunch L, ChainBufs B )
{
  RS_CHAIN_SETPRIO();
  const int prob = blockIdx.y;
  if( L.active[prob] == 0 ) return;
  chain_compose_block( B, prob, blockIdx.x, blockIdx.z );
}

// One chain walked by a workgroup of four waves.  `s` (wave 0's, uniform) is the exact running value.
//
// What a walk costs is set by two things.  Memory latency: a block that does not fit needs its segments' records, the segment that
// does not fit its 64 addends — two dependent round trips of ~2 us, ~20 times per chain.  And instruction issue: ONE wave issues
// ~250 instructions per microsecond, a wave-wide scan of 64 records is ~130.  So the walk FORECASTS where the chain will change
// binade, fetches ahead — every load of a round in flight together, the work of a round shared by the four waves — and has
// everything around a forecast crossing composed into single records beforehand.  Per 512 blocks (2 M source points):
//   1  the blocks' sums (quarter sums: k_chain_compose) and records.  The forecast of the chain at every block's start = the exact
//      value so far + the prefix of the blocks' sums (the records' own advances, their rounding drift included: k_chain_segrecs);
//      of each block record only the function for the forecast's binade is kept (S.ones); the first CH_PRE_BLKS blocks inside which
//      the forecast comes within CH_EPS of a power of two (or of zero) are the "fetched" blocks;
//   2  their segment records and sums: the same forecast by segments; the runs of segments between two forecast crossings composed
//      into one record each, for the binade the forecast has there (S.piece: one segmented scan per block);
//   3  the addends and the records of the first CH_PRE_SEGS segments the forecasts point at (S.xs, S.fseg).
// The walk then: a wave-wide scan over 64 block functions at a time; a fetched block piece by piece and crossing by crossing, one
// record each; a segment whose record does not hold the value is added up addend by addend (the reference's own operations).
// Whatever was not forecast (off by more than CH_EPS, more crossings than fit) is fetched when the walk gets there and scanned.
#define CH_PRE_BLKS 12
#define CH_PRE_SEGS 32
#define CH_SUPER 8                 // chunks of 64 blocks per round of forecasts
#define CH_EPS ( 1.0f / 2048.0f )
#define CH_CHK_MAX 4096            // (RS_HIP_CHAIN_DEBUG) steps of a walk logged for the self-check
#ifndef CH_BUDGET
#define CH_BUDGET 384              // segments a walk may add up addend by addend before it gives the problem up (ChainBufs::failed)
#endif
#define CH_PIECES 16               // pieces of a fetched block
#define CH_PIECE_BIG ( 1 << 27 )
struct ChainPiece { int es, lo, hi, D; };      // exponent | sign << 8 it is made for; M -> M + D [+ tau: ptau / bptau] for lo <= M <= hi
struct ChainOne { int es, lo, hi, Dt; };       // a block record's function for one binade: Dt = D * 16 + tau
// One step of the walk, made ahead: the record of a run of blocks / of a run of segments / of a segment the forecast has a crossing
// in, for the binade the forecast has there (tp: ChainWalkLds::ptau's form) — and what to fall back on when it does not hold the value:
// kind = type | chunk << 2 | block in chunk << 5 | from (or the segment) << 11 | to << 17 | slot in S.xs << 24 (63: not fetched)
enum { CH_IT_BLOCKS = 0, CH_IT_SEGS = 1, CH_IT_SEG = 2, CH_IT_BLOCK = 3 };       // a run of blocks, a run of segments, one segment, one whole block by its segments
struct ChainItem { int es, lo, hi, D, tp, kind; };
#ifndef CH_ITEMS
#define CH_ITEMS 448                // (12 fetched blocks of at most 15 crossing segments and the 16 runs around them, the runs of blocks between)
#endif
__device__ __forceinline__ int chain_item_kind( int type, int c, int at, int from, int to, int slot ) { return type | ( c << 2 ) | ( at << 5 ) | ( from << 11 ) | ( to << 17 ) | ( slot << 24 ); }
struct ChainWalkLds
{
  ChainOne ones[CH_SUPER * WAVE];               // the block records' functions for the forecast binade
  ChainPiece bpiece[CH_SUPER * WAVE];           // [c * 64 + l]: blocks (the forecast's last crossing block before l, l] of chunk c as one record
  int bptau[CH_SUPER][CH_PIECES];               // per piece: tau[0] | tau[1] << 4 | max tau << 8
  float bst[CH_SUPER * WAVE];                   // the forecast at the blocks' starts
  ChainPiece piece[CH_PRE_BLKS][CH_SEG];        // the same by segments inside fetched block k
  int ptau[CH_PRE_BLKS][CH_PIECES];
  ChainRec fseg[CH_PRE_SEGS];                   // the records of the segments the forecasts point at ...
  float xs[CH_PRE_SEGS + 1][CH_SEG];            // ... and their addends (the last row: those of a segment fetched on the way)
  unsigned long long stat[WAVES_PER_BLOCK][3], flag[CH_PRE_BLKS], fmask[CH_SUPER];
  int pblk[CH_PRE_BLKS], at_seg[CH_PRE_SEGS], mode[CH_PRE_BLKS], bmode[CH_SUPER];
  float pst[CH_PRE_BLKS], tot[CH_SUPER], s0;
  int round_end;                                // the first block this round does not cover
  ChainItem items[CH_ITEMS];                    // the walk's steps, in order
  int ctot[CH_SUPER], kbase[CH_PRE_BLKS];       // items per chunk; a fetched block's first item
};
// does a chain that goes from a to b (forecasts) change binade on the way, give or take a relative eps?
__device__ __forceinline__ bool chain_crosses( float a, float b, float eps )
{
  if( a == 0.0f && b == 0.0f ) return false;             // (a chain that has not left zero yet)
  if( !( a * b > 0.0f ) ) return true;                   // zero, a sign change, NaN
  const float lo = fminf( fabsf( a ), fabsf( b ) ) * ( 1.0f - eps ), hi = fmaxf( fabsf( a ), fabsf( b ) ) * ( 1.0f + eps );
  return ( __float_as_uint( lo ) >> 23 ) != ( __float_as_uint( hi ) >> 23 );
}
// does the record's function hold a forecast value, give or take CH_EPS of it?  (f: the record for the forecast's binade)

__device__ __forceinline__ bool chain_fits_forecast( const ChainFn& f, uint32_t vb )
{
  const int M = (int)( vb & 0x7fffffu ) | CH_M_LO, marg = (int)( CH_EPS * 8388608.0f );
  return f.lo <= f.hi && M - marg >= f.lo && M + marg + max( f.tau & 3, f.tau >> 2 ) <= f.hi;
}
// (field by field: a conditional copy of the whole struct is a memcpy through private memory, which then stays in scratch)
__device__ __forceinline__ void chain_rec_copy( ChainRec& d, const ChainRec& r )
{
  d.e_sign = r.e_sign;
#pragma unroll
  for( int c = 0; c < 3; ++c ) { d.lo[c] = r.lo[c]; d.hi[c] = r.hi[c]; d.D[c] = r.D[c]; }
}
__device__ __forceinline__ ChainFn chain_one_fn( const ChainOne& p, uint32_t vb )
{
  ChainFn f = chain_never();
  if( p.es == (int)( vb >> 23 ) ) { f.lo = p.lo; f.hi = p.hi; f.D = p.Dt >> 4; f.tau = p.Dt & 15; }
  return f;
}
// The runs of records between the forecast's crossings (the set bits of m; f0 there: the identity), each composed into ONE record
// for the binade `es` the forecast has there: one segmented scan makes them all — the exclusive prefix of D restarts after every
// crossing, the prefix max / min carry the piece number in the high bits — and lane l ends up with the record of (the last
// crossing before l, l].  The ties inside, piece by piece, as chain_compose_block.  (m has fewer than CH_PIECES bits.)
__device__ __forceinline__ void chain_pieces( const ChainFn& f0, int es, unsigned long long m, int lane, ChainPiece* out, int* ptau )
{
  const unsigned long long before = m & below( lane );
  const int pid = __builtin_popcountll( before );
  const int incD = (int)wave_scan( (uint32_t)f0.D, lane ), ex = incD - f0.D;
  const int first = before != 0ull ? 64 - __builtin_clzll( before ) : 0;       // my piece starts after the last crossing before me
  const int exs = ex - __shfl( ex, first );
  const bool wild = abs( exs ) > ( 1 << 25 );                                   // (no valid run adds that much inside one binade; keeps the sums below in range)
  int a = ( wild ? CH_M_HI : f0.lo - exs ) + pid * CH_PIECE_BIG, b = ( wild ? CH_M_LO : f0.hi - exs ) - pid * CH_PIECE_BIG;
  RS_DPP_PREFIX( "v_max_i32_dpp", a );
  RS_DPP_PREFIX( "v_min_i32_dpp", b );
  ChainPiece pc;
  pc.es = es; pc.lo = max( a - pid * CH_PIECE_BIG, CH_M_LO ); pc.hi = min( b + pid * CH_PIECE_BIG, CH_M_HI ); pc.D = exs + f0.D;
  out[lane] = pc;
  if( lane < CH_PIECES ) ptau[lane] = 0;
  wave_lds_fence();
  // (taus that outgrow their four bits: a 'max tau' no interval has room for — the piece is then never taken whole.  Clamping them
  //  instead was wrong by as many grid steps as were cut off: a run of 37 blocks, nine of them with ties, 4 ulps.)
  auto pack = []( int t0, int t1, int tmax ) -> int { return ( t0 > 15 || t1 > 15 ) ? ( 0x7fffff << 8 ) : ( t0 | ( t1 << 4 ) | ( tmax << 8 ) ); };
  int cur = -1, t0 = 0, t1 = 0, tmax = 0;
  for( unsigned long long tm = RS_BALLOT( f0.tau != 0 ); tm != 0ull; tm &= tm - 1ull )
  {
    const int kk = __builtin_ctzll( tm );
    const int pk = __builtin_amdgcn_readlane( pid, kk ), exk = __builtin_amdgcn_readlane( exs, kk ), tk = __builtin_amdgcn_readlane( f0.tau, kk );
    if( pk != cur ) { if( cur >= 0 && lane == 0 ) ptau[cur] = pack( t0, t1, tmax ); cur = pk; t0 = 0; t1 = 0; tmax = 0; }
    t0 += chain_tau( tk, exk + t0 ); t1 += chain_tau( tk, 1 + exk + t1 ); tmax += max( tk & 3, tk >> 2 );
  }
  if( cur >= 0 && lane == 0 ) ptau[cur] = pack( t0, t1, tmax );
}
// (every round's loads are unconditional, from clamped indices, masked afterwards: a load inside a branch is waited for there,
//  one round trip after the other)
__device__ __forceinline__ void chain_walk_row( const IcpLaunch& L, const ChainBufs& B, int prob, int row, ChainWalkLds& S )
{
  // (the wave's number through readfirstlane: the compiler then KNOWS that "wave 0 only" is uniform control flow — otherwise every
  //  loop of the walk is compiled as divergent, its counters in vector registers and an exec-mask dance around every branch)
  const int lane = threadIdx.x & ( WAVE - 1 ), wib = uni( (int)threadIdx.x / WAVE );
  const bool walker = wib == 0;
  const unsigned long long t_start = B.dbg ? wall_clock64() : 0ull;
  const ChainRec* blks = B.blk + ( (size_t)prob * CH_ROWS + row ) * B.n_blk;
  const ChainRec* segs = B.seg + ( (size_t)prob * CH_ROWS + row ) * B.n_seg;
  const double* ssum = B.segsum + ( (size_t)prob * CH_ROWS + row ) * B.n_seg;
  const double* qsum = B.blksum + ( (size_t)prob * CH_ROWS + row ) * ( B.n_blk * CH_QUARTERS );
  const float* Rf = reinterpret_cast<const float*>( L.rec + (size_t)prob * L.src.n * REC_F4 );
  const int comp = row == 0 ? 3 : ( row <= 3 ? row - 1 : row );      // a record's words: p.xyz at 0..2, dist² at 3, q.xyz at 4..6, dot at 7
  int* dbg = ( B.dbg && threadIdx.x == 0 ) ? B.dbg + ( (size_t)prob * CH_ROWS + row ) * ( 4 + 64 * 8 ) : nullptr;
  auto stamp = [&]( int k ) { if( dbg ) dbg[4 + 63 * 8 + k] = (int)( wall_clock64() - t_start ); };
  constexpr int CHUNKS_PER_WAVE = CH_SUPER / WAVES_PER_BLOCK, BLKS_PER_WAVE = CH_PRE_BLKS / WAVES_PER_BLOCK, SEGS_PER_WAVE = CH_PRE_SEGS / WAVES_PER_BLOCK;
  static_assert( CH_SUPER % WAVES_PER_BLOCK == 0 && CH_PRE_BLKS % WAVES_PER_BLOCK == 0 && CH_PRE_SEGS % WAVES_PER_BLOCK == 0, "the rounds' work is dealt to the waves" );
  static_assert( CH_PRE_BLKS <= WAVE && CH_SUPER <= WAVE, "one lane per fetched block / per chunk" );

  float bsl[CHUNKS_PER_WAVE]; ChainRec rc[CHUNKS_PER_WAVE];
  auto round1_loads = [&]( int B0 )
  {
#pragma unroll
    for( int i = 0; i < CHUNKS_PER_WAVE; ++i )
    {
      const int b = B0 + ( wib + i * WAVES_PER_BLOCK ) * WAVE + lane, bc = min( b, B.n_blk - 1 );
      const double2* q = reinterpret_cast<const double2*>( qsum + (size_t)bc * CH_QUARTERS );
      const double2 u = q[0], v = q[1];
      chain_rec_copy( rc[i], blks[bc] );
      bsl[i] = b < B.n_blk ? (float)( ( u.x + u.y ) + ( v.x + v.y ) ) : 0.0f;
      if( b >= B.n_blk ) rc[i].e_sign = -1;
    }
  };
  round1_loads( 0 );
  const float sd = chain_stats( L, prob, S.stat, nullptr );                  // (its loads go out with round 1's)
  ChainPar P; P.use_sd = sd > 0.000001; P.cut = 2.5f * sd; P.max_dist = L.radius;
  stamp( 0 );

  auto addend_of = [&]( float d2, float dt, float cv, bool inside ) -> float        // chain_addends, this chain's
  {
    const bool mt = d2 >= 0.0f && inside;
    float w = 0.0f;
    if( mt ) { w = ( 1.0f - __fdiv_rn( d2, P.max_dist ) ) * dt; if( P.use_sd && d2 > P.cut ) w = 0.0f; }
    return row == 0 ? w : ( mt ? cv * w : 0.0f );
  };

  float s = 0.0f;
  int resolved = 0, stuck = 0, steps = 0, hits = 0, piece_steps = 0, scans = 0, n_chk = 0;
  int* chk = B.chk ? B.chk + ( (size_t)prob * CH_ROWS + row ) * ( 4 + 3 * CH_CHK_MAX ) : nullptr;
  // advance over the records held by the lanes [from, count): as far as the value fits; returns the first lane that does not (count: all done)
  // (select( value bits ): the lane's record as a function for that value's binade)
  auto advance = [&]( auto&& select, int from, int count ) -> int
  {
    const uint32_t sb = (uint32_t)uni( __float_as_int( s ) );             // (uniform, and the compiler is told so: everything derived from it is scalar work)
    const int M = (int)( sb & 0x7fffffu ) | CH_M_LO;
    const bool mine_in = lane >= from && lane < count;
    const ChainFn f0 = !mine_in ? chain_identity() : select( sb );
    const ChainFn f = chain_prefix( f0, lane );
    ++scans;
    // records with ties inside (ChainFn): each adds the tau its own start's parity picks — until those are known the most they can add
    const unsigned long long tl = RS_BALLOT( f0.tau != 0 );
    int taumax = 0;
    for( unsigned long long t = tl; t != 0ull; t &= t - 1ull ) { const int tk = __builtin_amdgcn_readlane( f0.tau, __builtin_ctzll( t ) ); taumax += max( tk & 3, tk >> 2 ); }
    const bool fits = f.lo <= f.hi && M >= f.lo && M + taumax <= f.hi;
    const unsigned long long good = RS_BALLOT( fits );
    const int stop = good == ~0ull ? WAVE : __builtin_ctzll( ~good );       // the fitting lanes are a prefix: the intervals only shrink
    const int last = min( stop, count ) - 1;
    if( last >= from )
    {
      int extra = 0;
      for( unsigned long long t = tl & ( last >= WAVE - 1 ? ~0ull : below( last + 1 ) ); t != 0ull; t &= t - 1ull )
      {
        const int k = __builtin_ctzll( t );
        const int exk = __builtin_amdgcn_readlane( f.D, k ) - __builtin_amdgcn_readlane( f0.D, k );
        extra += chain_tau( __builtin_amdgcn_readlane( f0.tau, k ), M + exk + extra );
      }
      const int D = __builtin_amdgcn_readlane( f.D, last ) + extra;
      s = __uint_as_float( ( sb & 0xff800000u ) | ( (uint32_t)( M + D ) & 0x7fffffu ) );
    }
    return min( stop, count );
  };
  long long walk_cycles = 0;
  // A round covers up to 512 blocks — and ends early at the first crossing block its fetch slots do not hold (S.round_end):
  // the next round starts there, from the exact value, with fresh slots.
  for( int B0 = 0; B0 < B.n_blk; )
  {
    const int n_chunks = min( CH_SUPER, ( B.n_blk - B0 + WAVE - 1 ) / WAVE );
    if( B0 > 0 ) round1_loads( B0 );
    if( threadIdx.x == 0 ) S.round_end = min( B0 + CH_SUPER * WAVE, B.n_blk );
    // ---- the forecasts at the blocks' starts: the chunks' totals first ...
    float incl[CHUNKS_PER_WAVE];
#pragma unroll
    for( int i = 0; i < CHUNKS_PER_WAVE; ++i ) { incl[i] = wave_scan_f32( bsl[i] ); if( lane == WAVE - 1 ) S.tot[wib + i * WAVES_PER_BLOCK] = incl[i]; }
    if( threadIdx.x == 0 ) S.s0 = s;
    __syncthreads();
    unsigned long long fm_mine[CHUNKS_PER_WAVE]; float st_mine[CHUNKS_PER_WAVE];
    float tot_before;                      // lane c: what the chunks before c add (one read, one scan: a loop of dependent LDS reads costs ~100 cycles a turn)
    { const float t = lane < CH_SUPER ? S.tot[lane] : 0.0f; tot_before = wave_scan_f32( t ) - t; }
#pragma unroll
    for( int i = 0; i < CHUNKS_PER_WAVE; ++i )
    {
      const int c = wib + i * WAVES_PER_BLOCK;
      const float base = S.s0 + rl( tot_before, c );
      const float st = base + ( incl[i] - bsl[i] ), en = base + incl[i];
      const int b = B0 + c * WAVE + lane;
      // ... of a block's record the function for the binade the forecast has at its start (if the value gets there in another: by its segments)
      const uint32_t vb = __float_as_uint( st );
      const ChainFn f = rc[i].e_sign == -1 ? chain_never() : chain_fn_for( rc[i], vb );
      ChainOne one; one.es = (int)( vb >> 23 ); one.lo = f.lo; one.hi = f.hi; one.Dt = f.D * 16 + f.tau;
      S.ones[c * WAVE + lane] = one; S.bst[c * WAVE + lane] = st;
      // a crossing block: the forecast changes binade between its ends — or its record does not hold the forecast (the chain leaves the
      // binade INSIDE the block and is back at its end: a sum that hovers at a power of two does that block after block, and each such
      // block, not forecast, cost a scan of its segments and a round trip per segment that did not fit)
      const unsigned long long m = RS_BALLOT( b < B.n_blk && ( b == 0 || chain_crosses( st, en, CH_EPS ) || !chain_fits_forecast( f, vb ) ) );
      fm_mine[i] = m; st_mine[i] = st;
      // ... and the runs of blocks between the forecast's crossing blocks as one record each
      // (a round ends at its (CH_PRE_BLKS + 1)-th crossing block at the latest: the pieces beyond a chunk's first CH_PIECES - 1 crossing
      //  blocks are never walked — a chunk with more of them used to be taken "whole, by scans": a round trip per segment that did not fit)
      static_assert( CH_PRE_BLKS + 1 < CH_PIECES, "the pieces cover every block a round can reach" );
      const unsigned long long mp = lowest_bits( m, CH_PIECES - 1 );
      if( lane == 0 ) { S.fmask[c] = m; S.bmode[c] = 1; }
      chain_pieces( ( b >= B.n_blk || ( ( mp >> lane ) & 1ull ) ) ? chain_identity() : f, (int)( vb >> 23 ), mp, lane, &S.bpiece[c * WAVE], S.bptau[c] );
    }
    __syncthreads();
    // ---- the blocks to fetch: the first CH_PRE_BLKS of those, in order — every lane knows its block's rank
    int flagged_before, flagged_total;     // lane c: the crossing blocks in the chunks before c
    {
      const uint32_t cnt = lane < CH_SUPER ? (uint32_t)__builtin_popcountll( S.fmask[lane] ) : 0u;
      const uint32_t inc = wave_scan( cnt, lane );
      flagged_before = (int)( inc - cnt ); flagged_total = __builtin_amdgcn_readlane( (int)inc, WAVE - 1 );
#pragma unroll
      for( int i = 0; i < CHUNKS_PER_WAVE; ++i )
      {
        const int c = wib + i * WAVES_PER_BLOCK;
        const int rank = __builtin_amdgcn_readlane( flagged_before, c ) + __builtin_popcountll( fm_mine[i] & below( lane ) );
        if( ( ( fm_mine[i] >> lane ) & 1ull ) && rank < CH_PRE_BLKS ) { S.pblk[rank] = B0 + c * WAVE + lane; S.pst[rank] = st_mine[i]; }
        if( ( ( fm_mine[i] >> lane ) & 1ull ) && rank == CH_PRE_BLKS ) S.round_end = B0 + c * WAVE + lane;      // (the first one without a slot)
      }
      if( walker && lane >= flagged_total && lane < CH_PRE_BLKS ) { S.pblk[lane] = -1; S.pst[lane] = 0.0f; }
    }
    __syncthreads();
    const int round_end = S.round_end;
    stamp( 1 );
    // ---- round 2: those blocks' segment records and sums; the forecast by segments; the pieces
    {
      ChainRec got[BLKS_PER_WAVE]; float sv[BLKS_PER_WAVE]; int pb[BLKS_PER_WAVE];
#pragma unroll
      for( int i = 0; i < BLKS_PER_WAVE; ++i )
      {
        pb[i] = uni( S.pblk[wib * BLKS_PER_WAVE + i] );
        const int sg = max( pb[i], 0 ) * CH_BLK + lane, sgc = min( sg, B.n_seg - 1 );
        chain_rec_copy( got[i], segs[sgc] ); sv[i] = (float)ssum[sgc];
        if( pb[i] < 0 || sg >= B.n_seg ) { got[i].e_sign = -1; sv[i] = 0.0f; }
      }
#pragma unroll
      for( int i = 0; i < BLKS_PER_WAVE; ++i )
      {
        const int k = wib * BLKS_PER_WAVE + i;
        const float incs = wave_scan_f32( sv[i] ), st0 = S.pst[k];
        const float vst = st0 + ( incs - sv[i] );
        const bool in = pb[i] >= 0 && pb[i] * CH_BLK + lane < B.n_seg;
        const uint32_t vb = __float_as_uint( vst );
        const ChainFn fseg = in ? chain_fn_for( got[i], vb ) : chain_identity();
        const unsigned long long m = RS_BALLOT( in && ( chain_crosses( vst, st0 + incs, CH_EPS ) || !chain_fits_forecast( fseg, vb ) ) );      // (as for the blocks)
        const bool pieces = pb[i] >= 0 && __builtin_popcountll( m ) < CH_PIECES;
        // (a block of 16 crossing segments or more — a chain's first block when the coordinates straddle the origin — is walked by scans
        //  of its records, its segments' addends fetched on the way: it takes none of the round's fetch slots — it used to take them all, and
        //  every later crossing segment of the round then went without.  Loading such a block's 4 096 addends in one go was built too:
        //  the centred bench step 3.84 instead of 3.89 ms — and 15 us per iteration MORE on scans in one octant, which never run that
        //  code: the walk is one wave's instruction stream, and it got longer)
        if( lane == 0 ) { S.flag[k] = pieces ? m : 0ull; S.mode[k] = pieces ? 1 : 0; }
        if( pieces )
        {
          const ChainFn f0 = ( !in || ( ( m >> lane ) & 1ull ) ) ? chain_identity() : fseg;
          chain_pieces( f0, (int)( vb >> 23 ), m, lane, S.piece[k], S.ptau[k] );
        }
      }
    }
    __syncthreads();                                                      // (S.flag, S.piece)
    stamp( 2 );
    // ---- the first CH_PRE_SEGS of the segments the forecasts point at, in order: lane k (of every wave) works out block k's share
    unsigned long long l_segs = 0ull;     // lane k: the segments of fetched block k whose addends and records are in S.xs / S.fseg, from slot l_sbase on
    int l_sbase = 0;
    {
      const unsigned long long mine = lane < CH_PRE_BLKS ? S.flag[lane] : 0ull;
      const uint32_t cnt = (uint32_t)__builtin_popcountll( mine );
      l_sbase = (int)( wave_scan( cnt, lane ) - cnt );
      l_segs = lowest_bits( mine, CH_PRE_SEGS - l_sbase );
      if( walker )
      {
        const int pbk = lane < CH_PRE_BLKS ? S.pblk[lane] : 0;
        int slot = l_sbase;
        for( unsigned long long m = l_segs; m != 0ull; m &= m - 1ull ) S.at_seg[slot++] = pbk * CH_BLK + __builtin_ctzll( m );
        const int total = __builtin_amdgcn_readlane( l_sbase + (int)__builtin_popcountll( l_segs ), CH_PRE_BLKS - 1 );
        if( lane >= total && lane < CH_PRE_SEGS ) S.at_seg[lane] = 0;       // (none: segment 0's, not used)
      }
    }
    __syncthreads();                                                      // (S.at_seg)
    // ---- round 3: their addends and records (the loads now; what they bring is put away after the items below, which do not need it)
    float xd[SEGS_PER_WAVE], xw[SEGS_PER_WAVE], xc[SEGS_PER_WAVE]; int at3[SEGS_PER_WAVE], rw[SEGS_PER_WAVE];
    constexpr int REC_WORDS = sizeof( ChainRec ) / 4;
#pragma unroll
    for( int i = 0; i < SEGS_PER_WAVE; ++i )
    {
      const int sgm = uni( S.at_seg[wib * SEGS_PER_WAVE + i] );
      at3[i] = sgm * CH_SEG + lane;
      const float* rp = Rf + (size_t)min( at3[i], L.src.n - 1 ) * ( REC_F4 * 4 );
      xd[i] = rp[3]; xw[i] = rp[7]; xc[i] = rp[comp];
      rw[i] = reinterpret_cast<const int*>( segs + min( sgm, B.n_seg - 1 ) )[min( lane, REC_WORDS - 1 )];
    }
    // ---- the walk's steps, in order, one item each (ChainItem): how many per chunk ...
    auto lanes_below = [&]( int n ) -> unsigned long long { return n >= WAVE ? ~0ull : below( n ); };
    int it_cnt[CHUNKS_PER_WAVE], it_off[CHUNKS_PER_WAVE], it_k[CHUNKS_PER_WAVE];
#pragma unroll
    for( int i = 0; i < CHUNKS_PER_WAVE; ++i )
    {
      const int c = wib + i * WAVES_PER_BLOCK, nb = max( 0, min( WAVE, round_end - ( B0 + c * WAVE ) ) );
      const unsigned long long fm = fm_mine[i] & lanes_below( nb );
      const int rank = __builtin_amdgcn_readlane( flagged_before, c ) + __builtin_popcountll( fm & below( lane ) );
      const bool flagged = ( fm >> lane ) & 1ull, mine_in = lane < nb;
      int cnt = 0; it_k[i] = -1;
      if( c < n_chunks && mine_in )
      {
        if( !S.bmode[c] ) cnt = lane == 0 ? 1 : 0;                           // (too many crossings for pieces: the whole chunk by scans)
        else if( flagged )
        {
          cnt = 1;
          if( rank < CH_PRE_BLKS && S.mode[rank] )
          {
            // a fetched block: its crossing segments and the runs between them
            const int ns = min( CH_BLK, B.n_seg - ( B0 + c * WAVE + lane ) * CH_BLK );
            const unsigned long long m = S.flag[rank], in = lanes_below( ns );
            cnt = __builtin_popcountll( m & in ) + __builtin_popcountll( ~m & ( ( m << 1 ) | 1ull ) & in );
            it_k[i] = rank;
          }
        }
        else cnt = ( lane == nb - 1 || ( ( fm >> ( lane + 1 ) ) & 1ull ) ) ? 1 : 0;     // the last block of a run
      }
      it_cnt[i] = cnt;
      const int inc = (int)wave_scan( (uint32_t)cnt, lane );
      it_off[i] = inc - cnt;
      if( lane == WAVE - 1 ) S.ctot[c] = inc;
    }
    __syncthreads();
    // ... the runs of blocks and the blocks taken whole; where a fetched block's items start
    int n_items, items_before;             // lane c: the items of the chunks before c
    {
      const uint32_t cnt = lane < CH_SUPER ? (uint32_t)S.ctot[lane] : 0u;
      const uint32_t inc = wave_scan( cnt, lane );
      items_before = (int)( inc - cnt ); n_items = __builtin_amdgcn_readlane( (int)inc, WAVE - 1 );
    }
#pragma unroll
    for( int i = 0; i < CHUNKS_PER_WAVE; ++i )
    {
      const int c = wib + i * WAVES_PER_BLOCK, nb = max( 0, min( WAVE, round_end - ( B0 + c * WAVE ) ) );
      const int at = __builtin_amdgcn_readlane( items_before, c ) + it_off[i];
      if( it_cnt[i] > 0 && at < CH_ITEMS )
      {
        const unsigned long long fm = fm_mine[i] & lanes_below( nb );
        ChainItem it; it.es = -1; it.lo = CH_M_HI; it.hi = CH_M_LO; it.D = 0; it.tp = 0;
        if( !S.bmode[c] ) { it.kind = chain_item_kind( CH_IT_BLOCKS, c, 0, 0, nb, 63 ); S.items[at] = it; }
        else if( ( fm >> lane ) & 1ull )
        {
          if( it_k[i] >= 0 ) S.kbase[it_k[i]] = at;
          else { it.kind = chain_item_kind( CH_IT_BLOCK, c, lane, 0, 0, 63 ); S.items[at] = it; }
        }
        else
        {
          const unsigned long long before = fm & below( lane );
          const int from = before != 0ull ? 64 - __builtin_clzll( before ) : 0;
          const ChainPiece pc = S.bpiece[c * WAVE + lane];
          it.es = pc.es; it.lo = pc.lo; it.hi = pc.hi; it.D = pc.D; it.tp = S.bptau[c][__builtin_popcountll( before )];
          it.kind = chain_item_kind( CH_IT_BLOCKS, c, 0, from, lane + 1, 63 );
          S.items[at] = it;
        }
      }
    }
#pragma unroll
    for( int i = 0; i < SEGS_PER_WAVE; ++i )
    {
      S.xs[wib * SEGS_PER_WAVE + i][lane] = addend_of( xd[i], xw[i], xc[i], at3[i] < L.src.n );
      if( lane < REC_WORDS ) reinterpret_cast<int*>( &S.fseg[wib * SEGS_PER_WAVE + i] )[lane] = rw[i];
    }
    __syncthreads();                                                      // (S.xs, S.fseg, S.kbase)
    // ... and the fetched blocks' own
#pragma unroll
    for( int i = 0; i < BLKS_PER_WAVE; ++i )
    {
      const int k = wib * BLKS_PER_WAVE + i, pbk = S.pblk[k];
      if( pbk < 0 || !S.mode[k] ) continue;
      const int ns = min( CH_BLK, B.n_seg - pbk * CH_BLK ), c = ( pbk - B0 ) / WAVE, at_blk = ( pbk - B0 ) % WAVE;
      const unsigned long long m = S.flag[k];
      const bool flagged = ( m >> lane ) & 1ull;
      const bool run_end = !flagged && ( lane == ns - 1 || ( ( m >> ( lane + 1 ) ) & 1ull ) );
      const unsigned long long ends = RS_BALLOT( lane < ns && ( flagged || run_end ) );
      const int at = S.kbase[k] + __builtin_popcountll( ends & below( lane ) );
      if( ( ( ends >> lane ) & 1ull ) && at < CH_ITEMS )
      {
        const unsigned long long have = rl( l_segs, k );
        const int sbase = __builtin_amdgcn_readlane( l_sbase, k );
        const ChainPiece pc = S.piece[k][lane];
        ChainItem it; it.es = pc.es; it.lo = CH_M_HI; it.hi = CH_M_LO; it.D = 0; it.tp = 0;
        if( flagged )
        {
          int slot = 63;
          if( ( have >> lane ) & 1ull )
          {
            slot = sbase + __builtin_popcountll( have & below( lane ) );
            ChainRec r; chain_rec_copy( r, S.fseg[slot] );
            const ChainFn f = chain_fn_for( r, (uint32_t)pc.es << 23 );
            it.lo = f.lo; it.hi = f.hi; it.D = f.D; it.tp = chain_tau( f.tau, 0 ) | ( chain_tau( f.tau, 1 ) << 4 ) | ( max( f.tau & 3, f.tau >> 2 ) << 8 );
          }
          it.kind = chain_item_kind( CH_IT_SEG, c, at_blk, lane, lane + 1, slot );
        }
        else
        {
          const unsigned long long before = m & below( lane );
          const int from = before != 0ull ? 64 - __builtin_clzll( before ) : 0;
          it.lo = pc.lo; it.hi = pc.hi; it.D = pc.D; it.tp = S.ptau[k][__builtin_popcountll( before )];
          it.kind = chain_item_kind( CH_IT_SEGS, c, at_blk, from, lane + 1, 63 );
        }
        S.items[at] = it;
      }
    }
    __syncthreads();
    if( B0 == 0 && dbg ) dbg[1] = (int)( wall_clock64() - t_start );

    // ---- the walk: item after item, 64 of them in wave 0's registers at a time; an item that does not hold the value (the forecast
    // was off, or it is the segment where the chain changes binade) falls back on its own range — addend by addend for a segment,
    // wave-wide scans of the records for a run
    if( walker && !( stuck & 2 ) )
    {
      const long long c_walk = dbg ? clock64() : 0;
      // segment g: its 64 addends one after the other, in fp32 — the reference's own operations.  From LDS, four at a time, every
      // lane the same address: 16 reads + 64 adds (by readlane from a register: 64 + 64).
      auto one_by_one = [&]( int g, int slot )
      {
        if( dbg && resolved < 62 )
        {
          int* d = dbg + 4 + resolved * 8;
          d[0] = g; d[1] = __float_as_int( s ); d[2] = slot < CH_PRE_SEGS ? 3 : 0; d[3] = 0; d[7] = (int)( wall_clock64() - t_start );
        }
        hits += slot < CH_PRE_SEGS ? 1 : 0;
        if( slot >= CH_PRE_SEGS )
        {
          const int i = g * CH_SEG + lane;
          const float* rp = Rf + (size_t)min( i, L.src.n - 1 ) * ( REC_F4 * 4 );
          slot = CH_PRE_SEGS;
          S.xs[slot][lane] = addend_of( rp[3], rp[7], rp[comp], i < L.src.n );
          wave_lds_fence();
        }
        const float4* xp = reinterpret_cast<const float4*>( &S.xs[slot][0] );
        float4 xa[4], xb[4];                                          // (two sets of 16 addends in turn: 32 registers)
        auto add4 = [&]( const float4* x ) {
#pragma unroll
          for( int j = 0; j < 4; ++j ) { s = s + x[j].x; s = s + x[j].y; s = s + x[j].z; s = s + x[j].w; } };
#pragma unroll
        for( int j = 0; j < 4; ++j ) { xa[j] = xp[j]; xb[j] = xp[4 + j]; }
        add4( xa );
#pragma unroll
        for( int j = 0; j < 4; ++j ) xa[j] = xp[8 + j];
        add4( xb );
#pragma unroll
        for( int j = 0; j < 4; ++j ) xb[j] = xp[12 + j];
        add4( xa );
        add4( xb );
        if( ++resolved > CH_BUDGET ) stuck |= 2;
      };
      // the segments [sat, to) of the block that starts at segment g0 by wave-wide scans of their records (fetched now)
      auto segs_by_scans = [&]( int g0, int sat, int to )
      {
        const int ns = min( CH_BLK, B.n_seg - g0 );
        ChainRec smine; smine.e_sign = -1;
        if( lane < ns ) chain_rec_copy( smine, segs[g0 + lane] );
        while( sat < to && !( stuck & 2 ) )
        {
          const int sat_was = sat;
          if( ++steps > 8 * B.n_seg + 4096 ) { stuck |= 2; break; }       // (a walk takes at most one step per block + two per segment: guards against a loop that does not end)
          sat = advance( [&]( uint32_t vb ) -> ChainFn { return smine.e_sign == -1 ? chain_never() : chain_fn_for( smine, vb ); }, sat, to );
          if( sat < sat_was ) { stuck |= 1; sat = sat_was; }              // (cannot happen: the lanes before `sat` hold the identity — guards the loop against a wrong scan)
          if( sat >= to ) break;
          one_by_one( g0 + sat, 63 );
          ++sat;
        }
      };
      // the blocks [at, to) of chunk c by wave-wide scans of their functions
      auto blocks_by_scans = [&]( int c, int at, int to )
      {
        const ChainOne mine = S.ones[c * WAVE + lane];
        while( at < to && !( stuck & 2 ) )
        {
          const int at_was = at;
          if( ++steps > 8 * B.n_seg + 4096 ) { stuck |= 2; break; }
          at = advance( [&]( uint32_t vb ) -> ChainFn { return chain_one_fn( mine, vb ); }, at, to );
          if( at < at_was ) { stuck |= 1; at = at_was; }
          if( at >= to ) break;
          const int g0 = ( B0 + c * WAVE + at ) * CH_BLK;
          segs_by_scans( g0, 0, min( CH_BLK, B.n_seg - g0 ) );
          ++at;
        }
      };
      for( int i0 = 0; i0 < min( n_items, CH_ITEMS ) && !( stuck & 2 ); i0 += WAVE )
      {
        const ChainItem mine = S.items[min( i0 + lane, CH_ITEMS - 1 )];
        const int n_here = min( WAVE, min( n_items, CH_ITEMS ) - i0 );
        for( int i = 0; i < n_here && !( stuck & 2 ); ++i )
        {
          const uint32_t sb = (uint32_t)uni( __float_as_int( s ) );
          const int M = (int)( sb & 0x7fffffu ) | CH_M_LO;
          const int es = __builtin_amdgcn_readlane( mine.es, i ), lo = __builtin_amdgcn_readlane( mine.lo, i ), hi = __builtin_amdgcn_readlane( mine.hi, i );
          const int D = __builtin_amdgcn_readlane( mine.D, i ), tp = __builtin_amdgcn_readlane( mine.tp, i ), kind = __builtin_amdgcn_readlane( mine.kind, i );
          const int type = kind & 3, c = ( kind >> 2 ) & 7, at = ( kind >> 5 ) & 63, from = ( kind >> 11 ) & 63, to = ( kind >> 17 ) & 127, slot = ( kind >> 24 ) & 63;
          const int g0 = ( B0 + c * WAVE + at ) * CH_BLK;
          const bool whole = es == (int)( sb >> 23 ) && lo <= hi && M >= lo && M + ( tp >> 8 ) <= hi;
          if( whole )
          {
            const float s_rec = __uint_as_float( ( sb & 0xff800000u ) | ( (uint32_t)( M + D + ( ( M & 1 ) ? ( tp >> 4 ) & 15 : tp & 15 ) ) & 0x7fffffu ) );
            if( chk )      // (RS_HIP_CHAIN_DEBUG: the same step by scans / addend by addend, from the same value)
            {
              if( type == CH_IT_SEG ) one_by_one( g0 + from, slot );
              else if( type == CH_IT_SEGS ) segs_by_scans( g0, from, to );
              else if( type == CH_IT_BLOCK ) segs_by_scans( g0, 0, min( CH_BLK, B.n_seg - g0 ) );
              else blocks_by_scans( c, from, to );
              s = __int_as_float( uni( __float_as_int( s ) ) );
              if( __float_as_int( s ) != __float_as_int( s_rec ) && dbg && dbg[4 + 63 * 8 + 4] == 0 )
              {
                dbg[4 + 63 * 8 + 4] = 1 + n_chk; dbg[4 + 63 * 8 + 5] = es; dbg[4 + 63 * 8 + 6] = lo; dbg[4 + 63 * 8 + 7] = hi;
                dbg[4 + 62 * 8 + 0] = D; dbg[4 + 62 * 8 + 1] = tp; dbg[4 + 62 * 8 + 2] = (int)sb; dbg[4 + 62 * 8 + 3] = __float_as_int( s ); dbg[4 + 62 * 8 + 4] = __float_as_int( s_rec ); dbg[4 + 62 * 8 + 5] = kind;
              }
            }
            s = s_rec;
            ++piece_steps;
          }
          else if( type == CH_IT_SEG ) one_by_one( g0 + from, slot );
          else if( type == CH_IT_SEGS ) segs_by_scans( g0, from, to );
          else if( type == CH_IT_BLOCK ) segs_by_scans( g0, 0, min( CH_BLK, B.n_seg - g0 ) );
          else blocks_by_scans( c, from, to );
          if( chk && n_chk < CH_CHK_MAX )       // (RS_HIP_CHAIN_DEBUG: where this step ends and with what — held against the plain sum below)
          {
            const int end_seg = type == CH_IT_BLOCKS ? min( ( B0 + c * WAVE + to ) * CH_BLK, B.n_seg ) : ( type == CH_IT_SEGS ? g0 + to : ( type == CH_IT_SEG ? g0 + from + 1 : min( g0 + CH_BLK, B.n_seg ) ) );
            s = __int_as_float( uni( __float_as_int( s ) ) );
            if( lane == 0 ) { chk[4 + 3 * n_chk] = end_seg; chk[4 + 3 * n_chk + 1] = __float_as_int( s ); chk[4 + 3 * n_chk + 2] = kind | ( whole ? 1 << 30 : 0 ); }
            ++n_chk;
          }
        }
      }
      if( n_items > CH_ITEMS ) stuck |= 2;                                   // (more steps than the list holds: hundreds of binade changes in one round)
      if( dbg ) { s = __int_as_float( uni( __float_as_int( s ) ) ); walk_cycles += clock64() - c_walk; }
    }
    __syncthreads();                                                      // (the next round overwrites what this walk read)
    B0 = round_end;
  }
  if( chk && walker )
  {
    // the plain sum, 64 addends at a time, compared with what the walk had where each of its steps ended
    float sp = 0.0f; int next = 0, bad = -1, bad_bits = 0, crossing = 0;
    for( int g = 0; g < B.n_seg; ++g )
    {
      const uint32_t sp_was = __float_as_uint( sp );
      const int i = g * CH_SEG + lane;
      const float* rp = Rf + (size_t)min( i, L.src.n - 1 ) * ( REC_F4 * 4 );
      const float xr = addend_of( rp[3], rp[7], rp[comp], i < L.src.n );
#pragma unroll
      for( int j = 0; j < CH_SEG; ++j ) sp = sp + __int_as_float( __builtin_amdgcn_readlane( __float_as_int( xr ), j ) );
      sp = __int_as_float( uni( __float_as_int( sp ) ) );
      crossing += ( sp_was >> 23 ) != ( __float_as_uint( sp ) >> 23 ) ? 1 : 0;      // (segments that END in another binade than they start in: a lower bound of those that change binade)
      while( next < n_chk && chk[4 + 3 * next] <= g + 1 )
      {
        if( chk[4 + 3 * next] == g + 1 && bad < 0 && chk[4 + 3 * next + 1] != __float_as_int( sp ) ) { bad = next; bad_bits = __float_as_int( sp ); }
        ++next;
      }
    }
    if( lane == 0 ) { chk[0] = n_chk; chk[1] = bad; chk[2] = bad < 0 ? crossing : bad_bits; chk[3] = __float_as_int( sp ); }
  }
  // A chain that wanders around zero — coordinates that straddle the origin, summed in an order that keeps cancelling — changes binade
  // not fifteen times but thousands of times, and every such segment is 64 dependent additions on this one wave: milliseconds.  The
  // walk gives up after CH_BUDGET of them (or when its list of steps overflows, or a loop guard fires): the problem is marked failed
  // and inactive — every later launch of the call is a no-op for it — and the host runs it again with the seven sums by pass 2 of
  // the replay (rs_hip_icp_align_batch), whose speculative segments do not mind.
  if( threadIdx.x == 0 && ( stuck & 2 ) && B.failed ) { B.failed[prob] = 1; L.active[prob] = 0; }
  if( threadIdx.x == 0 )
  {
    B.totals[( (size_t)prob * 3 + 1 ) * ICP_NMOM + row] = (double)s;
    if( B.resolved ) atomicAdd( B.resolved + prob, resolved );
    if( dbg ) { dbg[0] = resolved | ( stuck << 30 ) | ( scans << 16 ); dbg[2] = hits | ( piece_steps << 16 ); dbg[3] = (int)( wall_clock64() - t_start ); dbg[4 + 63 * 8 + 3] = (int)walk_cycles; }
  }
}

__global__ __launch_bounds__( BLOCK ) void k_chain_walk( IcpLaunch L, ChainBufs B )
{
  RS_CHAIN_SETPRIO();
  __shared__ ChainWalkLds S;
  const int prob = blockIdx.y;
  if( L.active[prob] == 0 ) return;
  for( int rep = 0; rep < ( B.dbg ? B.dbg_reps : 1 ); ++rep ) { chain_walk_row( L, B, prob, blockIdx.x, S ); __syncthreads(); }
}
// The walks, the moments and the next iteration's guesses in ONE launch (none needs another's results): workgroups 0-6 walk a chain
// each with their first wave, the next 4 n_blk take a quarter block of the moments each, the last n_blk a block of the guesses (from
// the sums k_chain_segrecs and k_chain_compose have just left: read by the NEXT iteration's k_chain_segrecs).
__global__ __launch_bounds__( BLOCK ) void k_chain_walk_and_moments( IcpLaunch L, ChainBufs B )
{
  RS_CHAIN_SETPRIO();
  __shared__ union U { ChainWalkLds w; ChainMomLds m; __device__ U() {} } S;
  const int prob = blockIdx.y;
  if( L.active[prob] == 0 ) return;
  if( blockIdx.x < CH_ROWS )
  {
    chain_walk_row( L, B, prob, blockIdx.x, S.w );
    return;
  }
  const int qb = (int)blockIdx.x - CH_ROWS;
  if( qb < B.n_blk * CH_QUARTERS ) chain_moments_block( L, B, prob, qb, S.m, L.rec + (size_t)prob * L.src.n * REC_F4 );
  else chain_guess_block( L, B, prob, qb - B.n_blk * CH_QUARTERS, WAVES_PER_BLOCK );
}

// ------------------------------------------------------------------------------------------
// Lane chains (round 6): the same seven sums for OBJECT-sized sources — every icp_align call site of the reference
// (apps/pose_proposal/main.cpp:195-197, lib/rs/rs_database.h:227-229, apps/segment_transfer/database_update.cpp:65-67) —
// one wave per chain, any number of problems side by side (grid.y = problem, each bound to its own source: icp_bind).
//
// The grid chains above pay five launches and a forecast machinery to spread ONE chain over the chip; a source of a few
// ten thousand points does not need that.  A wave takes a stretch of 1 024 addends at a time, sixteen consecutive ones per lane
// (LC_PER_LANE; four stretches' loads in flight: LC_DEPTH), and applies the
// same fact — inside a binade the sum is an integer sum — directly: every addend scaled by 1 / ulp( s ) and rounded to
// nearest-even is what it adds to the mantissa; the sixteen of a lane are prefixed in registers, the lanes by one DPP scan; if every
// partial mantissa stays inside the binade (one grid step clear of its ends, as the records above) and no addend sits exactly
// half way between two grid points, the 1 024 additions ARE that integer addition.  Otherwise the stretch is cut at the first
// lane that does not fit: the lanes before it are taken by the integers, that lane's sixteen addends are added in fp32 one
// after the other — the reference's own operation, so a change of binade, a tie, a sum that is zero, denormal or not finite
// need no case of their own — and the rest is tried again from the new value.  A sum that hovers (coordinates of both
// signs) makes little headway per attempt; then the fp32 stretch doubles, up to four lanes: the worst case is the plain
// sequential sum plus an attempt per 64 addends.  Nothing is given up and nothing is forecast: the result is the
// sequential sum for any input (tests/test_gpu_parity.py: test_lane_chains_are_the_sequential_sums).
//   k_lane_chains_and_moments   workgroups 0-1: the seven walks (a wave each); the rest: the fp64 moments of a quarter block of
//                               1 024 source points each (chain_moments_block, shared with the grid chains)
//   k_icp_update_wide           the rest of the iteration, centred on the chains' centroids (L.exact_centroids)
// What it is NOT: the reference's bits.  The 27 + 6 accumulators of the normal equations are summed in fp64 where the reference
// rounds after every addition — measured on every reference fixture of this size (profiles/r06/estimator_policy.txt): at most
// 3e-6 from the reference's pose, iteration counts equal; rs_hip_icp_reference_order_below() brings the bits back.
// ------------------------------------------------------------------------------------------
#define LC_PER_LANE 16
#define LC_SUPER ( LC_PER_LANE * WAVE )
#define LC_DEPTH 4

// Where problem `prob`'s seven addend rows live (floats): eight rows' worth per problem so that every row starts on a 16-byte
// boundary whatever the sizes of the problems before it; a row holds ( n + 3 ) & ~3 floats.
__device__ __forceinline__ size_t lane_rows_base( const IcpLaunch& L, int prob ) { return 8 * ( (size_t)L.pt_off + 4 * (size_t)prob ); }
__device__ __forceinline__ int lane_row_stride( int n ) { return ( n + 3 ) & ~3; }

// (unconditional loads — a quad beyond the row reads the row's last quad instead and is zeroed afterwards — so that the loads of the
//  stretches ahead stay countable: a load under a branch made the compiler wait for ALL loads in flight at every step)
__device__ __forceinline__ void lane_chain_load( const float* row, int ns, int base, int lane, float4 ( &X )[LC_PER_LANE / 4] )
{
#pragma unroll
  for( int q = 0; q < LC_PER_LANE / 4; ++q )
  {
    const int i = base + lane * LC_PER_LANE + 4 * q;
    X[q] = *(const float4*)( row + min( i, ns - 4 ) );     // (ns is a multiple of 4, >= 4: lane_row_stride)
  }
}

// The sequential fp32 sum of the n addends of `row` (the reference's order), by one wave.  dbg (diagnostics, may be null): addends
// added one by one, attempts made.
//
// The integers are kept as FLOATS: with S = |s| in [2^e, 2^(e+1)), u = ulp( S ) and C = 1.5 * 2^e (same binade, even mantissa),
// RN( C + x ) - C  is x rounded to the grid of u, ties to the even grid point, for every |x| < 2^(e-1) — the addition rounds for us, no
// scaling, no conversion — and sums of such multiples of u below 2^(e+1) are exact in fp32.  So a lane's sixteen addends are
// rounded (two additions each), prefixed in registers, the lanes' totals by one DPP scan of float additions, and the partial sums
// S + prefix compared with the binade's ends as floats.  Every quantity that decides something for a lane is a sum over a
// contiguous range of addends BEFORE the first lane that does not fit, hence a multiple of u below 2^(e+1), hence exact; what lies
// beyond that lane may have rounded and is not looked at.
__device__ __forceinline__ float lane_chain_walk( const float* row, int n, int lane, int* dbg )
{
  float s = 0.0f;                                      // wave-uniform throughout
  int n_seq = 0, n_try = 0;
  const int ns = lane_row_stride( n );
  // Two groups of LC_DEPTH stretches in registers: the one being walked and the next, all of whose loads are issued before the walk of
  // the current group begins — the rows were written a launch ago by other CUs (another XCD's L2: they come from memory, 1-2 us
  // away), a group is walked in about that time.
  float4 X[LC_DEPTH][LC_PER_LANE / 4], Y[LC_DEPTH][LC_PER_LANE / 4];
#pragma unroll
  for( int k = 0; k < LC_DEPTH; ++k ) lane_chain_load( row, ns, k * LC_SUPER, lane, X[k] );
  for( int base0 = 0; base0 < n; base0 += LC_DEPTH * LC_SUPER )
  {
  const bool more = base0 + LC_DEPTH * LC_SUPER < n;
  if( more )
  {
#pragma unroll
    for( int k = 0; k < LC_DEPTH; ++k ) lane_chain_load( row, ns, base0 + ( LC_DEPTH + k ) * LC_SUPER, lane, Y[k] );
  }
#pragma unroll
  for( int k = 0; k < LC_DEPTH; ++k )
  {
    const int base = base0 + k * LC_SUPER;
    if( base >= n ) break;
    float x[LC_PER_LANE];
    {
      const int i0 = base + lane * LC_PER_LANE;
#pragma unroll
      for( int q = 0; q < LC_PER_LANE / 4; ++q )
      {
        const bool in = i0 + 4 * q < ns;
        x[4 * q] = in ? X[k][q].x : 0.0f; x[4 * q + 1] = in ? X[k][q].y : 0.0f; x[4 * q + 2] = in ? X[k][q].z : 0.0f; x[4 * q + 3] = in ? X[k][q].w : 0.0f;
      }
    }
    // the lane's addends' magnitudes, summed: decides whether the lane can go by the grid at all (below), and is inf or NaN when an
    // addend is not finite (or the sum overflows: beyond any binade's reach anyway)
    float mag = 0.0f;
#pragma unroll
    for( int j = 0; j < LC_PER_LANE; ++j ) mag = mag + fabsf( x[j] );
    int start = 0, seq = 1;
    while( start < WAVE )
    {
      const uint32_t sb = (uint32_t)uni( (int)__float_as_uint( s ) );      // (every lane holds the same value: branch on the scalar unit)
      const int E = (int)( ( sb >> 23 ) & 255u );
      int b = start;                                   // first lane the grid does not carry
      if( E >= 64 && E <= 253 )                        // (below 2^-63 — where an addend could be a denormal worth half a grid step — one by one)
      {
        ++n_try;
        const float sgn = ( sb >> 31 ) ? -1.0f : 1.0f;                                 // |s| grows by -x when s < 0
        const float S = __uint_as_float( sb & 0x7fffffffu );
        const float C = __uint_as_float( ( (uint32_t)E << 23 ) | 0x400000u );          // 1.5 * 2^e
        const float quarter = __uint_as_float( (uint32_t)( E - 1 ) << 23 );            // 2^(e-1): the rounding trick's range
        const float u = __uint_as_float( (uint32_t)( E - 23 ) << 23 ), uh = __uint_as_float( (uint32_t)( E - 24 ) << 23 );      // ulp( S ), half of it
        const float lo_end = __uint_as_float( (uint32_t)E << 23 ) + u, hi_end = __uint_as_float( (uint32_t)( E + 1 ) << 23 ) - u;   // the binade, a grid step clear of its ends
        float p[LC_PER_LANE], run = 0.0f, half = 0.0f;      // half: the largest | x - rounded x | of the lane; u / 2 = an addend exactly half way between two grid points
#pragma unroll
        for( int j = 0; j < LC_PER_LANE; ++j )
        {
          const float r = __builtin_fmaf( x[j], sgn, C ) - C;                          // x (signed for |s|) on the grid, ties to even
          half = fmaxf( half, fabsf( __builtin_fmaf( x[j], sgn, -r ) ) );              // (exact: x and r differ by at most u / 2)
          run = run + r; p[j] = run;
        }
        const float incl = wave_scan_f32( run ), excl = incl - run;
        float lo = p[0], hi = p[0];
#pragma unroll
        for( int j = 1; j < LC_PER_LANE; ++j ) { lo = fminf( lo, p[j] ); hi = fmaxf( hi, p[j] ); }
        // (written so that a NaN anywhere — a lane after one that does not fit — reads as "does not fit")
        const bool fits = mag < quarter && half < uh && S + ( excl + lo ) >= lo_end && S + ( excl + hi ) <= hi_end;
        const unsigned long long badm = __builtin_amdgcn_ballot_w64( !fits && lane >= start );
        b = badm ? (int)__builtin_ctzll( badm ) : WAVE;
        if( b > start )
        {
          const float adv = rl( b < WAVE ? excl : incl, b < WAVE ? b : WAVE - 1 );
          s = sgn * ( S + adv );
        }
      }
      else if( ( sb << 1 ) == 0u )
      {
        // a sum of zero stays zero through addends that are all zero (the unmatched points a source may well begin with)
        const unsigned long long nzm = __builtin_amdgcn_ballot_w64( !( mag == 0.0f ) && lane >= start );
        b = nzm ? (int)__builtin_ctzll( nzm ) : WAVE;
      }
      if( b >= WAVE ) break;
      // lanes [b, e): their addends one after the other in fp32, as the reference adds them
      seq = ( b - start >= 2 ) ? 1 : min( 2 * seq, 4 );
      const int e = min( b + seq, WAVE );
      for( int l = b; l < e; ++l )
      {
#pragma unroll
        for( int j = 0; j < LC_PER_LANE; ++j ) s = s + rl( x[j], l );
      }
      n_seq += ( e - b ) * LC_PER_LANE;
      start = e;
      // the lanes done add nothing from here on (their prefix in the next attempt's scan is zero)
#pragma unroll
      for( int j = 0; j < LC_PER_LANE; ++j ) x[j] = lane < start ? 0.0f : x[j];
      mag = lane < start ? 0.0f : mag;
    }
  }
  if( more )
  {
#pragma unroll
    for( int k = 0; k < LC_DEPTH; ++k )
#pragma unroll
      for( int q = 0; q < LC_PER_LANE / 4; ++q ) X[k][q] = Y[k][q];
  }
  }
  if( dbg ) { dbg[0] = n_seq; dbg[1] = n_try; }
  return s;
}

// Launch 1, every CU: the fp64 moments of a quarter block (1 024 source points) per workgroup, and the seven addends of its points
// into the rows the walks read (B.addends).
__global__ __launch_bounds__( BLOCK ) void k_lane_moments_and_addends( IcpLaunch L, ChainBufs B )
{
  RS_CHAIN_SETPRIO();
  __shared__ ChainMomLds S;
  const int prob = blockIdx.y;
  if( L.active[prob] == 0 ) return;
  icp_bind( L, prob );
  ChainBufs Bq = B; Bq.n_seg = ( L.src.n + CH_SEG - 1 ) / CH_SEG; Bq.refresh = 0;
  chain_moments_block( L, Bq, prob, (int)blockIdx.x, S, L.rec + (size_t)L.pt_off * REC_F4, B.addends + lane_rows_base( L, prob ) );
}

// Launch 2: ONE workgroup per problem — seven waves walk the seven chains (from the addend rows), the eighth sums the moments' partials
// (k_icp_update_wide's work, in the order a 256-thread workgroup per moment added them: thread t takes partials t, t + 256, ...; a wave
// tree per 64; the four waves' sums in turn), a barrier, and the rest of the iteration (icp.h:253-295,455-493) centred on the chains'
// centroids.  (Until late in round 6 this was 35 + 2 workgroups per problem and a ticket for "who finishes last": every one of them a
// release fence, i.e. an L2 write-back — 19 000 of them per launch at 512 problems, 1.19 ms for walks that take 50 us; a barrier
// inside one workgroup needs none.)
constexpr int LW_WAVES = 8;
static_assert( CH_ROWS < LW_WAVES, "a wave per chain and one for the moments" );
__global__ __launch_bounds__( LW_WAVES * WAVE ) void k_lane_walk_and_update( IcpLaunch L, ChainBufs B )
{
  RS_CHAIN_SETPRIO();
  const int prob = blockIdx.x;
  if( L.active[prob] == 0 ) return;
  icp_bind( L, prob );
  const int lane = threadIdx.x & ( WAVE - 1 ), wib = uni( (int)threadIdx.x / WAVE );
  if( wib < CH_ROWS )
  {
    const int row = wib;
    int d[2] = { 0, 0 };
    const unsigned long long t0 = B.dbg ? wall_clock64() : 0ull;
    const float s = lane_chain_walk( B.addends + lane_rows_base( L, prob ) + (size_t)row * lane_row_stride( L.src.n ), L.src.n, lane, d );
    if( lane == 0 )
    {
      B.totals[( (size_t)prob * 3 + 1 ) * ICP_NMOM + row] = (double)s;
      if( B.resolved ) atomicAdd( B.resolved + prob, d[0] );
      // (RS_HIP_LANE_DEBUG) per (problem, chain): ticks of 10 ns the walk took, attempts, addends added one by one — of the last iteration
      if( B.dbg ) { int* o = B.dbg + ( (size_t)prob * CH_ROWS + row ) * 4; o[0] = (int)( wall_clock64() - t0 ); o[1] = d[1]; o[2] = d[0]; o[3] = L.src.n; }
    }
  }
  else if( wib == CH_ROWS )
  {
    for( int k = 0; k < ICP_NMOM; ++k )
    {
      const double* in = L.mom_part + ( (size_t)prob * ICP_NMOM + k ) * L.n_mom_blocks;
      double r[WAVES_PER_BLOCK];
#pragma unroll
      for( int w = 0; w < WAVES_PER_BLOCK; ++w )
      {
        double v = 0.0;
        for( int b = w * WAVE + lane; b < L.n_mom_blocks; b += BLOCK ) v += in[b];
        r[w] = wave_sum( v );
      }
      double t = 0.0;
#pragma unroll
      for( int w = 0; w < WAVES_PER_BLOCK; ++w ) t += r[w];
      if( lane == 0 ) L.res[(size_t)prob * ICP_NRES + k] = t;
    }
  }
  __syncthreads();                                       // (the sums and totals above: this workgroup's own global writes)
  icp_update_tail( L, prob );
}

void launch_icp_lane_chains( const IcpLaunch& L, const ChainBufs& B, hipStream_t st )
{
  hipLaunchKernelGGL( k_lane_moments_and_addends, dim3( L.n_mom_blocks, L.n_prob ), dim3( BLOCK ), 0, st, L, B );      // (L.n_mom_blocks == ceil( max_n / 1024 ))
  hipLaunchKernelGGL( k_lane_walk_and_update, dim3( L.n_prob ), dim3( LW_WAVES * WAVE ), 0, st, L, B );
}

// The step WITHOUT the chains: the fp64 moments from the searches' records, centred on their own fp64 centroids (icp_solve without the
// reference's) — what an early iteration of a scan-sized call runs (rs_api.hip: icp_plain_iterations).  L.exact_centroids must be 0.
void launch_icp_plain_from_records( const IcpLaunch& L, const ChainBufs& B, hipStream_t st )
{
  ChainBufs Bq = B; Bq.refresh = 0;
  hipLaunchKernelGGL( k_chain_moments, dim3( B.n_blk * CH_QUARTERS, L.n_prob ), dim3( BLOCK ), 0, st, L, Bq );
  launch_icp_update_wide( L, B.done, st );
}

// The same step from the searches' matches (L.rec == null in its search: no records written): k_plain_moments' partials, one per
// workgroup — L.n_mom_blocks must be plain_moment_blocks( L.max_tiles ).
void launch_icp_plain_from_matches( const IcpLaunch& L, const ChainBufs& B, hipStream_t st )
{
  hipLaunchKernelGGL( k_plain_moments, dim3( L.n_mom_blocks, L.n_prob ), dim3( BLOCK ), 0, st, L );
  launch_icp_update_wide( L, B.done, st );
}

void launch_icp_chain_centroids( const IcpLaunch& L, const ChainBufs& B, hipStream_t st )
{
  const int n_tasks = ( B.n_seg + CHAIN_REC_TASK - 1 ) / CHAIN_REC_TASK;
  const dim3 rec_grid( ( n_tasks + WAVES_PER_BLOCK * CHAIN_REC_ROUNDS - 1 ) / ( WAVES_PER_BLOCK * CHAIN_REC_ROUNDS ), L.n_prob );
  if( B.refresh )
  {
    // the guesses anew: this iteration's fp64 sums first
    hipLaunchKernelGGL( k_chain_moments, dim3( B.n_blk * CH_QUARTERS, L.n_prob ), dim3( BLOCK ), 0, st, L, B );         // (L.n_mom_blocks == 4 B.n_blk)
    hipLaunchKernelGGL( k_chain_guess, dim3( B.n_blk, L.n_prob ), dim3( CH_ROWS * WAVE ), 0, st, L, B );
    hipLaunchKernelGGL( k_chain_segrecs, rec_grid, dim3( BLOCK ), 0, st, L, B );
    hipLaunchKernelGGL( k_chain_compose, dim3( B.n_blk, L.n_prob, CH_ROWS ), dim3( 3 * WAVE ), 0, st, L, B );
    hipLaunchKernelGGL( k_chain_walk, dim3( CH_ROWS, L.n_prob ), dim3( BLOCK ), 0, st, L, B );
  }
  else
  {
    hipLaunchKernelGGL( k_chain_segrecs, rec_grid, dim3( BLOCK ), 0, st, L, B );
    hipLaunchKernelGGL( k_chain_compose, dim3( B.n_blk, L.n_prob, CH_ROWS ), dim3( 3 * WAVE ), 0, st, L, B );
    hipLaunchKernelGGL( k_chain_walk_and_moments, dim3( CH_ROWS + B.n_blk * ( CH_QUARTERS + 1 ), L.n_prob ), dim3( BLOCK ), 0, st, L, B );
  }
  launch_icp_update_wide( L, B.done, st );                // (centred on the chains' totals: L.exact_centroids)
}

// The same from the searches' records (L.rec: the grid chains' own inputs — what a scan the chains give up is run with): the fp64
// moments by the chains' moment kernel (n, mean, stddev into L.res), pass 2 of the replay reading the records, the chains' update.
void launch_icp_exact_centroids_from_records( const IcpLaunch& L, const ReplayBufs& B, const ChainBufs& C, hipStream_t st )
{
  hipLaunchKernelGGL( k_chain_moments, dim3( C.n_blk * CH_QUARTERS, L.n_prob ), dim3( BLOCK ), 0, st, L, C );          // (L.n_mom_blocks == 4 C.n_blk)
  launch_replay_centroid_pass( L, B, st );
  launch_icp_update_wide( L, C.done, st );
}

} // namespace rs
