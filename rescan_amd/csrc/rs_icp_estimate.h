// What more than one ICP estimator unit uses (rs_icp_update.hip, rs_icp_faithful.hip, rs_icp_chain.hip): device helpers, all inline, and
// the host functions by which one unit has another's kernels launched.
#pragma once
#include "rs_search.h"
#include "rs_icp.h"
#include "rs_tail_dbg.h"      // TD_STAMP: phase stamps of the kernels that end an iteration (diagnostic builds; nothing otherwise)

namespace rs {

// ---- the fp64 moments' addends (layout: rs_icp_update.hip) ----
// One correspondence's share of the 35 moments above: weight w, source point p in the target's frame, matched target point q4 and normal n4
// (shared by k_icp_moments and k_plain_moments: the same expressions, so the same addends).
__device__ __forceinline__ void moments_add( double ( &acc )[ICP_NMOM], float w, float px, float py, float pz, const float4& q4, const float4& n4 )
{
  const double W = w, p[3] = { px, py, pz }, q[3] = { q4.x, q4.y, q4.z }, n[3] = { n4.x, n4.y, n4.z };
  const double a[3] = { p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0] };
  const double e = ( p[0] - q[0] ) * n[0] + ( p[1] - q[1] ) * n[1] + ( p[2] - q[2] ) * n[2];
  acc[0] += W;
  acc[1] += W * p[0]; acc[2] += W * p[1]; acc[3] += W * p[2];
  acc[4] += W * q[0]; acc[5] += W * q[1]; acc[6] += W * q[2];
  acc[7]  += W * a[0] * a[0]; acc[8]  += W * a[0] * a[1]; acc[9]  += W * a[0] * a[2];
  acc[10] += W * a[1] * a[1]; acc[11] += W * a[1] * a[2]; acc[12] += W * a[2] * a[2];
#pragma unroll
  for( int r = 0; r < 3; ++r )
#pragma unroll
    for( int c = 0; c < 3; ++c ) acc[13 + 3 * r + c] += W * a[r] * n[c];
  acc[22] += W * n[0] * n[0]; acc[23] += W * n[0] * n[1]; acc[24] += W * n[0] * n[2];
  acc[25] += W * n[1] * n[1]; acc[26] += W * n[1] * n[2]; acc[27] += W * n[2] * n[2];
  acc[28] += W * a[0] * e; acc[29] += W * a[1] * e; acc[30] += W * a[2] * e;
  acc[31] += W * n[0] * e; acc[32] += W * n[1] * e; acc[33] += W * n[2] * e;
  acc[34] += W * e * e;
}

// ---- the end of an iteration ----
// The rest of an iteration once the moments are summed (icp.h:455-493), in two halves: what it reads that the launch which ends the
// iteration does not itself write — the state words, n_corr, the chains' totals: all left by earlier launches, or by the workgroup's
// own waves before its barrier — and the solve with everything it writes.  k_icp_update_wide loads the first half before it knows
// that it is the workgroup which goes on.
struct IcpTailIn { float T1[16]; float err; int iters; double n_corr; double cen[7]; };
__device__ __forceinline__ IcpTailIn icp_tail_inputs( const IcpLaunch& L, int prob )
{
  IcpTailIn in;
#pragma unroll
  for( int k = 0; k < 16; ++k ) in.T1[k] = L.T1[prob * 16 + k];
  in.err = L.err[prob]; in.iters = L.iters[prob];
  in.n_corr = L.res[(size_t)prob * ICP_NRES + ICP_NMOM];
  const double* t2 = L.centroid_totals + ( (size_t)prob * 3 + 1 ) * ICP_NMOM;
#pragma unroll
  for( int a = 0; a < 7; ++a ) in.cen[a] = L.exact_centroids ? t2[a] : 0.0;
  return in;
}
// (thread 0 of the workgroup that ends the iteration; res: the 35 summed moments; dbg: diagnostic builds' stamps, else null)
__device__ __forceinline__ void icp_tail_finish( const IcpLaunch& L, int prob, const IcpTailIn& in, const double* res, unsigned long long* dbg = nullptr )
{
  // ---- icp.h:455-493 for this problem ----
  L.prev_err[prob] = in.err;
  L.iters[prob] = in.iters + 1;
  if( in.n_corr == 0.0 ) { L.active[prob] = 0; return; }              // icp.h:455-459: no correspondences
  Mat4 T;
  for( int k = 0; k < 16; ++k ) { T.m[k] = in.T1[k]; L.T1_prev[prob * 16 + k] = T.m[k]; }
  float e;
  float cen[6];
  if( L.exact_centroids )
  {
    // the reference's own centroids: c = Σw·p * ( 1.0f / Σw ), every sum its sequential fp32 chain (icp.h:136-148)
    const float total = (float)in.cen[0];
    if( total <= 1e-7 ) { L.active[prob] = 0; return; }                 // icp.h:466-470
    const float inv = __fdiv_rn( 1.0f, total );
    for( int a = 0; a < 6; ++a ) cen[a] = (float)in.cen[1 + a] * inv;
  }
  const bool solved = icp_solve( res, T, e, L.exact_centroids ? cen : nullptr );
  TD_STAMP( dbg, 6 );
  if( !solved ) { L.active[prob] = 0; return; }                         // icp.h:466-470: weights vanished
  for( int k = 0; k < 16; ++k ) L.T1[prob * 16 + k] = T.m[k];           // icp.h:295
  L.err[prob] = e;
  const float delta = fabsf( in.err - e );
  // (an estimator that is not the reference's own order follows the reference's errors to ~1e-7; a stop test decided by less than
  //  that margin may fall the other way — one iteration more or less, 1e-4 in the pose.  Such a problem is flagged: rs_api.hip)
  if( !L.fixed_iters && L.iter_index > 5 && L.stop_guard > 0.0f && fabsf( delta - 1e-5f ) < L.stop_guard ) L.ticket[prob] = 1;
  if( !L.fixed_iters && L.iter_index > 5 && delta < 1e-5 ) L.active[prob] = 0;   // icp.h:489
}

// ... for a workgroup whose own barrier stands between the sums in L.res and this call (the whole workgroup comes in; thread 0 solves).
__device__ __forceinline__ void icp_update_tail( const IcpLaunch& L, int prob, unsigned long long* dbg = nullptr )
{
  if( !L.solve ) return;
  icp_iteration_reset( L, prob );
  if( threadIdx.x != 0 ) return;
  const IcpTailIn in = icp_tail_inputs( L, prob );
  TD_STAMP_LOADED( dbg, 5 );
  icp_tail_finish( L, prob, in, L.res + (size_t)prob * ICP_NRES, dbg );
}

// ---- lane helpers: a lane's value read by the wave, lane masks, prefix scans over the 64 lanes ----
__device__ __forceinline__ int rl( int v, int lane ) { return __builtin_amdgcn_readlane( v, lane ); }
__device__ __forceinline__ uint32_t rl( uint32_t v, int lane ) { return (uint32_t)__builtin_amdgcn_readlane( (int)v, lane ); }
__device__ __forceinline__ long long rl( long long v, int lane )
{
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane( (int)(uint32_t)v, lane ), hi = (uint32_t)__builtin_amdgcn_readlane( (int)(uint32_t)( (unsigned long long)v >> 32 ), lane );
  return (long long)( ( (unsigned long long)hi << 32 ) | lo );
}
__device__ __forceinline__ unsigned long long rl( unsigned long long v, int lane ) { return (unsigned long long)rl( (long long)v, lane ); }
__device__ __forceinline__ uint32_t first_lane( uint32_t v ) { return (uint32_t)__builtin_amdgcn_readfirstlane( (int)v ); }
__device__ __forceinline__ unsigned long long first_lane( unsigned long long v )
{
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane( (int)(uint32_t)v ), hi = (uint32_t)__builtin_amdgcn_readfirstlane( (int)(uint32_t)( v >> 32 ) );
  return ( (unsigned long long)hi << 32 ) | lo;
}
__device__ __forceinline__ float rl( float v, int lane ) { return __int_as_float( __builtin_amdgcn_readlane( __float_as_int( v ), lane ) ); }
__device__ __forceinline__ unsigned long long below( int bit ) { return ( 1ull << bit ) - 1ull; }
// the lowest n set bits of m
__device__ __forceinline__ unsigned long long lowest_bits( unsigned long long m, int n )
{
  for( int c = __builtin_popcountll( m ); c > n && m != 0ull; --c ) m &= ~( 1ull << ( 63 - __builtin_clzll( m ) ) );
  return n > 0 ? m : 0ull;
}
// inclusive prefix max / min over the 64 lanes (signed), like wave_scan: lanes without a source lane keep their own value
#define RS_DPP_PREFIX( OP, v )                                                              \
  asm volatile( "s_nop 4\n\t"                                                               \
                OP " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"        \
                OP " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"        \
                OP " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"        \
                OP " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"        \
                OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"     \
                OP " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"         \
                : "+v"( v ) )
__device__ __forceinline__ double wave_scan_f64( double v, int lane )      // inclusive
{
#pragma unroll
  for( int d = 1; d < WAVE; d <<= 1 ) { const double up = __shfl_up( v, d ); if( lane >= d ) v += up; }
  return v;
}
// (inclusive; lanes without a source lane keep their value.  A forecast needs four digits, not sixteen: fp32 prefix sums, six DPP adds each)
__device__ __forceinline__ float wave_scan_f32( float v ) { RS_DPP_PREFIX( "v_add_f32_dpp", v ); return v; }

// ---- the chains' addends and fp64 moments from the searches' records (grid chains, lane chains; the statistics: k_plain_moments too) ----
struct ChainPar { bool use_sd; float cut, max_dist; };

// the seven addends of one source point (faith_terms<2>: icp.h:141-142, weights icp.h:387,396-401)
__device__ __forceinline__ void chain_addends( const float4& A, const float4& Bq, const ChainPar& P, float x[CH_ROWS], float& w )
{
  const bool m = A.w >= 0.0f;
  w = 0.0f;
  if( m )
  {
    w = ( 1.0f - __fdiv_rn( A.w, P.max_dist ) ) * Bq.w;
    if( P.use_sd && A.w > P.cut ) w = 0.0f;
  }
  x[0] = w;
  x[1] = m ? A.x * w : 0.0f;  x[2] = m ? A.y * w : 0.0f;  x[3] = m ? A.z * w : 0.0f;
  x[4] = m ? Bq.x * w : 0.0f; x[5] = m ? Bq.y * w : 0.0f; x[6] = m ? Bq.z * w : 0.0f;
}

// n_corr, mean, stddev of dist² from the searches' integer statistics (as k_icp_moments); every thread of the block gets the same bits
__device__ __forceinline__ float chain_stats( const IcpLaunch& L, int prob, unsigned long long ( *s_stat )[3], double* st_out )
{
  static_assert( STAT_SHARDS == BLOCK, "one shard per thread" );
  const unsigned long long* a = L.stat_acc + ( (size_t)prob * STAT_SHARDS + ( threadIdx.x & ( BLOCK - 1 ) ) ) * 4;
  const bool mine = threadIdx.x < BLOCK;
  const unsigned long long c0 = wave_sum_u64( mine ? a[0] : 0ull ), c1 = wave_sum_u64( mine ? a[1] : 0ull ), c2 = wave_sum_u64( mine ? a[2] : 0ull );
  if( mine && ( threadIdx.x & ( WAVE - 1 ) ) == 0 ) { unsigned long long* o = s_stat[threadIdx.x / WAVE]; o[0] = c0; o[1] = c1; o[2] = c2; }
  __syncthreads();
  unsigned long long t0 = 0, t1 = 0, t2 = 0;
#pragma unroll
  for( int w = 0; w < WAVES_PER_BLOCK; ++w ) { t0 += s_stat[w][0]; t1 += s_stat[w][1]; t2 += s_stat[w][2]; }
  const double n = (double)t0;
  const float mean = (float)( (double)t1 * L.stat_i1 / n );           // sum / (float)n
  const float sqm = (float)( (double)t2 * L.stat_i2 / n );            // sq_sum / (float)n
  const float var = sqm - mean * mean;
  const float sd = (float)sqrt( (double)var );                        // (float)sqrt( ... ), msh_std.h:1824
  if( st_out ) { st_out[0] = n; st_out[1] = mean; st_out[2] = sd; st_out[3] = (double)L.queue_count[prob]; }
  return sd;
}

// One workgroup per QUARTER of a block of 64 segments (1 024 source points in the reference's order): the fp64 moments' partials, the
// seven chains' fp64 sums per segment, and per quarter block.  Block 0 of the launch leaves n, mean, stddev and the cut's stddev
// in L.res for the kernels that follow.
#define CH_QUARTERS 4
struct ChainMomLds { double red[WAVES_PER_BLOCK][ICP_NMOM]; double bsum[WAVES_PER_BLOCK][CH_ROWS]; unsigned long long stat[WAVES_PER_BLOCK][3]; };
// (R: the problem's records — one source for the whole batch: L.rec + prob * n; a multi-source batch: L.rec + pt_off, see k_lane_chains_and_moments)
// (xrows: where to leave the seven addends of every point of the quarter block, row r at xrows + r * ( ( n + 3 ) & ~3 ) — the lane chains' input; null: not wanted)
__device__ __forceinline__ void chain_moments_block( const IcpLaunch& L, const ChainBufs& B, int prob, int qb, ChainMomLds& S, const float4* R, float* xrows = nullptr )
{
  // quarter block qb: segments [16 qb, 16 qb + 16)
  const float sd = chain_stats( L, prob, S.stat, ( qb == 0 && threadIdx.x == 0 ) ? L.res + (size_t)prob * ICP_NRES + ICP_NMOM : nullptr );
  ChainPar P; P.use_sd = sd > 0.000001; P.cut = 2.5f * sd; P.max_dist = L.radius;
  const int lane = threadIdx.x & ( WAVE - 1 ), wib = threadIdx.x / WAVE;

  double acc[ICP_NMOM], bs[CH_ROWS];
#pragma unroll
  for( int k = 0; k < ICP_NMOM; ++k ) acc[k] = 0.0;
#pragma unroll
  for( int r = 0; r < CH_ROWS; ++r ) bs[r] = 0.0;
  constexpr int SEGS = CH_BLK / CH_QUARTERS;
  for( int sb = wib; sb < SEGS; sb += WAVES_PER_BLOCK )              // a wave's 64 lanes = one segment
  {
    const int seg = qb * SEGS + sb;
    if( seg >= B.n_seg ) break;
    const int i = seg * CH_SEG + lane;
    float4 A = make_float4( 0.0f, 0.0f, 0.0f, -1.0f ), Q = make_float4( 0.0f, 0.0f, 0.0f, 0.0f ), N4 = Q;
    if( i < L.src.n ) { A = R[(size_t)i * REC_F4]; Q = R[(size_t)i * REC_F4 + 1]; N4 = R[(size_t)i * REC_F4 + 2]; }
    float x[CH_ROWS], w;
    chain_addends( A, Q, P, x, w );
    if( xrows )
    {
      const int ns = ( L.src.n + 3 ) & ~3;               // (the row's padding beyond n: zeros)
#pragma unroll
      for( int r = 0; r < CH_ROWS; ++r ) if( i < ns ) xrows[(size_t)r * ns + i] = x[r];
    }
    if( B.refresh )
    {
#pragma unroll
      for( int r = 0; r < CH_ROWS; ++r )
      {
        const double v = wave_sum( (double)x[r] );
        bs[r] += v;
        if( lane == 0 ) B.segsum[( (size_t)prob * CH_ROWS + r ) * B.n_seg + seg] = v;
      }
    }
    if( A.w < 0.0f ) continue;
    const double W = w, p[3] = { A.x, A.y, A.z }, q[3] = { Q.x, Q.y, Q.z }, n[3] = { N4.x, N4.y, N4.z };
    const double a[3] = { p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0] };
    const double e = ( p[0] - q[0] ) * n[0] + ( p[1] - q[1] ) * n[1] + ( p[2] - q[2] ) * n[2];
    acc[0] += W;
    acc[1] += W * p[0]; acc[2] += W * p[1]; acc[3] += W * p[2];
    acc[4] += W * q[0]; acc[5] += W * q[1]; acc[6] += W * q[2];
    acc[7]  += W * a[0] * a[0]; acc[8]  += W * a[0] * a[1]; acc[9]  += W * a[0] * a[2];
    acc[10] += W * a[1] * a[1]; acc[11] += W * a[1] * a[2]; acc[12] += W * a[2] * a[2];
#pragma unroll
    for( int r = 0; r < 3; ++r )
#pragma unroll
      for( int c = 0; c < 3; ++c ) acc[13 + 3 * r + c] += W * a[r] * n[c];
    acc[22] += W * n[0] * n[0]; acc[23] += W * n[0] * n[1]; acc[24] += W * n[0] * n[2];
    acc[25] += W * n[1] * n[1]; acc[26] += W * n[1] * n[2]; acc[27] += W * n[2] * n[2];
    acc[28] += W * a[0] * e; acc[29] += W * a[1] * e; acc[30] += W * a[2] * e;
    acc[31] += W * n[0] * e; acc[32] += W * n[1] * e; acc[33] += W * n[2] * e;
    acc[34] += W * e * e;
  }
  { const double v = wave_sums( acc, lane ); if( lane < ICP_NMOM ) S.red[wib][lane] = v; }
  if( lane == 0 ) { for( int r = 0; r < CH_ROWS; ++r ) S.bsum[wib][r] = bs[r]; }
  __syncthreads();
  if( threadIdx.x < ICP_NMOM )
  {
    double v = 0.0;
    for( int w = 0; w < WAVES_PER_BLOCK; ++w ) v += S.red[w][threadIdx.x];
    L.mom_part[( (size_t)prob * ICP_NMOM + threadIdx.x ) * L.n_mom_blocks + qb] = v;      // (moment-major: k_icp_update reads a moment's partials coalesced)
  }
  if( B.refresh && threadIdx.x >= WAVE && threadIdx.x < WAVE + CH_ROWS )
  {
    double v = 0.0;
    for( int w = 0; w < WAVES_PER_BLOCK; ++w ) v += S.bsum[w][threadIdx.x - WAVE];
    B.blksum[( (size_t)prob * CH_ROWS + ( threadIdx.x - WAVE ) ) * ( B.n_blk * CH_QUARTERS ) + qb] = v;
  }
}

// ---- a chain record as a function of the start mantissa (grid chains; tools/micro/chain_scan_test.hip) ----
#define CH_M_LO ( 1 << 23 )
#define CH_M_HI ( ( 1 << 24 ) - 1 )
// A record's function for one exponent is  M -> M + D, valid for lo <= M <= hi  (lo > hi: never).  A run of records f_0 .. f_l
// applies to a start mantissa M iff  lo_j <= M + D_0 + .. + D_(j-1) <= hi_j  for every j, i.e. iff
//     max_j ( lo_j - Dex_j )  <=  M  <=  min_j ( hi_j - Dex_j ),      Dex_j = the advance of the records before j,
// and then advances it by D_0 + .. + D_l: three integer prefix scans over the lanes (sum, max, min), each six DPP instructions.
// (A never-record has lo - Dex > hi - Dex, so the max passes the min from its lane on: nothing fits any more.)
//
// Ties.  An addend that lands exactly half way between two grid points is rounded to the EVEN one: M + k + ( ( M + k ) & 1 ) — what
// it adds depends on the parity of the value it meets, i.e. on the parity of the record's start mantissa.  After it the value is
// even, whatever it was: later ties of the same record are decided.  So a record with ties is  M -> M + D + tau[ M & 1 ]  with two
// small numbers tau[0], tau[1] (a segment: { c, 1 - c }; a block: composed, chain_compose) — kept in the low four bits of the D
// word — and its interval is narrowed by max tau.  The scans below take D alone; whoever applies a run of records adds, in order,
// the tau each start's parity picks (advance in chain_walk_row, chain_compose_block), having left room for the most they can add.
struct ChainFn { int lo, hi, D, tau; };
__device__ __forceinline__ ChainFn chain_never() { ChainFn f; f.lo = CH_M_HI; f.hi = CH_M_LO; f.D = 0; f.tau = 0; return f; }
__device__ __forceinline__ ChainFn chain_identity() { ChainFn f; f.lo = CH_M_LO; f.hi = CH_M_HI; f.D = 0; f.tau = 0; return f; }
// Lane l ends with the run f_0 .. f_l as one function (normalised like a record; the caller's M test is  lo <= M <= hi).
__device__ __forceinline__ ChainFn chain_prefix( const ChainFn& f, int lane )
{
  const int incl = (int)wave_scan( (uint32_t)f.D, lane );
  const int ex = incl - f.D;
  int a = f.lo - ex, b = f.hi - ex;                 // (|D| < 2^24 per valid record, 0 for a never-record: no overflow over 64 lanes)
  RS_DPP_PREFIX( "v_max_i32_dpp", a );
  RS_DPP_PREFIX( "v_min_i32_dpp", b );
  ChainFn g;
  g.lo = max( a, CH_M_LO ); g.hi = min( b, CH_M_HI ); g.D = incl; g.tau = f.tau;
  const bool never = g.lo > g.hi;
  g.lo = never ? CH_M_HI : g.lo; g.hi = never ? CH_M_LO : g.hi; g.D = never ? 0 : g.D;
  return g;
}

// ---- one unit's kernels launched for another (a kernel is launched by the unit that defines it; hidden: not among the library's symbols) ----
#define RS_INTERNAL __attribute__( ( visibility( "hidden" ) ) )
RS_INTERNAL void launch_icp_update_wide( const IcpLaunch& L, int* done, hipStream_t st );                  // rs_icp_update.hip: k_icp_update_wide
RS_INTERNAL void launch_replay_centroid_pass( const IcpLaunch& L, const ReplayBufs& B, hipStream_t st );  // rs_icp_faithful.hip: pass 2 of the replay, the seven centroid sums

} // namespace rs
