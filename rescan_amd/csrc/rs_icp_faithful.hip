// librescan_hip device code (gfx950, wave64) — ICP estimators: the reference's own order and precisions, as one sequential chain per accumulator and in parallel ("replay") (lib/rs/icp.h:136-148,210-298)
#include "rs_icp_estimate.h"

namespace rs {

// ------------------------------------------------------------------------------------------
// ICP estimator in the reference's own order and precisions  (lib/rs/icp.h:136-148,210-298,387-402)
//
// The reference sums everything one correspondence after the other in source order, in fp32 (dist²
// statistics, Σw, the two centroids, the 3x3 blocks, the right-hand side) and in fp64 only Σw·s² and Σw.
// On clouds of a few thousand points that rounding is part of its result: poses drift from the exact
// least-squares step in the 5th digit and the stop test (|Δerr| < 1e-5) can fire an iteration earlier
// or later.  k_icp_moments (rs_icp_update.hip) is the fast, more accurate step; this one reproduces the reference bit
// for bit.  fp32 addition does not associate, so each accumulator is ONE sequential chain over the
// correspondences — but the 35 accumulators are independent chains, and producing the addends is parallel:
//   k_icp_faith_gather   the correspondences in the source's original order, SoA, all threads
//   k_icp_faithful       one workgroup per problem, six waves:
//                          waves 2-5  turn 128 correspondences at a time into the addends of every accumulator (LDS; two threads per
//                                     correspondence)
//                          wave 0     lane a adds row a, entry after entry, to fp32 accumulator a
//                          wave 1     the same for the two fp64 accumulators (their rows arrive as doubles)
//                        double-buffered, so the chains never wait for the producers.
//   Two passes: dist² statistics AND weights, centroids — the statistics reach the centroids only through the 2.5 sigma cut of the
//   weights, taken at a guess and checked afterwards (a third pass, the centroids alone, when the guess cut differently: not once
//   in 349 iterations of 24 object-to-scan runs) — then the normal equations, which need the centroids; thread 0 runs the rest of
//   the iteration exactly as k_icp_update does.  What a pass costs is its longest chain: ~8.6 cycles per addition and row of
//   fp32 (6.5 with nothing else on the CU's LDS), 11.5 of fp64.
// Unmatched source points add +0 (no effect on an accumulator that started at +0).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__( BLOCK ) void k_icp_faith_gather( IcpLaunch L )
{
  const int prob = blockIdx.y;
  if( L.active[prob] == 0 ) return;
  icp_bind( L, prob );
  const int i = blockIdx.x * BLOCK + threadIdx.x, n = L.src.n;
  if( i >= n ) return;
  const int s = L.by_orig ? L.by_orig[i] : i;
  const size_t o = (size_t)L.pt_off + s;
  float* F = L.faith + (size_t)FAITH_REC * (size_t)L.pt_off + i;
  const int slot = L.m_slot[o];
  if( slot < 0 ) { F[0] = -1.0f; return; }
  Xform T1;
#pragma unroll
  for( int k = 0; k < 16; ++k ) T1.m[k] = L.T1[prob * 16 + k];
  const float4 p4 = L.src.pos[s];
  float tx, ty, tz, px, py, pz;
  xform3( T1, p4.x, p4.y, p4.z, 1.0f, tx, ty, tz );
  xform3( L.T2i, tx, ty, tz, 1.0f, px, py, pz );
  const float4 q4 = L.tgt.pos[slot], n4 = L.tgt.nor[slot];
  const size_t N = (size_t)n;
  F[0] = L.w_explicit ? 0.0f : L.m_d2[o];
  F[N] = L.w_explicit ? L.w_explicit[o] : L.m_dot[o];
  F[2 * N] = px;   F[3 * N] = py;   F[4 * N] = pz;
  F[5 * N] = q4.x; F[6 * N] = q4.y; F[7 * N] = q4.z;
  F[8 * N] = n4.x; F[9 * N] = n4.y; F[10 * N] = n4.z;
}

#define FAITH_CHUNK 128
#define FAITH_PITCH ( FAITH_CHUNK + 4 )          // rows stay 16-byte aligned (128-bit LDS reads) and a quarter-wave of them covers all banks once
// Two threads per correspondence of a chunk — four producer waves, two of them beside the chain waves on their SIMDs: the normal
// equations' 35 addends (~200 vector instructions, 35 + 2 LDS writes per correspondence) in two halves.  With one thread each the two
// producer waves set the pace of the last pass (880 k cycles at work over 420 chunks against 465 k of the fp32 chain wave, 620 k
// of the fp64 one: tools/faith_timing.py); with two they take 575 k and the fp64 chain does.  RS_FAITH_SPLIT=0: one thread each.
#ifndef RS_FAITH_SPLIT
#define RS_FAITH_SPLIT 1
#endif
#define FAITH_PRODUCERS ( ( RS_FAITH_SPLIT + 1 ) * FAITH_CHUNK )
#define FAITH_THREADS ( 2 * WAVE + FAITH_PRODUCERS )   // two chain waves + the producer waves

struct FaithRec { float v[FAITH_REC]; };
struct FaithPar
{
  bool  w_explicit, use_sd;
  float max_dist, cut;
  float c1[3], c2[3];
};

__device__ __forceinline__ void faith_load( const float* F, int n, int i, FaithRec& r )
{
  r.v[0] = -1.0f;
  if( i < n )
  {
#pragma unroll
    for( int k = 0; k < FAITH_REC; ++k ) r.v[k] = F[(size_t)k * n + i];
  }
}

__device__ __forceinline__ float faith_weight( const FaithRec& r, const FaithPar& P )
{
  if( P.w_explicit ) return r.v[1];
  float w = ( 1.0f - __fdiv_rn( r.v[0], P.max_dist ) ) * r.v[1];      // icp.h:387
  if( P.use_sd && r.v[0] > P.cut ) w = 0.0f;                           // icp.h:396-401
  return w;
}

// the addends of one correspondence for pass PASS, written to column t of `term` (RS_FAITH_SPLIT: of PASS 3 rows [0,18) for half 0,
// [18,35) for half 1; half 2: all)
template <int PASS>
__device__ __forceinline__ void faith_terms( const FaithRec& r, const FaithPar& P, float ( *term )[FAITH_PITCH], int t, int half = 2,
                                             double ( *termd )[FAITH_PITCH] = nullptr /* PASS 3: rows 33, 34 also as doubles */ )
{
  if( PASS != 3 && half == 1 ) return;
  const bool m = r.v[0] >= 0.0f;
  if( PASS == 1 || PASS == 12 )
  {
    constexpr int R0 = PASS == 12 ? 7 : 0;
    term[R0 + 0][t] = m ? r.v[0] : 0.0f;            // msh_compute_mean
    term[R0 + 1][t] = m ? r.v[0] * r.v[0] : 0.0f;   // msh_compute_stddev
    term[R0 + 2][t] = m ? 1.0f : 0.0f;              // n_corrs (exact in fp32 below 2^24)
  }
  if( PASS == 1 ) return;
  if( PASS == 2 || PASS == 12 )
  {
    const float w = m ? faith_weight( r, P ) : 0.0f;
    term[0][t] = w;                                 // icp.h:141  total += w
#pragma unroll
    for( int a = 0; a < 3; ++a )
    {
      term[1 + a][t] = m ? r.v[2 + a] * w : 0.0f;   // icp.h:142  c = c + p*w
      term[4 + a][t] = m ? r.v[5 + a] * w : 0.0f;
    }
  }
  else
  {
    if( !m )
    {
      if( half != 1 ) {
#pragma unroll
        for( int a = 0; a < 18; ++a ) term[a][t] = 0.0f;
      }
      if( half != 0 ) {
#pragma unroll
        for( int a = 18; a < ICP_NMOM; ++a ) term[a][t] = 0.0f;
        if( termd ) { termd[0][t] = 0.0; termd[1][t] = 0.0; }
      }
      return;
    }
    const float wi = faith_weight( r, P );
    const float p[3] = { r.v[2] - P.c1[0], r.v[3] - P.c1[1], r.v[4] - P.c1[2] };
    const float q[3] = { r.v[5] - P.c2[0], r.v[6] - P.c2[1], r.v[7] - P.c2[2] };
    const float nv[3] = { r.v[8], r.v[9], r.v[10] };
    const float d[3] = { p[0] - q[0], p[1] - q[1], p[2] - q[2] };
    const float cv[3] = { p[1] * nv[2] - p[2] * nv[1], p[2] * nv[0] - p[0] * nv[2], p[0] * nv[1] - p[1] * nv[0] };
    const float sd = d[0] * nv[0] + d[1] * nv[1] + d[2] * nv[2];
    if( half != 1 )
    {
#pragma unroll
      for( int col = 0; col < 3; ++col )
#pragma unroll
        for( int row = 0; row < 3; ++row )
        {
          term[3 * col + row][t]      = ( cv[row] * cv[col] ) * wi;   // icp.h:239-241, column-major blocks
          term[9 + 3 * col + row][t]  = ( cv[row] * nv[col] ) * wi;
        }
    }
    if( half == 0 ) return;
#pragma unroll
    for( int col = 0; col < 3; ++col )
#pragma unroll
      for( int row = 0; row < 3; ++row ) term[18 + 3 * col + row][t] = ( nv[row] * nv[col] ) * wi;
#pragma unroll
    for( int a = 0; a < 3; ++a )
    {
      term[27 + a][t] = wi * cv[a] * sd;            // icp.h:242-247
      term[30 + a][t] = wi * nv[a] * sd;
    }
    term[33][t] = wi * sd * sd;                     // icp.h:249 (a float product, summed in fp64)
    term[34][t] = wi;                               // icp.h:250
    if( termd ) { termd[0][t] = (double)( wi * sd * sd ); termd[1][t] = (double)wi; }
  }
}

// A chain wave's chunk: its row's 128 entries added one after the other, straight from LDS, sixteen at a time — the reads of the next
// sixteen go out before this group's additions.  Columns past the end of the cloud hold +0, so every chunk is a full one.
// (A whole row staged in registers first — two of them, 256 registers — pushed the kernel's allocation into AGPRs, one
// v_accvgpr_read per addend; reads placed between the additions one by one took 50 % longer.  None of it shows: a chunk takes what
// its 128 dependent additions take, ~8 cycles each.)
// (the two fp64 accumulators' rows arrive as doubles — the producers' conversion: with a v_cvt_f64_f32 in front of every addition the
//  fp64 wave took 1.5 times as long as the fp32 wave, and set the pace of the last pass together with the producers)
__device__ __forceinline__ void faith_chain_lds( const double* row, double& acc )
{
  const double2* row2 = reinterpret_cast<const double2*>( row );
  double2 a[4], b[4];
#pragma unroll
  for( int j = 0; j < 4; ++j ) a[j] = row2[j];
#pragma unroll
  for( int g = 0; g < FAITH_CHUNK / 8; ++g )
  {
    double2* cur = ( g & 1 ) ? b : a; double2* nxt = ( g & 1 ) ? a : b;
    if( g + 1 < FAITH_CHUNK / 8 )
    {
#pragma unroll
      for( int j = 0; j < 4; ++j ) nxt[j] = row2[( g + 1 ) * 4 + j];
    }
#pragma unroll
    for( int j = 0; j < 4; ++j ) { acc += cur[j].x; acc += cur[j].y; }
    __builtin_amdgcn_sched_barrier( 0 );
  }
}
template <class ACC>
__device__ __forceinline__ void faith_chain_lds( const float* row, ACC& acc )
{
  const float4* row4 = reinterpret_cast<const float4*>( row );
  float4 a[4], b[4];
#pragma unroll
  for( int j = 0; j < 4; ++j ) a[j] = row4[j];
#pragma unroll
  for( int g = 0; g < FAITH_CHUNK / 16; ++g )
  {
    float4* cur = ( g & 1 ) ? b : a; float4* nxt = ( g & 1 ) ? a : b;
    if( g + 1 < FAITH_CHUNK / 16 )
    {
#pragma unroll
      for( int j = 0; j < 4; ++j ) nxt[j] = row4[( g + 1 ) * 4 + j];
    }
#pragma unroll
    for( int j = 0; j < 4; ++j ) { acc += (ACC)cur[j].x; acc += (ACC)cur[j].y; acc += (ACC)cur[j].z; acc += (ACC)cur[j].w; }
    __builtin_amdgcn_sched_barrier( 0 );          // (the scheduler would gather all the row's reads in front of the chain)
  }
}

// One pass over the correspondences: rows [0,NF) end in accf of wave 0's lanes, rows [NF,NF+ND) in accd of wave 1's.
// Iteration k: the producers write chunk k (and keep FAITH_AHEAD chunks of loads in flight: a chunk is consumed faster
// than a load returns); the chain waves add up chunk k-1 from LDS.
#define FAITH_AHEAD 4
// PASS 12: statistics and centroids in ONE pass, the weights cut at a guess of 2.5 sigma (P.cut); band[0] / band[1] end as the largest
// dist² not above the guess and the smallest above it (bits: dist² >= 0) — the guess cut the weights exactly as the real value
// does iff the real value lies in [band[0], band[1]).
template <int PASS, int NF, int ND>
__device__ __forceinline__ void faith_pass( const float* F, int n, const FaithPar& P, float ( *term )[ICP_NMOM][FAITH_PITCH], double ( *termd )[2][FAITH_PITCH],
                                            float& accf, double& accd, unsigned* band = nullptr, int* timing = nullptr /* (experiment: -DRS_FAITH_TIMING=<pass>) */ )
{
  const int wib = threadIdx.x / WAVE, lane = threadIdx.x & ( WAVE - 1 );
  const int t = ( threadIdx.x - 2 * WAVE ) & ( FAITH_CHUNK - 1 );              // producer column ...
  const int half = RS_FAITH_SPLIT ? uni( (int)( threadIdx.x - 2 * WAVE ) / FAITH_CHUNK ) : 2;      // ... and which of its addends (RS_FAITH_SPLIT: half of them; wave-uniform)
  const int n_chunks = ( n + FAITH_CHUNK - 1 ) / FAITH_CHUNK;
  const int my_row = wib == 0 ? ( lane < NF ? lane : -1 ) : ( wib == 1 && lane < ND ? NF + lane : -1 );
  accf = 0.0f; accd = 0.0;
  FaithRec ring[FAITH_AHEAD];
  float d_below = 0.0f, d_above = INFINITY;
  const bool producer = wib >= 2;
#ifdef RS_FAITH_TIMING
  long long t_work = 0, t_wait = 0;
#endif
  if( producer )
  {
#pragma unroll
    for( int u = 0; u < FAITH_AHEAD; ++u ) faith_load( F, n, u * FAITH_CHUNK + t, ring[u] );
  }
  for( int k0 = 0; k0 <= n_chunks; k0 += FAITH_AHEAD )
  {
#pragma unroll
    for( int u = 0; u < FAITH_AHEAD; ++u )
    {
      const int k = k0 + u;
#ifdef RS_FAITH_TIMING
      const long long c0 = clock64();
#endif
      if( wib >= 2 )
      {
        if( producer && k < n_chunks )
        {
          if( PASS == 12 && half != 1 && ring[u].v[0] >= 0.0f )
          {
            if( ring[u].v[0] > P.cut ) d_above = fminf( d_above, ring[u].v[0] ); else d_below = fmaxf( d_below, ring[u].v[0] );
          }
          faith_terms<PASS>( ring[u], P, term[k & 1], t, half, PASS == 3 ? termd[k & 1] : nullptr );
          faith_load( F, n, ( k + FAITH_AHEAD ) * FAITH_CHUNK + t, ring[u] );
        }
      }
      else if( my_row >= 0 )
      {
        // chunk k - 1 (written during step k - 1, the barrier since), while the producers write chunk k into the other buffer
        if( k >= 1 && k <= n_chunks )
        {
          if( wib == 0 ) faith_chain_lds( term[( k - 1 ) & 1][my_row], accf ); else faith_chain_lds( termd[( k - 1 ) & 1][my_row - NF], accd );
        }
      }
#ifdef RS_FAITH_TIMING
      const long long c1 = clock64();
#endif
      __syncthreads();
#ifdef RS_FAITH_TIMING
      t_work += c1 - c0; t_wait += clock64() - c1;
#endif
    }
  }
#ifdef RS_FAITH_TIMING
  if( lane == 0 && PASS == RS_FAITH_TIMING && timing && wib < 4 ) { int* o = timing + 2 + 3 * wib; o[0] = (int)t_work; o[1] = (int)t_wait; o[2] = n_chunks; }
#endif
  if( PASS == 12 && producer ) { atomicMax( band, __float_as_uint( d_below ) ); atomicMin( band + 1, __float_as_uint( d_above ) ); }
}

__global__ __launch_bounds__( FAITH_THREADS ) void k_icp_faithful( IcpLaunch L )
{
  __shared__ __attribute__( ( aligned( 16 ) ) ) float term[2][ICP_NMOM][FAITH_PITCH];
  __shared__ __attribute__( ( aligned( 16 ) ) ) double termd[2][2][FAITH_PITCH];
  __shared__ float s_f[ICP_NMOM];
  __shared__ double s_d[2], s_g[FAITH_THREADS / WAVE][3];
  __shared__ unsigned s_band[2];
  const int prob = blockIdx.x;
  if( L.active[prob] == 0 ) return;
  icp_bind( L, prob );
  if( L.solve ) icp_iteration_reset( L, prob );            // (the search of this iteration is over: its queue has been consumed)
  const int wib = threadIdx.x / WAVE, lane = threadIdx.x & ( WAVE - 1 );
  const int n = L.src.n;
  const float* F = L.faith + (size_t)FAITH_REC * (size_t)L.pt_off;
  FaithPar P;
  P.w_explicit = L.w_explicit != nullptr; P.use_sd = false; P.max_dist = L.radius; P.cut = 0.0f;
  P.c1[0] = P.c1[1] = P.c1[2] = P.c2[0] = P.c2[1] = P.c2[2] = 0.0f;
  float accf; double accd;

  // ---- icp.h:393-402: mean and standard deviation of dist² over the correspondences; icp.h:136-148: Σw and the two weighted centroids ----
  // The statistics only reach the centroids through the 2.5 sigma cut of the weights (icp.h:396-401), a COMPARISON: with a guess of
  // sigma (fp64 sums, all threads, a few microseconds) both sets of chains run in one pass — ten rows instead of three, then
  // seven: a chain wave's time does not depend on how many of its lanes are rows — and the pass stands if no dist² lies between
  // the guessed and the real cut (and they agree on whether to cut at all).  Otherwise the centroids again, as before.
  bool have_centroids = false;
  if( !P.w_explicit )
  {
    {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0;
      for( int i = threadIdx.x; i < n; i += FAITH_THREADS ) { const float d = F[i]; if( d >= 0.0f ) { a0 += (double)d; a1 += (double)d * (double)d; a2 += 1.0; } }
      a0 = wave_sum( a0 ); a1 = wave_sum( a1 ); a2 = wave_sum( a2 );
      if( lane == 0 ) { s_g[wib][0] = a0; s_g[wib][1] = a1; s_g[wib][2] = a2; }
      if( threadIdx.x == 0 ) { s_band[0] = 0u; s_band[1] = __float_as_uint( INFINITY ); }
      __syncthreads();
      double t0 = 0.0, t1 = 0.0, t2 = 0.0;
      for( int w = 0; w < FAITH_THREADS / WAVE; ++w ) { t0 += s_g[w][0]; t1 += s_g[w][1]; t2 += s_g[w][2]; }
      const double mean_g = t2 > 0.0 ? t0 / t2 : 0.0, var_g = t2 > 0.0 ? t1 / t2 - mean_g * mean_g : 0.0;
      const float sd_g = (float)sqrt( var_g > 0.0 ? var_g : 0.0 );
      P.use_sd = sd_g > 0.000001; P.cut = 2.5f * sd_g * L.faith_guess_scale;
    }
    const bool guessed_use = P.use_sd;
    if( L.faith_guess_scale != 0.0f ) faith_pass<12, 10, 0>( F, n, P, term, termd, accf, accd, s_band, L.faith_redone );
    else                              faith_pass<1, 3, 0>( F, n, P, term, termd, accf, accd );
    const int r0 = L.faith_guess_scale != 0.0f ? 7 : 0;
    if( wib == 0 && lane < 10 ) s_f[lane] = accf;
    __syncthreads();
    const float cnt = s_f[r0 + 2];
    if( cnt == 0.0f )                                                   // icp.h:455-459: no correspondences
    {
      if( threadIdx.x == 0 && L.solve ) { L.prev_err[prob] = L.err[prob]; L.iters[prob] += 1; L.active[prob] = 0; }
      return;
    }
    const float mean = __fdiv_rn( s_f[r0], cnt );                       // msh_std.h:1800-1825
    const float var = __fdiv_rn( s_f[r0 + 1], cnt ) - mean * mean;
    const float sd = (float)sqrt( (double)var );
    P.use_sd = sd > 0.000001;
    P.cut = 2.5f * sd;
    have_centroids = L.faith_guess_scale != 0.0f && P.use_sd == guessed_use && ( !P.use_sd || ( __uint_as_float( s_band[0] ) <= P.cut && P.cut < __uint_as_float( s_band[1] ) ) );
    if( !have_centroids && L.faith_guess_scale != 0.0f && threadIdx.x == 0 && L.faith_redone ) atomicAdd( L.faith_redone, 1 );
    __syncthreads();                                                    // (s_f is rewritten below if the pass does not stand)
  }

  if( !have_centroids )
  {
    faith_pass<2, 7, 0>( F, n, P, term, termd, accf, accd );
    if( wib == 0 && lane < 7 ) s_f[lane] = accf;
    __syncthreads();
  }
  const float total = s_f[0];
  if( total <= 1e-7 )                                                   // icp.h:466-470: the weights vanished
  {
    if( threadIdx.x == 0 && L.solve ) { L.prev_err[prob] = L.err[prob]; L.iters[prob] += 1; L.active[prob] = 0; }
    return;
  }
  const float inv = __fdiv_rn( 1.0f, total );
#pragma unroll
  for( int a = 0; a < 3; ++a ) { P.c1[a] = s_f[1 + a] * inv; P.c2[a] = s_f[4 + a] * inv; }
  __syncthreads();

  // ---- icp.h:221-252: the normal equations ----
  faith_pass<3, 33, 2>( F, n, P, term, termd, accf, accd, nullptr, L.faith_redone );
  if( wib == 0 && lane < 33 ) s_f[lane] = accf;
  if( wib == 1 && lane < 2 ) s_d[lane] = accd;
  __syncthreads();
  if( threadIdx.x != 0 ) return;

  // ---- icp.h:253-295 and the loop's bookkeeping (icp.h:455-493), as in k_icp_update ----
  float A[33];
  for( int k = 0; k < 33; ++k ) A[k] = s_f[k];
  Mat4 T;
  for( int k = 0; k < 16; ++k ) { T.m[k] = L.T1[prob * 16 + k]; if( L.solve ) L.T1_prev[prob * 16 + k] = T.m[k]; }
  float e;
  icp_solve_ref_order( A, s_d[0], s_d[1], P.c1, T, e );
  for( int k = 0; k < 16; ++k ) L.T1[prob * 16 + k] = T.m[k];
  if( !L.solve ) { L.err[prob] = e; return; }
  L.prev_err[prob] = L.err[prob];
  L.iters[prob] += 1;
  L.err[prob] = e;
  const float delta = fabsf( L.prev_err[prob] - e );
  if( !L.fixed_iters && L.iter_index > 5 && delta < 1e-5 ) L.active[prob] = 0;   // icp.h:489
}

// ------------------------------------------------------------------------------------------
// The reference-order estimator, in parallel ("replay")
//
// k_icp_faithful above runs each of the reference's accumulators as ONE sequential chain: 10-12 ns per source point and
// iteration, 1.5 ms per iteration on a 134 k-point scan.  The same bits can be had in parallel, because of what an IEEE
// addition S + x does while S stays inside one binade [2^e, 2^(e+1)): it adds x ROUNDED TO THE BINADE'S GRID (ulp u), and that
// rounding does not depend on S — except for an exact tie (x mod u = u/2), which goes to the even neighbour, i.e. depends on
// the parity of S's mantissa.  So over a stretch of addends during which the accumulator stays inside its binade, the
// sequential sum is   S_out = S_in + D(parity of S_in),   with D a constant of the stretch.
//
//   k_replay_sums   cuts the source (original order) into segments of 128 points and sums every accumulator's addends per
//                   segment in fp64;
//   k_replay_scan   prefix-sums those per accumulator: a GUESS of the accumulator's value at every segment start (good to a
//                   few thousand ulps: the real chain's own rounding is what it misses);
//   k_replay_run    runs, for every segment and accumulator in parallel, the real fp32 (fp64) chain over the segment from the
//                   guess — once per CLASS of the start's mantissa modulo 4 — and records for which exact starts of that class
//                   the chain is the exact chain shifted: the shift delta = (exact start - class start), in units of the
//                   start's ulp, must keep every intermediate value strictly inside the binade the class's chain visits at
//                   that step (an interval for delta, intersected over the 128 steps — the chain may cross binades), and must
//                   be an EVEN number of grid steps in every binade visited (so that ties round the same way: delta a multiple
//                   of 2^(k+1) where the grid is 2^k coarser than the start's);
//   k_replay_walk   one wave per accumulator walks the segments in order with the EXACT value: if its sign / exponent are the
//                   guess's and delta passes the class's tests, the segment's result is the class's end value shifted by delta
//                   (in the end binade's grid) — exact, by the argument above; otherwise (a sign change inside the segment,
//                   the start of a chain, a guess in the wrong binade) the wave re-adds the segment's 128 addends one after
//                   the other.
//
// Three passes like k_icp_faithful (statistics -> weights and centroids -> normal equations), each needing the previous one's
// totals; every block recomputes the few scalars between passes itself.  Addends come from the same faith_terms<PASS> the
// sequential kernel uses.  Result: the reference's bits (tests: against k_icp_faithful and the reference-generated fixtures).
// ------------------------------------------------------------------------------------------
#define REPLAY_SEG 128
#define REPLAY_PITCH ( REPLAY_SEG + 4 )

template <int PASS> struct ReplayRows;
template <> struct ReplayRows<1> { enum { NF = 3, ND = 0 }; };     // Σd², Σd⁴, count
template <> struct ReplayRows<2> { enum { NF = 7, ND = 0 }; };     // Σw, Σw·p (3), Σw·q (3)
template <> struct ReplayRows<3> { enum { NF = 33, ND = 2 }; };    // 3x3 blocks, rhs | Σw·s², Σw (fp64 in the reference)

#define REPLAY_CLS 4
// What k_replay_run records per (accumulator, segment) and class c = (start mantissa mod 4) — start = the guess's bits with
// the two low mantissa bits cleared, class start = start | c.  With delta = m - (class start's mantissa): the record is
// usable iff sign + exponent match, dmin <= delta <= dmax (dmax < dmin: never) and delta is a multiple of 2 << need_k; the
// result is then `end` with its mantissa advanced by delta >> k_end (k_end >= 0) or delta << -k_end.
struct ReplayCls { long long dmin, dmax; unsigned long long end; int need_k, k_end; };
struct ReplaySeg { unsigned long long start; unsigned long long pad; ReplayCls cls[REPLAY_CLS]; };

// the scalars between the passes, from the totals of the finished passes (identical code to k_icp_faithful's)
__device__ __forceinline__ bool replay_params( const IcpLaunch& L, int prob, int pass, const double* totals /* ICP_NMOM per pass */, FaithPar& P )
{
  P.w_explicit = L.w_explicit != nullptr; P.use_sd = false; P.max_dist = L.radius; P.cut = 0.0f;
  P.c1[0] = P.c1[1] = P.c1[2] = P.c2[0] = P.c2[1] = P.c2[2] = 0.0f;
  if( pass >= 2 && !P.w_explicit && L.exact_centroids )
  {
    // the cut of k_icp_moments (same expressions, same bits: both take n, mean, stddev from the integer statistics of the search)
    const double* st = L.res + (size_t)prob * ICP_NRES + ICP_NMOM;
    if( st[0] == 0.0 ) return false;
    const float sd = (float)st[2];
    P.use_sd = sd > 0.000001;
    P.cut = 2.5f * sd;
  }
  else if( pass >= 2 && !P.w_explicit )
  {
    const double* t1 = totals;                                         // pass 1: Σd², Σd⁴, count (floats kept in doubles)
    const float cnt = (float)t1[2];
    if( cnt == 0.0f ) return false;
    const float mean = __fdiv_rn( (float)t1[0], cnt );                 // msh_std.h:1800-1825
    const float var = __fdiv_rn( (float)t1[1], cnt ) - mean * mean;
    const float sd = (float)sqrt( (double)var );
    P.use_sd = sd > 0.000001;
    P.cut = 2.5f * sd;
  }
  if( pass >= 3 )
  {
    const double* t2 = totals + ICP_NMOM;                              // pass 2: Σw, Σw·p, Σw·q
    const float total = (float)t2[0];
    if( total <= 1e-7 ) return false;
    const float inv = __fdiv_rn( 1.0f, total );
#pragma unroll
    for( int a = 0; a < 3; ++a ) { P.c1[a] = (float)t2[1 + a] * inv; P.c2[a] = (float)t2[4 + a] * inv; }
  }
  return true;
}

// One correspondence as the estimators' kernels take it: from k_icp_faith_gather's arrays — or, where the searches left their 48-byte
// records at the points' ORIGINAL indices (whole scans: the centroid sums by pass 2 here, when the grid chains give a scan up), straight
// from those: the same eleven numbers, without the gather launch (117 us at a million points).
template <int PASS>
__device__ __forceinline__ void replay_load( const IcpLaunch& L, int prob, int i, FaithRec& r )
{
  const int n = L.src.n;
#pragma unroll
  for( int k = 0; k < FAITH_REC; ++k ) r.v[k] = 0.0f;
  if( !L.rec ) { faith_load( L.faith + (size_t)prob * FAITH_REC * n, n, i, r ); return; }
  r.v[0] = -1.0f;
  if( i < n )
  {
    const float4* R = L.rec + ( (size_t)prob * n + i ) * REC_F4;
    const float4 a = R[0], b = R[1];
    r.v[0] = a.w; r.v[1] = b.w; r.v[2] = a.x; r.v[3] = a.y; r.v[4] = a.z; r.v[5] = b.x; r.v[6] = b.y; r.v[7] = b.z;
    if( PASS == 3 ) { const float4 c = R[2]; r.v[8] = c.x; r.v[9] = c.y; r.v[10] = c.z; }      // (the target's normal: the normal equations' alone)
  }
}
// the addends of segment g for pass PASS, into term[row][t] (all rows of the pass, 128 columns; columns past the cloud hold +0)
template <int PASS>
__device__ __forceinline__ void replay_terms( const IcpLaunch& L, int prob, int g, const FaithPar& P, float ( *term )[REPLAY_PITCH] )
{
  for( int t = threadIdx.x; t < REPLAY_SEG; t += blockDim.x )
  {
    FaithRec r; replay_load<PASS>( L, prob, g * REPLAY_SEG + t, r );
    faith_terms<PASS>( r, P, reinterpret_cast<float ( * )[FAITH_PITCH]>( term ), t );
  }
}
static_assert( REPLAY_PITCH == FAITH_PITCH, "replay_terms reuses faith_terms' LDS layout" );

// ONE accumulator's addend of one correspondence — the expressions of faith_terms<PASS>, row by row (the walk re-adds a segment of ONE
// row: producing all 35 rows' addends for it, as the kernels above do, was most of what a re-added segment cost)
template <int PASS>
__device__ __forceinline__ float faith_term_one( const FaithRec& r, const FaithPar& P, int row /* uniform */ )
{
  const bool m = r.v[0] >= 0.0f;
  if( PASS == 1 ) return row == 0 ? ( m ? r.v[0] : 0.0f ) : ( row == 1 ? ( m ? r.v[0] * r.v[0] : 0.0f ) : ( m ? 1.0f : 0.0f ) );
  if( PASS == 2 )
  {
    const float w = m ? faith_weight( r, P ) : 0.0f;
    if( row == 0 ) return w;
    const float v = row == 1 ? r.v[2] : row == 2 ? r.v[3] : row == 3 ? r.v[4] : row == 4 ? r.v[5] : row == 5 ? r.v[6] : r.v[7];
    return m ? v * w : 0.0f;
  }
  if( !m ) return 0.0f;
  const float wi = faith_weight( r, P );
  if( row == 34 ) return wi;
  const float p[3] = { r.v[2] - P.c1[0], r.v[3] - P.c1[1], r.v[4] - P.c1[2] };
  const float q[3] = { r.v[5] - P.c2[0], r.v[6] - P.c2[1], r.v[7] - P.c2[2] };
  const float nv[3] = { r.v[8], r.v[9], r.v[10] };
  const float d[3] = { p[0] - q[0], p[1] - q[1], p[2] - q[2] };
  const float cv[3] = { p[1] * nv[2] - p[2] * nv[1], p[2] * nv[0] - p[0] * nv[2], p[0] * nv[1] - p[1] * nv[0] };
  const float sd = d[0] * nv[0] + d[1] * nv[1] + d[2] * nv[2];
  auto pick = []( const float ( &x )[3], int k ) -> float { return k == 0 ? x[0] : ( k == 1 ? x[1] : x[2] ); };
  if( row < 27 )
  {
    const int blk = row / 9, in = row % 9, col = in / 3, rw = in % 3;
    const float a = blk == 2 ? pick( nv, rw ) : pick( cv, rw );              // cv cv | cv nv | nv nv
    const float b = blk == 0 ? pick( cv, col ) : pick( nv, col );
    return ( a * b ) * wi;                                                 // icp.h:239-241
  }
  if( row < 30 ) return wi * pick( cv, row - 27 ) * sd;                     // icp.h:242-247
  if( row < 33 ) return wi * pick( nv, row - 30 ) * sd;
  return wi * sd * sd;                                                     // icp.h:249
}
template <int PASS>
__device__ __forceinline__ void replay_term_row( const IcpLaunch& L, int prob, int g, const FaithPar& P, float ( *term )[REPLAY_PITCH], int row )
{
  for( int t = threadIdx.x; t < REPLAY_SEG; t += blockDim.x )
  {
    FaithRec r; replay_load<PASS>( L, prob, g * REPLAY_SEG + t, r );
    term[row][t] = faith_term_one<PASS>( r, P, row );
  }
}

template <int PASS>
__global__ __launch_bounds__( REPLAY_SEG ) void k_replay_sums( IcpLaunch L, ReplayBufs B )
{
  __shared__ __attribute__( ( aligned( 16 ) ) ) float term[ICP_NMOM][REPLAY_PITCH];
  const int prob = blockIdx.y, g = blockIdx.x;
  if( L.active[prob] == 0 ) return;
  FaithPar P;
  const double* totals = B.totals + (size_t)prob * 3 * ICP_NMOM;
  if( !replay_params( L, prob, PASS, totals, P ) ) return;
  replay_terms<PASS>( L, prob, g, P, term );
  __syncthreads();
  constexpr int NR = ReplayRows<PASS>::NF + ReplayRows<PASS>::ND;
  if( threadIdx.x < NR )
  {
    double a = 0.0;
    for( int t = 0; t < REPLAY_SEG; ++t ) a += (double)term[threadIdx.x][t];
    B.segsum[( (size_t)prob * ICP_NMOM + threadIdx.x ) * B.n_seg + g] = a;
  }
}

// exclusive prefix over the segments, per accumulator: the guesses (as the accumulator's own type: float rows, double rows).  One
// workgroup per accumulator: every thread a contiguous run of segments, the runs' totals scanned through LDS (any association will
// do: this is a guess).  (One wave looping over the segments 64 at a time took 76 us on a 1.15 M-point scan's 9 007 segments.)
#define REPLAY_SCAN_THREADS 256
template <int PASS>
__global__ __launch_bounds__( REPLAY_SCAN_THREADS ) void k_replay_scan( IcpLaunch L, ReplayBufs B )
{
  __shared__ double part[REPLAY_SCAN_THREADS];
  const int prob = blockIdx.y, row = blockIdx.x;
  if( L.active[prob] == 0 ) return;
  const int t = threadIdx.x;
  const double* in = B.segsum + ( (size_t)prob * ICP_NMOM + row ) * B.n_seg;
  double* out = B.guess + ( ( (size_t)prob * 3 + ( PASS - 1 ) ) * ICP_NMOM + row ) * B.n_seg;
  const int per = ( B.n_seg + REPLAY_SCAN_THREADS - 1 ) / REPLAY_SCAN_THREADS;
  const int g0 = min( t * per, B.n_seg ), g1 = min( g0 + per, B.n_seg );
  double sum = 0.0;
  for( int g = g0; g < g1; ++g ) sum += in[g];
  part[t] = sum;
  __syncthreads();
  for( int d = 1; d < REPLAY_SCAN_THREADS; d <<= 1 )       // inclusive scan of the runs' totals
  {
    const double up = t >= d ? part[t - d] : 0.0;
    __syncthreads();
    part[t] += up;
    __syncthreads();
  }
  double carry = part[t] - sum;                            // what the runs before this one add
  for( int g = g0; g < g1; ++g ) { out[g] = carry; carry += in[g]; }
}

// one accumulator type: the bit-level view of fp32 / fp64 the replay needs
template <class T> struct Bits;
template <> struct Bits<float>
{
  typedef uint32_t U; enum { MBITS = 23 };
  static __device__ __forceinline__ U of( float v ) { return __float_as_uint( v ); }
  static __device__ __forceinline__ float from( U b ) { return __uint_as_float( b ); }
};
template <> struct Bits<double>
{
  typedef unsigned long long U; enum { MBITS = 52 };
  static __device__ __forceinline__ U of( double v ) { return (U)__double_as_longlong( v ); }
  static __device__ __forceinline__ double from( U b ) { return __longlong_as_double( (long long)b ); }
};

// the chain of one (accumulator, segment, class)
// (fp32 rows keep their shift bounds in 32-bit integers: a value that RISES more than 7 binades inside one segment makes the record
//  unusable — the walk re-adds that segment — where the 64-bit form allowed 20; the loop is bound by instruction issue, and 64-bit
//  compares, selects and shifts were most of its ~40 instructions per addend)
template <class T> struct ReplayRunInt;
template <> struct ReplayRunInt<float>  { typedef int W; enum { KUP = 7 }; };
template <> struct ReplayRunInt<double> { typedef long long W; enum { KUP = 8 }; };
template <class T>
__device__ __forceinline__ void replay_run_chain( const float* row, double guess, int c, ReplaySeg& out )
{
  typedef typename Bits<T>::U U;
  typedef typename ReplayRunInt<T>::W W;
  constexpr int MB = Bits<T>::MBITS, EB = 8 * sizeof(T) - 1 - MB;
  constexpr int KUP = ReplayRunInt<T>::KUP, KDN = MB == 23 ? 20 : 8;      // (shifted mantissas must fit W)
  const U mmask = ( (U)1 << MB ) - 1, emax = ( (U)1 << EB ) - 1;
  const T gT = (T)guess;
  const U gb = Bits<T>::of( gT ) & ~(U)( REPLAY_CLS - 1 );
  const int e0 = (int)( ( gb >> MB ) & emax );
  const bool usable = e0 != 0 && e0 != (int)emax;               // normal, finite, non-zero
  if( c == 0 ) { out.start = (unsigned long long)gb; out.pad = 0ull; }
  const U sb = gb | (U)c;
  T acc = Bits<T>::from( sb );
  const W m0 = (W)( sb & mmask );
  W dmin = 1 - m0, dmax = (W)mmask - 1 - m0;
  int need_k = 0, k = 0;
  bool valid = usable;
  for( int t = 0; t < REPLAY_SEG; ++t )
  {
    acc += (T)row[t];
    const U b = Bits<T>::of( acc );
    const int e = (int)( ( b >> MB ) & emax );
    k = e - e0;
    valid = valid && !( ( b ^ sb ) >> ( 8 * sizeof(T) - 1 ) ) && e != 0 && e != (int)emax && k <= KUP && k >= -KDN;
    const int kk = valid ? k : 0;                              // (keeps the shifts below defined once the chain is lost)
    const W M = (W)( b & mmask );
    W lo = 1 - M, hi = (W)mmask - 1 - M;                       // allowed shift of this value, in its own binade's grid steps
    if( kk >= 0 ) { lo *= ( (W)1 << kk ); hi *= ( (W)1 << kk ); need_k = kk > need_k ? kk : need_k; }
    else
    {
      const int sh = -kk; const W rnd = ( (W)1 << sh ) - 1;
      lo = lo >= 0 ? ( ( lo + rnd ) >> sh ) : -( ( -lo ) >> sh );          // ceil( lo / 2^sh )
      hi = hi >= 0 ? ( hi >> sh ) : -( ( -hi + rnd ) >> sh );              // floor( hi / 2^sh )
    }
    dmin = lo > dmin ? lo : dmin; dmax = hi < dmax ? hi : dmax;
  }
  ReplayCls r;
  r.dmin = valid ? (long long)dmin : 1; r.dmax = valid ? (long long)dmax : 0;
  r.end = (unsigned long long)Bits<T>::of( acc );
  r.need_k = need_k; r.k_end = valid ? k : 0;
  out.cls[c] = r;
}

#define REPLAY_RUN_THREADS 192        // >= 35 rows x 4 classes and >= REPLAY_SEG term producers
template <int PASS>
__global__ __launch_bounds__( REPLAY_RUN_THREADS ) void k_replay_run( IcpLaunch L, ReplayBufs B )
{
  __shared__ __attribute__( ( aligned( 16 ) ) ) float term[ICP_NMOM][REPLAY_PITCH];
  const int prob = blockIdx.y, g = blockIdx.x;
  if( L.active[prob] == 0 ) return;
  FaithPar P;
  const double* totals = B.totals + (size_t)prob * 3 * ICP_NMOM;
  if( !replay_params( L, prob, PASS, totals, P ) ) return;
  replay_terms<PASS>( L, prob, g, P, term );
  __syncthreads();
  constexpr int NF = ReplayRows<PASS>::NF, NR = NF + ReplayRows<PASS>::ND;
  static_assert( NR * REPLAY_CLS <= REPLAY_RUN_THREADS, "one thread per (row, class)" );
  const int row = threadIdx.x / REPLAY_CLS, c = threadIdx.x % REPLAY_CLS;
  if( row < NR )
  {
    const size_t o = ( (size_t)prob * ICP_NMOM + row ) * B.n_seg + g;
    const double guess = B.guess[( ( (size_t)prob * 3 + ( PASS - 1 ) ) * ICP_NMOM + row ) * B.n_seg + g];
    if( row < NF ) replay_run_chain<float>( term[row], guess, c, B.seg[o] );
    else           replay_run_chain<double>( term[row], guess, c, B.seg[o] );
  }
}

// 64 consecutive segments composed into ONE record of the same form, per class of the first segment's start: the walk can then
// take 8 192 addends in a step.  With delta the (class-aligned) offset of the exact value at the superblock's start, the exact
// value entering segment s is  base_s + delta * 2^-K_s  (base_s: where the guess chains lead when delta = 0; K_s: how much
// coarser the grid has become); segment s's own tests on its delta_s = (base_s - its class start) + delta * 2^-K_s turn into an
// interval and a divisibility condition on delta, and its result into the next base.  Anything that does not fit (a base in
// another binade than the segment's guess, a constant part that fails the segment's divisibility) makes the class unusable, and
// the walk then steps through the superblock's segments one by one.
#define REPLAY_SUPER 64
template <class T>
__device__ __forceinline__ void replay_compose_chain( const ReplaySeg* segs, int n, int c0, ReplaySeg& out )
{
  typedef typename Bits<T>::U U;
  constexpr int MB = Bits<T>::MBITS;
  constexpr int KMAX = MB == 23 ? 20 : 8;
  const U mmask = ( (U)1 << MB ) - 1;
  const long long big = 1ll << ( MB + 3 );                        // |delta| < 2^MB
  U base = (U)segs[0].start | (U)c0;
  if( c0 == 0 ) { out.start = segs[0].start; out.pad = 0ull; }
  long long dmin = -big, dmax = big;
  int modlog = 2, K = 0;                                           // delta is a multiple of 4 (class); grid shift so far
  bool valid = true;
  for( int s = 0; s < n && valid; ++s )
  {
    const U st = (U)segs[s].start;
    if( ( ( base ^ st ) & ~mmask ) != 0 ) { valid = false; break; }
    const int c = (int)( base & ( REPLAY_CLS - 1 ) );
    const ReplayCls r = segs[s].cls[c];
    if( r.dmax < r.dmin ) { valid = false; break; }
    const long long cst = (long long)( base & mmask ) - (long long)( ( st & mmask ) | (U)c );        // a multiple of 4
    if( ( cst & ( ( 2ll << r.need_k ) - 1 ) ) != 0 ) { valid = false; break; }
    // r.dmin <= cst + delta * 2^-K <= r.dmax
    long long lo = r.dmin - cst, hi = r.dmax - cst;
    lo = lo < -big ? -big : lo; hi = hi > big ? big : hi;
    if( K >= 0 ) { lo *= ( 1ll << K ); hi *= ( 1ll << K ); }
    else { const int sh = -K; const long long rnd = ( 1ll << sh ) - 1; lo = lo >= 0 ? ( ( lo + rnd ) >> sh ) : -( ( -lo ) >> sh ); hi = hi >= 0 ? ( hi >> sh ) : -( ( -hi + rnd ) >> sh ); }
    dmin = lo > dmin ? lo : dmin; dmax = hi < dmax ? hi : dmax;
    // delta * 2^-K must keep the class (multiple of 4) and the segment's divisibility
    const int need = K + ( r.need_k + 1 > 2 ? r.need_k + 1 : 2 );
    modlog = need > modlog ? need : modlog;
    // next base, next grid
    const U eb = (U)r.end;
    const long long adv = r.k_end >= 0 ? ( cst >> r.k_end ) : cst * ( 1ll << -r.k_end );
    base = ( eb & ~mmask ) | (U)( (long long)( eb & mmask ) + adv );
    K += r.k_end;
    if( K > KMAX || K < -KMAX || modlog > MB ) valid = false;
  }
  ReplayCls q;
  q.dmin = valid ? dmin : 1; q.dmax = valid ? dmax : 0;
  q.end = (unsigned long long)base; q.need_k = modlog - 1; q.k_end = valid ? K : 0;
  out.cls[c0] = q;
}

// four accumulator rows per workgroup: their superblock's 64 records are staged in LDS (coalesced), then one thread per
// (row, class) composes from there (a thread chasing 64 dependent records in global memory took 50-100 us)
#define REPLAY_COMPOSE_ROWS 4
template <int PASS>
__global__ __launch_bounds__( WAVE ) void k_replay_compose( IcpLaunch L, ReplayBufs B )
{
  __shared__ __attribute__( ( aligned( 16 ) ) ) ReplaySeg stage[REPLAY_COMPOSE_ROWS][REPLAY_SUPER];
  static_assert( sizeof( ReplaySeg ) % 16 == 0, "staged with 16-byte copies" );
  const int prob = blockIdx.z, sb = blockIdx.x, row0 = blockIdx.y * REPLAY_COMPOSE_ROWS;
  if( L.active[prob] == 0 ) return;
  constexpr int NF = ReplayRows<PASS>::NF, NR = NF + ReplayRows<PASS>::ND;
  const int g0 = sb * REPLAY_SUPER, n = min( REPLAY_SUPER, B.n_seg - g0 );
  constexpr int Q = sizeof( ReplaySeg ) / 16;
  for( int r = 0; r < REPLAY_COMPOSE_ROWS && row0 + r < NR; ++r )
  {
    const uint4* src = reinterpret_cast<const uint4*>( B.seg + ( (size_t)prob * ICP_NMOM + row0 + r ) * B.n_seg + g0 );
    uint4* dst = reinterpret_cast<uint4*>( stage[r] );
    for( int k = threadIdx.x; k < n * Q; k += WAVE ) dst[k] = src[k];
  }
  __syncthreads();
  const int r = threadIdx.x / REPLAY_CLS, c = threadIdx.x % REPLAY_CLS, row = row0 + r;
  if( r >= REPLAY_COMPOSE_ROWS || row >= NR ) return;
  ReplaySeg& out = B.super[( (size_t)prob * ICP_NMOM + row ) * B.n_super + sb];
  if( row < NF ) replay_compose_chain<float>( stage[r], n, c, out );
  else           replay_compose_chain<double>( stage[r], n, c, out );
}

// The walk of one accumulator over its segments, with the exact value.  Lane l of the wave holds the record of segment g0 + l
// in registers; step j fetches lane j's fields with v_readlane (j is uniform), so the running value, the record and all the
// arithmetic of a step live in SCALAR registers: no memory access and no vector-ALU latency on the chain of 10^3-10^4 dependent
// steps (a version that read the records from LDS spent 740 cycles per step).
template <class T> struct ReplayFields;
template <> struct ReplayFields<float>  { typedef int I; };
template <> struct ReplayFields<double> { typedef long long I; };

// one lane's record, compact and typed, for the scalar walk.  Per class the tests are prepared as whole-word bounds — the value's sign,
// exponent and mantissa together: lo <= value <= hi holds the exponent / sign match and the interval of the shift at once — so that a
// step of the walk is five register reads and a dozen scalar instructions.
template <class T> struct ReplayLaneRec
{
  typedef typename Bits<T>::U U; typedef typename ReplayFields<T>::I I;
  U lo[REPLAY_CLS], hi[REPLAY_CLS], base[REPLAY_CLS], end[REPLAY_CLS]; int meta[REPLAY_CLS];
  __device__ __forceinline__ void clear() { for( int c = 0; c < REPLAY_CLS; ++c ) { lo[c] = 1; hi[c] = 0; base[c] = 0; end[c] = 0; meta[c] = 64 << 8; } }
  __device__ __forceinline__ void load( const ReplaySeg& q )
  {
    const U mmask = ( (U)1 << Bits<T>::MBITS ) - 1;
    const long long clampv = 1ll << ( Bits<T>::MBITS + 2 );       // |delta| < 2^MBITS: bounds beyond that say nothing
    const U st = (U)q.start, top = st & ~mmask;
#pragma unroll
    for( int c = 0; c < REPLAY_CLS; ++c )
    {
      const long long dlo = q.cls[c].dmin, dhi = q.cls[c].dmax;
      const long long bm = (long long)( ( st & mmask ) | (U)c );                                   // the class start's mantissa
      long long l = bm + ( dlo < -clampv ? -clampv : ( dlo > clampv ? clampv : dlo ) ), h = bm + ( dhi < -clampv ? -clampv : ( dhi > clampv ? clampv : dhi ) );
      l = l < 0 ? 0 : l; h = h > (long long)mmask ? (long long)mmask : h;
      const bool never = dhi < dlo || l > h;
      lo[c] = never ? (U)1 : ( top | (U)l ); hi[c] = never ? (U)0 : ( top | (U)h );
      base[c] = top | (U)bm;
      end[c] = (U)q.cls[c].end;
      meta[c] = q.cls[c].need_k | ( ( q.cls[c].k_end + 64 ) << 8 );
    }
  }
  // lane j's record applied to the (uniform) value sb: true and sb advanced, or false
  __device__ __forceinline__ bool apply( int j, U& sb ) const
  {
    const U mmask = ( (U)1 << Bits<T>::MBITS ) - 1;
    const int c = (int)( sb & ( REPLAY_CLS - 1 ) );
    U l, h, bs, eb; int m;
    switch( c )                                          // (uniform)
    {
      case 0:  l = rl( lo[0], j ); h = rl( hi[0], j ); bs = rl( base[0], j ); eb = rl( end[0], j ); m = rl( meta[0], j ); break;
      case 1:  l = rl( lo[1], j ); h = rl( hi[1], j ); bs = rl( base[1], j ); eb = rl( end[1], j ); m = rl( meta[1], j ); break;
      case 2:  l = rl( lo[2], j ); h = rl( hi[2], j ); bs = rl( base[2], j ); eb = rl( end[2], j ); m = rl( meta[2], j ); break;
      default: l = rl( lo[3], j ); h = rl( hi[3], j ); bs = rl( base[3], j ); eb = rl( end[3], j ); m = rl( meta[3], j ); break;
    }
    const I d = (I)( sb - bs );                                                               // (same sign and exponent where it counts: the mantissas' difference, a multiple of 4)
    const int need_k = m & 255, k_end = ( m >> 8 ) - 64;
    const bool ok = sb >= l && sb <= h && ( d & ( ( (I)2 << need_k ) - 1 ) ) == 0;
    if( ok )
    {
      const I adv = k_end >= 0 ? ( d >> k_end ) : d * ( (I)1 << -k_end );
      sb = ( eb & ~mmask ) | (U)( (I)( eb & mmask ) + adv );
    }
    return ok;
  }
};

template <class T, int PASS>
__device__ __forceinline__ T replay_walk_row( const IcpLaunch& L, const ReplayBufs& B, int prob, int row, const FaithPar& P,
                                               float ( *term )[REPLAY_PITCH], int lane, int* n_redone )
{
  typedef typename Bits<T>::U U;
  const ReplaySeg* segs = B.seg + ( (size_t)prob * ICP_NMOM + row ) * B.n_seg;
  const ReplaySeg* sups = B.super + ( (size_t)prob * ICP_NMOM + row ) * B.n_super;
  U sb = 0;                                             // the running value's bits (uniform): +0
  int redone = 0;
  // (Fetching superblock S + 1's segment records while S is walked — they do not depend on the value — was tried for the chains that fit
  //  none of their superblocks' composed records: 1 028 instead of 970 us per iteration on the centred 1.15 M-point scans, 640 instead of
  //  628 at 84 k points: the fetch and its 60 instructions of unpacking are then paid at EVERY superblock.)
  for( int s0 = 0; s0 < B.n_super; s0 += WAVE )
  {
    ReplayLaneRec<T> sup; sup.clear();                  // lane l: superblock s0 + l
    if( s0 + lane < B.n_super ) sup.load( sups[s0 + lane] );
    const int n_sup = min( WAVE, B.n_super - s0 );
    for( int js = 0; js < n_sup; ++js )
    {
      if( sup.apply( js, sb ) ) continue;               // 64 segments in one step
      // step through the superblock's segments
      const int g0 = ( s0 + js ) * REPLAY_SUPER, n_here = min( REPLAY_SUPER, B.n_seg - g0 );
      ReplayLaneRec<T> seg; seg.clear();
      if( lane < n_here ) seg.load( segs[g0 + lane] );
      for( int j = 0; j < n_here; ++j )
      {
        if( seg.apply( j, sb ) ) continue;
        // re-add the segment's addends one after the other (uniform over the wave: the value and the record are)
        ++redone;
        __syncthreads();                                // (one wave per block: orders the reuse of `term`)
        replay_term_row<PASS>( L, prob, g0 + j, P, term, row );
        __syncthreads();
        T acc = Bits<T>::from( sb );
        const float4* row4 = reinterpret_cast<const float4*>( term[row] );
#pragma unroll 8
        for( int t4 = 0; t4 < REPLAY_SEG / 4; ++t4 ) { const float4 v = row4[t4]; acc += (T)v.x; acc += (T)v.y; acc += (T)v.z; acc += (T)v.w; }
        sb = first_lane( Bits<T>::of( acc ) );
      }
    }
  }
  if( n_redone ) *n_redone = redone;
  return Bits<T>::from( sb );
}

template <int PASS>
__global__ __launch_bounds__( WAVE ) void k_replay_walk( IcpLaunch L, ReplayBufs B )
{
  __shared__ __attribute__( ( aligned( 16 ) ) ) float term[ICP_NMOM][REPLAY_PITCH];
  const int prob = blockIdx.y, row = blockIdx.x;
  if( L.active[prob] == 0 ) return;
  FaithPar P;
  double* totals = B.totals + (size_t)prob * 3 * ICP_NMOM;
  if( !replay_params( L, prob, PASS, totals, P ) ) return;
  constexpr int NF = ReplayRows<PASS>::NF;
  const int lane = threadIdx.x;
  int redone = 0;
  double v;
  if( row < NF ) v = (double)replay_walk_row<float, PASS>( L, B, prob, row, P, term, lane, &redone );
  else           v = replay_walk_row<double, PASS>( L, B, prob, row, P, term, lane, &redone );
  if( lane == 0 )
  {
    totals[( PASS - 1 ) * ICP_NMOM + row] = v;        // (floats are exact in a double)
    if( B.redone ) atomicAdd( B.redone + prob, redone );
  }
}

// the rest of the iteration (icp.h:253-295, 455-493), as k_icp_faithful's last thread does it
__global__ __launch_bounds__( WAVE ) void k_replay_finish( IcpLaunch L, ReplayBufs B )
{
  const int prob = blockIdx.x;
  if( L.active[prob] == 0 ) return;
  icp_bind( L, prob );
  if( L.solve ) icp_iteration_reset( L, prob );            // (by the whole wave: it averages a sample of per-tile counts)
  if( threadIdx.x != 0 ) return;
  const double* totals = B.totals + (size_t)prob * 3 * ICP_NMOM;
  FaithPar P;
  const bool ok = replay_params( L, prob, 3, totals, P );
  if( !ok )                                             // icp.h:455-459 / 466-470: no correspondences, or the weights vanished
  {
    if( L.solve ) { L.prev_err[prob] = L.err[prob]; L.iters[prob] += 1; L.active[prob] = 0; }
    return;
  }
  const double* t3 = totals + 2 * ICP_NMOM;
  float A[33];
  for( int k = 0; k < 33; ++k ) A[k] = (float)t3[k];
  Mat4 T;
  for( int k = 0; k < 16; ++k ) { T.m[k] = L.T1[prob * 16 + k]; if( L.solve ) L.T1_prev[prob * 16 + k] = T.m[k]; }
  float e;
  icp_solve_ref_order( A, t3[33], t3[34], P.c1, T, e );
  for( int k = 0; k < 16; ++k ) L.T1[prob * 16 + k] = T.m[k];
  if( !L.solve ) { L.err[prob] = e; return; }
  L.prev_err[prob] = L.err[prob];
  L.iters[prob] += 1;
  L.err[prob] = e;
  const float delta = fabsf( L.prev_err[prob] - e );
  if( !L.fixed_iters && L.iter_index > 5 && delta < 1e-5 ) L.active[prob] = 0;   // icp.h:489
}

template <int PASS>
static void launch_replay_pass( const IcpLaunch& L, const ReplayBufs& B, hipStream_t st )
{
  constexpr int NR = ReplayRows<PASS>::NF + ReplayRows<PASS>::ND;
  hipLaunchKernelGGL( k_replay_sums<PASS>, dim3( B.n_seg, L.n_prob ), dim3( REPLAY_SEG ), 0, st, L, B );
  hipLaunchKernelGGL( k_replay_scan<PASS>, dim3( NR, L.n_prob ), dim3( REPLAY_SCAN_THREADS ), 0, st, L, B );
  hipLaunchKernelGGL( k_replay_run<PASS>, dim3( B.n_seg, L.n_prob ), dim3( REPLAY_RUN_THREADS ), 0, st, L, B );
  hipLaunchKernelGGL( k_replay_compose<PASS>, dim3( B.n_super, ( NR + REPLAY_COMPOSE_ROWS - 1 ) / REPLAY_COMPOSE_ROWS, L.n_prob ), dim3( WAVE ), 0, st, L, B );
  hipLaunchKernelGGL( k_replay_walk<PASS>, dim3( NR, L.n_prob ), dim3( WAVE ), 0, st, L, B );
}
void launch_icp_replay( const IcpLaunch& L, const ReplayBufs& B, hipStream_t st )
{
  hipLaunchKernelGGL( k_icp_faith_gather, dim3( ( L.src.n + BLOCK - 1 ) / BLOCK, L.n_prob ), dim3( BLOCK ), 0, st, L );
  if( !L.w_explicit ) launch_replay_pass<1>( L, B, st );
  launch_replay_pass<2>( L, B, st );
  launch_replay_pass<3>( L, B, st );
  hipLaunchKernelGGL( k_replay_finish, dim3( L.n_prob ), dim3( WAVE ), 0, st, L, B );
}
void launch_replay_centroid_pass( const IcpLaunch& L, const ReplayBufs& B, hipStream_t st ) { launch_replay_pass<2>( L, B, st ); }
int replay_segments( int n_source ) { return ( n_source + REPLAY_SEG - 1 ) / REPLAY_SEG; }
int replay_superblocks( int n_source ) { return ( replay_segments( n_source ) + REPLAY_SUPER - 1 ) / REPLAY_SUPER; }
size_t replay_seg_bytes() { return sizeof( ReplaySeg ); }

void launch_icp_faithful( const IcpLaunch& L, hipStream_t st )
{
  hipLaunchKernelGGL( k_icp_faith_gather, dim3( ( L.max_n + BLOCK - 1 ) / BLOCK, L.n_prob ), dim3( BLOCK ), 0, st, L );
  hipLaunchKernelGGL( k_icp_faithful, dim3( L.n_prob ), dim3( FAITH_THREADS ), 0, st, L );
}

} // namespace rs
