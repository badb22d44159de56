// librescan_hip device code (gfx950, wave64) — ICP estimators: the fp64 moments in one pass over the matches, and the kernels that end an iteration (lib/rs/icp.h:210-298,387-402,455-493)
#define RS_TAIL_DBG_UPD 1    // (diagnostic builds: this unit holds k_icp_update_wide's stamps and the dump, rs_tail_dbg.h)
#include "rs_icp_estimate.h"
#include "rs_switches.h"     // sw_int( SW_UPDATE_FENCED ): which hand-over launch_icp_update_wide launches

namespace rs {

// ------------------------------------------------------------------------------------------
// ICP: weights + normal-equation moments  (lib/rs/icp.h:387,393-402,210-252)
//
// The reference centres the correspondences on their weighted centroids c1, c2 and
// accumulates  Σw·c cᵀ, Σw·c nᵀ, Σw·n nᵀ, Σw·(c,n)·s, Σw·s²  with c = (p-c1)×n,
// s = ((p-c1)-(q-c2))·n.  All of those are polynomials in the UNcentred moments below, so
// one pass in fp64 suffices and the host finishes the algebra (rs_api.hip: icp_solve):
//   [0] Σw   [1..3] Σw·p   [4..6] Σw·q   [7..12] Σw·a aᵀ (xx,xy,xz,yy,yz,zz), a = p×n
//   [13..21] Σw·a nᵀ (row-major a_i n_j)   [22..27] Σw·n nᵀ   [28..30] Σw·a·e   [31..33] Σw·n·e
//   [34] Σw·e²,  e = (p-q)·n
// ------------------------------------------------------------------------------------------

__global__ __launch_bounds__( BLOCK ) void k_icp_moments( IcpLaunch L )
{
  __shared__ double red[WAVES_PER_BLOCK][ICP_NMOM];
  const int prob = blockIdx.y;
  if( L.active[prob] == 0 ) return;
  icp_bind( L, prob );
  Xform T1;
#pragma unroll
  for( int k = 0; k < 16; ++k ) T1.m[k] = L.T1[prob * 16 + k];
  // n_corr, mean, stddev of dist² (icp.h:393-402) from the integer accumulators: every workgroup adds up the same
  // STAT_SHARDS integers, so all of them hold the same bits
  __shared__ unsigned long long s_stat[WAVES_PER_BLOCK][3];
  float sd = 0.0f;
  if( L.stat_acc )
  {
    static_assert( STAT_SHARDS == BLOCK, "one shard per thread" );
    const unsigned long long* a = L.stat_acc + ( (size_t)prob * STAT_SHARDS + threadIdx.x ) * 4;
    const unsigned long long c0 = wave_sum_u64( a[0] ), c1 = wave_sum_u64( a[1] ), c2 = wave_sum_u64( a[2] );
    if( ( threadIdx.x & ( WAVE - 1 ) ) == 0 ) { unsigned long long* o = s_stat[threadIdx.x / WAVE]; o[0] = c0; o[1] = c1; o[2] = c2; }
    __syncthreads();
    unsigned long long t0 = 0, t1 = 0, t2 = 0;
#pragma unroll
    for( int w = 0; w < WAVES_PER_BLOCK; ++w ) { t0 += s_stat[w][0]; t1 += s_stat[w][1]; t2 += s_stat[w][2]; }
    const double n = (double)t0;
    const float mean = (float)( (double)t1 * L.stat_i1 / n );           // sum / (float)n
    const float sqm = (float)( (double)t2 * L.stat_i2 / n );            // sq_sum / (float)n
    const float var = sqm - mean * mean;
    sd = (float)sqrt( (double)var );                                    // (float)sqrt( ... ), msh_std.h:1824
    if( blockIdx.x == 0 && threadIdx.x == 0 )
    {
      double* st = L.res + (size_t)prob * ICP_NRES + ICP_NMOM;
      st[0] = n; st[1] = mean; st[2] = sd; st[3] = (double)L.queue_count[prob];
    }
  }
  const bool use_sd = sd > 0.000001;
  const float cut = 2.5f * sd;

  double acc[ICP_NMOM];
#pragma unroll
  for( int k = 0; k < ICP_NMOM; ++k ) acc[k] = 0.0;

  for( int i = blockIdx.x * BLOCK + threadIdx.x; i < L.src.n; i += gridDim.x * BLOCK )
  {
    const size_t o = (size_t)L.pt_off + i;
    const int slot = L.m_slot[o];
    if( slot < 0 ) continue;
    const float d2 = L.m_d2[o];
    float w;
    if( L.w_explicit ) { w = L.w_explicit[o]; }
    else
    {
      w = ( 1.0f - __fdiv_rn( d2, L.radius ) ) * L.m_dot[o];         // icp.h:387
      if( use_sd && d2 > cut ) w = 0.0f;                              // icp.h:396-401
    }
    float4 p4 = L.src.pos[i];
    float tx, ty, tz, px, py, pz;
    xform3( T1, p4.x, p4.y, p4.z, 1.0f, tx, ty, tz );
    xform3( L.T2i, tx, ty, tz, 1.0f, px, py, pz );
    const float4 q4 = L.tgt.pos[slot], n4 = L.tgt.nor[slot];
    moments_add( acc, w, px, py, pz, q4, n4 );
  }
  const int lane = threadIdx.x & ( WAVE - 1 ), wib = threadIdx.x / WAVE;
#pragma unroll
  for( int k = 0; k < ICP_NMOM; ++k ) { double v = wave_sum( acc[k] ); if( lane == 0 ) red[wib][k] = v; }
  __syncthreads();
  if( threadIdx.x < ICP_NMOM )
  {
    double v = 0.0;
    for( int w = 0; w < WAVES_PER_BLOCK; ++w ) v += red[w][threadIdx.x];
    L.mom_part[( (size_t)prob * L.n_mom_blocks + blockIdx.x ) * ICP_NMOM + threadIdx.x] = v;
  }

}

// One workgroup per problem: fixed-order sum of the per-workgroup partials (moment k by wave k mod 16;
// lane l adds partials l, l+64, l+128, ..., then the wave tree) and — inside the ICP loop — the
// rest of the iteration (icp.h:455-493), which the reference runs on the CPU: 6x6 solve, pose
// update, stop tests.  Nothing goes back to the host between two searches.
#define UPDATE_WAVES 16
__global__ __launch_bounds__( UPDATE_WAVES * WAVE ) void k_icp_update( IcpLaunch L )
{
  const int prob = blockIdx.x;
  if( L.active[prob] == 0 ) return;
  icp_bind( L, prob );
  const int lane = threadIdx.x & ( WAVE - 1 ), wib = threadIdx.x / WAVE;
  const double* in = L.mom_part + (size_t)prob * L.n_mom_blocks * ICP_NMOM;
  double* res = L.res + (size_t)prob * ICP_NRES;
  for( int k = wib; k < ICP_NMOM; k += UPDATE_WAVES )
  {
    double v = 0.0;
    if( L.rec )
    {
      // k_chain_moments' layout (moment-major: coalesced), eight loads in flight per lane; the order of the additions is fixed
      for( int b0 = lane; b0 < L.n_mom_blocks; b0 += 8 * WAVE )
      {
        double t[8];
#pragma unroll
        for( int j = 0; j < 8; ++j ) { const int b = b0 + j * WAVE; t[j] = b < L.n_mom_blocks ? in[(size_t)k * L.n_mom_blocks + b] : 0.0; }
#pragma unroll
        for( int j = 0; j < 8; ++j ) v += t[j];
      }
    }
    else for( int b = lane; b < L.n_mom_blocks; b += WAVE ) v += in[(size_t)b * ICP_NMOM + k];
    v = wave_sum( v );
    if( lane == 0 ) res[k] = v;
  }
  __syncthreads();
  icp_update_tail( L, prob );
}

// The same for the chains' estimator, whose partials come by the thousand (one per 1 024 source points, moment-major): one
// workgroup per MOMENT sums its row (a single workgroup took 14 us over the 400 KB of a 1 M-point scan), the last one to finish
// does the rest of the iteration.  Fixed order throughout: thread t adds partials t, t + 256, ..., then the wave tree, then the
// four waves in turn.
// The hand-over inside the launch is ONE double per workgroup.  Each publishes its sum with an agent-scope atomic (write-through) store,
// waits for it, and draws a relaxed agent-scope ticket; the workgroup whose ticket is the last reads the 35 sums with agent-scope
// atomic loads, which no CU's L1 serves.  (Until round 11: a plain store and __threadfence() — an L2 write-back and invalidate — before
// every ticket, and a second one in the last workgroup: FENCED, kept for A/B runs and tests behind rs_hip_icp_update_fenced( 1 ) /
// RS_HIP_UPDATE_FENCED=1.)  Later launches read L.res and the state as before: the kernel boundary publishes them.
// What the solve reads besides the sums (icp_tail_inputs) was written by earlier launches: thread 0 of EVERY workgroup asks for it before
// its partials, so the loads are long back when the last ticket is drawn; and what has to be reset between two searches
// (icp_iteration_reset) touches nothing the solve reads, so workgroup 0 does it beside the others instead of the last one in front of its solve.
// Measured (profiles/r11/iteration_tail_breakdown.txt, the last workgroup's path of 9 us): one lane's fence over 8 fresh bytes is cheap —
// the two together 1.1-1.3 us, the new hand-over 0.7; the load chain that stood behind the second fence 1.0-1.2 -> 0.5-0.8 (the sums alone);
// the rest of the launch's 13 -> 8.6 us is the reset out of the last workgroup's way and 34 workgroups that no longer fence before they
// leave.  icp_solve on one lane is 4 of the 8.6.
#define RS_WAIT_VMCNT0 0x0F70      // s_waitcnt vmcnt(0) alone (gfx9 encoding: expcnt and lgkmcnt at their maxima)
template <bool FENCED>
__global__ __launch_bounds__( BLOCK ) void k_icp_update_wide( IcpLaunch L, int* done )
{
  RS_CHAIN_SETPRIO();
  __shared__ double s_part[WAVES_PER_BLOCK];
  __shared__ int s_last;
  const int prob = blockIdx.y, k = blockIdx.x;
  if( L.active[prob] == 0 ) return;
  icp_bind( L, prob );
#if RS_TAIL_DBG
  unsigned long long* const dbg = ( prob == 0 && threadIdx.x == 0 ) ? d_upd_dbg[L.iter_index & ( TD_ITERS - 1 )][k] : nullptr;
  if( dbg ) { dbg[4] = 0ull; dbg[5] = 0ull; dbg[6] = 0ull; }
#else
  unsigned long long* const dbg = nullptr;
#endif
  TD_STAMP( dbg, 0 );
  IcpTailIn in{};
  if( !FENCED && L.solve && threadIdx.x == 0 ) in = icp_tail_inputs( L, prob );
  const int lane = threadIdx.x & ( WAVE - 1 ), wib = threadIdx.x / WAVE;
  const double* in_part = L.mom_part + ( (size_t)prob * ICP_NMOM + k ) * L.n_mom_blocks;
  double* const res = L.res + (size_t)prob * ICP_NRES;
  double v = 0.0;
  for( int b = threadIdx.x; b < L.n_mom_blocks; b += BLOCK ) v += in_part[b];
  v = wave_sum( v );
  if( lane == 0 ) s_part[wib] = v;
  __syncthreads();
  if( threadIdx.x == 0 )
  {
    double t = 0.0;
    for( int w = 0; w < WAVES_PER_BLOCK; ++w ) t += s_part[w];
    TD_STAMP( dbg, 1 );
    if( FENCED )
    {
      res[k] = t;
      __threadfence();
      TD_STAMP( dbg, 2 );
      s_last = atomicAdd( done + prob, 1 ) == ICP_NMOM - 1 ? 1 : 0;
    }
    else
    {
      __hip_atomic_store( res + k, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
      // (the ticket must not pass the sum: the store has left the CU before the add is issued; the signal fences keep the compiler from
      //  moving either across the wait)
      __atomic_signal_fence( __ATOMIC_SEQ_CST );
      __builtin_amdgcn_s_waitcnt( RS_WAIT_VMCNT0 );
      __atomic_signal_fence( __ATOMIC_SEQ_CST );
      TD_STAMP( dbg, 2 );
      s_last = __hip_atomic_fetch_add( done + prob, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT ) == ICP_NMOM - 1 ? 1 : 0;
    }
    TD_STAMP( dbg, 3 );
  }
  __syncthreads();
  if( FENCED )
  {
    if( !s_last ) return;
    __threadfence();                                       // (the other workgroups' sums)
    TD_STAMP( dbg, 4 );
    if( threadIdx.x == 0 ) done[prob] = 0;
    icp_update_tail( L, prob, dbg );
    return;
  }
  if( k == 0 && L.solve ) icp_iteration_reset( L, prob );
  if( !s_last || threadIdx.x != 0 ) return;
  __hip_atomic_store( done + prob, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );      // (zero between launches; a call's first fill zeroes it too)
  if( !L.solve ) return;
  double m[ICP_NMOM];
#pragma unroll
  for( int j = 0; j < ICP_NMOM; ++j ) m[j] = __hip_atomic_load( res + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
  TD_STAMP_LOADED( dbg, 5 );
  icp_tail_finish( L, prob, in, m, dbg );
}
void launch_icp_update_wide( const IcpLaunch& L, int* done, hipStream_t st )
{
  if( sw_int( SW_UPDATE_FENCED ) ) hipLaunchKernelGGL( k_icp_update_wide<true>, dim3( ICP_NMOM, L.n_prob ), dim3( BLOCK ), 0, st, L, done );
  else hipLaunchKernelGGL( k_icp_update_wide<false>, dim3( ICP_NMOM, L.n_prob ), dim3( BLOCK ), 0, st, L, done );
}

void launch_icp_moments( const IcpLaunch& L, hipStream_t st )
{
  hipLaunchKernelGGL( k_icp_moments, dim3( L.n_mom_blocks, L.n_prob ), dim3( BLOCK ), 0, st, L );
  hipLaunchKernelGGL( k_icp_update, dim3( L.n_prob ), dim3( UPDATE_WAVES * WAVE ), 0, st, L );
}

} // namespace rs
