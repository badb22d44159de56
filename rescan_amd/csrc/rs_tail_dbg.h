// Diagnostics of the two kernels that end a plain ICP iteration (k_plain_moments: rs_icp_chain.hip, k_icp_update_wide: rs_icp_update.hip).
// Every estimator unit sees the macros (through rs_icp_estimate.h); a kernel's stamps live in its own unit's code object, so the unit that
// defines RS_TAIL_DBG_MOM holds k_plain_moments' and hands them out, the one that defines RS_TAIL_DBG_UPD holds the others and the dump.
// Build: tools/variant.sh taildbg -DRS_TAIL_DBG=1, load with RS_HIP_LIB=.../librescan_hip_taildbg.so, run an ICP call, then call
//   extern "C" int rs_hip_debug_tail_dump( int n_iters );      (ctypes: declared nowhere else — it exists in that build only)
// profiles/r11/iteration_tail_breakdown.txt is its output, condensed.
#pragma once
#include "rs_search.h"
// wall_clock64() stamps at the phase boundaries of the two kernels that end a plain
// iteration, per workgroup / per wave of problem 0, one set per iteration; rs_hip_debug_tail_dump() prints them.  Off in the shipped build.
#ifndef RS_TAIL_DBG
#define RS_TAIL_DBG 0
#endif
#if RS_TAIL_DBG
#include <algorithm>
#include <cstdio>
#include <vector>
namespace rs {
constexpr int TD_ITERS = 16, TD_UPD = 8, TD_WAVES = 2048, TD_MOM = 16, TD_TILES = 11;
hipError_t td_read_mom( unsigned long long* out );
#ifdef RS_TAIL_DBG_UPD
__device__ unsigned long long d_upd_dbg[TD_ITERS][ICP_NMOM][TD_UPD];   // [iteration][workgroup][phase]
#endif
#ifdef RS_TAIL_DBG_MOM
__device__ unsigned long long d_mom_dbg[TD_ITERS][TD_WAVES][TD_MOM];   // [iteration][wave]{ start, loop entered, after tile 0.., [13] loop left, [14] end, [15] tiles }
hipError_t td_read_mom( unsigned long long* out ) { return hipMemcpyFromSymbol( out, HIP_SYMBOL( d_mom_dbg ), sizeof( d_mom_dbg ) ); }
#endif
#define TD_STAMP( p, s ) do { if( p ) { __builtin_amdgcn_sched_barrier( 0 ); ( p )[s] = wall_clock64(); __builtin_amdgcn_sched_barrier( 0 ); } } while( 0 )
// ... after everything the thread has loaded so far has arrived
#define TD_STAMP_LOADED( p, s ) do { if( p ) { __atomic_signal_fence( __ATOMIC_SEQ_CST ); __builtin_amdgcn_s_waitcnt( 0x0F70 ); TD_STAMP( p, s ); } } while( 0 )
} // namespace rs

#ifdef RS_TAIL_DBG_UPD
// (diagnostic build only) The stamps of the last call, as a table on stdout: per iteration, k_plain_moments per wave and k_icp_update_wide
// per workgroup; times in microseconds (wall_clock64 ticks of 10 ns).
extern "C" int rs_hip_debug_tail_dump( int n_iters )
{
  using namespace rs;
  typedef unsigned long long u64;
  std::vector<u64> U( (size_t)TD_ITERS * ICP_NMOM * TD_UPD ), M( (size_t)TD_ITERS * TD_WAVES * TD_MOM );
  if( hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol( U.data(), HIP_SYMBOL( d_upd_dbg ), U.size() * 8 ) != hipSuccess ||
      td_read_mom( M.data() ) != hipSuccess ) return -1;
  auto stats = []( std::vector<double>& v, double& lo, double& med, double& hi, double& mean )
  { lo = med = hi = mean = 0.0; if( v.empty() ) return; std::sort( v.begin(), v.end() ); lo = v.front(); hi = v.back(); med = v[v.size() / 2]; for( double x : v ) mean += x; mean /= (double)v.size(); };
  for( int it = 0; it < std::min( n_iters, TD_ITERS ); ++it )
  {
    const u64* m = M.data() + (size_t)it * TD_WAVES * TD_MOM;
    u64 t0 = ~0ull, t1 = 0; int waves = 0;
    std::vector<double> pro, tile, epi, tot, nt, first_end, last_start;
    for( int w = 0; w < TD_WAVES; ++w )
    {
      const u64* r = m + (size_t)w * TD_MOM;
      if( !r[0] || !r[14] ) continue;
      ++waves; t0 = std::min( t0, r[0] ); t1 = std::max( t1, r[14] );
      const int n = (int)r[15];
      nt.push_back( n ); tot.push_back( ( r[14] - r[0] ) / 100.0 ); epi.push_back( ( r[14] - r[13] ) / 100.0 );
      if( n > 0 ) pro.push_back( ( r[1] - r[0] ) / 100.0 );
      for( int j = 0; j < std::min( n, TD_TILES ); ++j ) tile.push_back( ( r[2 + j] - ( j ? r[1 + j] : r[1] ) ) / 100.0 );
    }
    for( int w = 0; w < TD_WAVES; ++w ) { const u64* r = m + (size_t)w * TD_MOM; if( r[0] && r[14] ) { first_end.push_back( ( r[14] - t0 ) / 100.0 ); last_start.push_back( ( r[0] - t0 ) / 100.0 ); } }
    double a, b, c, d;
    if( waves )
    {
      printf( "iteration %d  k_plain_moments: %d waves stamped, first start to last end %.2f us\n", it, waves, ( t1 - t0 ) / 100.0 );
      stats( last_start, a, b, c, d ); printf( "    wave start after the first   min %.2f  median %.2f  max %.2f  mean %.2f\n", a, b, c, d );
      stats( nt, a, b, c, d );         printf( "    tiles per wave               min %.0f  median %.0f  max %.0f  mean %.2f\n", a, b, c, d );
      stats( pro, a, b, c, d );        printf( "    statistics + first tile words min %.2f  median %.2f  max %.2f  mean %.2f\n", a, b, c, d );
      stats( tile, a, b, c, d );       printf( "    one tile (loads + 35 sums)   min %.2f  median %.2f  max %.2f  mean %.2f\n", a, b, c, d );
      stats( epi, a, b, c, d );        printf( "    wave sums + barrier + store  min %.2f  median %.2f  max %.2f  mean %.2f\n", a, b, c, d );
      stats( tot, a, b, c, d );        printf( "    a wave, start to end         min %.2f  median %.2f  max %.2f  mean %.2f\n", a, b, c, d );
      stats( first_end, a, b, c, d );  printf( "    wave end after the first start  min %.2f  median %.2f  max %.2f\n", a, b, c );
    }
    const u64* u = U.data() + (size_t)it * ICP_NMOM * TD_UPD;
    u64 u0 = ~0ull; int last = -1, n_wg = 0;
    for( int k = 0; k < ICP_NMOM; ++k ) if( u[k * TD_UPD] ) { ++n_wg; u0 = std::min( u0, u[k * TD_UPD] ); if( u[k * TD_UPD + 6] || u[k * TD_UPD + 5] ) last = k; }
    if( !n_wg ) continue;
    std::vector<double> st, ph1, ph2, ph3, tk;
    for( int k = 0; k < ICP_NMOM; ++k )
    {
      const u64* r = u + k * TD_UPD; if( !r[0] ) continue;
      st.push_back( ( r[0] - u0 ) / 100.0 ); ph1.push_back( ( r[1] - r[0] ) / 100.0 ); ph2.push_back( ( r[2] - r[1] ) / 100.0 ); ph3.push_back( ( r[3] - r[2] ) / 100.0 ); tk.push_back( ( r[3] - u0 ) / 100.0 );
    }
    printf( "iteration %d  k_icp_update_wide: %d workgroups stamped%s\n", it, n_wg, waves ? "" : "  (no k_plain_moments stamps: not a plain iteration from the matches)" );
    stats( st, a, b, c, d );  printf( "    workgroup start after the first    min %.2f  median %.2f  max %.2f\n", a, b, c );
    stats( ph1, a, b, c, d ); printf( "    partials loaded and summed         min %.2f  median %.2f  max %.2f\n", a, b, c );
    stats( ph2, a, b, c, d ); printf( "    sum published (fence / store+wait) min %.2f  median %.2f  max %.2f\n", a, b, c );
    stats( ph3, a, b, c, d ); printf( "    ticket drawn                       min %.2f  median %.2f  max %.2f\n", a, b, c );
    stats( tk, a, b, c, d );  printf( "    ticket back after the first start  min %.2f  median %.2f  max %.2f\n", a, b, c );
    if( last >= 0 )
    {
      const u64* r = u + last * TD_UPD;
      auto at = [&]( int s ) { return r[s] ? ( r[s] - u0 ) / 100.0 : -1.0; };
      printf( "    last workgroup (%d), after the first start: start %.2f | partials %.2f | published %.2f | ticket %.2f | second fence %.2f | tail's loads %.2f | solve %.2f   (-1: no such phase)\n",
              last, at( 0 ), at( 1 ), at( 2 ), at( 3 ), at( 4 ), at( 5 ), at( 6 ) );
    }
  }
  fflush( stdout );
  return 0;
}
#endif
#else
#define TD_STAMP( p, s ) do { } while( 0 )
#define TD_STAMP_LOADED( p, s ) do { } while( 0 )
#endif
