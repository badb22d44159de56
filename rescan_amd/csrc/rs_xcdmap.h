// Tile map of phase A's natural part (rs_icp_search.hip: k_icp_corr): which natural block a workgroup takes, how large the natural
// part of the grid is, and which XCD class a tile belongs to.  Plain integer code that compiles with and without HIP: the kernel, its
// launch and the census of icp_debug_after use exactly these functions, and tests/host/xcdmap_check.cpp holds them to their contract.
//
// Workgroups are dealt round-robin over the 8 XCDs, so workgroup b of the natural part runs with XCD class c = b & 7, as the p-th
// (p = b >> 3) of its class.  Everything here is in NATURAL BLOCKS: PA_WAVES consecutive tiles of the source's (Hilbert) order, nb of
// them in a problem.  The order is cut into chunks of C = 2^k blocks and chunk j belongs to class j & 7: the p-th workgroup of class c
// takes block ( ( p >> k ) * 8 + c ) * C + ( p & ( C - 1 ) ).  Within a class the blocks ascend with b, so all eight XCDs move along
// the curve together and a chunk's target lines are fetched by one XCD (and the seams).  The natural part is padded to a whole
// number of rounds of eight chunks, which makes the map a permutation of [0, grid) for every grid of that form: a problem smaller
// than the one the grid was sized for finds each of its blocks once, and its other workgroups land beyond nb.
// k < 0: the contiguous eighths of rounds 1 to 19 — class c walks blocks [c * per, ( c + 1 ) * per), per = ceil( nb / 8 ).
#pragma once
#include <limits.h>

#if defined( __HIPCC__ )
#define RS_XM_FN __host__ __device__ __forceinline__
#else
#define RS_XM_FN inline
#endif

// RS_XCD_MAP=0: no map at all, workgroup b takes block b (measurements, tools/variant.sh)
#ifndef RS_XCD_MAP
#define RS_XCD_MAP 1
#endif
// waves (tiles) per workgroup of phase A: the natural block (why it is 1: rs_icp_search.hip)
#ifndef RS_PA_WAVES
#define RS_PA_WAVES 1
#endif
// log2 of the chunk, in natural blocks; negative: contiguous eighths.  Chosen by measurement (profiles/r20/ab_xcd_chunks.txt): chunks
// for the cold launch (k_icp_corr<false>), contiguous eighths for the warm launches (k_icp_corr<true>).
#ifndef RS_XCD_CHUNK_LOG2
#define RS_XCD_CHUNK_LOG2 6
#endif
#ifndef RS_XCD_CHUNK_WARM_LOG2
#define RS_XCD_CHUNK_WARM_LOG2 -1
#endif

namespace rs {

constexpr int XCD_CLASSES = 8;

RS_XM_FN int xm_blocks( int n_tiles, int pa_waves ) { return ( n_tiles + pa_waves - 1 ) / pa_waves; }
RS_XM_FN int xm_per_class( int nb ) { return ( nb + XCD_CLASSES - 1 ) / XCD_CLASSES; }      // (k < 0)

// workgroups of the natural part for a problem of nb blocks (the launch takes the largest problem's): a multiple of 8
RS_XM_FN int xm_grid( int nb, int k )
{
  if( k < 0 ) return XCD_CLASSES * xm_per_class( nb );
  const int chunks = ( nb + ( 1 << k ) - 1 ) >> k;
  return ( ( ( chunks + XCD_CLASSES - 1 ) / XCD_CLASSES ) * XCD_CLASSES ) << k;
}

// the natural block of workgroup b, for a workgroup that is not xm_beyond
RS_XM_FN int xm_block( int b, int nb, int k )
{
  const int c = b & ( XCD_CLASSES - 1 ), p = b >> 3;
  if( k < 0 ) return c * xm_per_class( nb ) + p;
  return ( ( ( p >> k ) * XCD_CLASSES + c ) << k ) + ( p & ( ( 1 << k ) - 1 ) );
}

// whether workgroup b has no block of this problem (the grid is a larger problem's, or the last round of chunks is not full): it exits.
// (k < 0: past the class's own eighth, where xm_block would run into the next class's.  The last eighth may still end beyond nb:
// the caller tests its tile against the problem's tiles in any case, the last block may be a partial one.)
RS_XM_FN bool xm_beyond( int b, int nb, int k )
{
  if( k < 0 ) return ( b >> 3 ) >= xm_per_class( nb );
  return xm_block( b, nb, k ) >= nb;
}

// the class whose workgroups take natural block `block` (block < nb)
RS_XM_FN int xm_class( int block, int nb, int k )
{
  if( k < 0 ) { const int c = block / xm_per_class( nb ); return c < XCD_CLASSES - 1 ? c : XCD_CLASSES - 1; }
  return ( block >> k ) & ( XCD_CLASSES - 1 );
}

} // namespace rs
