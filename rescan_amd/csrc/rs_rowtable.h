// Index arithmetic of the cooperative sweep's row table (rs_search.h: sweep_stream).  Plain integer code that compiles with and
// without HIP: the kernels use exactly these functions, and tests/host/rowtable_check.cpp holds them to a linear walk on the host.
//
// A shell's (y,z) cell rows are numbered 0 .. n_rows - 1 and swept in SUPER-BATCHES of NW x 64 rows, NW the waves of the workgroup.
// Within a super-batch wave w, lane l describes row 64 w + l of the table (entry e = 64 w + l): up to two pieces
// [seg_a, seg_a + len_a) and [seg_b, seg_b + len_b) of the cell-sorted cloud.  pre[e] is the number of candidates of the entries
// before e in the SAME block of 64 (each wave's own prefix sum); blk[w] is the number of candidates of the blocks before w.
// Candidate j of the super-batch is found in two levels: its block from the <= 8 block offsets, then the 6-step binary search
// inside that block's 64 entries.  Chunk c — the 64 candidates from 64 c — belongs to wave c mod NW.
#pragma once
#include <stdint.h>

#if defined( __HIPCC__ )
#define RS_RT_FN __host__ __device__ __forceinline__
#define RS_RT_UNROLL _Pragma( "unroll" )
#else
#define RS_RT_FN inline
#define RS_RT_UNROLL
#endif

namespace rs {

#define RT_BLOCK 64      // entries per block: one wave's lanes

// rows one table holds, and the super-batches a shell of n_rows rows takes
RS_RT_FN int rt_table_rows( int nw ) { return nw * RT_BLOCK; }
RS_RT_FN int rt_super_batches( int n_rows, int nw ) { return ( n_rows + rt_table_rows( nw ) - 1 ) / rt_table_rows( nw ); }
// the shell row that entry `e` of super-batch `sb` describes (the caller tests it against n_rows)
RS_RT_FN int rt_row_of_entry( int sb, int nw, int e ) { return sb * rt_table_rows( nw ) + e; }

// blk[w] = candidates of the blocks before w, from the blocks' totals; returns the super-batch's total
template <int NW>
RS_RT_FN uint32_t rt_block_offsets( const uint32_t* block_total, uint32_t ( &blk )[NW] )
{
  uint32_t s = 0;
  RS_RT_UNROLL
  for( int w = 0; w < NW; ++w ) { blk[w] = s; s += block_total[w]; }
  return s;
}

// last block whose first candidate number is <= j (j < total): an empty block shares its offset with the next one and is passed over.
// *first = that block's offset.  (The offsets ascend, so the last block that passes the test wins: a chain of selects on values, so
// that nothing here indexes the offsets with a run-time number and they can stay in registers.)
template <int NW>
RS_RT_FN int rt_block_of( const uint32_t ( &blk )[NW], uint32_t j, uint32_t* first )
{
  int b = 0;
  uint32_t f = blk[0];
  RS_RT_UNROLL
  for( int w = 1; w < NW; ++w ) { const bool at = blk[w] <= j; b = at ? w : b; f = at ? blk[w] : f; }
  *first = f;
  return b;
}

// last entry of a block whose first candidate number is <= jj (jj < the block's total); `pre` points at the block's 64 offsets
RS_RT_FN int rt_entry_in_block( const uint32_t* pre, uint32_t jj )
{
  int e = 0;
  RS_RT_UNROLL
  for( int step = RT_BLOCK / 2; step > 0; step >>= 1 ) { if( pre[e + step] <= jj ) e += step; }
  return e;
}

// candidate j of the super-batch -> its position in the cell-sorted cloud; *entry (optional) = the table entry it came from
template <int NW>
RS_RT_FN uint32_t rt_source( const uint32_t ( &blk )[NW], const uint32_t* pre, const uint32_t* seg_a, const uint32_t* len_a, const uint32_t* seg_b,
                             uint32_t j, int* entry = nullptr )
{
  uint32_t first;
  const int b = rt_block_of<NW>( blk, j, &first );
  const uint32_t jj = j - first;
  const int e = b * RT_BLOCK + rt_entry_in_block( pre + b * RT_BLOCK, jj );
  const uint32_t off = jj - pre[e];
  const uint32_t la = len_a[e];
  if( entry ) *entry = e;
  return ( off < la ) ? ( seg_a[e] + off ) : ( seg_b[e] + ( off - la ) );
}

// the deal of chunks to waves: wave w takes the chunks w, w + NW, ... — candidates rt_first( w ), + rt_stride( nw ), ... while < total
// (the last chunk of a super-batch may be partial)
RS_RT_FN uint32_t rt_first( int w ) { return (uint32_t)w * RT_BLOCK; }
RS_RT_FN uint32_t rt_stride( int nw ) { return (uint32_t)nw * RT_BLOCK; }
RS_RT_FN int rt_chunk_owner( uint32_t chunk, int nw ) { return (int)( chunk % (uint32_t)nw ); }

} // namespace rs
