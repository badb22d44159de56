// Voxel overlap of two placed shapes and the non-maximum suppression of pose proposals built on it:
// isect_get_overlap_factor (lib/rs/intersect.h:309-368) and mgs_non_maxima_suppresion
// (apps/pose_proposal/pose_proposal.cpp:371-452) — rs_hip_overlap_factors, rs_hip_nms.
//
// Everything the reference decides is an integer (cell indices, cell counts) or one fp32 division of two of them, so the
// results are the reference's, bit for bit.  The fp32 arithmetic that leads to the integers keeps its operations and their
// order: the transform is xform3 (msh_mat4_vec3_mul), the cell of a point is floorf( ( p - origin ) / voxel ) with a
// correctly rounded DIVISION (intersect.h:222-225; not the multiply by 1 / voxel of cell_from_world_space, :100-103),
// and the library is built with -ffp-contract=off and hipcc's default correctly rounded fp32 divide.
//
// How a call runs (the choice the header leaves to the implementation):
//   1. k_isect_boxes   one wave per (cloud, pose): min / max of pose * p over the EXTENT cloud (the reference's level 3,
//                      :111-122).  The boxes are read back (24 bytes each).
//   2. the host        does what depends on boxes alone, in fp32 like the reference: the intersect test
//                      (msh_geometry.h:1010-1015; no intersection = overlap 0, no grid), the union box fattened by 0.3f
//                      and the grid's resolution (:59-75), the refusals that need no grid (a line of more than 4096
//                      cells, :132-133), and the route of every pair.
//   3. k_isect<route>  one workgroup per pair.  Each of the two grids is a bitmap of BOUNDARY cells and a bitmap of INSIDE
//                      cells (two 1-bit planes); an x line (y, z) is padded to whole 32-bit words, so that bit x of word
//                      ( y * z_res + z ) * wpr + x / 32 is cell y * x_res * z_res + z * x_res + x of the reference.
//                        rasterise   atomic-or of the boundary clouds' cells (:219-232); a point outside the grid (the
//                                    reference's assert, :227-229) flags the pair and nothing of the call is handed over
//                        fill x      per x line: the scanline's two parities (:126-174) are prefix-XORs over the words of
//                                    the transition masks ~B & ( B << 1 ) and ~B & ( B >> 1 ); one line per lane
//                        fill z      per (y, word): 32 z lines side by side, bit-sliced — a first walk along z takes the
//                                    backward transitions' total parity, a second one carries both parities along
//                        count       popcounts of B | I of both grids and of their AND, wave reductions, one LDS add per
//                                    wave (integers: the order does not matter)
//                      route LDS: the four planes sit in dynamic LDS (up to ISECT_LDS_BYTES; an object pair at 0.1 m voxels
//                      needs a few KB); route global: the same code on a slab of global memory, for grids beyond that.
//   4. the host        overlap = (float)both / (float)max-or-min count (:350-357), 1.0f when that count is 0.
//
// rs_hip_nms drives the reference's rounds on the host: the boxes of all n proposals are taken ONCE (they depend on the pose
// alone), every round picks its keep, settles on the host what the two cheap tests (distance of the transformed centroids,
// score < 0.01f) or disjoint boxes settle, and evaluates the remaining (keep, i) pairs in ONE launch with one small
// read-back (12 bytes per pair).  Skipping the overlap where a cheap test already discards changes no mark: the reference
// ORs the three tests (:422).
#include "rs_host.h"
#include "rs_search.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace rs;

#define ISECT_BLOCK 256
#define ISECT_LDS_BYTES 61440          // dynamic LDS of the LDS route (the static words of the kernel come on top; 64 KiB per workgroup)
#define ISECT_MAX_LINE 4096            // the reference's scanline arrays (:132-133)
#define ISECT_MAX_RES ( 1 << 20 )      // cells per axis (keeps every cell index exact in fp32 compares)
#define ISECT_SLAB_BYTES ( (size_t)256 << 20 )   // global route: planes of one launch

namespace {

struct IsectBoxJob { const float4* pos; int n; int pad; Xform pose; };

struct IsectPair
{
  const float4* a_pos; const float4* b_pos;
  int a_n, b_n;
  Xform pa, pb;
  float ox, oy, oz, voxel;
  int x_res, y_res, z_res, wpr;          // wpr: 32-bit words of one x line
  unsigned long long slab;               // global route: first word of the pair's planes
  int out, pad;                          // row of counts / status
};

__device__ __forceinline__ float wave_min( float v ) { for( int o = 32; o; o >>= 1 ) { const float w = __shfl_xor( v, o, 64 ); v = ( w < v ) ? w : v; } return v; }
__device__ __forceinline__ float wave_max( float v ) { for( int o = 32; o; o >>= 1 ) { const float w = __shfl_xor( v, o, 64 ); v = ( w > v ) ? w : v; } return v; }
__device__ __forceinline__ int   wave_sum( int v )   { for( int o = 32; o; o >>= 1 ) v += __shfl_xor( v, o, 64 ); return v; }

// isect_get_transformed_aabbox (:111-122) from mshgeo_bbox_init's +-1e9 (msh_geometry.h:945-969); one wave per job
__global__ __launch_bounds__( ISECT_BLOCK ) void k_isect_boxes( const IsectBoxJob* jobs, int n_jobs, float* boxes )
{
  const int job = blockIdx.x * ( ISECT_BLOCK / 64 ) + ( threadIdx.x >> 6 ), lane = threadIdx.x & 63;
  if( job >= n_jobs ) return;
  const IsectBoxJob& J = jobs[job];
  const Xform M = J.pose;
  float mn[3] = { 1e9f, 1e9f, 1e9f }, mx[3] = { -1e9f, -1e9f, -1e9f };
  for( int i = lane; i < J.n; i += 64 )
  {
    const float4 p = J.pos[i];
    float q[3];
    xform3( M, p.x, p.y, p.z, 1.0f, q[0], q[1], q[2] );
    for( int a = 0; a < 3; ++a ) { mn[a] = ( mn[a] < q[a] ) ? mn[a] : q[a]; mx[a] = ( mx[a] > q[a] ) ? mx[a] : q[a]; }
  }
  for( int a = 0; a < 3; ++a ) { mn[a] = wave_min( mn[a] ); mx[a] = wave_max( mx[a] ); }
  if( lane == 0 ) for( int a = 0; a < 3; ++a ) { boxes[6 * job + a] = mn[a]; boxes[6 * job + 3 + a] = mx[a]; }
}

__device__ __forceinline__ uint32_t prefix_xor32( uint32_t v ) { v ^= v << 1; v ^= v << 2; v ^= v << 4; v ^= v << 8; v ^= v << 16; return v; }   // bit i = parity of bits 0..i
__device__ __forceinline__ uint32_t suffix_xor32( uint32_t v ) { v ^= v >> 1; v ^= v >> 2; v ^= v >> 4; v ^= v >> 8; v ^= v >> 16; return v; }   // bit i = parity of bits i..31

// boundary cells of one placed cloud (:219-232)
__device__ __forceinline__ void isect_rasterise( const float4* pos, int n, const Xform& M, const IsectPair& P, uint32_t* B, int* bad )
{
  for( int i = threadIdx.x; i < n; i += ISECT_BLOCK )
  {
    const float4 p = pos[i];
    float qx, qy, qz;
    xform3( M, p.x, p.y, p.z, 1.0f, qx, qy, qz );
    const float fx = floorf( ( qx - P.ox ) / P.voxel ), fy = floorf( ( qy - P.oy ) / P.voxel ), fz = floorf( ( qz - P.oz ) / P.voxel );
    // (in fp32, so that a NaN fails too; the resolutions are below 2^24)
    if( !( fx >= 0.0f && fx < (float)P.x_res && fy >= 0.0f && fy < (float)P.y_res && fz >= 0.0f && fz < (float)P.z_res ) ) { *bad = 1; continue; }
    const int x = (int)fx, y = (int)fy, z = (int)fz;
    atomicOr( &B[(size_t)( y * P.z_res + z ) * P.wpr + ( x >> 5 )], 1u << ( x & 31 ) );
  }
}

// One workgroup per pair of `list`.  GLOBAL: the planes live in `slab`, else in dynamic LDS.
template <bool GLOBAL>
__global__ __launch_bounds__( ISECT_BLOCK ) void k_isect( const IsectPair* pairs, const int* list, uint32_t* slab, int fill, int* counts, int* status )
{
  extern __shared__ uint32_t s_planes[];
  __shared__ int s_bad, s_cnt[3];
  const IsectPair P = pairs[list[blockIdx.x]];                   // (uniform: scalar registers)
  const int tid = threadIdx.x;
  const int lines = P.y_res * P.z_res, wpr = P.wpr;
  const size_t nw = (size_t)lines * wpr;                          // words of one plane
  uint32_t* base = GLOBAL ? slab + P.slab : s_planes;            // planes: B of a, B of b, then (fill only) I of a, I of b
  if( tid == 0 ) { s_bad = 0; s_cnt[0] = s_cnt[1] = s_cnt[2] = 0; }
  for( size_t i = tid; i < ( fill ? 4 : 2 ) * nw; i += ISECT_BLOCK ) base[i] = 0u;
  __syncthreads();
  isect_rasterise( P.a_pos, P.a_n, P.pa, P, base, &s_bad );
  isect_rasterise( P.b_pos, P.b_n, P.pb, P, base + nw, &s_bad );
  __syncthreads();
  if( s_bad ) { if( tid == 0 ) status[P.out] = 1; return; }
  if( fill )
  {
    // x lines (isect__compute_occupancy_within_slice, dir 0): a cell is INSIDE when it is not BOUNDARY and an odd number of
    // "FREE directly after BOUNDARY" transitions lies at or before it, counted from either end of the line
    const uint32_t last_mask = ( P.x_res & 31 ) ? ( ( 1u << ( P.x_res & 31 ) ) - 1u ) : ~0u;
    for( int l = tid; l < 2 * lines; l += ISECT_BLOCK )
    {
      const int g = l >= lines;
      const uint32_t* b = base + (size_t)g * nw + (size_t)( l - g * lines ) * wpr;
      uint32_t* in = base + (size_t)( 2 + g ) * nw + (size_t)( l - g * lines ) * wpr;
      uint32_t carry = 0u, next = 0u;                            // backward: parity of the transitions in the words above
      for( int w = wpr - 1; w >= 0; --w )
      {
        const uint32_t cur = b[w];
        const uint32_t s = suffix_xor32( ~cur & ( ( cur >> 1 ) | ( next << 31 ) ) ) ^ ( 0u - carry );
        in[w] = s;
        carry = s & 1u; next = cur;
      }
      uint32_t prev = 0u; carry = 0u;                            // forward, and the line's answer
      for( int w = 0; w < wpr; ++w )
      {
        const uint32_t cur = b[w];
        const uint32_t f = prefix_xor32( ~cur & ( ( cur << 1 ) | ( prev >> 31 ) ) ) ^ ( 0u - carry );
        in[w] = ~cur & f & in[w] & ( w == wpr - 1 ? last_mask : ~0u );
        carry = f >> 31; prev = cur;
      }
    }
    __syncthreads();
    // z lines (dir 1), 32 of them per item, and the combination of the two directions (:249-260): INSIDE only if both say so
    const int cols = P.y_res * wpr;
    for( int c = tid; c < 2 * cols; c += ISECT_BLOCK )
    {
      const int g = c >= cols, cc = c - g * cols, y = cc / wpr, w = cc - y * wpr;
      const uint32_t* b = base + (size_t)g * nw + (size_t)y * P.z_res * wpr + w;
      uint32_t* in = base + (size_t)( 2 + g ) * nw + (size_t)y * P.z_res * wpr + w;
      uint32_t total = 0u, prev = b[0];                          // parity of all backward transitions ~B[z] & B[z+1]
      for( int z = 1; z < P.z_res; ++z ) { const uint32_t cur = b[(size_t)z * wpr]; total ^= ~prev & cur; prev = cur; }
      uint32_t fwd = 0u, before = 0u, cur = b[0];                // before: the backward transitions below z
      prev = 0u;
      for( int z = 0; z < P.z_res; ++z )
      {
        const uint32_t nxt = ( z + 1 < P.z_res ) ? b[(size_t)( z + 1 ) * wpr] : 0u;
        fwd ^= ~cur & prev;
        in[(size_t)z * wpr] &= fwd & ( total ^ before );
        before ^= ~cur & nxt;
        prev = cur; cur = nxt;
      }
    }
    __syncthreads();
  }
  int ca = 0, cb = 0, cab = 0;
  for( size_t i = tid; i < nw; i += ISECT_BLOCK )
  {
    const uint32_t a = fill ? ( base[i] | base[2 * nw + i] ) : base[i], b = fill ? ( base[nw + i] | base[3 * nw + i] ) : base[nw + i];
    ca += __popc( a ); cb += __popc( b ); cab += __popc( a & b );
  }
  ca = wave_sum( ca ); cb = wave_sum( cb ); cab = wave_sum( cab );
  if( ( tid & 63 ) == 0 ) { atomicAdd( &s_cnt[0], ca ); atomicAdd( &s_cnt[1], cb ); atomicAdd( &s_cnt[2], cab ); }
  __syncthreads();
  if( tid < 3 ) counts[3 * P.out + tid] = s_cnt[tid];
}

// ------------------------------------------------------------------------------------------

struct IsectWorkspace { Buf jobs, boxes, pairs, list, out, slab, h_in{ nullptr, 0, true }, h_out{ nullptr, 0, true }; };
thread_local IsectWorkspace g_isect_ws;
int g_isect_lds_bytes = ISECT_LDS_BYTES;
int64_t g_isect_evaluated = 0, g_isect_skipped = 0;

struct HostShape { const GridView* boundary; const GridView* extent; };

int host_shape( const rs_hip_isect_shape_t* s, HostShape& h )
{
  if( !s || !s->boundary || !s->extent ) return RS_HIP_E_ARG;
  h.boundary = api_cloud_view( s->boundary ); h.extent = api_cloud_view( s->extent );
  return RS_HIP_OK;
}

// boxes[6 j ..] = {min, max} of job j's transformed cloud
int run_boxes( const std::vector<IsectBoxJob>& jobs, float* boxes, hipStream_t st )
{
  IsectWorkspace& W = g_isect_ws;
  const size_t n = jobs.size();
  if( !n ) return RS_HIP_OK;
  RS_TRY( W.jobs.ensure( n * sizeof(IsectBoxJob) ), "isect: buffers" );
  RS_TRY( W.boxes.ensure( n * 24 ), "isect: buffers" );
  RS_TRY( W.h_in.ensure( n * sizeof(IsectBoxJob) ), "isect: buffers" );
  RS_TRY( W.h_out.ensure( n * 24 ), "isect: buffers" );
  std::memcpy( W.h_in.p, jobs.data(), n * sizeof(IsectBoxJob) );
  RS_TRY( hipMemcpyAsync( W.jobs.p, W.h_in.p, n * sizeof(IsectBoxJob), hipMemcpyHostToDevice, st ), "isect: upload" );
  {
    ProfSpan span( "isect" );
    hipLaunchKernelGGL( k_isect_boxes, dim3( blocks_for( (long long)n, ISECT_BLOCK / 64 ) ), dim3( ISECT_BLOCK ), 0, st,
                        (const IsectBoxJob*)W.jobs.p, (int)n, (float*)W.boxes.p );
  }
  RS_TRY( hipGetLastError(), "isect: boxes launch" );
  RS_TRY( hipMemcpyAsync( W.h_out.p, W.boxes.p, n * 24, hipMemcpyDeviceToHost, st ), "isect: download" );
  RS_TRY( hipStreamSynchronize( st ), "isect: boxes" );
  std::memcpy( boxes, W.h_out.p, n * 24 );
  return RS_HIP_OK;
}

// One pair as the caller names it; `name` is its index in the caller's terms (error texts).
struct PairIn { const GridView* a; const GridView* b; const float* pose_a; const float* pose_b; const float* box_a; const float* box_b; int name; };

inline bool boxes_intersect( const float* a, const float* b )          // msh_geometry.h:1010-1015
{
  return ( a[3] >= b[0] && b[3] >= a[0] ) && ( a[4] >= b[1] && b[4] >= a[1] ) && ( a[5] >= b[2] && b[5] >= a[2] );
}

// counts[3 k ..] = {count_a, count_b, both} of pair k; has_grid[k] = 0 where the boxes do not intersect (counts 0).  Refusals
// return their code with nothing written.
int run_pairs( const std::vector<PairIn>& in, float voxel, int fill, int32_t* counts, uint8_t* has_grid, hipStream_t st )
{
  IsectWorkspace& W = g_isect_ws;
  const size_t n = in.size();
  std::vector<IsectPair> pairs; pairs.reserve( n );
  std::vector<int> lds_list, glb_list;
  std::vector<size_t> plane_words;
  size_t lds_max = 0;
  const int planes = fill ? 4 : 2;
  for( size_t k = 0; k < n; ++k )
  {
    const PairIn& q = in[k];
    has_grid[k] = 0; counts[3 * k] = counts[3 * k + 1] = counts[3 * k + 2] = 0;
    if( !boxes_intersect( q.box_a, q.box_b ) ) continue;
    // the union of the four corners from +-1e9 (:324-328), fattened (:61-65); the resolutions (:67-69), all in fp32
    float mn[3], mx[3]; int res[3];
    for( int a = 0; a < 3; ++a )
    {
      float lo = 1e9f, hi = -1e9f;
      for( const float v : { q.box_a[a], q.box_a[3 + a], q.box_b[a], q.box_b[3 + a] } ) { lo = ( lo < v ) ? lo : v; hi = ( hi > v ) ? hi : v; }
      mn[a] = lo - 0.3f; mx[a] = hi + 0.3f;
      const float cells = ceilf( ( mx[a] - mn[a] ) / voxel );
      if( !( cells >= 0.0f && cells < (float)ISECT_MAX_RES ) )
      {
        char msg[160]; snprintf( msg, sizeof(msg), "isect: pair %d: more than %d cells along an axis (or no finite box)", q.name, ISECT_MAX_RES );
        return fail( RS_HIP_E_CAPACITY, msg );
      }
      res[a] = (int)cells + 1;
    }
    if( fill && ( res[0] > ISECT_MAX_LINE || res[2] > ISECT_MAX_LINE ) )
    {
      char msg[160]; snprintf( msg, sizeof(msg), "isect: pair %d: a line of %d cells exceeds the reference's scanline arrays (%d)", q.name, std::max( res[0], res[2] ), ISECT_MAX_LINE );
      return fail( RS_HIP_E_CAPACITY, msg );
    }
    const int wpr = ( res[0] + 31 ) / 32;
    const double cells_all = (double)res[0] * res[1] * res[2], words = (double)wpr * res[1] * res[2] * planes;
    if( cells_all > 2147483647.0 || words * 4.0 > (double)ISECT_SLAB_BYTES )
    {
      char msg[160]; snprintf( msg, sizeof(msg), "isect: pair %d: a grid of %d x %d x %d cells exceeds the scratch slab", q.name, res[0], res[1], res[2] );
      return fail( RS_HIP_E_CAPACITY, msg );
    }
    IsectPair P{};
    P.a_pos = q.a->pos; P.a_n = q.a->n; P.b_pos = q.b->pos; P.b_n = q.b->n;
    std::memcpy( P.pa.m, q.pose_a, 64 ); std::memcpy( P.pb.m, q.pose_b, 64 );
    P.ox = mn[0]; P.oy = mn[1]; P.oz = mn[2]; P.voxel = voxel;
    P.x_res = res[0]; P.y_res = res[1]; P.z_res = res[2]; P.wpr = wpr;
    P.out = (int)k;
    const size_t w = (size_t)words;
    if( w * 4 <= (size_t)g_isect_lds_bytes ) { lds_list.push_back( (int)pairs.size() ); lds_max = std::max( lds_max, w * 4 ); }
    else glb_list.push_back( (int)pairs.size() );
    plane_words.push_back( w );
    pairs.push_back( P );
    has_grid[k] = 1;
  }
  if( pairs.empty() ) return RS_HIP_OK;
  // global route: launches of at most ISECT_SLAB_BYTES of planes
  std::vector<std::pair<size_t, size_t>> glb_chunks;            // [first, end) in glb_list
  size_t slab_bytes = 0;
  for( size_t i = 0; i < glb_list.size(); )
  {
    size_t used = 0, j = i;
    while( j < glb_list.size() && ( used + plane_words[glb_list[j]] ) * 4 <= ISECT_SLAB_BYTES ) { pairs[glb_list[j]].slab = used; used += plane_words[glb_list[j]]; ++j; }
    glb_chunks.emplace_back( i, j ); slab_bytes = std::max( slab_bytes, used * 4 ); i = j;
  }
  const size_t np = pairs.size(), nl = lds_list.size() + glb_list.size();
  const size_t in_bytes = np * sizeof(IsectPair) + nl * 4, out_bytes = n * 16;      // counts x 3 + status
  RS_TRY( W.pairs.ensure( np * sizeof(IsectPair) ), "isect: buffers" );
  RS_TRY( W.list.ensure( nl * 4 ), "isect: buffers" );
  RS_TRY( W.out.ensure( out_bytes ), "isect: buffers" );
  RS_TRY( W.h_in.ensure( in_bytes ), "isect: buffers" );
  RS_TRY( W.h_out.ensure( out_bytes ), "isect: buffers" );
  if( slab_bytes ) RS_TRY( W.slab.ensure( slab_bytes ), "isect: scratch slab" );
  char* h = (char*)W.h_in.p;
  std::memcpy( h, pairs.data(), np * sizeof(IsectPair) );
  int* hl = (int*)( h + np * sizeof(IsectPair) );
  std::copy( lds_list.begin(), lds_list.end(), hl ); std::copy( glb_list.begin(), glb_list.end(), hl + lds_list.size() );
  RS_TRY( hipMemcpyAsync( W.pairs.p, h, np * sizeof(IsectPair), hipMemcpyHostToDevice, st ), "isect: upload" );
  RS_TRY( hipMemcpyAsync( W.list.p, hl, nl * 4, hipMemcpyHostToDevice, st ), "isect: upload" );
  RS_TRY( hipMemsetAsync( W.out.p, 0, out_bytes, st ), "isect: clear" );
  int* d_counts = (int*)W.out.p; int* d_status = d_counts + 3 * n;
  {
    ProfSpan span( "isect" );
    if( !lds_list.empty() )
    {
      const size_t dyn = ( std::max<size_t>( lds_max, 1024 ) + 1023 ) / 1024 * 1024;     // whole KB: a few launch shapes only
      hipLaunchKernelGGL( k_isect<false>, dim3( (unsigned)lds_list.size() ), dim3( ISECT_BLOCK ), dyn, st,
                          (const IsectPair*)W.pairs.p, (const int*)W.list.p, (uint32_t*)nullptr, fill, d_counts, d_status );
    }
    for( const auto& c : glb_chunks )
      hipLaunchKernelGGL( k_isect<true>, dim3( (unsigned)( c.second - c.first ) ), dim3( ISECT_BLOCK ), 0, st,
                          (const IsectPair*)W.pairs.p, (const int*)W.list.p + lds_list.size() + c.first, (uint32_t*)W.slab.p, fill, d_counts, d_status );
  }
  RS_TRY( hipGetLastError(), "isect: launch" );
  RS_TRY( hipMemcpyAsync( W.h_out.p, W.out.p, out_bytes, hipMemcpyDeviceToHost, st ), "isect: download" );
  RS_TRY( hipStreamSynchronize( st ), "isect" );
  const int* hc = (const int*)W.h_out.p; const int* hs = hc + 3 * n;
  for( size_t k = 0; k < n; ++k )
    if( hs[k] )
    {
      char msg[200]; snprintf( msg, sizeof(msg), "isect: pair %d: a boundary point lies outside the grid of the extent clouds (the reference asserts, intersect.h:227-229)", in[k].name );
      return fail( RS_HIP_E_ARG, msg );
    }
  std::memcpy( counts, hc, n * 12 );
  g_isect_evaluated += (int64_t)np;
  return RS_HIP_OK;
}

inline float overlap_of( const int32_t* c, bool has_grid, int by_smaller )       // :350-357
{
  if( !has_grid ) return 0.0f;
  const int32_t denom = by_smaller ? std::min( c[0], c[1] ) : std::max( c[0], c[1] );
  return denom > 0 ? (float)c[2] / (float)denom : 1.0f;
}

inline void host_xform3( const float* m, const float* v, float* o )             // msh_mat4_vec3_mul, a point
{
  o[0] = m[0] * v[0] + m[4] * v[1] + m[ 8] * v[2] + 1.0f * m[12];
  o[1] = m[1] * v[0] + m[5] * v[1] + m[ 9] * v[2] + 1.0f * m[13];
  o[2] = m[2] * v[0] + m[6] * v[1] + m[10] * v[2] + 1.0f * m[14];
}

} // namespace

extern "C" {

int rs_hip_overlap_factors( const rs_hip_isect_shape_t* shapes, int32_t n_shapes,
                            const int32_t* shape_a, const float* poses_a, const int32_t* shape_b, const float* poses_b,
                            int32_t n_pairs, float voxel_size, int voxelize_inside, int normalize_by_smaller,
                            float* overlap, int32_t* counts )
{
  if( !shapes || n_shapes <= 0 || n_pairs < 0 || !( voxel_size > 0.0f ) || ( n_pairs > 0 && ( !shape_a || !shape_b || !poses_a || !poses_b || !overlap ) ) )
    return fail( RS_HIP_E_ARG, "overlap_factors: bad arguments" );
  for( int32_t k = 0; k < n_pairs; ++k )
    if( shape_a[k] < 0 || shape_a[k] >= n_shapes || shape_b[k] < 0 || shape_b[k] >= n_shapes )
    {
      char msg[128]; snprintf( msg, sizeof(msg), "overlap_factors: pair %d names a shape outside [0, %d)", k, n_shapes );
      return fail( RS_HIP_E_ARG, msg );
    }
  for( int32_t s = 0; s < n_shapes; ++s ) if( !shapes[s].boundary || !shapes[s].extent ) return fail( RS_HIP_E_ARG, "overlap_factors: a shape without a boundary or an extent cloud" );
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  if( n_pairs == 0 ) return RS_HIP_OK;
  std::vector<HostShape> hs( n_shapes );
  for( int32_t s = 0; s < n_shapes; ++s ) host_shape( &shapes[s], hs[s] );
  std::vector<IsectBoxJob> jobs( 2 * (size_t)n_pairs );
  for( int32_t k = 0; k < n_pairs; ++k )
    for( int side = 0; side < 2; ++side )
    {
      IsectBoxJob& J = jobs[2 * (size_t)k + side];
      const GridView* e = hs[side ? shape_b[k] : shape_a[k]].extent;
      J.pos = e->pos; J.n = e->n; J.pad = 0;
      std::memcpy( J.pose.m, ( side ? poses_b : poses_a ) + 16 * (size_t)k, 64 );
    }
  std::vector<float> boxes( 12 * (size_t)n_pairs );
  rc = run_boxes( jobs, boxes.data(), st ); if( rc ) return rc;
  std::vector<PairIn> in( n_pairs );
  for( int32_t k = 0; k < n_pairs; ++k )
    in[k] = PairIn{ hs[shape_a[k]].boundary, hs[shape_b[k]].boundary, poses_a + 16 * (size_t)k, poses_b + 16 * (size_t)k,
                    &boxes[12 * (size_t)k], &boxes[12 * (size_t)k + 6], k };
  std::vector<int32_t> cnt( 3 * (size_t)n_pairs ); std::vector<uint8_t> grid( n_pairs );
  rc = run_pairs( in, voxel_size, voxelize_inside != 0, cnt.data(), grid.data(), st ); if( rc ) return rc;
  for( int32_t k = 0; k < n_pairs; ++k ) overlap[k] = overlap_of( &cnt[3 * (size_t)k], grid[k] != 0, normalize_by_smaller );
  if( counts ) std::memcpy( counts, cnt.data(), cnt.size() * 4 );
  return RS_HIP_OK;
}

int rs_hip_nms( const rs_hip_isect_shape_t* shape, const float centroid[3], const float* poses, const float* scores, int32_t n,
                float dist_threshold, int32_t* marks, int32_t* keep_idx, int32_t* n_keep, int32_t* n_rounds )
{
  if( !shape || !shape->boundary || !shape->extent || !centroid || n < 0 || !n_keep || ( n > 0 && ( !poses || !scores || !marks || !keep_idx ) ) )
    return fail( RS_HIP_E_ARG, "nms: bad arguments" );
  for( int32_t i = 0; i < n; ++i )
    if( !( scores[i] > -1e9f ) )             // NaN too: the reference's arg-max would find nothing and index with -1 (:396-407)
    {
      char msg[128]; snprintf( msg, sizeof(msg), "nms: score %d is NaN or <= -1e9", i );
      return fail( RS_HIP_E_ARG, msg );
    }
  hipStream_t st = nullptr;
  int rc = api_ready( &st ); if( rc ) return rc;
  if( n == 0 ) { *n_keep = 0; if( n_rounds ) *n_rounds = 0; return RS_HIP_OK; }       // (:385)
  HostShape hs; host_shape( shape, hs );
  std::vector<IsectBoxJob> jobs( n );
  for( int32_t i = 0; i < n; ++i ) { jobs[i].pos = hs.extent->pos; jobs[i].n = hs.extent->n; jobs[i].pad = 0; std::memcpy( jobs[i].pose.m, poses + 16 * (size_t)i, 64 ); }
  std::vector<float> boxes( 6 * (size_t)n ), cen( 3 * (size_t)n );
  rc = run_boxes( jobs, boxes.data(), st ); if( rc ) return rc;
  for( int32_t i = 0; i < n; ++i ) host_xform3( poses + 16 * (size_t)i, centroid, &cen[3 * (size_t)i] );
  std::vector<int32_t> mk( n, 0 ), cnt; std::vector<uint8_t> grid; std::vector<PairIn> in; std::vector<int32_t> who;
  int32_t marked = 0, rounds = 0;
  while( marked != n )
  {
    int32_t best = -1; float best_score = -1e9f;                                   // :396-405
    for( int32_t i = 0; i < n; ++i ) if( mk[i] == 0 && scores[i] > best_score ) { best_score = scores[i]; best = i; }
    mk[best] = 1; ++marked; ++rounds;
    in.clear(); who.clear();
    for( int32_t i = 0; i < n; ++i )
    {
      if( mk[i] != 0 ) continue;
      const float d[3] = { cen[3 * (size_t)best] - cen[3 * (size_t)i], cen[3 * (size_t)best + 1] - cen[3 * (size_t)i + 1], cen[3 * (size_t)best + 2] - cen[3 * (size_t)i + 2] };
      const float dist = sqrtf( d[0] * d[0] + d[1] * d[1] + d[2] * d[2] );       // msh_vec3_norm: (float)sqrt of the fp32 sum
      if( dist < dist_threshold || scores[i] < 0.01f ) { mk[i] = 2; ++marked; ++g_isect_skipped; continue; }
      if( !boxes_intersect( &boxes[6 * (size_t)best], &boxes[6 * (size_t)i] ) ) { ++g_isect_skipped; continue; }      // overlap 0
      in.push_back( PairIn{ hs.boundary, hs.boundary, poses + 16 * (size_t)best, poses + 16 * (size_t)i, &boxes[6 * (size_t)best], &boxes[6 * (size_t)i], i } );
      who.push_back( i );
    }
    if( in.empty() ) continue;
    cnt.resize( 3 * in.size() ); grid.resize( in.size() );
    rc = run_pairs( in, 0.1f, 1, cnt.data(), grid.data(), st ); if( rc ) return rc;                  // :419-421
    for( size_t k = 0; k < in.size(); ++k )
      if( overlap_of( &cnt[3 * k], grid[k] != 0, 0 ) > 0.5f ) { mk[who[k]] = 2; ++marked; }
  }
  int32_t nk = 0;
  for( int32_t i = 0; i < n; ++i ) { marks[i] = mk[i]; if( mk[i] == 1 ) keep_idx[nk++] = i; }     // :441-447: in index order
  *n_keep = nk;
  if( n_rounds ) *n_rounds = rounds;
  return RS_HIP_OK;
}

int32_t rs_hip_isect_lds_budget( int32_t bytes )
{
  const int32_t before = g_isect_lds_bytes;
  if( bytes >= 0 ) g_isect_lds_bytes = std::min( bytes, (int32_t)ISECT_LDS_BYTES );
  return before;
}

void rs_hip_isect_pairs( int64_t* evaluated, int64_t* skipped, int32_t reset )
{
  if( evaluated ) *evaluated = g_isect_evaluated;
  if( skipped ) *skipped = g_isect_skipped;
  if( reset ) g_isect_evaluated = g_isect_skipped = 0;
}

} // extern "C"
