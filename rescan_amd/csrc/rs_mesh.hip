// Uniform resampling of a mesh to the level-0 cloud: rs_pointcloud_uniform_resample (lib/rs/rs_pointcloud.h:1132-1227),
// bit for bit — rs_hip_resample_plan, rs_hip_uniform_resample, rs_hip_cloud_create_resampled.
//
// The reference's loop looks sequential because it threads two PCG32 generators through it (msh_std.h:1413-1470): one
// picks the face through an alias table (msh_std.h:1935-1941), one draws the barycentric coordinates (:1114-1130).  Each
// sample takes exactly two draws from each, and the LCG under PCG32 can be jumped ahead, so sample i is a pure function of
// i, the mesh and a small table (rs_mesh.h: JumpTable).
//
// How a call runs:
//   1. the host (rs_mesh.h)  everything sequential: face areas and their double sum (:1143-1154), the sample count
//                            (:1157-1158), the alias table (msh_std.h:1843-1849,1863-1925: a data-dependent stack loop,
//                            one O(n_faces) pass), the seeding, the jump table, and every refusal — before any launch.
//   2. upload                vertices packed into one 48-byte record each (pos, nor, col, radius, class, instance): a
//                            sampled face costs three record reads of three 16-byte loads, not eighteen scattered words;
//                            faces as they are (12 bytes); the alias table as 16-byte (prob, alias) entries.
//   3. k_mesh_sample         one lane per sample of the window [first, first + count).  Lane i derives both generator
//                            states 2 i steps after the seeding from the table, over the set bits of 2 i, in 64-bit
//                            arithmetic; then the alias lookup with the fp64 compare, three record reads, the
//                            interpolation in the reference's operation order, and coalesced stores.  Nothing of a
//                            lane's result depends on the launch geometry or on the window.
// The fp32 arithmetic matches the reference's because the library is built with -ffp-contract=off and hipcc's default
// correctly rounded fp32 divide and square root.
//
// The step before it, for a mesh that comes without normals: rs_pointcloud__compute_normals (lib/rs/rs_pointcloud.h:556-596) and the
// loader's pass over its result (:743-751), bit for bit — rs_hip_vertex_normals, rs_hip_cloud_create_from_mesh.  A vertex normal is a
// running mean over the faces that name the vertex, taken in face order: one vertex's chain is sequential, the chains of different
// vertices are independent.
//   k_face_cross     one lane per face: the unnormalised cross product, once, as a 16-byte record; and the face's three corners as
//                    (vertex, 3 face + corner) pairs.
//   stable sort      of the pairs by vertex over the bits n_vertices - 1 needs (hipCUB's radix sort, rs_build.hip): a vertex's corners
//                    become one span, in ascending corner id, i.e. in the reference's order.  No atomic decides an order.
//   k_span_start     where each vertex's span starts.
//   k_vertex_chain   one lane per vertex walks its span: t once per face from the count before it, the lerp once per corner, then
//                    the finish (:586-592) and, where asked, the loader's pass.  It writes where k_mesh_sample reads.
#include "rs_host.h"
#include "rs_mesh.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

namespace rs {

constexpr int MESH_BLOCK = 256;

struct MeshVertex            // 48 bytes: three 16-byte loads
{
  float px, py, pz, nx;
  float ny, nz, cr, cg;
  float cb, radius; int32_t cls, inst;
};
static_assert( sizeof(MeshVertex) == 48, "MeshVertex is read as three float4" );
struct MeshAlias { double prob; int32_t alias; int32_t pad; };      // one 16-byte load
static_assert( sizeof(MeshAlias) == 16, "MeshAlias is read as one 16-byte word" );

struct MeshSampleArgs
{
  const MeshVertex* vert; const int32_t* faces; const MeshAlias* table;
  int32_t n_faces; int32_t n_bits;           // n_bits: bits of 2 * (first + count - 1) the jump has to look at
  long long first, count;
  float* out_pos; float* out_nor; float* out_col; float* out_radii; int32_t* out_class; int32_t* out_instance; int32_t* out_face;   // null: skipped
  mesh::JumpTable jump;
};

__device__ __forceinline__ uint32_t pcg_draw( uint64_t& s, uint64_t inc )     // msh_rand_next, msh_std.h:1447-1455
{
  const uint64_t old = s;
  s = old * mesh::PCG_MUL + inc;
  const uint32_t xorshifted = (uint32_t)( ( ( old >> 18 ) ^ old ) >> 27 );
  const uint32_t rot = (uint32_t)( old >> 59 );
  return ( xorshifted >> rot ) | ( xorshifted << ( ( 0u - rot ) & 31u ) );
}
__device__ __forceinline__ float unit_float( uint32_t u )                     // msh_rand__float_normalized_from_u32, msh_std.h:1412-1421
{
  return __uint_as_float( 0x3F800000u | ( u >> 9 ) ) - 1.0f;
}
__device__ __forceinline__ MeshVertex load_vertex( const MeshVertex* v )
{
  const float4* p = (const float4*)v;
  const float4 a = p[0], b = p[1], c = p[2];
  MeshVertex r;
  r.px = a.x; r.py = a.y; r.pz = a.z; r.nx = a.w; r.ny = b.x; r.nz = b.y; r.cr = b.z; r.cg = b.w; r.cb = c.x; r.radius = c.y;
  r.cls = __float_as_int( c.z ); r.inst = __float_as_int( c.w );
  return r;
}
// ( v0 w0 + v1 w1 ) + v2 w2: msh_vec3_scalar_mul three times, msh_vec3_add twice (:1180-1183)
__device__ __forceinline__ float mix3( float a, float b, float c, float w0, float w1, float w2 ) { return ( a * w0 + b * w1 ) + c * w2; }

__global__ __launch_bounds__( MESH_BLOCK ) void k_mesh_sample( MeshSampleArgs A )
{
  const long long t = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if( t >= A.count ) return;
  const uint64_t steps = 2ull * (uint64_t)( A.first + t );
  uint64_t sa = A.jump.state[0], sb = A.jump.state[1];
  for( int k = 1; k < A.n_bits; ++k )
    if( ( steps >> k ) & 1 ) { sa = sa * A.jump.mul[k] + A.jump.add[0][k]; sb = sb * A.jump.mul[k] + A.jump.add[1][k]; }
  const uint64_t inc_a = A.jump.add[0][0], inc_b = A.jump.add[1][0];

  // msh_discrete_distribution_sample (msh_std.h:1935-1941): msh_rand_range's fp32 product, then the coin toss in double
  const float f_col = unit_float( pcg_draw( sa, inc_a ) );
  const float f_coin = unit_float( pcg_draw( sa, inc_a ) );
  int32_t column = (int32_t)( f_col * (float)A.n_faces );
  column = min( column, A.n_faces - 1 );                 // never taken for n_faces <= 2^24 (rs_mesh.h: MAX_FACES); keeps the read in bounds
  const MeshAlias e = A.table[column];
  const int32_t face = (double)f_coin < e.prob ? column : e.alias;

  // rs_pointcloud__random_barycentric_coords (:1114-1130)
  double s = unit_float( pcg_draw( sb, inc_b ) );
  double u = unit_float( pcg_draw( sb, inc_b ) );
  if( s + u > 1.0 ) { s = 1.0 - s; u = 1.0 - u; }
  const double q = 1.0 - s - u;
  const float w0 = (float)q, w1 = (float)s, w2 = (float)u;

  const int32_t* f = A.faces + 3 * (size_t)face;
  const MeshVertex v0 = load_vertex( A.vert + f[0] ), v1 = load_vertex( A.vert + f[1] ), v2 = load_vertex( A.vert + f[2] );
  const size_t o = (size_t)t;
  A.out_pos[3 * o] = mix3( v0.px, v1.px, v2.px, w0, w1, w2 );
  A.out_pos[3 * o + 1] = mix3( v0.py, v1.py, v2.py, w0, w1, w2 );
  A.out_pos[3 * o + 2] = mix3( v0.pz, v1.pz, v2.pz, w0, w1, w2 );
  if( A.out_nor )
  {
    const float x = mix3( v0.nx, v1.nx, v2.nx, w0, w1, w2 ), y = mix3( v0.ny, v1.ny, v2.ny, w0, w1, w2 ), z = mix3( v0.nz, v1.nz, v2.nz, w0, w1, w2 );
    const float denom = 1.0f / sqrtf( x * x + y * y + z * z );       // msh_vec3_normalize, msh_vec_math.h:868
    A.out_nor[3 * o] = x * denom; A.out_nor[3 * o + 1] = y * denom; A.out_nor[3 * o + 2] = z * denom;
  }
  if( A.out_col )
  {
    A.out_col[3 * o] = mix3( v0.cr, v1.cr, v2.cr, w0, w1, w2 );
    A.out_col[3 * o + 1] = mix3( v0.cg, v1.cg, v2.cg, w0, w1, w2 );
    A.out_col[3 * o + 2] = mix3( v0.cb, v1.cb, v2.cb, w0, w1, w2 );
  }
  if( A.out_radii )                                                  // :1195-1198: fp32 products, summed in double
  {
    const double ra = v0.radius * w0, rb = v1.radius * w1, rc = v2.radius * w2;
    A.out_radii[o] = (float)( ra + rb + rc );
  }
  // :1200-1222: the ids of the vertex with the smallest weight, vertex 0 tested first, then vertex 1
  const float m = fminf( fminf( w0, w1 ), w2 );
  const int pick = w0 == m ? 0 : w1 == m ? 1 : 2;
  if( A.out_class ) A.out_class[o] = pick == 0 ? v0.cls : pick == 1 ? v1.cls : v2.cls;
  if( A.out_instance ) A.out_instance[o] = pick == 0 ? v0.inst : pick == 1 ? v1.inst : v2.inst;
  if( A.out_face ) A.out_face[o] = face;
}

// ---- vertex normals from faces (rs_pointcloud__compute_normals, lib/rs/rs_pointcloud.h:556-596) ---------------------------------

struct NormalArgs
{
  const float* pos; int32_t pos_stride;        // vertex v's position: pos + v * pos_stride (floats): 3 for a plain array, 12 for MeshVertex records
  float* nor; int32_t nor_stride;              // ... and its normal, likewise
  const int32_t* faces; int32_t n_vertices, n_faces, loader_pass;
  float4* face_nor;                            // n_faces
  uint32_t *key, *val;                         // 3 n_faces each: the corner list before the sort ...
  const uint32_t *skey, *sval;                 // ... and after
  int32_t* start;                              // n_vertices: the first entry of a vertex's span, -1 where no face names it
  int32_t* counts;                             // n_vertices or null
};

__global__ __launch_bounds__( MESH_BLOCK ) void k_face_cross( NormalArgs A )
{
  const int32_t f = (int32_t)( blockIdx.x * MESH_BLOCK + threadIdx.x );
  if( f >= A.n_faces ) return;
  const int32_t i1 = A.faces[3 * (size_t)f], i2 = A.faces[3 * (size_t)f + 1], i3 = A.faces[3 * (size_t)f + 2];
  const float* p1 = A.pos + (size_t)i1 * A.pos_stride, *p2 = A.pos + (size_t)i2 * A.pos_stride, *p3 = A.pos + (size_t)i3 * A.pos_stride;
  const float ax = p2[0] - p1[0], ay = p2[1] - p1[1], az = p2[2] - p1[2];
  const float bx = p3[0] - p1[0], by = p3[1] - p1[1], bz = p3[2] - p1[2];
  A.face_nor[f] = make_float4( ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx, 0.0f );      // msh_vec3_cross, msh_vec_math.h:974-979
  const uint32_t c = 3u * (uint32_t)f;
  A.key[c] = (uint32_t)i1; A.key[c + 1] = (uint32_t)i2; A.key[c + 2] = (uint32_t)i3;
  A.val[c] = c; A.val[c + 1] = c + 1; A.val[c + 2] = c + 2;
}

__global__ __launch_bounds__( MESH_BLOCK ) void k_span_start( NormalArgs A )
{
  const int64_t j = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if( j >= 3 * (int64_t)A.n_faces ) return;
  const uint32_t v = A.skey[j];
  if( j == 0 || A.skey[j - 1] != v ) A.start[v] = (int32_t)j;
}

__global__ __launch_bounds__( MESH_BLOCK ) void k_vertex_chain( NormalArgs A )
{
  const int32_t v = (int32_t)( blockIdx.x * MESH_BLOCK + threadIdx.x );
  if( v >= A.n_vertices ) return;
  const int64_t n_corners = 3 * (int64_t)A.n_faces;
  float x = 0.0f, y = 0.0f, z = 0.0f;
  int32_t count = 0;
  int64_t j = A.start[v];
  if( j >= 0 )
  {
    uint32_t face = 0xFFFFFFFFu;
    float4 fn = make_float4( 0.0f, 0.0f, 0.0f, 0.0f );
    float t = 0.0f, u = 0.0f;
    for( ; j < n_corners && A.skey[j] == (uint32_t)v; ++j )
    {
      const uint32_t f = A.sval[j] / 3u;
      if( f != face )                                  // counts advance after the face's three corners (:580-583): one t per face
      {
        face = f; fn = A.face_nor[f];
        t = 1.0f / ( (float)count + 1.0f ); u = 1.0f - t;
      }
      x = t * fn.x + u * x; y = t * fn.y + u * y; z = t * fn.z + u * z;        // msh_vec3_lerp, msh_vec_math.h:1032-1036
      ++count;
    }
  }
  // :586-592.  norm = (float)sqrt( (double)sum ) is positive exactly where the fp32 sum is (the root of the smallest denormal is a
  // normal float); a NaN fails the compare, an infinite sum passes it and normalises to NaN
  const float sum = x * x + y * y + z * z;
  if( sum > 0.0f ) { const float d = 1.0f / sqrtf( sum ); x *= d; y *= d; z *= d; }
  else { x = 0.0f; y = 1.0f; z = 0.0f; }
  if( A.loader_pass )                                  // :743-751
  {
    const float d = 1.0f / sqrtf( x * x + y * y + z * z );
    x *= d; y *= d; z *= d;
    if( x != x || y != y || z != z ) { x = 0.0f; y = 0.0f; z = 0.0f; }
  }
  float* o = A.nor + (size_t)v * A.nor_stride;
  o[0] = x; o[1] = y; o[2] = z;
  if( A.counts ) A.counts[v] = count;
}

} // namespace rs

using namespace rs;

namespace {

struct MeshWorkspace
{
  Buf vert, faces, table, out[7];
  Buf n_pos, n_nor, n_counts, face_nor, key, skey, val, sval, start, tmp;      // the vertex normals' (rs_hip_vertex_normals, rs_hip_cloud_create_from_mesh)
};
thread_local MeshWorkspace g_mesh_ws;

struct MeshIn
{
  const float *pos, *nor, *col, *radii; const int32_t *cls, *inst; int64_t n_vertices; const int32_t* faces; int64_t n_faces;
};

// plan + upload: leaves the records, the faces and the alias table in the thread's workspace, the rest of the arguments in A
int mesh_prepare( const MeshIn& M, int64_t* n_samples, MeshSampleArgs& A, hipStream_t* st )
{
  char err[256] = "";
  std::vector<double> prob( (size_t)std::max<int64_t>( M.n_faces, 0 ) ); std::vector<int32_t> alias( prob.size() );
  if( M.n_faces > mesh::MAX_FACES ) { prob.clear(); alias.clear(); }        // (refused below, before the table)
  int rc = mesh::plan( M.pos, M.n_vertices, M.faces, M.n_faces, n_samples, nullptr, prob.empty() ? nullptr : prob.data(),
                       alias.empty() ? nullptr : alias.data(), err, sizeof(err) );
  if( rc ) return fail( rc, err );
  rc = api_ready( st ); if( rc ) return rc;
  MeshWorkspace& W = g_mesh_ws;
  const size_t nv = (size_t)M.n_vertices, nf = (size_t)M.n_faces;
  std::vector<MeshVertex> rec( nv );
  for( size_t i = 0; i < nv; ++i )
  {
    MeshVertex& r = rec[i];
    r.px = M.pos[3 * i]; r.py = M.pos[3 * i + 1]; r.pz = M.pos[3 * i + 2];
    r.nx = M.nor ? M.nor[3 * i] : 0.0f; r.ny = M.nor ? M.nor[3 * i + 1] : 0.0f; r.nz = M.nor ? M.nor[3 * i + 2] : 0.0f;
    r.cr = M.col ? M.col[3 * i] : 0.0f; r.cg = M.col ? M.col[3 * i + 1] : 0.0f; r.cb = M.col ? M.col[3 * i + 2] : 0.0f;
    r.radius = M.radii ? M.radii[i] : 0.0f; r.cls = M.cls ? M.cls[i] : 0; r.inst = M.inst ? M.inst[i] : 0;
  }
  std::vector<MeshAlias> tab( nf );
  for( size_t i = 0; i < nf; ++i ) { tab[i].prob = prob[i]; tab[i].alias = alias[i]; tab[i].pad = 0; }
  RS_TRY( W.vert.ensure( nv * sizeof(MeshVertex) ), "resample: buffers" );
  RS_TRY( W.faces.ensure( nf * 12 ), "resample: buffers" );
  RS_TRY( W.table.ensure( nf * sizeof(MeshAlias) ), "resample: buffers" );
  RS_TRY( hipMemcpyAsync( W.vert.p, rec.data(), nv * sizeof(MeshVertex), hipMemcpyHostToDevice, *st ), "resample: upload" );
  RS_TRY( hipMemcpyAsync( W.faces.p, M.faces, nf * 12, hipMemcpyHostToDevice, *st ), "resample: upload" );
  RS_TRY( hipMemcpyAsync( W.table.p, tab.data(), nf * sizeof(MeshAlias), hipMemcpyHostToDevice, *st ), "resample: upload" );
  RS_TRY( hipStreamSynchronize( *st ), "resample: upload" );          // the staging vectors go out of scope below
  A = MeshSampleArgs{};
  A.vert = (const MeshVertex*)W.vert.p; A.faces = (const int32_t*)W.faces.p; A.table = (const MeshAlias*)W.table.p;
  A.n_faces = (int32_t)M.n_faces;
  A.jump = mesh::jump_table();
  return RS_HIP_OK;
}

// the window [first, first + count), count > 0, inside [0, n_samples]; A's outputs are set
int mesh_launch( MeshSampleArgs& A, int64_t first, int64_t count, hipStream_t st )
{
  A.first = first; A.count = count;
  const uint64_t last_steps = 2ull * (uint64_t)( first + count - 1 );
  int bits = 1; while( bits < mesh::JUMP_BITS && ( last_steps >> bits ) ) ++bits;
  A.n_bits = bits;
  {
    ProfSpan span( "mesh_sample" );
    hipLaunchKernelGGL( k_mesh_sample, dim3( blocks_for( count, MESH_BLOCK ) ), dim3( MESH_BLOCK ), 0, st, A );
  }
  RS_TRY( hipGetLastError(), "resample: launch" );
  return RS_HIP_OK;
}

// What rs_hip_vertex_normals refuses, before a device is touched.  scan_indices false: the caller's plan looks at every index anyway.
int normals_refusal( const float* pos, int64_t n_vertices, const int32_t* faces, int64_t n_faces, bool scan_indices )
{
  char msg[200];
  if( !pos || !faces ) return fail( RS_HIP_E_ARG, "vertex_normals: pos and faces are required" );
  if( n_vertices <= 0 || n_vertices > INT32_MAX ) { snprintf( msg, sizeof(msg), "vertex_normals: %lld vertices: between 1 and INT32_MAX", (long long)n_vertices ); return fail( RS_HIP_E_ARG, msg ); }
  if( n_faces <= 0 ) { snprintf( msg, sizeof(msg), "vertex_normals: %lld faces: the reference leaves its normals unwritten without one", (long long)n_faces ); return fail( RS_HIP_E_ARG, msg ); }
  if( n_faces > INT32_MAX / 3 ) { snprintf( msg, sizeof(msg), "vertex_normals: %lld faces: 3 n_faces exceeds INT32_MAX", (long long)n_faces ); return fail( RS_HIP_E_ARG, msg ); }
  if( scan_indices )
    for( int64_t i = 0; i < 3 * n_faces; ++i )
      if( faces[i] < 0 || faces[i] >= n_vertices )
      {
        snprintf( msg, sizeof(msg), "vertex_normals: face %lld names vertex %d, outside [0, %lld)", (long long)( i / 3 ), faces[i], (long long)n_vertices );
        return fail( RS_HIP_E_ARG, msg );
      }
  return RS_HIP_OK;
}

// The three launches and the sort, queued on st.  pos / nor / faces (and counts, may be null) are device pointers; every index in
// faces is inside [0, n_vertices): the callers' refusals have seen to it.
int normals_device( const float* pos, int32_t pos_stride, float* nor, int32_t nor_stride, int32_t n_vertices, const int32_t* faces,
                    int32_t n_faces, int32_t loader_pass, int32_t* counts, hipStream_t st )
{
  MeshWorkspace& W = g_mesh_ws;
  const size_t nc = 3 * (size_t)n_faces;
  int key_bits = 1; while( key_bits < 32 && ( (uint32_t)( n_vertices - 1 ) >> key_bits ) ) ++key_bits;
  const size_t tmp_bytes = build_sort_temp_bytes( (int)nc, key_bits );
  RS_TRY( W.face_nor.ensure( (size_t)n_faces * sizeof(float4) ), "vertex_normals: buffers" );
  for( Buf* b : { &W.key, &W.skey, &W.val, &W.sval } ) RS_TRY( b->ensure( nc * 4 ), "vertex_normals: buffers" );
  RS_TRY( W.start.ensure( (size_t)n_vertices * 4 ), "vertex_normals: buffers" );
  RS_TRY( W.tmp.ensure( tmp_bytes ), "vertex_normals: buffers" );
  NormalArgs A{};
  A.pos = pos; A.pos_stride = pos_stride; A.nor = nor; A.nor_stride = nor_stride;
  A.faces = faces; A.n_vertices = n_vertices; A.n_faces = n_faces; A.loader_pass = loader_pass;
  A.face_nor = W.face_nor.as<float4>(); A.key = W.key.as<uint32_t>(); A.val = W.val.as<uint32_t>();
  A.skey = W.skey.as<uint32_t>(); A.sval = W.sval.as<uint32_t>(); A.start = W.start.as<int32_t>(); A.counts = counts;
  {
    ProfSpan span( "normals_cross" );
    hipLaunchKernelGGL( k_face_cross, dim3( blocks_for( n_faces, MESH_BLOCK ) ), dim3( MESH_BLOCK ), 0, st, A );
  }
  RS_TRY( hipGetLastError(), "vertex_normals: launch" );
  {
    ProfSpan span( "normals_group" );
    if( build_sort_pairs( W.tmp.p, tmp_bytes, A.key, W.skey.as<uint32_t>(), A.val, W.sval.as<uint32_t>(), (int)nc, key_bits, st ) )
      return fail( RS_HIP_E_RUNTIME, "vertex_normals: device sort failed" );
    RS_TRY( hipMemsetAsync( W.start.p, 0xFF, (size_t)n_vertices * 4, st ), "vertex_normals: launch" );
    hipLaunchKernelGGL( k_span_start, dim3( blocks_for( (long long)nc, MESH_BLOCK ) ), dim3( MESH_BLOCK ), 0, st, A );
  }
  RS_TRY( hipGetLastError(), "vertex_normals: launch" );
  {
    ProfSpan span( "normals_chain" );
    hipLaunchKernelGGL( k_vertex_chain, dim3( blocks_for( n_vertices, MESH_BLOCK ) ), dim3( MESH_BLOCK ), 0, st, A );
  }
  RS_TRY( hipGetLastError(), "vertex_normals: launch" );
  return RS_HIP_OK;
}

// the prepared mesh sampled into the level builder's workspace and indexed there
rs_hip_cloud_t* cloud_from_prepared( MeshSampleArgs& A, hipStream_t st, int64_t count, bool with_nor, float cell_size )
{
  // positions and normals go straight into the workspace the index build reads (as rs_hip_cloud_create_level's gather does)
  float *d_pos = nullptr, *d_nor = nullptr;
  if( api_level_workspace( (size_t)count, with_nor, &d_pos, &d_nor ) ) return nullptr;
  A.out_pos = d_pos; A.out_nor = d_nor;
  if( count > 0 && mesh_launch( A, 0, count, st ) ) return nullptr;
  return api_cloud_from_level_workspace( with_nor, (int32_t)count, cell_size );
}

} // namespace

extern "C" {

int rs_hip_resample_plan( const float* pos, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                          int64_t* n_samples, double* total_area, double* prob, int32_t* alias )
{
  char err[256] = "";
  const int rc = mesh::plan( pos, n_vertices, faces, n_faces, n_samples, total_area, prob, alias, err, sizeof(err) );
  if( rc ) api_set_err( err );
  return rc;
}

int rs_hip_uniform_resample( const float* pos, const float* nor, const float* col, const float* radii,
                             const int32_t* class_ids, const int32_t* instance_ids, int64_t n_vertices,
                             const int32_t* faces, int64_t n_faces, int64_t first, int64_t count,
                             float* out_pos, float* out_nor, float* out_col, float* out_radii,
                             int32_t* out_class, int32_t* out_instance, int32_t* out_face )
{
  if( !pos || !out_pos ) return fail( RS_HIP_E_ARG, "uniform_resample: pos and out_pos are required" );
  // the plan alone first: a window is judged against n_samples before anything is uploaded
  int64_t n_samples = 0;
  {
    char err[256] = "";
    const int rc = mesh::plan( pos, n_vertices, faces, n_faces, &n_samples, nullptr, nullptr, nullptr, err, sizeof(err) );
    if( rc ) return fail( rc, err );
  }
  if( first < 0 || count < 0 || first > n_samples || count > n_samples - first )
  {
    char msg[160]; snprintf( msg, sizeof(msg), "uniform_resample: the window [%lld, %lld + %lld) is not inside the %lld samples", (long long)first, (long long)first, (long long)count, (long long)n_samples );
    return fail( RS_HIP_E_ARG, msg );
  }
  if( count == 0 ) return RS_HIP_OK;
  const MeshIn M{ pos, nor, col, radii, class_ids, instance_ids, n_vertices, faces, n_faces };
  MeshSampleArgs A; hipStream_t st = nullptr;
  int rc = mesh_prepare( M, &n_samples, A, &st ); if( rc ) return rc;
  // an attribute whose input or output is null is skipped
  void* host[7] = { out_pos, nor ? out_nor : nullptr, col ? out_col : nullptr, radii ? out_radii : nullptr,
                    class_ids ? out_class : nullptr, instance_ids ? out_instance : nullptr, out_face };
  const size_t words[7] = { 3, 3, 3, 1, 1, 1, 1 };
  MeshWorkspace& W = g_mesh_ws;
  void* dev[7];
  for( int a = 0; a < 7; ++a )
  {
    dev[a] = nullptr;
    if( !host[a] ) continue;
    RS_TRY( W.out[a].ensure( (size_t)count * words[a] * 4 ), "resample: buffers" );
    dev[a] = W.out[a].p;
  }
  A.out_pos = (float*)dev[0]; A.out_nor = (float*)dev[1]; A.out_col = (float*)dev[2]; A.out_radii = (float*)dev[3];
  A.out_class = (int32_t*)dev[4]; A.out_instance = (int32_t*)dev[5]; A.out_face = (int32_t*)dev[6];
  rc = mesh_launch( A, first, count, st ); if( rc ) return rc;
  for( int a = 0; a < 7; ++a )
    if( host[a] ) RS_TRY( hipMemcpyAsync( host[a], dev[a], (size_t)count * words[a] * 4, hipMemcpyDeviceToHost, st ), "resample: download" );
  RS_TRY( hipStreamSynchronize( st ), "resample: kernel" );
  return RS_HIP_OK;
}

rs_hip_cloud_t* rs_hip_cloud_create_resampled( const float* pos, const float* nor, int64_t n_vertices,
                                               const int32_t* faces, int64_t n_faces, float cell_size, int64_t* n_samples )
{
  if( !pos ) { fail( RS_HIP_E_ARG, "cloud_create_resampled: pos is required" ); return nullptr; }
  const MeshIn M{ pos, nor, nullptr, nullptr, nullptr, nullptr, n_vertices, faces, n_faces };
  MeshSampleArgs A; hipStream_t st = nullptr; int64_t count = 0;
  if( mesh_prepare( M, &count, A, &st ) ) return nullptr;
  if( n_samples ) *n_samples = count;
  return cloud_from_prepared( A, st, count, nor != nullptr, cell_size );
}

int rs_hip_vertex_normals( const float* pos, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                           int32_t loader_pass, float* out_nor, int32_t* counts )
{
  if( !out_nor ) return fail( RS_HIP_E_ARG, "vertex_normals: out_nor is required" );
  int rc = normals_refusal( pos, n_vertices, faces, n_faces, true ); if( rc ) return rc;
  hipStream_t st = nullptr;
  rc = api_ready( &st ); if( rc ) return rc;
  MeshWorkspace& W = g_mesh_ws;
  const size_t nv = (size_t)n_vertices, nf = (size_t)n_faces;
  RS_TRY( W.n_pos.ensure( nv * 12 ), "vertex_normals: buffers" );
  RS_TRY( W.n_nor.ensure( nv * 12 ), "vertex_normals: buffers" );
  RS_TRY( W.faces.ensure( nf * 12 ), "vertex_normals: buffers" );
  if( counts ) RS_TRY( W.n_counts.ensure( nv * 4 ), "vertex_normals: buffers" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( W.n_pos.p, pos, nv * 12, hipMemcpyHostToDevice, st ), "vertex_normals: upload" );
  RS_TRY_DRAIN( st, hipMemcpyAsync( W.faces.p, faces, nf * 12, hipMemcpyHostToDevice, st ), "vertex_normals: upload" );
  rc = normals_device( W.n_pos.as<float>(), 3, W.n_nor.as<float>(), 3, (int32_t)n_vertices, W.faces.as<int32_t>(), (int32_t)n_faces,
                       loader_pass ? 1 : 0, counts ? W.n_counts.as<int32_t>() : nullptr, st );
  if( rc ) { (void)hipStreamSynchronize( st ); return rc; }
  RS_TRY_DRAIN( st, hipMemcpyAsync( out_nor, W.n_nor.p, nv * 12, hipMemcpyDeviceToHost, st ), "vertex_normals: download" );
  if( counts ) RS_TRY_DRAIN( st, hipMemcpyAsync( counts, W.n_counts.p, nv * 4, hipMemcpyDeviceToHost, st ), "vertex_normals: download" );
  RS_TRY( hipStreamSynchronize( st ), "vertex_normals: kernel" );
  return RS_HIP_OK;
}

rs_hip_cloud_t* rs_hip_cloud_create_from_mesh( const float* pos, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                                               float cell_size, int64_t* n_samples )
{
  if( normals_refusal( pos, n_vertices, faces, n_faces, false ) ) return nullptr;
  const MeshIn M{ pos, nullptr, nullptr, nullptr, nullptr, nullptr, n_vertices, faces, n_faces };
  MeshSampleArgs A; hipStream_t st = nullptr; int64_t count = 0;
  if( mesh_prepare( M, &count, A, &st ) ) return nullptr;            // (the plan refuses an index outside the vertices)
  if( n_samples ) *n_samples = count;
  // the normals go into the records k_mesh_sample reads: floats 3..5 of a vertex's twelve
  MeshWorkspace& W = g_mesh_ws;
  if( normals_device( W.vert.as<float>(), 12, W.vert.as<float>() + 3, 12, (int32_t)n_vertices, W.faces.as<int32_t>(), (int32_t)n_faces,
                      1, nullptr, st ) ) { (void)hipStreamSynchronize( st ); return nullptr; }
  return cloud_from_prepared( A, st, count, true, cell_size );
}

} // extern "C"
