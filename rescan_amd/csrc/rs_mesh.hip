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
#include "rs_host.h"
#include "rs_mesh.h"

#include <algorithm>
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

} // namespace rs

using namespace rs;

namespace {

struct MeshWorkspace { Buf vert, faces, table, out[7]; };
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
  // positions and normals go straight into the workspace the index build reads (as rs_hip_cloud_create_level's gather does)
  float *d_pos = nullptr, *d_nor = nullptr;
  if( api_level_workspace( (size_t)count, nor != nullptr, &d_pos, &d_nor ) ) return nullptr;
  A.out_pos = d_pos; A.out_nor = d_nor;
  if( count > 0 && mesh_launch( A, 0, count, st ) ) return nullptr;
  return api_cloud_from_level_workspace( nor != nullptr, (int32_t)count, cell_size );
}

} // extern "C"
