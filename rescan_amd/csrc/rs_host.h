// Host runtime shared by the translation units with entry points of their own (rs_knn.hip, rs_isect.hip, rs_arrange.hip,
// rs_mesh.hip, rs_fuse.hip, rs_planes.hip, rs_propose.hip, rs_levels.hip): what they need from the host side of the C ABI, a growable buffer, the failure
// path, a profiling span and the grid size of a launch.  Host only: no kernel file needs it.  The api_* functions are defined by the unit
// that owns what they reach: api_level_workspace / api_cloud_from_level_workspace in rs_rows_api.hip, api_score_poses_device in
// rs_score.hip, api_cloud_* / api_clouds_from_device in rs_cloud_api.hip, the others in rs_api.hip.
#pragma once
#include "../../include/rescan_hip.h"
#include "rs_device.h"

#include <algorithm>
#include <cstdio>

namespace rs {

// the runtime state of the C ABI's host side
int             api_ready( hipStream_t* st );              // ensure_ready(); *st = the calling thread's stream
void            api_set_err( const char* what );           // rs_hip_last_error()'s text
const GridView* api_cloud_view( const struct ::rs_hip_cloud* c );
void*           api_prof_begin();                          // rs_hip_profile_enable: an event on the thread's stream (null: profiling off)
void            api_prof_end( const char* name, void* begin );   // ... and the span since then, booked under `name`
// the level builder's gather target, for a producer in another unit (rs_mesh.hip): room for n points (normals: *nor, else null) ...
int             api_level_workspace( size_t n, bool with_nor, float** pos, float** nor );
// ... and the cloud over the n points written there (the index build of rs_hip_cloud_create_level); null on failure
struct ::rs_hip_cloud* api_cloud_from_level_workspace( bool with_nor, int32_t n, float cell_size );
// one cloud per segment of device arrays (packed xyz; nor may be null), segment k being the points [first[k], first[k] + count[k]): the
// batched index build of rs_hip_cloud_create_many; all or nothing: RS_HIP_OK and out[0 .. n_segments) set, or an error code and out
// untouched.  Synchronises the stream.
int             api_clouds_from_device( const float* pos, const float* nor, const int64_t* first, const int64_t* count, int32_t n_segments, float cell_size,
                                        struct ::rs_hip_cloud** out );
// the same with a normals flag and a cell size per segment (rs_levels.hip: levels of bases with and without normals, each level with
// its own cell): segment k has normals iff has_nor[k], read at nor + 3 * first[k]; an empty segment with the flag set is an empty
// cloud with normals
int             api_clouds_from_device_each( const float* pos, const float* nor, const int64_t* first, const int64_t* count, const int32_t* has_nor,
                                             const float* cell_sizes, int32_t n_segments, struct ::rs_hip_cloud** out );
// a cloud as a query set (Hilbert order, tiles) for a sweep in another unit (rs_levels.hip)
const QueryView* api_cloud_query( const struct ::rs_hip_cloud* c );
// a cloud's points for a reader in another unit (rs_fuse.hip): the query layout (Hilbert order, 16-byte records) and the map from an
// original index to its slot there; nor is null for a cloud without normals
struct CloudPoints { const float4* qpos; const float4* qnor; const int* by_orig; int n; };
CloudPoints     api_cloud_points( const struct ::rs_hip_cloud* c );
bool            api_cloud_has_normals( const struct ::rs_hip_cloud* c );
// rs_hip_alignment_scores without its upload and read-back, for a caller in another unit (rs_propose.hip): n_poses >= 1 device poses
// of an object of >= 1 points scored into device scores, queued on the calling thread's stream, booked under nn_score.  query_box
// (lo[3], hi[3]; may be null): where the object's points can fall under these poses, which the scene-space route's lattice is cut to.
int             api_score_poses_device( const struct ::rs_hip_cloud* object, const struct ::rs_hip_cloud* scene, const float* d_poses,
                                        const float* query_box, int32_t n_poses, float radius, int32_t max_n_neigh, float* d_scores );

// A device (or pinned host) buffer grown on demand and kept between calls, one per member of a unit's thread_local workspace.
// NO destructor on purpose: a thread_local's destructor of the main thread runs at process exit, where the HIP runtime may
// already be gone, and freeing into it is worse than leaving the memory to the process.
struct Buf
{
  void* p = nullptr; size_t cap = 0; bool pinned = false;
  hipError_t ensure( size_t bytes )
  {
    if( bytes <= cap ) return hipSuccess;
    if( p ) { hipError_t e = pinned ? hipHostFree( p ) : hipFree( p ); if( e != hipSuccess ) return e; p = nullptr; cap = 0; }
    const size_t want = bytes + bytes / 4 + 256;
    hipError_t e = pinned ? hipHostMalloc( &p, want, hipHostMallocDefault ) : hipMalloc( &p, want );
    if( e == hipSuccess ) cap = want;
    return e;
  }
  hipError_t release()
  {
    if( !p ) return hipSuccess;
    const hipError_t e = pinned ? hipHostFree( p ) : hipFree( p );
    p = nullptr; cap = 0;
    return e;
  }
  template <class T> T* as() { return (T*)p; }
};

// sets rs_hip_last_error()'s text to `what` (and the HIP error's, if any) and hands rc back
inline int fail( int rc, const char* what, hipError_t e = hipSuccess )
{
  char msg[384];
  snprintf( msg, sizeof(msg), "%s%s%s", what, e != hipSuccess ? ": " : "", e != hipSuccess ? hipGetErrorString( e ) : "" );
  api_set_err( msg );
  return rc;
}
#define RS_TRY( expr, what ) do { hipError_t e_ = ( expr ); if( e_ != hipSuccess ) return ::rs::fail( RS_HIP_E_RUNTIME, what, e_ ); } while( 0 )
// (a failed step leaves the call at once, but not before the stream has drained: copies to or from the pinned buffers and the
//  caller's arrays may be in flight, and the next call reuses or frees them)
#define RS_TRY_DRAIN( st, expr, what ) do { hipError_t e_ = ( expr ); if( e_ != hipSuccess ) { (void)hipStreamSynchronize( st ); return ::rs::fail( RS_HIP_E_RUNTIME, what, e_ ); } } while( 0 )

// The launches between its construction and the end of its scope, booked under `name` while profiling is on.  Any return closes it.
struct ProfSpan
{
  const char* name; void* begin;
  explicit ProfSpan( const char* n ) : name( n ), begin( api_prof_begin() ) {}
  ~ProfSpan() { api_prof_end( name, begin ); }
  ProfSpan( const ProfSpan& ) = delete;
  ProfSpan& operator=( const ProfSpan& ) = delete;
};

// workgroups of `block` lanes that cover n items, one at least
inline unsigned blocks_for( long long n, int block ) { return (unsigned)std::max<long long>( 1, ( n + block - 1 ) / block ); }

} // namespace rs
