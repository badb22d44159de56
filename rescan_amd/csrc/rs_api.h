// What the five host units of the C ABI share — rs_api.hip, rs_cloud_api.hip, rs_icp_api.hip, rs_rows_api.hip and the host part of
// rs_score.hip — and nobody else: the error text, the calling thread's stream, the growable buffers their workspaces are made of,
// profiling spans, the cloud object, its construction, and the two rules every search launch takes its radius and its hand-off from.
// Definitions: a cloud's construction in rs_cloud_api.hip, the rest in rs_api.hip, except the trivial inlines.  Host only.  (The
// units with kernels AND entry points of their own include rs_host.h instead, whose buffer and failure path have another return
// contract and message format: DESIGN.md §3.h.)
#pragma once
#include "../../include/rescan_hip.h"
#include "rs_device.h"

#include <atomic>
#include <cstdint>
#include <vector>

namespace rs {

void set_err( const char* fmt, ... );      // rs_hip_last_error()'s text

#define HIP_TRY( expr, code_on_fail )                                                        \
  do { hipError_t e_ = ( expr );                                                               \
       if( e_ != hipSuccess ) { set_err( "%s failed: %s (%s:%d)", #expr, hipGetErrorString( e_ ), __FILE__, __LINE__ ); \
                                return code_on_fail; } } while( 0 )

int ensure_ready();      // rs_hip_init if nobody called it; the calling thread's stream on its first call

// Every host thread that calls the library gets its own HIP stream and its own workspaces, so
// independent operators (an ICP chain, a score batch, a label transfer) issued from different
// threads overlap on the GPU: the tail of one kernel is filled by the others.  Clouds are
// immutable after creation and may be shared between threads.
extern thread_local hipStream_t g_stream;

// growable device / pinned-host buffers, kept for the life of the process (NO destructor, for rs_host.h: Buf's reason: a
// thread_local's destructor of the main thread runs at process exit, where the HIP runtime may already be gone)
struct DevBuf
{
  void* p = nullptr; size_t cap = 0;
  int ensure( size_t bytes )
  {
    if( bytes <= cap ) return RS_HIP_OK;
    if( p ) { HIP_TRY( hipFree( p ), RS_HIP_E_RUNTIME ); p = nullptr; cap = 0; }
    size_t want = bytes + bytes / 4 + 256;
    HIP_TRY( hipMalloc( &p, want ), RS_HIP_E_RUNTIME );
    cap = want;
    return RS_HIP_OK;
  }
  template <class T> T* as() { return (T*)p; }
};
struct PinBuf
{
  void* p = nullptr; size_t cap = 0;
  int ensure( size_t bytes )
  {
    if( bytes <= cap ) return RS_HIP_OK;
    if( p ) { HIP_TRY( hipHostFree( p ), RS_HIP_E_RUNTIME ); p = nullptr; cap = 0; }
    size_t want = bytes + bytes / 4 + 256;
    HIP_TRY( hipHostMalloc( &p, want, hipHostMallocDefault ), RS_HIP_E_RUNTIME );
    cap = want;
    return RS_HIP_OK;
  }
  template <class T> T* as() { return (T*)p; }
};

// ---- profiling (rs_hip_profile_enable) ----
extern bool g_prof;
extern unsigned long long* g_evals;  // device counter of staged-and-evaluated candidates (all threads, all kernels) while profiling
// one event recorded on the calling thread's stream (null if profiling is off or events ran out)
hipEvent_t prof_event();
void prof_span( const char* name, hipEvent_t a, hipEvent_t b );      // the time between two such events, booked under `name`

struct ProfScope
{
  const char* name; hipEvent_t start = nullptr;
  ProfScope( const char* n ) : name( n ) { if( g_prof ) start = prof_event(); }
  ~ProfScope() { if( start ) prof_span( name, start, prof_event() ); }
};

} // namespace rs

namespace rs {
// One device allocation that holds every array of the clouds a batched build made together (cloud_create_many_impl); the last of
// them that is destroyed frees it.
struct CloudBlock { void* p = nullptr; std::atomic<int> clouds{ 0 }; };
} // namespace rs

struct rs_hip_cloud
{
  int32_t n = 0;
  bool has_nor = false;
  rs::GridView view{};
  float4* d_pos = nullptr;
  float4* d_nor = nullptr;
  uint32_t* d_cell_start = nullptr;
  // query layout: the same points in Hilbert order, cut into tiles (one wave each)
  rs::QueryView qview{};
  float4* d_qpos = nullptr;
  float4* d_qnor = nullptr;
  uint32_t* d_tiles = nullptr;
  int* d_qby_orig = nullptr;      // original index -> query slot (the reference-order estimator walks the source in its own order)
  std::vector<int32_t> qorder;    // query slot -> original index
  std::vector<int32_t> order;     // sorted slot -> original index
  std::vector<float> h_pos, h_nor;  // original-order host copies (AoS)
  float nor_max = 1.0f;             // max |normal| (bounds how fast a gate value can change with the query normal)
  float cell = 0.0f;
  int64_t occupied = 0;             // occupied cells as handed to query_extent_limit (brute layout: the estimate of a 0.1 m grid)
  float extent_limit = 0.0f;        // the tile extent limit the query layout was cut with
  int64_t bytes = 0;
  rs::CloudBlock* block = nullptr;  // null: the d_* arrays are allocations of this cloud's own; else sub-ranges of the block
  // as an ICP source whose centroid chains gave a problem up (sums that hover around zero: rs_hip_icp_align_batch): the next calls
  // this many go straight to pass 2 of the replay instead of paying for the attempt first
  mutable std::atomic<int> chains_wander{ 0 };
};

namespace rs {

// rs_hip_cloud_create (from_device: pos / nor are device pointers — a level gathered on the device); null on failure
rs_hip_cloud_t* cloud_create_impl( const float* pos, const float* nor, int32_t n, float cell_size, bool from_device );

// rs_hip_cloud_create_many: the clouds of K segments built together, each to the byte what cloud_create_impl makes of its segment.
// All or nothing: RS_HIP_OK and out[0 .. K) set, or an error code, rs_hip_last_error()'s text and out untouched.
struct ManyInput { const float* pos; const float* nor; int32_t n; float cell_size; };
int cloud_create_many_impl( const ManyInput* segments, int32_t n_segments, bool from_device, rs_hip_cloud_t** out );

inline float radius_sq_of( float r ) { return (float)( (double)r * (double)r ); }   // msh_hash_grid.h:1104,1111 + :828

// the hand-off rule of a search launch of so many tiles (rs_search.h: tile_search)
int handoff_threshold( long long total_tiles );

} // namespace rs
