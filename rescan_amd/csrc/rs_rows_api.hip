// librescan_hip host side: the entry points of include/rescan_hip.h over the kernels of rs_rows.hip — label transfer (with its
// folds, ids and attribute gathers), generic radius-search rows, the neighbourhood graph, the level builder and the
// scene-coverage term.  Host only: no kernel is defined here.  Runtime state and profiling: rs_api.hip, clouds:
// rs_cloud_api.hip, both through rs_api.h.

#include "../../include/rescan_hip.h"
#include "rs_api.h"
#include "rs_buildplan.h"
#include "rs_device.h"
#include "rs_host.h"
#include "rs_math.h"
#include "rs_switches.h"
#include "rs_voxel.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <array>
#include <atomic>

using namespace rs;

namespace {
struct RowsWorkspace
{
  DevBuf plc, labels, mind, fold_off, labels_o, mind_o, rows_o, ids_tab, ids_out, attr_in, attr_out;                 // labels (state in query order; *_o: input order)
  DevBuf q4, rd2, ridx, rnn, rows, qtiles;                                      // rows / misc (qtiles: the tile starts of a radius search's queries)
  DevBuf bld_pos, bld_k0, bld_k1, bld_v0, bld_v1, bld_v2, bld_small, bld_tmp;   // ... the query layout of a radius search, built like a cloud's (rs_build.hip)
  DevBuf enor, ecount, eoffset, e1, e2, ew;                                     // neighbourhood edges
  DevBuf cov_bits, cov_plc, cov_agree;                                          // coverage scores
  DevBuf lvl_pos, lvl_nor, lvl_cnt, lvl_within, lvl_offset, lvl_adj, lvl_state, lvl_misc, lvl_flags, lvl_scan, lvl_samples, lvl_tmp, lvl_cursor, lvl_work_a, lvl_work_b;   // level builder
  PinBuf h_a, h_b, h_c;      // h_a / h_b: a radius search's rows and queries; h_c: the label entry points' placements (an entry point that returns without a synchronisation — rs_hip_label_partial_device — may still be uploading from h_c)
};
thread_local RowsWorkspace g_ws;
} // namespace

extern "C" {

// ------------------------------------------------------------------------------------------
// label transfer
// ------------------------------------------------------------------------------------------

static int label_upload_placements( const rs_hip_placement_t* pl, int32_t n )
{
  int rc;
  if( ( rc = g_ws.plc.ensure( (size_t)n * sizeof(PlacementDev) ) ) || ( rc = g_ws.h_c.ensure( (size_t)n * sizeof(PlacementDev) ) ) ) return rc;
  PlacementDev* h = g_ws.h_c.as<PlacementDev>();
  for( int i = 0; i < n; ++i )
  {
    if( !pl[i].object || !pl[i].object->has_nor ) { set_err( "labels: placement %d has no object cloud with normals", i ); return RS_HIP_E_ARG; }
    Mat4 pose; std::memcpy( pose.m, pl[i].pose, 64 );
    Mat4 inv = mat4_inverse( pose ), nm = mat4_transpose( pose );       // rs_pointcloud_filters.cpp:750-751
    h[i].g = pl[i].object->view; h[i].g.evals = g_prof ? g_evals : nullptr;
    std::memcpy( h[i].inv.m, inv.m, 64 ); std::memcpy( h[i].nmat.m, nm.m, 64 );
    h[i].radius = pl[i].radius; h[i].radius_sq = radius_sq_of( pl[i].radius );
  }
  HIP_TRY( hipMemcpyAsync( g_ws.plc.p, h, (size_t)n * sizeof(PlacementDev), hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  return RS_HIP_OK;
}

// The label state of a scene lives on the device in the scene's QUERY order (g_ws.labels / g_ws.mind) while a call works on
// it; host arrays are in input order.  The two orders are exchanged by gathering (rs_rows.hip: k_label_to_*_order).
static int label_state_upload( const rs_hip_cloud_t* scene, const int8_t* labels, const float* min_dists )
{
  const size_t ns = (size_t)scene->n;
  int rc;
  if( ( rc = g_ws.labels.ensure( ns ) ) || ( rc = g_ws.mind.ensure( ns * 4 ) ) || ( rc = g_ws.labels_o.ensure( ns ) ) || ( rc = g_ws.mind_o.ensure( ns * 4 ) ) ) return rc;
  HIP_TRY( hipMemcpyAsync( g_ws.labels_o.p, labels, ns, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( g_ws.mind_o.p, min_dists, ns * 4, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  launch_label_to_query_order( scene->d_qpos, (long long)ns, g_ws.mind_o.as<float>(), g_ws.mind.as<float>(), g_ws.labels_o.as<int8_t>(), g_ws.labels.as<int8_t>(), g_stream );
  return RS_HIP_OK;
}
static int label_state_download( const rs_hip_cloud_t* scene, int8_t* labels, float* min_dists )
{
  const size_t ns = (size_t)scene->n;
  int rc;
  if( ( rc = g_ws.labels_o.ensure( ns ) ) || ( rc = g_ws.mind_o.ensure( ns * 4 ) ) ) return rc;
  launch_label_to_input_order( scene->d_qby_orig, (long long)ns, g_ws.mind.as<float>(), g_ws.mind_o.as<float>(), min_dists ? 1 : 0, g_ws.labels.as<int8_t>(), g_ws.labels_o.as<int8_t>(), g_stream );
  HIP_TRY( hipMemcpyAsync( labels, g_ws.labels_o.p, ns, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  if( min_dists ) HIP_TRY( hipMemcpyAsync( min_dists, g_ws.mind_o.p, ns * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  return RS_HIP_OK;
}
// one launch of the placement loop over the uploaded placements [first, first + n) (label_upload_placements) on the device-resident state
static int label_chain( const rs_hip_cloud_t* scene, int32_t first, int32_t n, int32_t label_base, bool fresh )
{
  int rc;
  const size_t ns = (size_t)scene->n;
  if( ( rc = g_ws.labels.ensure( ns ) ) || ( rc = g_ws.mind.ensure( ns * 4 ) ) ) return rc;
  LabelLaunch L{};
  L.scene = scene->qview; L.pl = g_ws.plc.as<PlacementDev>() + first; L.n_pl = n;
  L.label_base = label_base; L.gate_tmin = label_gate_threshold();
  L.labels = g_ws.labels.as<int8_t>(); L.min_d = g_ws.mind.as<float>(); L.rows = nullptr; L.fresh = fresh ? 1 : 0;
  { ProfScope ps( "nn_label" ); launch_label( L, g_stream ); }
  return RS_HIP_OK;
}

int rs_hip_assign_labels( const rs_hip_cloud_t* scene, const rs_hip_placement_t* placements,
                          int32_t n, int32_t label_base, int8_t* labels, float* min_dists )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( !scene || !scene->has_nor || !labels || !min_dists || n < 0 || ( n > 0 && !placements ) ) { set_err( "assign_labels: bad arguments" ); return RS_HIP_E_ARG; }
  if( label_base + n > 127 ) { set_err( "assign_labels: more than 127 placements do not fit the reference's int8 labels" ); return RS_HIP_E_CAPACITY; }
  if( n == 0 || scene->n == 0 ) return RS_HIP_OK;
  if( ( rc = label_upload_placements( placements, n ) ) || ( rc = label_state_upload( scene, labels, min_dists ) ) || ( rc = label_chain( scene, 0, n, label_base, false ) ) ) return rc;
  return label_state_download( scene, labels, min_dists );
}

int rs_hip_label_rows( const rs_hip_cloud_t* scene, const rs_hip_placement_t* placements,
                       int32_t n, float* rows, int rows_device )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( !scene || !scene->has_nor || !rows || n < 0 || ( n > 0 && !placements ) || rows_device < 0 || rows_device > 2 ) { set_err( "label_rows: bad arguments" ); return RS_HIP_E_ARG; }
  if( n == 0 || scene->n == 0 ) return RS_HIP_OK;
  const size_t ns = (size_t)scene->n;
  if( ( rc = label_upload_placements( placements, n ) ) ) return rc;
  // the kernel writes a row in the scene's query order (coalesced); rows_device = 2 hands that to the caller as it is
  float* d_rows = rows;
  if( rows_device != 2 ) { if( ( rc = g_ws.rows.ensure( (size_t)n * ns * 4 ) ) ) return rc; d_rows = g_ws.rows.as<float>(); }
  LabelLaunch L{};
  L.scene = scene->qview; L.pl = g_ws.plc.as<PlacementDev>(); L.n_pl = n;
  L.label_base = 0; L.gate_tmin = label_gate_threshold(); L.labels = nullptr; L.min_d = nullptr; L.rows = d_rows;
  { ProfScope ps( "nn_label" ); launch_label( L, g_stream ); }
  if( rows_device == 2 ) return RS_HIP_OK;
  float* d_out = rows;
  if( rows_device == 0 ) { if( ( rc = g_ws.rows_o.ensure( (size_t)n * ns * 4 ) ) ) return rc; d_out = g_ws.rows_o.as<float>(); }
  launch_label_to_input_order( scene->d_qby_orig, (long long)ns, d_rows, d_out, n, nullptr, nullptr, g_stream );
  if( rows_device == 0 )
  {
    HIP_TRY( hipMemcpyAsync( rows, d_out, (size_t)n * ns * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
    HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  }
  return RS_HIP_OK;
}

int rs_hip_label_partial_device( const rs_hip_cloud_t* scene, const rs_hip_placement_t* placements, int32_t n, int32_t label_base,
                                 float* min_dists_device, int8_t* labels_device )
{
  int rc = ensure_ready(); if( rc ) return rc;
  // normals are required even for an empty run: the kernel loads a lane's scene normal before it looks at the placement count
  if( !scene || !scene->has_nor || !min_dists_device || !labels_device || n < 0 || ( n > 0 && !placements ) ) { set_err( "label_partial_device: bad arguments" ); return RS_HIP_E_ARG; }
  if( label_base + n > 127 ) { set_err( "label_partial_device: more than 127 placements do not fit the reference's int8 labels" ); return RS_HIP_E_CAPACITY; }
  if( scene->n == 0 ) return RS_HIP_OK;
  if( n > 0 && ( rc = label_upload_placements( placements, n ) ) ) return rc;
  // the placement loop over this run, from the loop's initial state, its running (min_dist, label) written where the caller wants
  // them — in the scene cloud's query order, the order the kernel works in
  LabelLaunch L{};
  L.scene = scene->qview; L.pl = g_ws.plc.as<PlacementDev>(); L.n_pl = n;
  L.label_base = label_base; L.gate_tmin = label_gate_threshold(); L.labels = labels_device; L.min_d = min_dists_device; L.rows = nullptr; L.fresh = 1;
  { ProfScope ps( "nn_label" ); launch_label( L, g_stream ); }
  return RS_HIP_OK;
}

int rs_hip_fold_label_partials_device( const float* base_device, const int64_t* min_offsets, const int64_t* label_offsets, int32_t n_parts, int64_t scene_n,
                                       int8_t* labels, float* min_dists, const rs_hip_cloud_t* in_query_order_of )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( n_parts < 0 || scene_n < 0 || !labels || !min_dists || ( n_parts > 0 && ( !base_device || !min_offsets || !label_offsets ) ) ) { set_err( "fold_label_partials_device: bad arguments" ); return RS_HIP_E_ARG; }
  const rs_hip_cloud_t* qc = in_query_order_of;
  if( qc && qc->n != scene_n ) { set_err( "fold_label_partials_device: the cloud has %d points, the partials %lld", qc->n, (long long)scene_n ); return RS_HIP_E_ARG; }
  if( scene_n == 0 ) return RS_HIP_OK;
  const size_t ns = (size_t)scene_n;
  if( ( rc = g_ws.labels.ensure( ns ) ) || ( rc = g_ws.mind.ensure( ns * 4 ) ) || ( rc = g_ws.fold_off.ensure( (size_t)std::max( 1, n_parts ) * 16 ) ) ) return rc;
  std::vector<int64_t> off( (size_t)std::max( 1, n_parts ) * 2 );
  for( int r = 0; r < n_parts; ++r ) { off[r] = min_offsets[r]; off[(size_t)n_parts + r] = label_offsets[r]; }
  HIP_TRY( hipMemcpyAsync( g_ws.fold_off.p, off.data(), (size_t)std::max( 1, n_parts ) * 16, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );          // (off is a local)
  { ProfScope ps( "label_fold" );
    launch_label_fold_partials( base_device, g_ws.fold_off.as<long long>(), g_ws.fold_off.as<long long>() + n_parts, n_parts, (long long)scene_n,
                                g_ws.labels.as<int8_t>(), g_ws.mind.as<float>(), g_stream ); }
  if( qc ) return label_state_download( qc, labels, min_dists );
  HIP_TRY( hipMemcpyAsync( labels, g_ws.labels.p, ns, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( min_dists, g_ws.mind.p, ns * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  return RS_HIP_OK;
}

void rs_hip_combine_label_rows( const float* rows, int32_t n_rows, int64_t scene_n, int32_t label_base,
                                int8_t* labels, float* min_dists )
{
  for( int32_t k = 0; k < n_rows; ++k )
  {
    const float* r = rows + (size_t)k * scene_n;
    for( int64_t j = 0; j < scene_n; ++j )
      if( r[j] < min_dists[j] ) { min_dists[j] = r[j]; labels[j] = (int8_t)( label_base + k + 1 ); }   // rs_pointcloud_filters.cpp:763,772-773
  }
}

int rs_hip_fold_label_rows_device( const float* rows_device, const int64_t* row_offsets, int32_t n_rows, int64_t scene_n,
                                   int32_t label_base, int8_t* labels, float* min_dists, int32_t fresh,
                                   const rs_hip_cloud_t* rows_in_query_order_of )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( n_rows < 0 || scene_n < 0 || !labels || !min_dists || ( n_rows > 0 && ( !rows_device || !row_offsets ) ) ) { set_err( "fold_label_rows_device: bad arguments" ); return RS_HIP_E_ARG; }
  if( label_base + n_rows > 127 ) { set_err( "fold_label_rows_device: more than 127 placements do not fit the reference's int8 labels" ); return RS_HIP_E_CAPACITY; }
  const rs_hip_cloud_t* qc = rows_in_query_order_of;
  if( qc && qc->n != scene_n ) { set_err( "fold_label_rows_device: the cloud has %d points, the rows %lld", qc->n, (long long)scene_n ); return RS_HIP_E_ARG; }
  if( n_rows == 0 || scene_n == 0 ) return RS_HIP_OK;
  const size_t ns = (size_t)scene_n;
  if( ( rc = g_ws.labels.ensure( ns ) ) || ( rc = g_ws.mind.ensure( ns * 4 ) ) || ( rc = g_ws.fold_off.ensure( (size_t)n_rows * 8 ) ) ) return rc;
  if( !fresh )
  {
    if( qc ) { if( ( rc = label_state_upload( qc, labels, min_dists ) ) ) return rc; }
    else
    {
      HIP_TRY( hipMemcpyAsync( g_ws.labels.p, labels, ns, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
      HIP_TRY( hipMemcpyAsync( g_ws.mind.p, min_dists, ns * 4, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
    }
  }
  HIP_TRY( hipMemcpyAsync( g_ws.fold_off.p, row_offsets, (size_t)n_rows * 8, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  { ProfScope ps( "label_fold" );
    launch_label_fold( rows_device, g_ws.fold_off.as<long long>(), n_rows, (long long)scene_n, label_base, g_ws.labels.as<int8_t>(), g_ws.mind.as<float>(), fresh != 0, g_stream ); }
  if( qc ) return label_state_download( qc, labels, min_dists );
  HIP_TRY( hipMemcpyAsync( labels, g_ws.labels.p, ns, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( min_dists, g_ws.mind.p, ns * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  return RS_HIP_OK;
}

// rspf_arrangement_to_labels :780-848 on the device-resident state: order, the two passes.  Leaves the state in g_ws.labels /
// g_ws.mind (query order) and the sorted order in `ord`; *launched = 0 when there was nothing to launch (n = 0 or an empty scene).
static int arrangement_passes( const rs_hip_cloud_t* scene, const float* poses, const rs_hip_cloud_t* const* objects,
                               const int32_t* is_static, const int32_t* class_idx, int32_t n, float radius, int prioritize_static,
                               std::vector<int32_t>& ord, int* launched )
{
  int rc;
  *launched = 0;
  if( !scene || n < 0 || ( n > 0 && ( !poses || !objects || !is_static || !class_idx ) ) ) { set_err( "arrangement_to_labels: bad arguments" ); return RS_HIP_E_ARG; }
  for( int i = 0; i < n; ++i ) if( !objects[i] || !objects[i]->has_nor ) { set_err( "arrangement_to_labels: placement %d has no object cloud with normals", i ); return RS_HIP_E_ARG; }
  const int64_t ns = scene->n;
  if( n > 127 ) { set_err( "arrangement_to_labels: more than 127 placements do not fit the reference's int8 labels" ); return RS_HIP_E_CAPACITY; }
  if( !scene->has_nor && ns > 0 && n > 0 ) { set_err( "arrangement_to_labels: the scene cloud needs normals" ); return RS_HIP_E_ARG; }
  // :823-827 — qsort by (is_static << 10 | class_idx); glibc's qsort is a stable merge sort
  ord.resize( (size_t)n );
  for( int i = 0; i < n; ++i ) ord[i] = i;
  std::stable_sort( ord.begin(), ord.end(), [&]( int a, int b ) {
    return ( ( is_static[a] << 10 ) | class_idx[a] ) < ( ( is_static[b] << 10 ) | class_idx[b] ); } );
  int first_static = 0;                                                                      // :830-835
  for( int i = 0; i < n; ++i ) if( is_static[ord[i]] ) { first_static = i; break; }
  std::vector<rs_hip_placement_t> pl( n );
  for( int i = 0; i < n; ++i )
  {
    std::memcpy( pl[i].pose, poses + 16 * ord[i], 64 ); pl[i].object = objects[ord[i]];
    pl[i].radius = ( i < first_static ) ? radius : ( prioritize_static ? radius : 1.5f * radius );   // :837-848
  }
  if( ns == 0 || n == 0 ) return RS_HIP_OK;
  // Both passes run on the device-resident state (query order), which starts from (label 0, min_dist 1e9) inside the first
  // launch; only the final labels / min_dists come back (one gather to input order, one download).
  if( ( rc = label_upload_placements( pl.data(), n ) ) ) return rc;          // all of them once: the two launches read their parts
  bool have_state = false;
  if( first_static > 0 ) { if( ( rc = label_chain( scene, 0, first_static, 0, true ) ) ) return rc; have_state = true; }
  if( prioritize_static && have_state )                                                      // :841-844: min_dists start over, labels stay
  {
    const float big = 1e9f; uint32_t bits; std::memcpy( &bits, &big, 4 );
    HIP_TRY( hipMemsetD32Async( (hipDeviceptr_t)g_ws.mind.p, (int)bits, (size_t)ns, g_stream ), RS_HIP_E_RUNTIME );
  }
  if( ( rc = label_chain( scene, first_static, n - first_static, first_static, !have_state ) ) ) return rc;
  *launched = 1;
  return RS_HIP_OK;
}

int rs_hip_arrangement_to_labels( const rs_hip_cloud_t* scene,
                                  const float* poses, const rs_hip_cloud_t* const* objects,
                                  const int32_t* is_static, const int32_t* class_idx, int32_t n,
                                  float radius, int prioritize_static,
                                  int8_t* labels, float* min_dists, int32_t* sorted_order )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( !labels ) { set_err( "arrangement_to_labels: bad arguments" ); return RS_HIP_E_ARG; }      // (min_dists may be null: not wanted)
  std::vector<int32_t> ord; int launched = 0;
  if( ( rc = arrangement_passes( scene, poses, objects, is_static, class_idx, n, radius, prioritize_static, ord, &launched ) ) ) return rc;
  if( sorted_order ) for( int i = 0; i < n; ++i ) sorted_order[i] = ord[i];
  if( !launched ) { for( int64_t j = 0; j < scene->n; ++j ) { labels[j] = 0; if( min_dists ) min_dists[j] = 1e9; } return RS_HIP_OK; }     // :799-802, :820
  return label_state_download( scene, labels, min_dists );
}

int rs_hip_arrangement_to_ids( const rs_hip_cloud_t* scene,
                               const float* poses, const rs_hip_cloud_t* const* objects,
                               const int32_t* is_static, const int32_t* class_idx, const int32_t* uidx, int32_t n,
                               float radius, int prioritize_static, int32_t unlabelled_class_idx,
                               int32_t* class_ids, int32_t* instance_ids, int8_t* labels, float* min_dists, int32_t* sorted_order )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( !class_ids || !instance_ids || ( n > 0 && !uidx ) ) { set_err( "arrangement_to_ids: bad arguments" ); return RS_HIP_E_ARG; }
  std::vector<int32_t> ord; int launched = 0;
  if( ( rc = arrangement_passes( scene, poses, objects, is_static, class_idx, n, radius, prioritize_static, ord, &launched ) ) ) return rc;
  if( sorted_order ) for( int i = 0; i < n; ++i ) sorted_order[i] = ord[i];
  const size_t ns = (size_t)scene->n;
  if( !launched )
  {
    for( size_t j = 0; j < ns; ++j ) { class_ids[j] = unlabelled_class_idx; instance_ids[j] = 1024; if( labels ) labels[j] = 0; if( min_dists ) min_dists[j] = 1e9; }
    return RS_HIP_OK;
  }
  // :851-869 on the device, fused with the move from query order to input order
  std::vector<int32_t> tab( (size_t)2 * n );
  for( int i = 0; i < n; ++i ) { tab[i] = class_idx[ord[i]]; tab[n + i] = uidx[ord[i]]; }
  if( ( rc = g_ws.ids_tab.ensure( tab.size() * 4 ) ) || ( rc = g_ws.ids_out.ensure( ns * 8 ) ) || ( rc = g_ws.labels_o.ensure( ns ) ) || ( rc = g_ws.mind_o.ensure( ns * 4 ) ) ) return rc;
  HIP_TRY( hipMemcpyAsync( g_ws.ids_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  int* d_cls = g_ws.ids_out.as<int>(); int* d_inst = d_cls + ns;
  launch_label_ids_to_input_order( scene->d_qby_orig, (long long)ns, g_ws.labels.as<int8_t>(), g_ws.mind.as<float>(), g_ws.ids_tab.as<int>(), g_ws.ids_tab.as<int>() + n,
                                   unlabelled_class_idx, d_cls, d_inst, g_ws.labels_o.as<int8_t>(), g_ws.mind_o.as<float>(), g_stream );
  HIP_TRY( hipMemcpyAsync( class_ids, d_cls, ns * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( instance_ids, d_inst, ns * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  if( labels ) HIP_TRY( hipMemcpyAsync( labels, g_ws.labels_o.p, ns, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  if( min_dists ) HIP_TRY( hipMemcpyAsync( min_dists, g_ws.mind_o.p, ns * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );               // (`tab` is still alive here)
  return RS_HIP_OK;
}

// The attribute gathers that end rs_pointcloud__compute_level_poisson (lib/rs/rs_pointcloud.h:1090-1099): every per-point
// array of level 0 at the sample indices.  Arrays are host pointers (any of them may be NULL), `words` 32-bit words per point.
int rs_hip_gather_attributes( const int32_t* sample_idx, int32_t count, int32_t n_src,
                              const void* const* src, const int32_t* words, void* const* dst, int32_t n_arrays )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( count < 0 || n_src < 0 || n_arrays < 0 || ( count > 0 && !sample_idx ) || ( n_arrays > 0 && ( !src || !words || !dst ) ) ) { set_err( "gather_attributes: bad arguments" ); return RS_HIP_E_ARG; }
  if( count == 0 || n_arrays == 0 ) return RS_HIP_OK;
  for( int32_t i = 0; i < count; ++i ) if( sample_idx[i] < 0 || sample_idx[i] >= n_src ) { set_err( "gather_attributes: sample index %d out of range", sample_idx[i] ); return RS_HIP_E_ARG; }
  if( ( rc = g_ws.lvl_samples.ensure( (size_t)count * 4 ) ) ) return rc;
  HIP_TRY( hipMemcpyAsync( g_ws.lvl_samples.p, sample_idx, (size_t)count * 4, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  for( int a = 0; a < n_arrays; ++a )
  {
    if( !src[a] || !dst[a] ) continue;
    if( words[a] <= 0 ) { set_err( "gather_attributes: array %d has no width", a ); return RS_HIP_E_ARG; }
    const size_t in_b = (size_t)n_src * words[a] * 4, out_b = (size_t)count * words[a] * 4;
    if( ( rc = g_ws.attr_in.ensure( in_b ) ) || ( rc = g_ws.attr_out.ensure( out_b ) ) ) return rc;
    HIP_TRY( hipMemcpyAsync( g_ws.attr_in.p, src[a], in_b, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
    launch_gather_words( g_ws.attr_in.as<uint32_t>(), g_ws.lvl_samples.as<int>(), count, words[a], g_ws.attr_out.as<uint32_t>(), g_stream );
    HIP_TRY( hipMemcpyAsync( dst[a], g_ws.attr_out.p, out_b, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
    HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );      // the two staging buffers are reused by the next array
  }
  return RS_HIP_OK;
}

// ------------------------------------------------------------------------------------------
// generic rows
// ------------------------------------------------------------------------------------------

int rs_hip_radius_search( const rs_hip_cloud_t* target, const float* query, int64_t n_query,
                          float radius, int32_t k, float* distances_sq, int32_t* indices, size_t* n_neighbors,
                          uint64_t* total )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( !target || !query || !distances_sq || !indices || n_query < 0 || k <= 0 || !( radius > 0.0f ) ) { set_err( "radius_search: bad arguments" ); return RS_HIP_E_ARG; }
  if( n_query > 0x7fffffff / 2 ) { set_err( "radius_search: too many queries for one call" ); return RS_HIP_E_CAPACITY; }
  if( total ) *total = 0;
  if( n_query == 0 ) return RS_HIP_OK;
  const int nq = (int)n_query;
  const GridView& g = target->view;
  RowsWorkspace& W = g_ws;
  const size_t nn = (size_t)nq, nk = nn * k;
  // Long rows, or few queries: one wave per query in the caller's order (k_rows_wave) — one launch between the upload and
  // the download, which is what the reference's unchanged consumers need (mgs_compute_object_alignment_score calls this
  // tens of thousands of times with a few hundred queries and K = 64, pose_proposal.cpp:115-124).  Short rows of many
  // queries stay with the tiled successive-minima kernel below, whose cost grows with K but whose tiles share their sweeps.
  const int wave_path_max_k = 1024;
  const long long tiled_from = sw_i64( SW_ROWS_TILED_FROM );      // (read per call: tests switch it)
  if( k <= wave_path_max_k && ( k >= 16 || nq < tiled_from ) && !sw_flag( SW_NO_ROWS_WAVE ) )
  {
    // One upload, one launch, one download, one synchronisation: the call is latency (the unchanged pose_proposal makes
    // ~35 k of them per run).  Queries and the overflow flag travel in one pinned block; counts, distances and indices
    // come back in one, and are handed to the caller's arrays on the host.
    const size_t up_words = nn * 3, down_words = ( nn + 1 ) + 2 * nk;
    if( ( rc = W.bld_pos.ensure( up_words * 4 ) ) || ( rc = W.rows.ensure( down_words * 4 ) ) ||
        ( rc = W.h_a.ensure( down_words * 4 ) ) || ( rc = W.h_b.ensure( up_words * 4 ) ) ) return rc;
    float* h_up = W.h_b.as<float>();
    std::memcpy( h_up, query, nn * 12 );
    int* h_nn = W.h_a.as<int>();
    // Small calls go without the two copies: the pinned blocks are device-visible, the kernel reads the queries from host memory
    // and stores counts and rows straight into it (a few tens of KB over PCIe), so a call is ONE launch and one synchronisation.
    const size_t zero_copy_below = (size_t)sw_i64( SW_ROWS_ZERO_COPY_BELOW );
    if( down_words * 4 <= zero_copy_below )
    {
      // (RS_HIP_ROWS_POLL=1, off by default: instead of synchronising the stream the host polls the counts — every wave stores its
      //  row, then, after a system-scope fence, the row's count, which the host pre-set to a sentinel.  3 us less per call, and not
      //  safe: in one of ~60 suite runs a row was read before it had arrived — writes to host memory over PCIe may pass each
      //  other, a fence on the device does not order their ARRIVAL; only the runtime's completion signal does.)
      const bool poll = sw_flag( SW_ROWS_POLL );
      const int pending = INT_MIN;
      if( poll ) for( int i = 0; i < nq; ++i ) ( (volatile int*)h_nn )[i] = pending;
      { ProfScope ps( "nn_rows" );
        launch_rows_wave( g, h_up, nq, k, radius, radius_sq_of( radius ), (float*)( h_nn + nn + 1 ), h_nn + nn + 1 + nk, h_nn, h_nn + nq, g_stream ); }
      bool done = false;
      if( poll )
      {
        const auto t0 = std::chrono::steady_clock::now();
        int i = 0;
        for( unsigned spins = 0; ; ++spins )
        {
          while( i < nq && ( (volatile int*)h_nn )[i] != pending ) ++i;
          if( i == nq ) { done = true; break; }
          __builtin_ia32_pause();
          if( ( spins & 1023 ) == 1023 && std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count() > 2e-3 ) break;
        }
        std::atomic_thread_fence( std::memory_order_acquire );
      }
      if( !done ) HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
    }
    else
    {
      float* d_up = W.bld_pos.as<float>();
      int* d_nn = W.rows.as<int>();                    // [nq] counts (-1: more than 1024 points within the radius), one spare word, then the rows
      float* d_d2 = W.rows.as<float>() + ( nn + 1 ); int* d_idx = W.rows.as<int>() + ( nn + 1 ) + nk;
      HIP_TRY( hipMemcpyAsync( d_up, h_up, up_words * 4, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
      { ProfScope ps( "nn_rows" );
        launch_rows_wave( g, d_up, nq, k, radius, radius_sq_of( radius ), d_d2, d_idx, d_nn, d_nn + nq, g_stream ); }
      HIP_TRY( hipMemcpyAsync( h_nn, d_nn, down_words * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
      HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
    }
    bool overflow = false;
    for( int i = 0; i < nq; ++i ) overflow |= h_nn[i] < 0;
    if( !overflow )
    {
      // rows are written up to their counts only: copy exactly those (the caller's arrays keep whatever else they held, like the reference's)
      const float* hd = (const float*)( h_nn + nn + 1 ); const int* hi = h_nn + nn + 1 + nk;
      uint64_t tot = 0;
      for( int i = 0; i < nq; ++i )
      {
        const size_t c = (size_t)h_nn[i];
        std::memcpy( distances_sq + (size_t)i * k, hd + (size_t)i * k, c * 4 );
        std::memcpy( indices + (size_t)i * k, hi + (size_t)i * k, c * 4 );
        tot += c; if( n_neighbors ) n_neighbors[i] = c;
      }
      if( total ) *total = tot;
      return RS_HIP_OK;
    }
    // some query has more than 1024 points within the radius: the storage-free kernel below takes the whole call
  }
  // order the queries along a Hilbert curve and tile them on the device, exactly like a cloud's query layout
  const size_t tmp_bytes = std::max( build_sort_temp_bytes( nq, 32 ), build_scan_temp_bytes( nn + 1 ) );
  if( ( rc = W.bld_pos.ensure( nn * 12 ) ) || ( rc = W.bld_k0.ensure( ( nn + 1 ) * 4 ) ) || ( rc = W.bld_k1.ensure( ( nn + 1 ) * 4 ) ) || ( rc = W.bld_v0.ensure( nn * 4 ) ) ||
      ( rc = W.bld_v1.ensure( nn * 4 ) ) || ( rc = W.bld_v2.ensure( nn * 4 ) ) || ( rc = W.bld_small.ensure( 64 ) ) || ( rc = W.bld_tmp.ensure( tmp_bytes + 256 ) ) ||
      ( rc = W.q4.ensure( nn * 16 ) ) || ( rc = W.qtiles.ensure( ( nn + 2 ) * 4 ) ) || ( rc = W.rd2.ensure( nk * 4 ) ) || ( rc = W.ridx.ensure( nk * 4 ) ) || ( rc = W.rnn.ensure( nn * 4 ) ) ) return rc;
  float* d_raw = W.bld_pos.as<float>();
  uint32_t *k0 = W.bld_k0.as<uint32_t>(), *k1 = W.bld_k1.as<uint32_t>(), *v0 = W.bld_v0.as<uint32_t>(), *v1 = W.bld_v1.as<uint32_t>(), *v2 = W.bld_v2.as<uint32_t>();
  unsigned* d_small = W.bld_small.as<unsigned>();
  HIP_TRY( hipMemcpyAsync( d_raw, query, nn * 12, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  const unsigned init[8] = { ~0u, ~0u, ~0u, 0u, 0u, 0u, 0u, 0u };
  unsigned got[8];
  HIP_TRY( hipMemcpyAsync( d_small, init, 32, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  launch_build_bounds( d_raw, nullptr, nq, d_small, g_stream );
  HIP_TRY( hipMemcpyAsync( got, d_small, 32, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  float mn[3], ext = 0.0f;
  for( int a = 0; a < 3; ++a )
  {
    mn[a] = bp_bounds_decode( got[a] ); const float hi = bp_bounds_decode( got[3 + a] );
    if( !( hi >= mn[a] ) || !std::isfinite( mn[a] ) || !std::isfinite( hi ) ) mn[a] = 0.0f;
    else if( hi - mn[a] > ext ) ext = hi - mn[a];
  }
  launch_build_hilbert( d_raw, nq, mn, ext > 0.0f ? 1024.0f / ext : 0.0f, k0, v0, g_stream );
  if( build_sort_pairs( W.bld_tmp.p, tmp_bytes, k0, k1, v0, v2, nq, 30, g_stream ) ) { set_err( "radius_search: device sort failed" ); return RS_HIP_E_RUNTIME; }
  launch_build_gather( d_raw, nullptr, v2, nq, W.q4.as<float4>(), nullptr, g_stream );          // {x, y, z, bitcast(original query index)}
  uint32_t* flags = k0; uint32_t* scanned = k1;
  HIP_TRY( hipMemsetAsync( flags + nq, 0, 4, g_stream ), RS_HIP_E_RUNTIME );
  launch_build_tile_flags( W.q4.as<float4>(), nq, std::max( 0.25f, 4.0f * radius ), flags, v0, v1, g_stream );
  if( build_exclusive_scan( W.bld_tmp.p, tmp_bytes, flags, scanned, nn + 1, g_stream ) ) { set_err( "radius_search: device scan failed" ); return RS_HIP_E_RUNTIME; }
  unsigned n_tiles_u = 0;
  HIP_TRY( hipMemcpyAsync( &n_tiles_u, scanned + nq, 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  const int n_tiles = (int)n_tiles_u;
  launch_build_tile_scatter( flags, scanned, nq, W.qtiles.as<uint32_t>(), g_stream );
  const uint32_t last = (uint32_t)nq;
  HIP_TRY( hipMemcpyAsync( W.qtiles.as<uint32_t>() + n_tiles, &last, 4, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemsetAsync( g_ws.rd2.p, 0, nk * 4, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemsetAsync( g_ws.ridx.p, 0, nk * 4, g_stream ), RS_HIP_E_RUNTIME );
  RowsLaunch L{};
  L.tgt = g; L.q.pos = g_ws.q4.as<float4>(); L.q.nor = nullptr; L.q.tiles = g_ws.qtiles.as<uint32_t>(); L.q.n = nq; L.q.n_tiles = n_tiles;
  L.K = k; L.radius = radius; L.radius_sq = radius_sq_of( radius );
  L.d2 = g_ws.rd2.as<float>(); L.idx = g_ws.ridx.as<int>(); L.nn = g_ws.rnn.as<int>();
  { ProfScope ps( "nn_rows" ); launch_rows( L, g_stream ); }
  std::vector<int> counts( nq );
  HIP_TRY( hipMemcpyAsync( distances_sq, L.d2, nk * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( indices, L.idx, nk * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( counts.data(), L.nn, (size_t)nq * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  uint64_t tot = 0;
  for( int i = 0; i < nq; ++i ) { tot += (uint64_t)counts[i]; if( n_neighbors ) n_neighbors[i] = (size_t)counts[i]; }
  if( total ) *total = tot;
  return RS_HIP_OK;
}

} // extern "C"

// ------------------------------------------------------------------------------------------
// neighbourhood graph
// ------------------------------------------------------------------------------------------

extern "C" int rs_hip_compute_neighborhood( const rs_hip_cloud_t* cloud, int32_t max_nn, float radius_sq,
                                            float dist_exp, float angle_exp,
                                            int32_t* idx1, int32_t* idx2, float* weight, int64_t capacity, int64_t* n_edges )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( !cloud || !cloud->has_nor || max_nn <= 0 || !( radius_sq > 0.0f ) || !idx1 || !idx2 || !weight || !n_edges )
  { set_err( "compute_neighborhood: bad arguments" ); return RS_HIP_E_ARG; }
  *n_edges = 0;
  const int n = cloud->n, K = max_nn;
  if( n == 0 ) return RS_HIP_OK;
  if( capacity < (int64_t)n * K ) { set_err( "compute_neighborhood: capacity must be >= n*max_nn" ); return RS_HIP_E_ARG; }
  const size_t nk = (size_t)n * K;
  if( ( rc = g_ws.rd2.ensure( nk * 4 ) ) || ( rc = g_ws.ridx.ensure( nk * 4 ) ) || ( rc = g_ws.rnn.ensure( (size_t)n * 4 ) ) ||
      ( rc = g_ws.enor.ensure( (size_t)n * 12 ) ) || ( rc = g_ws.ecount.ensure( (size_t)n * 4 ) ) || ( rc = g_ws.eoffset.ensure( ( (size_t)n + 1 ) * 4 ) ) ||
      ( rc = g_ws.e1.ensure( nk * 4 ) ) || ( rc = g_ws.e2.ensure( nk * 4 ) ) || ( rc = g_ws.ew.ensure( nk * 4 ) ) )
    return rc;
  // 1. self-search rows (rs_pointcloud_filters.cpp:685-693): radius = (float)sqrt(radius_sq), K = max_nn
  const float radius = (float)std::sqrt( (double)radius_sq );
  RowsLaunch R{};
  R.tgt = cloud->view; R.q = cloud->qview; R.K = K; R.radius = radius; R.radius_sq = radius_sq_of( radius );
  R.d2 = g_ws.rd2.as<float>(); R.idx = g_ws.ridx.as<int>(); R.nn = g_ws.rnn.as<int>();
  { ProfScope ps( "nn_rows" ); launch_rows( R, g_stream ); }
  // 2. rows -> unique weighted edges
  HIP_TRY( hipMemcpyAsync( g_ws.enor.p, cloud->h_nor.data(), (size_t)n * 12, hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
  EdgeLaunch E{};
  E.n = n; E.K = K; E.row_d2 = R.d2; E.row_idx = R.idx; E.row_nn = R.nn; E.nor = g_ws.enor.as<float>();
  E.radius_sq = radius_sq; E.dist_exp = dist_exp; E.angle_exp = angle_exp;
  auto small_int = []( float e ) { return ( e >= 0.0f && e <= 64.0f && e == std::floor( e ) ) ? (int)e : -1; };
  E.dist_int = small_int( dist_exp ); E.angle_int = small_int( angle_exp );
  E.count = g_ws.ecount.as<int>(); E.offset = g_ws.eoffset.as<unsigned>();
  E.e1 = g_ws.e1.as<int>(); E.e2 = g_ws.e2.as<int>(); E.ew = g_ws.ew.as<float>();
  { ProfScope ps( "edges" ); launch_edge_count( E, g_stream ); launch_edge_scan( E, g_stream ); launch_edge_write( E, g_stream ); }
  unsigned total = 0;
  HIP_TRY( hipMemcpyAsync( &total, E.offset + n, 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( idx1, E.e1, (size_t)total * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( idx2, E.e2, (size_t)total * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( weight, E.ew, (size_t)total * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  *n_edges = (int64_t)total;
  return RS_HIP_OK;
}

// ------------------------------------------------------------------------------------------
// level builder (rs_rows.hip: k_level_*)
// ------------------------------------------------------------------------------------------

// the samples of a level, left on the device in g_ws.lvl_samples (increasing original indices)
static int level_samples_device( const rs_hip_cloud_t* cloud, float radius, int32_t max_n_neigh, int32_t* n_samples, int32_t* n_rounds )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( !cloud || !( radius > 0.0f ) || max_n_neigh <= 0 || !n_samples ) { set_err( "level_samples: bad arguments" ); return RS_HIP_E_ARG; }
  *n_samples = 0; if( n_rounds ) *n_rounds = 0;
  const int n = cloud->n;
  if( n == 0 ) return RS_HIP_OK;
  const size_t n1 = (size_t)n + 1;
  const size_t tmp_bytes = build_scan_temp_bytes( n1 );
  if( ( rc = g_ws.lvl_cnt.ensure( n1 * 4 ) ) || ( rc = g_ws.lvl_within.ensure( n1 * 4 ) ) || ( rc = g_ws.lvl_offset.ensure( n1 * 4 ) ) ||
      ( rc = g_ws.lvl_state.ensure( n1 * 4 ) ) || ( rc = g_ws.lvl_misc.ensure( 64 ) ) || ( rc = g_ws.lvl_flags.ensure( n1 * 4 ) ) ||
      ( rc = g_ws.lvl_scan.ensure( n1 * 4 ) ) || ( rc = g_ws.lvl_samples.ensure( n1 * 4 ) ) || ( rc = g_ws.lvl_tmp.ensure( tmp_bytes ) ) ||
      ( rc = g_ws.lvl_cursor.ensure( n1 * 4 ) ) || ( rc = g_ws.lvl_work_a.ensure( n1 * 4 ) ) || ( rc = g_ws.lvl_work_b.ensure( n1 * 4 ) ) )
    return rc;
  LevelLaunch L{};
  L.tgt = cloud->view; L.q = cloud->qview; L.by_orig = cloud->d_qby_orig; L.n = n;
  L.radius = radius; L.radius_sq = radius_sq_of( radius ); L.max_n_neigh = max_n_neigh;
  L.n_earlier = g_ws.lvl_cnt.as<int>(); L.n_later = g_ws.lvl_within.as<int>(); L.offset = g_ws.lvl_offset.as<unsigned>();
  L.state = g_ws.lvl_state.as<int>(); L.word = g_ws.lvl_cursor.as<int>();
  L.flags = g_ws.lvl_flags.as<unsigned>(); L.flag_scan = g_ws.lvl_scan.as<unsigned>(); L.samples = g_ws.lvl_samples.as<int>();
  const int BATCH = 16;
  int* misc = g_ws.lvl_misc.as<int>();            // [0..BATCH] frontier lengths of a batch of steps (entry r: input of step r), [31] over-cap flag
  L.over_cap = misc + 31;
  HIP_TRY( hipMemsetAsync( misc, 0, 128, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemsetAsync( L.n_later + n, 0, 4, g_stream ), RS_HIP_E_RUNTIME );
  // 1. who is within the radius of whom: counts, row offsets, rows of later neighbours
  { ProfScope ps( "level_neighbours" ); launch_level_neighbours( L, false, g_stream ); }
  if( build_exclusive_scan( g_ws.lvl_tmp.p, tmp_bytes, (const uint32_t*)L.n_later, g_ws.lvl_offset.as<uint32_t>(), n1, g_stream ) )
  { set_err( "level_samples: device scan failed" ); return RS_HIP_E_RUNTIME; }
  unsigned total = 0; int over = 0;
  HIP_TRY( hipMemcpyAsync( &total, L.offset + n, 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipMemcpyAsync( &over, L.over_cap, 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  if( over ) { set_err( "level_samples: a point has more than max_n_neigh = %d points within the radius (a reference search would be truncated)", max_n_neigh ); return RS_HIP_E_CAPACITY; }
  if( ( rc = g_ws.lvl_adj.ensure( std::max<size_t>( 1, total ) * 4 ) ) ) return rc;
  L.adj = g_ws.lvl_adj.as<int>();
  { ProfScope ps( "level_neighbours" ); launch_level_neighbours( L, true, g_stream ); }
  // 2. propagate: one launch per frontier, the host looks at the frontier lengths once per batch of steps
  int* front[2] = { g_ws.lvl_work_a.as<int>(), g_ws.lvl_work_b.as<int>() };
  L.front_out = front[0]; L.front_count_out = misc;           // the first frontier: points without earlier neighbours
  launch_level_init( L, g_stream );
  // lanes per frontier item from the average row length
  const double avg_row = (double)total / (double)n;
  const int G = avg_row >= 24.0 ? 64 : ( avg_row >= 3.0 ? 8 : 1 );
  const int per_block = 256 / G;
  int rounds = 0, blocks = std::min( ( n + per_block - 1 ) / per_block, 16384 ); bool done = false, first = true;
  while( !done )
  {
    if( rounds > n + BATCH ) { set_err( "level_samples: no fixed point after %d steps", rounds ); return RS_HIP_E_RUNTIME; }
    if( !first ) HIP_TRY( hipMemcpyAsync( misc, misc + BATCH, 4, hipMemcpyDeviceToDevice, g_stream ), RS_HIP_E_RUNTIME );
    HIP_TRY( hipMemsetAsync( misc + 1, 0, BATCH * 4, g_stream ), RS_HIP_E_RUNTIME );
    { ProfScope ps( "level_rounds" );
      for( int b = 0; b < BATCH; ++b )
      {
        const int r = rounds + b;
        L.front_in = front[r & 1]; L.front_count_in = misc + b;
        L.front_out = front[( r + 1 ) & 1]; L.front_count_out = misc + b + 1;
        launch_level_frontier( L, G, blocks, g_stream );
      } }
    int len[BATCH + 1];
    HIP_TRY( hipMemcpyAsync( len, misc, ( BATCH + 1 ) * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
    HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
    int widest = 1;
    for( int b = 0; b <= BATCH && !done; ++b ) { if( len[b] == 0 ) done = true; else { if( b < BATCH ) rounds++; widest = std::max( widest, len[b] ); } }
    blocks = std::min( ( n + per_block - 1 ) / per_block, std::max( 256, 2 * ( ( widest + per_block - 1 ) / per_block ) ) );     // the next batch's frontiers are about as wide as this one's
    first = false;
  }
  // 3. the samples in increasing index order
  launch_level_flags( L, g_stream );
  if( build_exclusive_scan( g_ws.lvl_tmp.p, tmp_bytes, L.flags, g_ws.lvl_scan.as<uint32_t>(), n1, g_stream ) )
  { set_err( "level_samples: device scan failed" ); return RS_HIP_E_RUNTIME; }
  launch_level_scatter( L, g_stream );
  unsigned count = 0;
  HIP_TRY( hipMemcpyAsync( &count, L.flag_scan + n, 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  *n_samples = (int32_t)count;
  if( n_rounds ) *n_rounds = rounds;
  return RS_HIP_OK;
}

extern "C" int rs_hip_level_samples( const rs_hip_cloud_t* cloud, float radius, int32_t max_n_neigh,
                                     int32_t* sample_idx, int32_t* n_samples, int32_t* n_rounds )
{
  if( !sample_idx || !n_samples ) { set_err( "level_samples: bad arguments" ); return RS_HIP_E_ARG; }
  int rc = level_samples_device( cloud, radius, max_n_neigh, n_samples, n_rounds );
  if( rc || *n_samples == 0 ) return rc;
  HIP_TRY( hipMemcpyAsync( sample_idx, g_ws.lvl_samples.p, (size_t)*n_samples * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  return RS_HIP_OK;
}

// rs_pointcloud__compute_level_poisson + rs_pointcloud_compute_search_grid (rs_pointcloud.h:984-1106,849-863) without
// leaving the device: samples -> gather of the level's positions / normals -> index build.
extern "C" rs_hip_cloud_t* rs_hip_cloud_create_level( const rs_hip_cloud_t* base, float radius, int32_t max_n_neigh, float cell_size,
                                                      int32_t* sample_idx, int32_t* n_samples )
{
  int32_t count = 0;
  if( level_samples_device( base, radius, max_n_neigh, &count, nullptr ) ) return nullptr;
  if( n_samples ) *n_samples = count;
  const size_t nn = (size_t)std::max( 1, count );
  if( g_ws.lvl_pos.ensure( nn * 12 ) || ( base->has_nor && g_ws.lvl_nor.ensure( nn * 12 ) ) ) return nullptr;
  if( count > 0 )
  {
    launch_level_gather( g_ws.lvl_samples.as<int>(), count, base->d_qby_orig, base->d_qpos, base->has_nor ? base->d_qnor : nullptr,
                         g_ws.lvl_pos.as<float>(), base->has_nor ? g_ws.lvl_nor.as<float>() : nullptr, g_stream );
    if( sample_idx && hipMemcpyAsync( sample_idx, g_ws.lvl_samples.p, (size_t)count * 4, hipMemcpyDeviceToHost, g_stream ) != hipSuccess )
    { set_err( "cloud_create_level: copy of the sample indices failed" ); return nullptr; }
  }
  return cloud_create_impl( g_ws.lvl_pos.as<float>(), base->has_nor ? g_ws.lvl_nor.as<float>() : nullptr, count, cell_size, true );
}

// ------------------------------------------------------------------------------------------
// scene-coverage term
// ------------------------------------------------------------------------------------------

// (struct rs_hip_coverage: rs_voxel.h, shared with rs_arrange.hip)

extern "C" rs_hip_coverage_t* rs_hip_coverage_create( const float bbox_min[3], const float bbox_max[3], float voxel_size,
                                                      const float* scene_pos, const float* scene_quality, int64_t n_scene,
                                                      float quality_threshold )
{
  if( ensure_ready() ) return nullptr;
  if( !bbox_min || !bbox_max || !( voxel_size > 0.0f ) || n_scene < 0 || ( n_scene > 0 && !scene_pos ) ) { set_err( "coverage_create: bad arguments" ); return nullptr; }
  rs_hip_coverage_t* c = new rs_hip_coverage_t();
  // isect_grid3d_init (lib/rs/intersect.h:59-75), same float operations (rs_voxel.h)
  double cells = 0.0;
  if( !vox_grid_init( bbox_min, bbox_max, voxel_size, c->grid, &cells ) ) { set_err( "coverage_create: %g voxels do not fit the reference's int32 cell index", cells ); delete c; return nullptr; }
  c->voxel_size = voxel_size; c->origin[0] = c->grid.ox; c->origin[1] = c->grid.oy; c->origin[2] = c->grid.oz;
  c->n_words = ( c->grid.n_cells + 31 ) / 32;
  auto fail = [&]( const char* what ) { set_err( "coverage_create: %s", what ); if( c->d_bits ) (void)hipFree( c->d_bits ); delete c; return (rs_hip_coverage_t*)nullptr; };
  if( hipMalloc( &c->d_bits, (size_t)c->n_words * 4 ) != hipSuccess ) return fail( "hipMalloc failed" );
  if( hipMemsetAsync( c->d_bits, 0, (size_t)c->n_words * 4, g_stream ) != hipSuccess ) return fail( "memset failed" );
  float *d_pos = nullptr, *d_q = nullptr; int* d_cnt = nullptr;
  bool ok = hipMalloc( &d_cnt, 4 ) == hipSuccess && hipMemsetAsync( d_cnt, 0, 4, g_stream ) == hipSuccess;
  if( ok && n_scene > 0 )
  {
    ok = hipMalloc( &d_pos, (size_t)n_scene * 12 ) == hipSuccess &&
         hipMemcpyAsync( d_pos, scene_pos, (size_t)n_scene * 12, hipMemcpyHostToDevice, g_stream ) == hipSuccess;
    if( ok && scene_quality )
      ok = hipMalloc( &d_q, (size_t)n_scene * 4 ) == hipSuccess &&
           hipMemcpyAsync( d_q, scene_quality, (size_t)n_scene * 4, hipMemcpyHostToDevice, g_stream ) == hipSuccess;
    if( ok ) launch_voxel_mark( c->grid, d_pos, d_q, quality_threshold, n_scene, c->d_bits, g_stream );
  }
  int valid = 0;
  if( ok ) { launch_popcount( c->d_bits, c->n_words, d_cnt, g_stream ); ok = hipMemcpyAsync( &valid, d_cnt, 4, hipMemcpyDeviceToHost, g_stream ) == hipSuccess; }
  ok = ok && hipStreamSynchronize( g_stream ) == hipSuccess;
  if( d_pos ) (void)hipFree( d_pos );
  if( d_q ) (void)hipFree( d_q );
  if( d_cnt ) (void)hipFree( d_cnt );
  if( !ok ) return fail( "device step failed" );
  c->valid = valid;
  return c;
}

extern "C" void rs_hip_coverage_destroy( rs_hip_coverage_t* c )
{
  if( !c ) return;
  if( c->d_bits ) (void)hipFree( c->d_bits );
  delete c;
}

extern "C" int rs_hip_coverage_info( const rs_hip_coverage_t* c, int32_t res[3], float origin[3], int64_t* n_cells, int64_t* valid_cells )
{
  if( !c ) { set_err( "coverage_info: null handle" ); return RS_HIP_E_ARG; }
  if( res ) { res[0] = c->grid.x_res; res[1] = c->grid.y_res; res[2] = c->grid.z_res; }
  if( origin ) { origin[0] = c->origin[0]; origin[1] = c->origin[1]; origin[2] = c->origin[2]; }
  if( n_cells ) *n_cells = c->grid.n_cells;
  if( valid_cells ) *valid_cells = c->valid;
  return RS_HIP_OK;
}

extern "C" int rs_hip_coverage_scene_grid( const rs_hip_coverage_t* c, uint8_t* data )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( !c || !data ) { set_err( "coverage_scene_grid: bad arguments" ); return RS_HIP_E_ARG; }
  std::vector<uint32_t> bits( (size_t)c->n_words );
  HIP_TRY( hipMemcpyAsync( bits.data(), c->d_bits, bits.size() * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );
  for( int i = 0; i < c->grid.n_cells; ++i ) data[i] = ( bits[(size_t)i >> 5] >> ( i & 31 ) ) & 1u;
  return RS_HIP_OK;
}

extern "C" int rs_hip_coverage_scores( rs_hip_coverage_t* c, const rs_hip_cloud_t* const* objects, const float* poses,
                                       const int32_t* is_static, const int32_t* first_placement, int32_t n_arr,
                                       float* scores, int32_t* agree )
{
  int rc = ensure_ready(); if( rc ) return rc;
  if( !c || n_arr < 0 || !scores || ( n_arr > 0 && !first_placement ) ) { set_err( "coverage_scores: bad arguments" ); return RS_HIP_E_ARG; }
  if( n_arr == 0 ) return RS_HIP_OK;
  const int n_plc_all = first_placement[n_arr];
  if( n_plc_all < 0 || ( n_plc_all > 0 && ( !objects || !poses || !is_static ) ) ) { set_err( "coverage_scores: bad placement lists" ); return RS_HIP_E_ARG; }
  if( (double)n_arr * c->n_words * 4 > 8.0e9 ) { set_err( "coverage_scores: batch of %d arrangements needs more than 8 GB of voxel bitmaps", n_arr ); return RS_HIP_E_CAPACITY; }
  std::vector<CoveragePlacement> h;
  int max_pts = 0;
  for( int a = 0; a < n_arr; ++a )
  {
    if( first_placement[a] > first_placement[a + 1] ) { set_err( "coverage_scores: first_placement must be non-decreasing" ); return RS_HIP_E_ARG; }
    for( int k = first_placement[a]; k < first_placement[a + 1]; ++k )
    {
      if( is_static[k] ) continue;                              // :1095-1096
      if( !objects[k] ) { set_err( "coverage_scores: placement %d has no object cloud", k ); return RS_HIP_E_ARG; }
      CoveragePlacement p{};
      p.pos = objects[k]->view.pos; p.n = objects[k]->n; p.arrangement = a;
      std::memcpy( p.pose.m, poses + 16 * (size_t)k, 64 );
      if( p.n > 0 ) { h.push_back( p ); max_pts = std::max( max_pts, p.n ); }
    }
  }
  const size_t bits_bytes = (size_t)n_arr * c->n_words * 4;
  if( ( rc = g_ws.cov_bits.ensure( bits_bytes ) ) || ( rc = g_ws.cov_agree.ensure( (size_t)n_arr * 4 ) ) ||
      ( rc = g_ws.cov_plc.ensure( std::max<size_t>( 1, h.size() ) * sizeof(CoveragePlacement) ) ) ) return rc;
  HIP_TRY( hipMemsetAsync( g_ws.cov_bits.p, 0, bits_bytes, g_stream ), RS_HIP_E_RUNTIME );      // :1090 memset
  HIP_TRY( hipMemsetAsync( g_ws.cov_agree.p, 0, (size_t)n_arr * 4, g_stream ), RS_HIP_E_RUNTIME );
  if( !h.empty() )
  {
    HIP_TRY( hipMemcpyAsync( g_ws.cov_plc.p, h.data(), h.size() * sizeof(CoveragePlacement), hipMemcpyHostToDevice, g_stream ), RS_HIP_E_RUNTIME );
    CoverageLaunch L{};
    L.grid = c->grid; L.scene_bits = c->d_bits; L.arr_bits = g_ws.cov_bits.as<uint32_t>(); L.n_words = c->n_words;
    L.plc = g_ws.cov_plc.as<CoveragePlacement>(); L.n_plc = (int)h.size(); L.max_pts = max_pts; L.agree = g_ws.cov_agree.as<int>();
    { ProfScope ps( "coverage" ); launch_coverage( L, g_stream ); }
  }
  std::vector<int> cnt( (size_t)n_arr );
  HIP_TRY( hipMemcpyAsync( cnt.data(), g_ws.cov_agree.p, (size_t)n_arr * 4, hipMemcpyDeviceToHost, g_stream ), RS_HIP_E_RUNTIME );
  HIP_TRY( hipStreamSynchronize( g_stream ), RS_HIP_E_RUNTIME );      // also keeps `h` alive until the upload is done
  for( int a = 0; a < n_arr; ++a )
  {
    float s = (float)cnt[a] / (float)c->valid;                   // :366
    if( c->valid == 0 ) s = 0.0f;                                // :367
    scores[a] = s;
    if( agree ) agree[a] = cnt[a];
  }
  return RS_HIP_OK;
}

// ------------------------------------------------------------------------------------------
// what the translation units with entry points of their own need from this one (declared in rs_host.h)
// ------------------------------------------------------------------------------------------

namespace rs {
int api_level_workspace( size_t n, bool with_nor, float** pos, float** nor )
{
  int rc = ensure_ready(); if( rc ) return rc;
  const size_t nn = std::max<size_t>( 1, n );
  if( ( rc = g_ws.lvl_pos.ensure( nn * 12 ) ) || ( with_nor && ( rc = g_ws.lvl_nor.ensure( nn * 12 ) ) ) ) return rc;
  *pos = g_ws.lvl_pos.as<float>(); *nor = with_nor ? g_ws.lvl_nor.as<float>() : nullptr;
  return RS_HIP_OK;
}
rs_hip_cloud* api_cloud_from_level_workspace( bool with_nor, int32_t n, float cell_size )
{
  return cloud_create_impl( g_ws.lvl_pos.as<float>(), with_nor ? g_ws.lvl_nor.as<float>() : nullptr, n, cell_size, true );
}
} // namespace rs
