/* rescan_dropin.h — the reference's own entry points for the hot path, re-implemented on top of
 * librescan_hip.so and exported under the reference's names by librescan_dropin.so, so that
 * apps/pose_proposal and apps/segment_transfer link against it unchanged (INTEGRATION.md shows
 * the two shadow headers a maintainer adds).
 *
 * Types are layout-identical to the reference's (sizes/offsets are checked by static asserts in
 * rs_dropin.cpp and by tests/test_dropin_cpu.py):
 *   msh_vec3_t        12 bytes {x,y,z}                       lib/msh/msh_vec_math.h:159-164
 *   msh_mat4_t        64 bytes, column-major float[16]       lib/msh/msh_vec_math.h:187-191
 *   msh_hash_grid_t   120 bytes, caller-allocated, zeroed    lib/msh/msh_hash_grid.h:248-269
 *   msh_hash_grid_search_desc_t                              lib/msh/msh_hash_grid.h:196-216
 */
#ifndef RESCAN_DROPIN_H
#define RESCAN_DROPIN_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsd_vec3 { float x, y, z; } rsd_vec3_t;                 /* == msh_vec3_t */
typedef struct rsd_mat4 { float data[16]; } rsd_mat4_t;               /* == msh_mat4_t */

typedef struct rsd_hash_grid                                           /* == msh_hash_grid_t */
{
  size_t width, height, depth;
  double cell_size;
  float  min_pt[3];
  float  max_pt[3];
  void*  bin_table;        /* unused by the shim (NULL) */
  void*  data_buffer;      /* holds the shim's handle of this grid (host copy of the points + lazily built device cloud) */
  void*  offsets;          /* unused by the shim (NULL) */
  int32_t  _slab_size;
  double   _inv_cell_size;
  uint8_t  _pts_dim;
  uint16_t _num_threads;
  int32_t  _dont_use_omp;
  uint32_t max_n_pts_in_bin;
  size_t   _n_pts;
} rsd_hash_grid_t;

typedef struct rsd_search_desc                                         /* == msh_hash_grid_search_desc_t */
{
  float*   query_pts;
  size_t   n_query_pts;
  float*   distances_sq;
  int32_t* indices;
  size_t*  n_neighbors;
  float    radius;
  union { size_t k; size_t max_n_neigh; };
  int      sort;
} rsd_search_desc_t;

/* lib/msh/msh_hash_grid.h:218-230 */
void   msh_hash_grid_init_3d( rsd_hash_grid_t* hg, const float* pts, const int32_t n_pts, const float radius );
void   msh_hash_grid_init_2d( rsd_hash_grid_t* hg, const float* pts, const int32_t n_pts, const float radius );   /* :544-548: (x, y) pairs, kept as (x, y, 0) */
void   msh_hash_grid_term( rsd_hash_grid_t* hg );
size_t msh_hash_grid_radius_search( const rsd_hash_grid_t* hg, rsd_search_desc_t* search_desc );
/* :1294-1447 — the reference's shell-by-shell traversal (not an exact k-nearest search: it stops one shell of bins after k points are
 * stored), restated on the host on a grid of the reference's own geometry; no caller on the hot path.  Rows ascending in
 * (dist², index); ends where the reference would overrun its 128-bin stack array or never return (rs_dropin.cpp: KnnGrid). */
size_t msh_hash_grid_knn_search( const rsd_hash_grid_t* hg, rsd_search_desc_t* search_desc );

/* lib/rs/icp.h:83-115 */
float icp_align( rsd_vec3_t* pts1, rsd_vec3_t* nor1, int32_t n_pts1,
                 rsd_vec3_t* pts2, rsd_vec3_t* nor2, int32_t n_pts2,
                 rsd_mat4_t* T1, rsd_mat4_t T2, float max_dist, float max_angle, bool verbose );
float icp_estimate_rigid_xform_pt2pt( rsd_vec3_t* pts1, rsd_vec3_t* pts2, float* weights, int32_t n_pts, rsd_mat4_t* T1 );   /* icp.h:153-206: a stub in the reference (returns 1.0f) */
float icp_estimate_rigid_xform_pt2pl( rsd_vec3_t* pts1, rsd_vec3_t* pts2, rsd_vec3_t* nor2, float* weights,
                                      int32_t n_pts, rsd_mat4_t* T1 );
void  icp_find_corrs( rsd_vec3_t* pts1, rsd_vec3_t* nor1, int32_t n_pts1, rsd_hash_grid_t* idx1,
                      rsd_vec3_t* pts2, rsd_vec3_t* nor2, int32_t n_pts2, rsd_hash_grid_t* idx2,
                      rsd_mat4_t T1, rsd_mat4_t T2,
                      rsd_vec3_t** corr_pts1, rsd_vec3_t** corr_nor1, rsd_vec3_t** corr_pts2, rsd_vec3_t** corr_nor2,
                      float** weights, int32_t* n_corrs, float max_dist, float max_angle );

/* The two C++-linkage consumers take rs_pointcloud_t / rsdb_t, which the shim does not know; the
 * shadow copies of those functions call these flat entry points instead.
 *
 * mgs_compute_object_alignment_score (apps/pose_proposal/pose_proposal.cpp:93-158) for one pose:
 * obj_* = object->positions/normals[query_lvl], scn_* = scene->positions/normals[search_lvl]. */
float rsd_alignment_score( const rsd_vec3_t* obj_pos, const rsd_vec3_t* obj_nor, int32_t n_obj,
                           const rsd_vec3_t* scn_pos, const rsd_vec3_t* scn_nor, int32_t n_scn,
                           rsd_mat4_t xform, float search_radius, int32_t max_n_neigh );
/* the same for a batch of poses (the grid-search loops at pose_proposal.cpp:213-244, 283-298) */
int   rsd_alignment_scores( const rsd_vec3_t* obj_pos, const rsd_vec3_t* obj_nor, int32_t n_obj,
                            const rsd_vec3_t* scn_pos, const rsd_vec3_t* scn_nor, int32_t n_scn,
                            const rsd_mat4_t* xforms, int32_t n_poses, float search_radius, int32_t max_n_neigh,
                            float* scores );
/* mgs_propose_poses (apps/pose_proposal/pose_proposal.cpp:325-369) for the objects the caller names (it leaves the static ones
 * out: rsdb_is_object_static), the whole cascade on the device (rs_hip_propose_poses).  Entry [o * n_levels + l] of obj_pos /
 * obj_nor / n_obj = objects[o].shape->positions / normals / n_pts of level RSPC_N_LEVELS - 1 - l; scn_* = the scan's level 1;
 * bbox_* = input_scan->bbox; the reference's constants: opts->search_grid_spacing, opts->search_grid_angle_delta, height 0,
 * thresholds { 0.25f, 0.35f, 0.40f }, search_radius 0.1f, max_n_neigh 64.  counts[o] proposals of object o in
 * xforms[o * capacity ..] / scores[o * capacity ..], in the reference's order, the ones marked -1 included.  More than
 * `capacity` for an object: RS_HIP_E_CAPACITY (-4), counts hold what is needed, nothing else is written. */
int   rsd_propose_poses( const rsd_vec3_t* const* obj_pos, const rsd_vec3_t* const* obj_nor, const int32_t* n_obj, int32_t n_objects,
                         int32_t n_levels, const rsd_vec3_t* scn_pos, const rsd_vec3_t* scn_nor, int32_t n_scn,
                         const rsd_vec3_t* bbox_min, const rsd_vec3_t* bbox_max, float spacing, float angle_delta, float height,
                         const float* thresholds, float search_radius, int32_t max_n_neigh, int32_t capacity,
                         int32_t* counts, rsd_mat4_t* xforms, float* scores );
/* isect_get_overlap_factor (lib/rs/intersect.h:309-368) of two placed shapes, bit for bit: *_lvl1 = shape->positions[1] (the
 * points that are rasterised), *_lvl3 = shape->positions[3] (the points whose boxes size the grid).  *overlap is written on
 * success only (0; < 0: an RS_HIP_E_* code, see rs_hip_overlap_factors). */
int   rsd_overlap_factor( const rsd_vec3_t* a_lvl1, int32_t a_n1, const rsd_vec3_t* a_lvl3, int32_t a_n3, const rsd_mat4_t* pose_a,
                          const rsd_vec3_t* b_lvl1, int32_t b_n1, const rsd_vec3_t* b_lvl3, int32_t b_n3, const rsd_mat4_t* pose_b,
                          float voxel_size, int voxelize_inside, int normalize_by_smaller, float* overlap );
/* mgs_non_maxima_suppresion (apps/pose_proposal/pose_proposal.cpp:377-451) for ONE object's proposals: lvl1 / lvl3 as above,
 * centroid = rs_pointcloud_centroid( shape, 0 ), poses[i] = proposals[i].xform, scores[i] = proposals[i].score.  marks[i] = 1
 * keep / 2 discard; keep_idx[0 .. *n_keep) ascending: the caller copies proposals[keep_idx[k]] in that order (:441-447). */
int   rsd_non_maxima_suppression( const rsd_vec3_t* lvl1, int32_t n1, const rsd_vec3_t* lvl3, int32_t n3, const rsd_vec3_t* centroid,
                                  const rsd_mat4_t* poses, const float* scores, int32_t n, float dist_threshold,
                                  int32_t* marks, int32_t* keep_idx, int32_t* n_keep );
/* rspf_arrangement_to_labels' search part (lib/rs/rs_pointcloud_filters.cpp:796-848): placements in
 * arrangement order with per-placement static flag and class index; writes int8 labels (1-based
 * index into the sorted arrangement, whose permutation is returned in sorted_order). */
int   rsd_arrangement_to_labels( const rsd_vec3_t* scn_pos, const rsd_vec3_t* scn_nor, int32_t n_scn,
                                 const rsd_vec3_t* const* obj_pos, const rsd_vec3_t* const* obj_nor, const int32_t* obj_n,
                                 const rsd_mat4_t* poses, const int32_t* is_static, const int32_t* class_idx, int32_t n_plc,
                                 float radius, bool prioritize_static, int8_t* labels, int32_t* sorted_order );

/* The whole of rspf_arrangement_to_labels (lib/rs/rs_pointcloud_filters.cpp:780-879) including its tail (:851-869): the
 * outputs are in_pc->class_ids[lvl] / instance_ids[lvl] themselves — class of the labelled placement's object, the
 * placement's uidx, (rsdb_get_class_idx( rsdb, "unlabelled" ), RSPF_MAX_INSTANCES) where no placement claimed the point. */
int   rsd_arrangement_to_ids( const rsd_vec3_t* scn_pos, const rsd_vec3_t* scn_nor, int32_t n_scn,
                              const rsd_vec3_t* const* obj_pos, const rsd_vec3_t* const* obj_nor, const int32_t* obj_n,
                              const rsd_mat4_t* poses, const int32_t* is_static, const int32_t* class_idx, const int32_t* uidx, int32_t n_plc,
                              float radius, bool prioritize_static, int32_t unlabelled_class_idx,
                              int32_t* class_ids, int32_t* instance_ids );

/* rspf_compute_neighborhood (lib/rs/rs_pointcloud_filters.cpp:674-722) on pc->positions/normals[lvl]:
 * fills the caller's edge arrays (capacity >= n*max_nn; the reference's hashtable would hold as many),
 * idx1/idx2/weight being the fields of its edge_t (:664-669).  Returns the edge count (< 0: error). */
int64_t rsd_compute_neighborhood( const rsd_vec3_t* pos, const rsd_vec3_t* nor, int32_t n,
                                  int32_t max_nn, float radius_sq, float dist_exp, float angle_exp,
                                  int32_t* idx1, int32_t* idx2, float* weight );

/* rs_pointcloud__compute_level_poisson (lib/rs/rs_pointcloud.h:984-1106) on pc->positions[0]: the indices of the
 * level's samples, increasing — the caller fills positions/normals/colors/... [level][i] = [0][sample_idx[i]] as the
 * reference does (:1090-1099).  voxel_size = pc->voxel_size[level]; the reference's cap on a search,
 * max_n_neigh = 1024 * level / (RSPC_N_LEVELS - 1) or 256 (:995-996), is derived from `level`.  sample_idx has
 * capacity n.  Returns the number of samples (< 0: error; RS_HIP_E_CAPACITY if a point has more than max_n_neigh
 * points within voxel_size, where a reference search would be truncated). */
int32_t rsd_level_poisson( const rsd_vec3_t* pos, int32_t n, float voxel_size, int32_t level, int32_t* sample_idx );

/* The levels first_level .. first_level + n_levels - 1 of one cloud in one call — the loop of rs_pointcloud_compute_levels
 * (lib/rs/rs_pointcloud.h:1311-1315), every level sampled from pc->positions[0] as the reference does.  voxel_size is indexed by the
 * level NUMBER (pass pc->voxel_size); the caps are derived from the level numbers as rsd_level_poisson derives its own.
 * sample_idx[k] (capacity n) and counts[k] receive what rsd_level_poisson( pos, n, voxel_size[first_level + k], first_level + k, . )
 * returns.  At most 8 levels.  Returns 0 (< 0: error, nothing written; RS_HIP_E_CAPACITY as above, for any of the levels). */
int32_t rsd_levels_poisson( const rsd_vec3_t* pos, int32_t n, const float* voxel_size, int32_t first_level, int32_t n_levels,
                            int32_t* const* sample_idx, int32_t* counts );

/* rs_pointcloud_uniform_resample (lib/rs/rs_pointcloud.h:1132-1227) on in_mesh's level 0 and faces_ind: the level-0 arrays of
 * out_pc, bit for bit (qualities stay unset, as in the reference).  Returns the sample count — what the caller passes to
 * rs_pointcloud__allocate_level — or a negative RS_HIP_E_* code with nothing written.  A call with every output NULL returns the
 * count only and needs no device; otherwise pos is required, any other attribute with a NULL input or output is skipped, and
 * `capacity` (the outputs' length in samples) below the count gives RS_HIP_E_ARG. */
int64_t rsd_uniform_resample( const rsd_vec3_t* pos, const rsd_vec3_t* nor, const rsd_vec3_t* col, const float* radii,
                              const int32_t* class_ids, const int32_t* instance_ids, int64_t n_vertices,
                              const int32_t* faces_ind, int64_t n_faces, int64_t capacity,
                              rsd_vec3_t* out_pos, rsd_vec3_t* out_nor, rsd_vec3_t* out_col, float* out_radii,
                              int32_t* out_class, int32_t* out_instance );

/* rs_pointcloud__compute_normals (lib/rs/rs_pointcloud.h:556-596) on pc->positions[0] and faces_ind: pc->normals[0], bit for bit
 * (where the reference's value is NaN, a NaN).  The loader's own pass (:743-751) stays where it is.  Returns 0, or a negative
 * RS_HIP_E_* code with nothing written: no face, an index outside [0, n), counts above INT32_MAX (include/rescan_hip.h:
 * rs_hip_vertex_normals). */
int32_t rsd_compute_normals( const rsd_vec3_t* positions, int64_t n, const int32_t* faces_ind, int64_t n_faces, rsd_vec3_t* normals );

/* The body of rsdu_augment_database's `if( extracted_shape )` block (apps/segment_transfer/database_update.cpp:58-90) for one
 * placement, extraction included: the points of input_scan's level 1 that carry uidx, aligned to cur_shape's level 0 by icp_align
 * ( .., 0.05, msh_deg2rad( 10 ) ) from inverse( pose ) unless is_static, transformed, merged with cur_shape and shuffled — the level-0
 * arrays of merged_shape, allocated with malloc (rs_pointcloud_free releases them), every instance id set to uidx.  The model's
 * instance ids are not an input: the reference overwrites them.  xform (may be NULL): the pose the points were moved by.  Returns the
 * merged count; 0 with nothing allocated when no scan point carries uidx (the reference then leaves the object as it is); a negative
 * RS_HIP_E_* code on failure.  Bit for bit the reference's arrays up to 16 384 extracted points (include/rescan_hip.h). */
int64_t rsd_augment_model( const rsd_vec3_t* scan_pos, const rsd_vec3_t* scan_nor, const rsd_vec3_t* scan_col, const float* scan_radii,
                           const float* scan_qual, const int32_t* scan_class, const int32_t* scan_instance, int32_t n_scan,
                           const rsd_vec3_t* model_pos, const rsd_vec3_t* model_nor, const rsd_vec3_t* model_col, const float* model_radii,
                           const float* model_qual, const int32_t* model_class, int32_t n_model,
                           const rsd_mat4_t* pose, int32_t uidx, int32_t is_static,
                           rsd_vec3_t** out_pos, rsd_vec3_t** out_nor, rsd_vec3_t** out_col, float** out_radii, float** out_qual,
                           int32_t** out_class, int32_t** out_instance, rsd_mat4_t* xform );

/* rsd_augment_model for all placements of an arrangement in one device call (rs_hip_cloud_fuse_arrangement): the scan's ids go to
 * the device once and are cut once, and every round of placements shares one permutation pass and one merge launch.  The scan's
 * arrays as above; per placement p: the model's six arrays (entries of arrays of n_placements pointers) with n_model[p], the pose,
 * uidx and is_static, and model_from[p]: -1, or the index q < p of an earlier placement whose resulting shape is p's model — its
 * merged arrays, or q's own model when no scan point carries q's uidx — which is what the reference's loop sees when the same
 * object is placed twice or a novel object copies a shape an earlier placement replaced (database_update.cpp:40-56, :89); p's own
 * model arrays are then ignored and may be NULL.  Outputs: arrays of n_placements pointers, entry p malloc'ed as rsd_augment_model
 * allocates it (every instance id uidx[p]) or NULL with out_n[p] = 0 when no scan point carries uidx[p]; xforms (may be NULL): one
 * per placement.  Returns 0, or a negative RS_HIP_E_* code with nothing allocated.  Placement by placement the arrays are those of
 * rsd_augment_model given the same model. */
int32_t rsd_augment_models( const rsd_vec3_t* scan_pos, const rsd_vec3_t* scan_nor, const rsd_vec3_t* scan_col, const float* scan_radii,
                            const float* scan_qual, const int32_t* scan_class, const int32_t* scan_instance, int32_t n_scan,
                            int32_t n_placements,
                            const rsd_vec3_t* const* model_pos, const rsd_vec3_t* const* model_nor, const rsd_vec3_t* const* model_col,
                            const float* const* model_radii, const float* const* model_qual, const int32_t* const* model_class,
                            const int32_t* n_model, const int32_t* model_from,
                            const rsd_mat4_t* poses, const int32_t* uidx, const int32_t* is_static,
                            rsd_vec3_t** out_pos, rsd_vec3_t** out_nor, rsd_vec3_t** out_col, float** out_radii, float** out_qual,
                            int32_t** out_class, int32_t** out_instance, int64_t* out_n, rsd_mat4_t* xforms );

/* The loop of seg2rsdb's pointcloud_to_rsdb (apps/seg2rsdb/main.cpp:80-136) on pointcloud's level-0 arrays: the instances in order
 * of first appearance, every instance's points cut out in input order and, unless the class of its first point is among
 * static_classes (the caller's rsdb_is_class_static, which needs the class table), moved by msh_translate( identity, -centroid ) with
 * centroid.y = 0.  inst_ids / class_of / xforms / poses (one per instance; poses[k] = msh_mat4_inverse( xforms[k] ) is the placement's;
 * xforms may be NULL) and offsets (one more) have room for `capacity` instances; order, out_pos and out_nor for n points: instance
 * k's shape is out_pos / out_nor [offsets[k] .. offsets[k + 1]), and its colours, radii, qualities, class and instance ids are the
 * scan's at order[offsets[k] ..].  Bit for bit the reference's arrays (include/rescan_hip.h: rs_hip_scan_to_objects).  Without a
 * device the library's host plan answers (rs_hip_split_plan: the same arrays; rsd_device_failures() counts such calls).  Returns the
 * number of instances, or a negative RS_HIP_E_* code: RS_HIP_E_CAPACITY, with nothing written, when the scan holds more than
 * `capacity` (or more than 4096) instances. */
int32_t rsd_scan_to_objects( const rsd_vec3_t* pos, const rsd_vec3_t* nor, const int32_t* class_ids, const int32_t* instance_ids, int64_t n,
                             const int32_t* static_classes, int32_t n_static, int32_t capacity,
                             int32_t* inst_ids, int32_t* class_of, int64_t* offsets, int32_t* order,
                             rsd_vec3_t* out_pos, rsd_vec3_t* out_nor, rsd_mat4_t* xforms, rsd_mat4_t* poses );

/* The plane stage of segment_transfer (lib/rs/rs_pointcloud_filters.cpp), on host arrays as the reference holds them.  A plane
 * model crosses as plain arrays, model m at centers[m], normals[m], axes[9m] (msh_mat3_t's data: column-major), extends[4m]
 * (msh_vec4_t's x, y, z, w), valid[m], normal_up_dot[m] = features.normal_up_dot (include/rescan_hip.h).  INTEGRATION.md §3 has
 * the patches.
 *
 * rsd_detect_floor_and_walls replaces rspf__detect_floor + rspf__detect_walls (:506-507) on pc's level 2: the models they push, in
 * their order, n_inliers = each one's votes, *n_floors / *n_walls their return values.  Returns the number of models (<= capacity),
 * or a negative RS_HIP_E_* code with nothing written (include/rescan_hip.h lists the refusals).
 *
 * rsd_gather_model_inliers replaces rspf__gather_model_inliers (:517, :640): *index = one malloc'ed array (the caller frees it) with
 * model m's inlier indices, increasing, at [offsets[m], offsets[m + 1]); offsets has n_models + 1 entries.  Returns the total, or a
 * negative code with *index = NULL.
 *
 * rsd_relabel_walls_and_floors replaces the gather and the loop of rspf_relabel_walls_and_floors (:632-667) on pc's level 1:
 * class_ids / instance_ids are rewritten in place.  0, or a negative code with both arrays as they were. */
int32_t rsd_detect_floor_and_walls( const rsd_vec3_t* pos, const rsd_vec3_t* nor, int64_t n, float dot_threshold, float dist_threshold,
                                    int64_t count_threshold, int32_t capacity, rsd_vec3_t* centers, rsd_vec3_t* normals, int64_t* n_inliers,
                                    int32_t* n_floors, int32_t* n_walls );
int64_t rsd_gather_model_inliers( const rsd_vec3_t* pos, const rsd_vec3_t* nor, int64_t n, const rsd_vec3_t* centers, const rsd_vec3_t* normals,
                                  const float* axes, const float* extends, const int8_t* valid, int32_t n_models, float dot_threshold,
                                  float dist_threshold, int32_t check_validity, int32_t check_extends, int32_t** index, int64_t* offsets );
int     rsd_relabel_walls_and_floors( const rsd_vec3_t* pos, const rsd_vec3_t* nor, int64_t n, const rsd_vec3_t* centers, const rsd_vec3_t* normals,
                                      const float* axes, const float* extends, const int8_t* valid, const float* normal_up_dot, int32_t n_models,
                                      int32_t floor_idx, int32_t wall_idx, int32_t unlabelled_idx, int32_t* class_ids, int32_t* instance_ids );

/* Scene-coverage term of the arrangement optimiser (apps/segment_transfer/arrangement_optimization.cpp:344-373).
 * rsd_coverage_create replaces isect_grid3d_init + rsao_rasterize_scene_to_grid for opts->scn_grd
 * (apps/segment_transfer/main.cpp:323-339); rsd_coverage_score replaces the body of
 * rsao__compute_scene_coverage_score: obj_* = rsdb->objects[arrangement[i].object_idx].shape level 2,
 * is_static[i] = rsdb_is_object_static(...).  Returns the score; < 0 on a device error. */
void* rsd_coverage_create( const rsd_vec3_t* bbox_min, const rsd_vec3_t* bbox_max, float voxel_size,
                           const rsd_vec3_t* scene_pos, const float* scene_quality, int32_t n_scene, float quality_threshold );
float rsd_coverage_score( void* coverage, const rsd_vec3_t* const* obj_pos, const int32_t* obj_n,
                          const rsd_mat4_t* poses, const int32_t* is_static, int32_t n_plc );
void  rsd_coverage_destroy( void* coverage );
/* The coverage term of rsao_greedy_step's trial arrangements (arrangement_optimization.cpp:1012-1020) in one call: scores[k] =
 * rsao__compute_scene_coverage_score of cur_arrangement + proposals[k], bit for bit (rs_hip_coverage_extensions).  base_* =
 * cur_arrangement as for rsd_coverage_score; cand_* = the proposals' level-2 clouds and poses.  0, or an RS_HIP_E_* code with
 * nothing written. */
int   rsd_coverage_extensions( void* coverage, const rsd_vec3_t* const* base_pos, const int32_t* base_n, const rsd_mat4_t* base_poses,
                               const int32_t* base_static, int32_t n_base,
                               const rsd_vec3_t* const* cand_pos, const int32_t* cand_n, const rsd_mat4_t* cand_poses, int32_t n_cand,
                               float* scores );
/* The coverage term of rsao_simulated_annealing's 25 000 arrangements (arrangement_optimization.cpp:388 ff.) without a device call
 * per iteration (rs_hip_coverage_footprints, rs_hip_footprints_scores).  Before the loop, ONE rsd_coverage_footprints over every
 * placement the loop can hold — each proposal of each dynamic object of the scene, then the placements of the starting arrangement:
 * obj_* / poses / is_static as for rsd_coverage_score.  Returns a handle (host memory), NULL on failure.  Inside
 * rsao__compute_scene_coverage_score, rsd_footprints_score( handle, members, n ) is the score of the arrangement whose placements
 * are members[0 .. n) — indices into the list given to rsd_coverage_footprints, found by (object_idx, the pose's 64 bytes), NOT by
 * pose_idx, which the move action leaves stale (:513-516) — bit for bit; < 0 on a bad index.  It touches no device.  One thread
 * at a time per handle. */
void* rsd_coverage_footprints( void* coverage, const rsd_vec3_t* const* obj_pos, const int32_t* obj_n, const rsd_mat4_t* poses,
                               const int32_t* is_static, int32_t n_plc );
float rsd_footprints_score( void* footprints, const int32_t* members, int32_t n_members );
void  rsd_footprints_destroy( void* footprints );
/* rsao_compute_scene_saliency (arrangement_optimization.cpp:1109-1160, 1292-1295; apps/segment_transfer/main.cpp:337) for one
 * scene: quality[i] replaces scn->qualities[0][i].  bbox = the scene cloud's, voxel_size = 0.15f (main.cpp:327); obj_* =
 * rsdb->objects[o].shape level 2; proposal k = (object, rsdb->proposed_poses[scene][object][pose], rsdb_is_object_static);
 * scene_pos / scene_class = scn->positions[0] / class_ids[0]; wall_class / floor_class = rsdb_get_class_idx (-1: absent).
 * 0, or an RS_HIP_E_* code with nothing written. */
int   rsd_scene_saliency( const rsd_vec3_t* bbox_min, const rsd_vec3_t* bbox_max, float voxel_size,
                          const rsd_vec3_t* const* obj_pos, const int32_t* obj_n, int32_t n_objects,
                          const int32_t* prop_object, const rsd_mat4_t* prop_poses, const int32_t* prop_static, int32_t n_props,
                          const rsd_vec3_t* scene_pos, const int32_t* scene_class, int32_t n_scene,
                          int32_t wall_class, int32_t floor_class, float* quality );

/* ---- the on-disk formats either side of the path ---------------------------------
 * Pose-proposal blob (writer apps/pose_proposal/main.cpp:61-89, reader apps/segment_transfer/main.cpp:143-193):
 * int32 n_arrays; int32 count[n_arrays]; then per proposal 16 floats (column-major pose) + 1 float score,
 * arrays back to back, host byte order.  `records` holds sum(count) x 17 floats.  The reader allocates
 * *counts and *records with malloc (caller frees); like the reference's, it accepts a truncated file only
 * up to the last complete array and reports the failure (RSD_FORMAT_ERR). */
#define RSD_FORMAT_ERR (-20)
int rsd_pose_bin_write( const char* path, int32_t n_arrays, const int32_t* counts, const float* records );
int rsd_pose_bin_read( const char* path, int32_t* n_arrays, int32_t** counts, float** records );
/* One `pose` line of an .rsdb database (lib/rs/rs_database.h:379-401 parser, :597-606 writer): the 4x4 pose
 * is printed row by row with "%f", i.e. rounded to 6 decimals — poses lose precision between pose_proposal and
 * segment_transfer, and that is reference behaviour.  format returns the length written (no newline). */
int rsd_rsdb_format_pose_line( char* out, size_t capacity, int32_t uidx, int32_t arrangement_idx, int32_t object_idx,
                               float score, const rsd_mat4_t* pose );
int rsd_rsdb_parse_pose_line( const char* line, int32_t* uidx, int32_t* arrangement_idx, int32_t* object_idx,
                              float* score, rsd_mat4_t* pose );

/* The shim caches device uploads of host arrays by (pointers, count, content hash) — SURVEY.md §8b's "(pointer, n,
 * generation)" key.  Arrays of up to 4 MB each (RS_DROPIN_FULL_HASH_BELOW, bytes) are hashed whole on every call: an in-place
 * edit of any byte is seen.  Larger arrays are keyed by a ~1 KB sample and their full hash is re-checked on the first and then
 * every 16th hit: a caller that edits a LARGE array in place (same pointer, same count) MUST call rsd_cache_invalidate( ptr )
 * before the next call that passes it — or set RS_DROPIN_FULL_HASH=1 (environment: whole arrays hashed on every call, 40 us
 * per MB).  msh_hash_grid_term() invalidates what was built from its grid's array (the reference terminates a level's grid
 * right before it frees or rebuilds the level, lib/rs/rs_pointcloud.h:879-901); rsd_cache_clear drops everything.  A cached
 * cloud that a call is using stays alive until that call returns, whatever is evicted or invalidated meanwhile. */
void  rsd_cache_clear( void );
void  rsd_cache_invalidate( const void* host_array );

/* msh_hash_grid_radius_search calls that hit a HIP error on an initialised grid and were therefore answered from the grid's
 * host copy (the reference's search always fills its rows and counts, lib/msh/msh_hash_grid.h:1090-1259, and its callers
 * walk them; the first such call complains on stderr).  0 in a healthy run: tests assert it. */
unsigned long long rsd_device_failures( void );

#ifdef __cplusplus
}
#endif
#endif
