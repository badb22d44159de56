// FIXTURE GENERATION ONLY — not product code, not run by any test.
//
// A flat C interface over the reference's own functions, for tools/split_fixture/gen.py.  This file includes the reference's
// apps/seg2rsdb/main.cpp by path (gen.py renames its main on the command line) and only CALLS its functions:
//   fx_split     pointcloud_to_rsdb itself (apps/seg2rsdb/main.cpp:45-159) on a level 0 assembled from the scan's seven arrays, with the
//                class table rsdb_load reads from the file gen.py wrote; then the objects' level-0 arrays, uidx and class_idx, and
//                the placements' poses, read back from the database it filled.
//   fx_centroid  what pointcloud_to_rsdb does between :113 and :126 for one instance id, statement by statement, to read out the two
//                values it does not keep: rs_pointcloud_copy_by_ids, rs_pointcloud_centroid (before centroid.y = 0), and
//                msh_translate( msh_mat4_identity(), msh_vec3_invert( centroid ) ) after it; with the transformed positions and
//                normals of rs_pointcloud_transform and msh_mat4_inverse of the transform.  gen.py checks them against fx_split.
#include "apps/seg2rsdb/main.cpp"

// the seven arrays of one level
struct fx_arrays { float* pos; float* nor; float* col; float* radii; float* qual; int32_t* cls; int32_t* inst; };

static rs_pointcloud_t* fx_cloud( const fx_arrays* a, int64_t n )
{
  rs_pointcloud_t* pc = rs_pointcloud_init( 1 );
  rs_pointcloud__allocate_level( pc, 0, (int32_t)n );
  memcpy( pc->positions[0], a->pos, n * 12 );
  memcpy( pc->normals[0], a->nor, n * 12 );
  memcpy( pc->colors[0], a->col, n * 12 );
  memcpy( pc->radii[0], a->radii, n * 4 );
  memcpy( pc->qualities[0], a->qual, n * 4 );
  memcpy( pc->class_ids[0], a->cls, n * 4 );
  memcpy( pc->instance_ids[0], a->inst, n * 4 );
  return pc;
}

extern "C" {

// Returns the number of objects (their arrays concatenated in out, counts[k] points each), or -1 when the class table cannot be
// read, -2 when there are more than `capacity`.  seconds: pointcloud_to_rsdb alone.
int32_t fx_split( const char* class_table, const fx_arrays* scan, int64_t n, int32_t capacity, int32_t* inst_ids, int32_t* class_of,
                  int64_t* counts, float* poses, const fx_arrays* out, double* seconds )
{
  rsdb_t* in_rsdb = rsdb_init();
  rsdb_t* out_rsdb = rsdb_init();
  if( rsdb_load( in_rsdb, class_table, 0 ) ) return -1;
  rs_pointcloud_t* pointcloud = fx_cloud( scan, n );
  options_t opts;
  opts.in_ply_filename = (char*)"scan.ply"; opts.in_rsdb_filename = (char*)class_table; opts.out_rsdb_filename = (char*)"out.rsdb"; opts.print_verbose = 0;
  const uint64_t t0 = msh_time_now();
  pointcloud_to_rsdb( in_rsdb, pointcloud, out_rsdb, &opts );
  *seconds = msh_time_diff_ms( msh_time_now(), t0 ) * 1e-3;
  const int32_t n_obj = (int32_t)msh_array_len( out_rsdb->objects );
  if( n_obj > capacity ) return -2;
  size_t at = 0;
  for( int32_t k = 0; k < n_obj; ++k )
  {
    const rs_object_t* obj = &out_rsdb->objects[k];
    const rs_obj_plcmnt_t* plc = &out_rsdb->arrangements[0][k];
    const size_t m = obj->shape->n_pts[0];
    inst_ids[k] = obj->uidx; class_of[k] = obj->class_idx; counts[k] = (int64_t)m;
    memcpy( poses + 16 * k, plc->pose.data, 64 );
    memcpy( out->pos + 3 * at, obj->shape->positions[0], m * 12 );
    memcpy( out->nor + 3 * at, obj->shape->normals[0], m * 12 );
    memcpy( out->col + 3 * at, obj->shape->colors[0], m * 12 );
    memcpy( out->radii + at, obj->shape->radii[0], m * 4 );
    memcpy( out->qual + at, obj->shape->qualities[0], m * 4 );
    memcpy( out->cls + at, obj->shape->class_ids[0], m * 4 );
    memcpy( out->inst + at, obj->shape->instance_ids[0], m * 4 );
    at += m;
  }
  return n_obj;
}

// One instance, dynamic: centroid (3, as rs_pointcloud_centroid returns it), xform and pose (16 each), pos / nor (3 per point of the
// instance) after rs_pointcloud_transform.  Returns the instance's point count.
int64_t fx_centroid( const fx_arrays* scan, int64_t n, int32_t id, float* centroid_out, float* xform_out, float* pose_out, float* pos, float* nor )
{
  rs_pointcloud_t* pointcloud = fx_cloud( scan, n );
  rs_pointcloud_t* shape = rs_pointcloud_copy_by_ids( pointcloud, 0, RS_PT_INSTANCE_ID, &id, 1, 0 );
  if( !shape ) return 0;
  msh_vec3_t centroid = rs_pointcloud_centroid( shape, 0 );
  memcpy( centroid_out, &centroid, 12 );
  centroid.y = 0;
  msh_mat4_t xform = msh_translate( msh_mat4_identity(), msh_vec3_invert( centroid ) );
  rs_pointcloud_transform( shape, xform, 0 );
  msh_mat4_t pose = msh_mat4_inverse( xform );
  memcpy( xform_out, xform.data, 64 ); memcpy( pose_out, pose.data, 64 );
  const size_t m = shape->n_pts[0];
  memcpy( pos, shape->positions[0], m * 12 ); memcpy( nor, shape->normals[0], m * 12 );
  return (int64_t)m;
}

} // extern "C"
