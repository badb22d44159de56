"""NumPy restatement of what include/rescan_hip.h documents for rs_hip_scene_saliency, rs_hip_coverage_create / _scores and
rs_hip_coverage_extensions: fp32 operations in the reference's order, integers from there on.  tests/test_arrange_cpu.py holds it
against the reference's own numbers (tests/golden/arrange_*.npz); tools/arrange_fixture/gen.py uses it to check that the fixtures
contain the cases they are meant to contain."""
import numpy as np

F = np.float32


def grid_shape(bbox_min, bbox_max, voxel):
    """isect_grid3d_init (lib/rs/intersect.h:59-75): (origin float32[3], res int[3])."""
    voxel = F(voxel)
    mn = np.asarray(bbox_min, F) - F(0.3)
    mx = np.asarray(bbox_max, F) + F(0.3)
    res = np.ceil((mx - mn) / voxel).astype(np.int64) + 1
    return mn, res


def xform(pose, pts):
    """msh_mat4_vec3_mul( pose, p, 1 ): column-major, products summed left to right in fp32."""
    m = np.asarray(pose, F).ravel()
    pts = np.asarray(pts, F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):                     # (0 * inf of a non-finite point: NaN, as in the reference)
        return np.stack([m[r] * pts[:, 0] + m[4 + r] * pts[:, 1] + m[8 + r] * pts[:, 2] + F(1.0) * m[12 + r] for r in range(3)], axis=1)


def cell_coords(origin, voxel, pts):
    """floorf( ( p - origin ) * ( 1.0f / voxel ) ) per axis (intersect.h:100-103), as integers.  A floor that no int32 holds (NaN,
    +-inf, beyond 2^31) becomes INT_MIN, as the reference's x86 conversion makes it: outside every grid."""
    inv = F(1.0) / F(voxel)
    with np.errstate(invalid="ignore"):
        f = np.floor((np.asarray(pts, F).reshape(-1, 3) - origin[None, :]) * inv)
        fits = np.abs(f) < F(2147483648.0)                     # (False for NaN)
    return np.where(fits, f, F(-2147483648.0)).astype(np.int64)


def cells(origin, res, voxel, pts):
    """isect_grid3d_cell_from_world_space (:97-109): the cell's index y * x_res * z_res + z * x_res + x, -1 outside the grid."""
    c = cell_coords(origin, voxel, pts)
    inside = ((c >= 0) & (c < res[None, :])).all(axis=1)
    idx = c[:, 1] * res[0] * res[2] + c[:, 2] * res[0] + c[:, 0]
    return np.where(inside, idx, -1)


def saliency(bbox_min, bbox_max, voxel, objects, prop_obj, prop_pose, prop_static, scene_pos, scene_class, wall, floor):
    """rsao__compute_scene_saliency_grid (arrangement_optimization.cpp:1109-1160): (grid uint8[n_cells], quality float32[n])."""
    origin, res = grid_shape(bbox_min, bbox_max, voxel)
    grid = np.zeros(int(res.prod()), np.uint8)
    for phase, value in ((0, 1), (1, 0)):                  # all dynamic proposals set, then all static ones clear (:1126-1131)
        for k in range(len(prop_obj)):
            if bool(prop_static[k]) != bool(phase):
                continue
            c = cells(origin, res, voxel, xform(prop_pose[k], objects[int(prop_obj[k])]))
            grid[c[c >= 0]] = value
    c = cells(origin, res, voxel, scene_pos)
    cls = np.asarray(scene_class)
    lit = np.zeros(len(c), bool)
    lit[c >= 0] = grid[c[c >= 0]] == 1
    quality = np.where((cls == wall) | (cls == floor), False, lit).astype(F)      # :1141-1154
    return grid, quality


def scene_grid(bbox_min, bbox_max, voxel, pos, quality, threshold):
    """rsao_rasterize_scene_to_grid (:1064-1079): uint8[n_cells]."""
    origin, res = grid_shape(bbox_min, bbox_max, voxel)
    grid = np.zeros(int(res.prod()), np.uint8)
    keep = np.ones(len(pos), bool) if quality is None else ~(np.asarray(quality, F) < F(threshold))
    c = cells(origin, res, voxel, np.asarray(pos, F)[keep])
    grid[c[c >= 0]] = 1
    return grid


def placement_cells(bbox_min, bbox_max, voxel, objects, placements):
    """The distinct cells rsao__rasterize_arrangement_to_grid (:1083-1106) lights: placements = (object, pose, is_static)."""
    origin, res = grid_shape(bbox_min, bbox_max, voxel)
    out = [np.zeros(0, np.int64)]
    for obj, pose, static in placements:
        if static:
            continue                                        # :1095-1096
        c = cells(origin, res, voxel, xform(pose, objects[int(obj)]))
        out.append(c[c >= 0])
    return np.unique(np.concatenate(out))


def score_of(agree, valid):
    """(float)agree / (float)valid, 0 when the scene grid has no valid cell (:366-368)."""
    return F(0.0) if valid == 0 else F(agree) / F(valid)


def coverage(scn_grid, bbox_min, bbox_max, voxel, objects, placements):
    """rsao__compute_scene_coverage_score (:344-373): (agree, valid, score)."""
    hit = placement_cells(bbox_min, bbox_max, voxel, objects, placements)
    agree = int((scn_grid[hit] > 0).sum())
    valid = int((scn_grid > 0).sum())
    return agree, valid, score_of(agree, valid)


def extensions(scn_grid, bbox_min, bbox_max, voxel, objects, base, candidates):
    """rs_hip_coverage_extensions as documented: (base_agree, fresh[C], agree[C], scores[C]); candidates = (object, pose)."""
    valid = int((scn_grid > 0).sum())
    base_hit = placement_cells(bbox_min, bbox_max, voxel, objects, base)
    base_hit = base_hit[scn_grid[base_hit] > 0]
    base_agree = len(base_hit)
    fresh = np.zeros(len(candidates), np.int64)
    for k, (obj, pose) in enumerate(candidates):
        c = placement_cells(bbox_min, bbox_max, voxel, objects, [(obj, pose, 0)])
        c = c[scn_grid[c] > 0]
        fresh[k] = len(np.setdiff1d(c, base_hit, assume_unique=True))
    agree = base_agree + fresh
    scores = np.array([score_of(int(a), valid) for a in agree], F)
    return base_agree, fresh, agree.astype(np.int32), scores


def live_box_bytes(scn_grid, bbox_min, bbox_max, voxel, objects, base, candidate):
    """Bytes of the bit sub-box rs_arrange.hip gives a candidate: the box of its cells that are scene-active and not hit by the base."""
    origin, res = grid_shape(bbox_min, bbox_max, voxel)
    base_hit = placement_cells(bbox_min, bbox_max, voxel, objects, base)
    obj, pose = candidate
    pts = xform(pose, objects[int(obj)])
    idx = cells(origin, res, voxel, pts)
    cc = cell_coords(origin, voxel, pts)[idx >= 0]
    idx = idx[idx >= 0]
    live = (scn_grid[idx] > 0) & ~np.isin(idx, base_hit)
    if not live.any():
        return 0
    ext = cc[live].max(0) - cc[live].min(0) + 1
    return int((int(ext.prod()) + 31) // 32 * 4)
