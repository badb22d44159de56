"""NumPy restatement of what include/rescan_hip.h documents for rs_hip_coverage_footprints and rs_hip_footprints_scores, on top of
tests/ao_restate.py: a placement's footprint is the sorted set of distinct scene-active cells its transformed points fall into; an
arrangement's agreeing cells are the union of its members' footprints.  tests/test_footprints_cpu.py holds the identity against the
reference's own numbers (tests/golden/arrange_*.npz)."""
import numpy as np

import ao_restate as R

F = np.float32


def footprint(scn_grid, bbox_min, bbox_max, voxel, objects, placement):
    """int32, ascending, duplicate-free: the cells of placement_cells (:1083-1106) that are active in the scene grid (:363-364).
    placement = (object, pose, is_static); a static placement has none (:1095-1096)."""
    c = R.placement_cells(bbox_min, bbox_max, voxel, objects, [placement])
    return c[scn_grid[c] > 0].astype(np.int32)


def union_score(footprints, members, valid):
    """(agree, score) of the arrangement whose placements are footprints[m] for m in members: :366-368."""
    agree = len(np.unique(np.concatenate([np.zeros(0, np.int32)] + [footprints[int(m)] for m in members])))
    return agree, R.score_of(agree, valid)


def footprint_box_bytes(scn_grid, bbox_min, bbox_max, voxel, objects, placement):
    """Bytes of the bit sub-box rs_arrange.hip gives a placement's footprint: the box of its scene-active cells, WITHOUT a base to
    exclude (ao_restate.live_box_bytes has one).  0: no such cell, no sub-box."""
    obj, pose, static = placement
    if static:
        return 0
    origin, res = R.grid_shape(bbox_min, bbox_max, voxel)
    pts = R.xform(pose, objects[int(obj)])
    idx = R.cells(origin, res, voxel, pts)
    cc = R.cell_coords(origin, voxel, pts)[idx >= 0]
    idx = idx[idx >= 0]
    act = scn_grid[idx] > 0
    if not act.any():
        return 0
    ext = cc[act].max(0) - cc[act].min(0) + 1
    return int((int(ext.prod()) + 31) // 32 * 4)


def csr(footprints):
    """(offsets int64[n + 1], cells int32) of a list of footprints."""
    off = np.zeros(len(footprints) + 1, np.int64)
    off[1:] = np.cumsum([len(f) for f in footprints])
    return off, np.concatenate([np.zeros(0, np.int32)] + list(footprints)).astype(np.int32)
