"""NumPy restatement of the voxel overlap and the non-maximum suppression the library runs on the GPU
(include/rescan_hip.h: rs_hip_overlap_factors, rs_hip_nms; the reference's lib/rs/intersect.h:59-368 and
apps/pose_proposal/pose_proposal.cpp:377-451), in float32 with the reference's operations in their order.  The scanline
parities are cumulative sums here and prefix-XORs of words on the device: two statements of the same count."""
import numpy as np

F = np.float32


class OutsideGrid(Exception):
    pass


class LineTooLong(Exception):
    pass


def xform(pose16, pts):
    """msh_mat4_vec3_mul of points: m0 x + m4 y + m8 z + 1 m12, every operation rounded to float32."""
    m = np.asarray(pose16, F)
    x, y, z = (np.ascontiguousarray(pts[:, k], F) for k in range(3))
    return np.stack([m[r] * x + m[4 + r] * y + m[8 + r] * z + F(1.0) * m[12 + r] for r in range(3)], axis=1)


def box(pose16, extent):
    q = xform(pose16, extent)
    lo = np.minimum(F(1e9), q.min(axis=0)) if len(q) else np.full(3, 1e9, F)
    hi = np.maximum(F(-1e9), q.max(axis=0)) if len(q) else np.full(3, -1e9, F)
    return lo.astype(F), hi.astype(F)


def boxes_intersect(a, b):
    return bool(np.all(a[1] >= b[0]) and np.all(b[1] >= a[0]))


def grid_of(box_a, box_b, voxel):
    lo = np.minimum(np.minimum(box_a[0], box_a[1]), np.minimum(box_b[0], box_b[1]))
    hi = np.maximum(np.maximum(box_a[0], box_a[1]), np.maximum(box_b[0], box_b[1]))
    lo = np.minimum(F(1e9), lo).astype(F) - F(0.3)
    hi = np.maximum(F(-1e9), hi).astype(F) + F(0.3)
    res = (np.ceil((hi - lo) / F(voxel)).astype(np.int64) + 1)
    return lo, res          # origin, (x_res, y_res, z_res)


def cells(pose16, boundary, origin, voxel):
    o = xform(pose16, boundary) - origin[None, :]
    with np.errstate(invalid="ignore"):
        f = np.floor(o / F(voxel))
        fits = np.abs(f) < F(2147483648.0)                 # (False for NaN: no cell of any grid, like a floor beyond int32)
    return np.where(fits, f, F(-1.0)).astype(np.int64)


def boundary_grid(pose16, boundary, origin, res, voxel):
    c = cells(pose16, boundary, origin, voxel)
    if len(c) and (np.any(c < 0) or np.any(c >= res[None, :])):
        raise OutsideGrid()
    g = np.zeros((res[1], res[2], res[0]), bool)          # [y, z, x]
    g[c[:, 1], c[:, 2], c[:, 0]] = True
    return g


def parities(b, axis):
    """(forward, backward): per cell, whether an odd number of "FREE directly after BOUNDARY" transitions lies at or before it,
    counted from the low end and from the high end of its line along `axis` (intersect.h:126-161)."""
    prev = np.roll(b, 1, axis=axis)
    idx = [slice(None)] * 3
    idx[axis] = 0
    prev[tuple(idx)] = False
    nxt = np.roll(b, -1, axis=axis)
    idx[axis] = -1
    nxt[tuple(idx)] = False
    fwd = np.cumsum(~b & prev, axis=axis) % 2 == 1
    tb = ~b & nxt
    bwd = np.flip(np.cumsum(np.flip(tb, axis), axis=axis), axis) % 2 == 1
    return fwd, bwd


def _inside_along(b, axis):
    fwd, bwd = parities(b, axis)
    return ~b & fwd & bwd


def occupancy(b):
    """(boundary | inside) of isect_compute_occupancy_grid: inside = both scan directions of the y slice say inside."""
    return b | (_inside_along(b, 2) & _inside_along(b, 1))


def overlap(shape_a, pose_a, shape_b, pose_b, voxel, inside, by_smaller):
    """shape = (boundary [n, 3], extent [m, 3]).  Returns (overlap float32, (count_a, count_b, both))."""
    ba, bb = box(pose_a, shape_a[1]), box(pose_b, shape_b[1])
    if not boxes_intersect(ba, bb):
        return F(0.0), (0, 0, 0)
    origin, res = grid_of(ba, bb, voxel)
    if inside and (res[0] > 4096 or res[2] > 4096):
        raise LineTooLong()
    ga = boundary_grid(pose_a, shape_a[0], origin, res, voxel)
    gb = boundary_grid(pose_b, shape_b[0], origin, res, voxel)
    if inside:
        ga, gb = occupancy(ga), occupancy(gb)
    ca, cb, both = int(ga.sum()), int(gb.sum()), int((ga & gb).sum())
    denom = min(ca, cb) if by_smaller else max(ca, cb)
    return (F(both) / F(denom) if denom > 0 else F(1.0)), (ca, cb, both)


def nms(shape, centroid, poses, scores, dist_threshold, trace=None):
    """marks (1 keep, 2 discard), keep_idx, rounds, and the discards that overlap alone decided.  `trace` (a list) receives
    (round, i, grid resolution or None) for every pair the cheap tests leave to the overlap."""
    n = len(scores)
    scores = np.asarray(scores, F)
    if n and not np.all(scores > F(-1e9)):
        raise ValueError("score NaN or <= -1e9")
    marks = np.zeros(n, np.int32)
    cen = np.stack([xform(poses[i], np.asarray(centroid, F)[None, :])[0] for i in range(n)]) if n else np.zeros((0, 3), F)
    rounds, alone = 0, []
    while (marks == 0).any():
        best, best_score = -1, F(-1e9)
        for i in range(n):
            if marks[i] == 0 and scores[i] > best_score:
                best, best_score = i, scores[i]
        marks[best] = 1
        rounds += 1
        for i in np.flatnonzero(marks == 0):
            d = cen[best] - cen[i]
            dist = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2], dtype=F)
            if dist < F(dist_threshold) or scores[i] < F(0.01):
                marks[i] = 2
                continue
            if trace is not None:
                ba, bb = box(poses[best], shape[1]), box(poses[i], shape[1])
                trace.append((rounds, int(i), grid_of(ba, bb, F(0.1))[1] if boxes_intersect(ba, bb) else None))
            ov, _ = overlap(shape, poses[best], shape, poses[i], F(0.1), 1, 0)
            if ov > F(0.5):
                marks[i] = 2
                alone.append(int(i))
    return marks, np.flatnonzero(marks == 1).astype(np.int32), rounds, alone
