"""NumPy restatement of the pose search's host planner and bookkeeping (include/rescan_hip.h: rs_hip_pose_grid_plan,
rs_hip_cell_best, rs_hip_verify_marks, the final copy of rs_hip_propose_poses), written from the reference's loops
(apps/pose_proposal/pose_proposal.cpp:203-242, 283-297, 347-359) in explicit float32 / float64.  Scores are inputs here: where they
come from (the reference's lists, capi.alignment_scores) is the caller's choice."""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in (_libm.sinf, _libm.cosf):
    _f.restype, _f.argtypes = ctypes.c_float, [ctypes.c_float]
TWO_PI_LITERAL = np.float64(6.2831853072)        # MSH_TWO_PI, a double literal (lib/msh/msh_std.h:619)


def offsets(length, spacing):
    """for( float o = -spacing; o < length + spacing; o += spacing ) — counter, bound and compare in float32 (:213, :215)."""
    length, spacing = F(length), F(spacing)
    bound = F(length + spacing)
    out, o = [], F(-spacing)
    while o < bound:
        out.append(o)
        o = F(o + spacing)
    return np.array(out, F)


def yaw_angles(angle_delta):
    """for( float a = 0.0f; a < MSH_TWO_PI; a += delta ) — a float32 counter compared in float64 (:219)."""
    d = F(angle_delta)
    out, a = [], F(0.0)
    while np.float64(a) < TWO_PI_LITERAL:
        out.append(a)
        a = F(a + d)
    return np.array(out, F)


def rotate_y(angle, sin=None, cos=None):
    """msh_rotate( identity, angle, (0, 1, 0) ) (lib/msh/msh_vec_math.h:2089-2132), column-major float32[16].  sin / cos default to
    the host libm's sinf / cosf, which is what the reference calls (numpy's float32 loops are not libm's)."""
    s = F(_libm.sinf(float(F(angle)))) if sin is None else F(sin)
    c = F(_libm.cosf(float(F(angle)))) if cos is None else F(cos)
    t = F(F(1.0) - c)
    ax = (F(0.0), F(1.0), F(0.0))
    R = np.zeros(9, F)
    R[0] = F(c + F(F(ax[0] * ax[0]) * t)); R[4] = F(c + F(F(ax[1] * ax[1]) * t)); R[8] = F(c + F(F(ax[2] * ax[2]) * t))
    p, q = F(F(ax[0] * ax[1]) * t), F(ax[2] * s); R[1] = F(p + q); R[3] = F(p - q)
    p, q = F(F(ax[0] * ax[2]) * t), F(ax[1] * s); R[2] = F(p - q); R[6] = F(p + q)
    p, q = F(F(ax[1] * ax[2]) * t), F(ax[0] * s); R[5] = F(p + q); R[7] = F(p - q)
    a = np.eye(4, dtype=F).T.ravel()            # identity, column-major
    o = a.copy()
    for j in range(3):
        for r in range(4):
            o[4 * j + r] = F(F(a[r] * R[3 * j]) + F(F(a[4 + r] * R[3 * j + 1]) + F(a[8 + r] * R[3 * j + 2])))
    return o


def grid_plan(bbox_min, bbox_max, spacing, angle_delta):
    lo, hi = np.asarray(bbox_min, F), np.asarray(bbox_max, F)
    ox, oz = offsets(F(hi[0] - lo[0]), spacing), offsets(F(hi[2] - lo[2]), spacing)
    ang = yaw_angles(angle_delta)
    yaw = np.stack([rotate_y(a) for a in ang]) if len(ang) else np.zeros((0, 16), F)
    return ox, oz, yaw


def grid_poses(bbox_min, height, ox, oz, yaw):
    """Every pose of the grid in the reference's order: x outer, z inner, yaw innermost (:213-222)."""
    lo = np.asarray(bbox_min, F)
    P = np.zeros((len(ox), len(oz), len(yaw), 16), F)
    P[:] = yaw[None, None, :, :]
    P[..., 12] = (lo[0] + ox)[:, None, None]
    P[..., 13] = F(height)
    P[..., 14] = (lo[2] + oz)[None, :, None]
    P[..., 15] = F(1.0)
    return P.reshape(-1, 16)


def cell_best(scores, threshold):
    """Per cell: best from 0 by strict > in yaw order; keep = the proposing cells' slots, -1 elsewhere (:217-242)."""
    scores = np.asarray(scores, F)
    n_cells, n_yaw = scores.shape
    by, bs, keep = np.full(n_cells, -1, np.int32), np.zeros(n_cells, F), np.full(n_cells, -1, np.int32)
    slot = 0
    for c in range(n_cells):
        best, arg = F(0.0), -1
        for k in range(n_yaw):
            if scores[c, k] > best:
                best, arg = scores[c, k], k
        by[c], bs[c] = arg, best
        if best > F(threshold):
            keep[c] = slot
            slot += 1
    return by, bs, keep


def verify_marks(old, new, threshold):
    """:283-297 — only entries > 0 are scored again; each becomes new > threshold ? new : -1."""
    old, new = np.asarray(old, F), np.asarray(new, F)
    out = old.copy()
    for i in range(len(old)):
        if old[i] > F(0.0):
            out[i] = new[i] if new[i] > F(threshold) else F(-1.0)
    return out


def final_copy(poses, scores):
    """:347-359 — every entry with fabsf( score ) > 0.000001f, in order (the -1 marks among them)."""
    scores = np.asarray(scores, F)
    m = np.abs(scores) > F(0.000001)
    return np.asarray(poses, F).reshape(-1, 16)[m], scores[m]


def cascade(score_fn, n_levels, bbox_min, bbox_max, spacing, angle_delta, height, thresholds):
    """The whole search of one object composed on the host: score_fn( level, poses ) -> float32 scores.  Returns the final
    (poses, scores) and per level (n_scored, n_kept) with n_kept = the entries > 0 after the level."""
    ox, oz, yaw = grid_plan(bbox_min, bbox_max, spacing, angle_delta)
    P = grid_poses(bbox_min, height, ox, oz, yaw)
    n_cells = len(ox) * len(oz)
    s0 = np.asarray(score_fn(0, P), F).reshape(n_cells, len(yaw))
    by, bs, keep = cell_best(s0, thresholds[0])
    cells = np.flatnonzero(keep >= 0)
    poses = np.stack([P[c * len(yaw) + by[c]] if by[c] >= 0 else np.zeros(16, F) for c in cells]) if len(cells) else np.zeros((0, 16), F)
    scores = bs[cells].copy()
    trace = [(len(P), int((scores > 0).sum()))]
    for l in range(1, n_levels):
        act = np.flatnonzero(scores > F(0.0))
        new = np.zeros(len(scores), F)
        if len(act):
            new[act] = np.asarray(score_fn(l, poses[act]), F)
        scores = verify_marks(scores, new, thresholds[l])
        trace.append((len(act), int((scores > 0).sum())))
    fp, fs = final_copy(poses, scores)
    return fp, fs, trace, (poses, scores)
