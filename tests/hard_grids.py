"""Seeded scenes, objects and search boxes on which the pose search (rs_hip_propose_poses) is easy to get subtly wrong, for
tests/test_hard_grids_cpu.py (what the cases are, by the oracle) and tests/test_gpu_hard_grids.py (what the device makes of them).
NumPy only, deterministic, small: a scene has about 6 000 points, an object level 9 to 3 000, a grid a few hundred to a few thousand
poses (one case, `chunk`, passes 65 535).

The scene is a floor (y = 0, normals +y), a wall (x = 0, normals +x, 0.6 m high) and two instances of the object standing on the
floor, one under the grid's first rotation and one under its fourth.  The object is an L-shaped solid (0.5 x 0.4 m foot with a
quarter cut out, 0.3 m high: no rotation maps it onto itself, so the yaw maxima of a cell are not tied by symmetry) sampled on its
top, its six sides and a `lip`, a copy of the foot 3 cm above the ground facing up: the lip matches the floor wherever the object
stands in the room (a score of about the lip's share of the points), the rest only where an instance stands.

A case is a dict:
  scene_pos, scene_nor                 (n, 3) float32
  objects                              per object a list of levels, coarsest first, each (pos, nor); a level may have 0 points
  bbox_min, bbox_max, spacing, angle_delta, height, thresholds (one per level), radius (0.1), max_n_neigh (64)
  object_cell                          the cell_size the object clouds are made with (-1: their own grid; 0: the brute layout, for
                                       which the search has no query box of its own)
  margin                               True where the tests also hold the device to the oracle scorer (the CPU test bounds how
                                       close the oracle's scores come to a decision)
  plan                                 (n_x, n_z, n_yaw) the planner must give
`ties` gets its thresholds from scores (tie_thresholds), so it ties under whichever scorer the test runs."""
import functools

import numpy as np

import propose_restate as R

F = np.float32
RADIUS, MAX_N_NEIGH = 0.1, 64
SCORE_TOL = 2e-6                                                             # as tests/test_gpu_hard_clouds.py
DELTA10 = F(np.float64(6.2831853072) / np.float64(F(10.0)))                  # the application's step: 10 rotations
ROOM = (1.6, 0.6, 1.2)
HEIGHT_OBJ = 0.3
# the L's sides: (x0, z0, x1, z1, normal)
_SIDES = ((-0.25, -0.2, 0.25, -0.2, (0, 0, -1)), (0.25, -0.2, 0.25, 0.0, (1, 0, 0)), (0.0, 0.0, 0.25, 0.0, (0, 0, 1)),
          (0.0, 0.0, 0.0, 0.2, (1, 0, 0)), (-0.25, 0.2, 0.0, 0.2, (0, 0, 1)), (-0.25, -0.2, -0.25, 0.2, (-1, 0, 0)))

MARGIN = ("base", "offset", "overhang", "inside")
SHAPES = ("smallest", "cells_255", "cells_256", "cells_258", "cells_510", "cells_512", "cells_513", "yaw_1", "yaw_2")
PLACEMENTS = ("tall_clear", "tall_low", "brute_object")
THRESHOLDS = ("ties", "negative", "zero", "four_levels", "repeated")
CASES = MARGIN + PLACEMENTS + SHAPES + ("inside_out", "chunk") + THRESHOLDS + ("batch",)


def _foot(rng, m):
    """m points uniform over the L's foot (x, z)."""
    out = np.zeros((0, 2))
    while len(out) < m:
        c = rng.uniform((-0.25, -0.2), (0.25, 0.2), (2 * m + 8, 2))
        out = np.concatenate([out, c[~((c[:, 0] > 0.0) & (c[:, 1] > 0.0))]])
    return out[:m]


def l_solid(seed, n, lip=0.25, lift=0.0):
    """n points of the L-shaped solid in its own frame (the foot's box centred on the origin, standing on y = lift)."""
    rng = np.random.default_rng([seed, n])
    n_lip = int(round(n * lip)) if lip > 0 else 0
    n_top = max(1, int(round(n * 0.35)))
    n_side = n - n_lip - n_top
    assert n_side >= 1
    pos, nor = np.zeros((n, 3)), np.zeros((n, 3))
    f = _foot(rng, n_lip + n_top)
    pos[:n_lip + n_top, 0], pos[:n_lip + n_top, 2] = f[:, 0], f[:, 1]
    pos[:n_lip, 1], pos[n_lip:n_lip + n_top, 1] = 0.03, HEIGHT_OBJ
    nor[:n_lip + n_top, 1] = 1.0
    length = np.array([abs(s[2] - s[0]) + abs(s[3] - s[1]) for s in _SIDES])
    which = rng.choice(len(_SIDES), n_side, p=length / length.sum())
    t = rng.uniform(0.0, 1.0, n_side)
    for k, j in enumerate(which):
        x0, z0, x1, z1, nn = _SIDES[j]
        pos[n_lip + n_top + k] = (x0 + t[k] * (x1 - x0), rng.uniform(0.0, HEIGHT_OBJ), z0 + t[k] * (z1 - z0))
        nor[n_lip + n_top + k] = nn
    pos[:, 1] += lift
    o = rng.permutation(n)
    return np.ascontiguousarray(pos[o], F), np.ascontiguousarray(nor[o], F)


def _placed(pos, nor, yaw16, t):
    M = np.asarray(yaw16, np.float64).reshape(4, 4).T[:3, :3]
    return pos.astype(np.float64) @ M.T + np.asarray(t, np.float64), nor.astype(np.float64) @ M.T


def room(seed=0, offset=(0.0, 0.0, 0.0)):
    """The scene, moved by `offset` in float64 before it is narrowed to float32."""
    rng = np.random.default_rng([seed, 1])
    w, h, d = ROOM
    floor = np.stack([rng.uniform(0, w, 2500), np.zeros(2500), rng.uniform(0, d, 2500)], 1)
    wall = np.stack([np.zeros(900), rng.uniform(0, h, 900), rng.uniform(0, d, 900)], 1)
    yaw = R.grid_plan((0, 0, 0), (1, 1, 1), 0.1, DELTA10)[2]
    a = _placed(*l_solid(seed + 100, 1200, lip=0.0), yaw[0], (0.513, 0.0, 0.477))
    b = _placed(*l_solid(seed + 101, 1200, lip=0.0), yaw[3], (1.15, 0.0, 0.78))
    pos = np.concatenate([floor, wall, a[0], b[0]]) + np.asarray(offset, np.float64)
    nor = np.concatenate([np.tile((0.0, 1.0, 0.0), (2500, 1)), np.tile((1.0, 0.0, 0.0), (900, 1)), a[1], b[1]])
    o = rng.permutation(len(pos))
    return np.ascontiguousarray(pos[o], F), np.ascontiguousarray(nor[o], F)


def length_for(steps, spacing):
    """A box length for which R.offsets gives `steps` steps (>= 2)."""
    length = F((steps - 2.5) * float(F(spacing)))
    assert len(R.offsets(length, spacing)) == steps, (steps, spacing)
    return float(length)


def levels(seed, sizes, lip=0.25, lift=0.0):
    return [l_solid(seed + 7 * l, n, lip, lift) if n > 0 else (np.zeros((0, 3), F), np.zeros((0, 3), F)) for l, n in enumerate(sizes)]


def _box_of_cells(lo, n_x, n_z, spacing, y=(0.0, ROOM[1])):
    lo = np.array([lo[0], y[0], lo[1]], np.float64)
    hi = lo + np.array([length_for(n_x, spacing), y[1] - y[0], length_for(n_z, spacing)])
    return lo.astype(F), hi.astype(F)


@functools.lru_cache(maxsize=None)
def make(name):
    scene = room()
    c = dict(name=name, objects=[levels(11, (300, 600, 1200))], bbox_min=np.zeros(3, F), bbox_max=np.array(ROOM, F), spacing=0.1,
             angle_delta=DELTA10, height=0.0, thresholds=np.array([0.3, 0.4, 0.5], F), radius=RADIUS, max_n_neigh=MAX_N_NEIGH,
             object_cell=-1.0, margin=name in MARGIN)
    if name == "base":
        pass
    elif name == "offset":
        # 1e4 m out with mixed signs, as tests/hard_clouds.py: the query box's relative pad 1e-5 |q| is then 0.1 m, and a
        # coordinate's rounding 2^-11 m
        off = np.array([1e4 + 0.3, -1e4 - 0.7, -5e3 + 0.1])
        scene = room(offset=off)
        c.update(bbox_min=off.astype(F), bbox_max=(off + np.array(ROOM)).astype(F), height=float(F(off[1])))
    elif name == "overhang":
        # half a metre of cells beyond the scene on every side: whole rows of cells whose queries all lie outside the scene's
        # box grown by the radius, and rows that straddle it
        c.update(bbox_min=np.array([-0.5, 0.0, -0.5], F), bbox_max=np.array([ROOM[0] + 0.5, ROOM[1], ROOM[2] + 0.5], F))
    elif name == "inside":
        # a box of 6 cm around the first instance: the object's box under the rotations is ten times the grid
        c.update(bbox_min=np.array([0.49, 0.0, 0.45], F), bbox_max=np.array([0.55, 0.3, 0.51], F), spacing=0.02)
    elif name == "tall_clear":
        c.update(height=2.0)                                     # nothing of the object within the radius of anything
    elif name == "tall_low":
        # the object stands 5 cm above the wall's top: only the lowest 5 cm of its sides can match (the wall's upper edge), and
        # only where they face the way the wall does
        c.update(height=ROOM[1] + 0.05, thresholds=np.array([0.002, 0.002, 0.002], F))
    elif name == "brute_object":
        c.update(object_cell=0.0)
    elif name == "smallest":
        c.update(bbox_min=np.array([0.5, 0.0, 0.45], F), bbox_max=np.array([0.5, 0.3, 0.45], F))   # length 0: two steps per axis
    elif name.startswith("cells_"):
        n_x, n_z = {255: (15, 17), 256: (16, 16), 258: (6, 43), 510: (17, 30), 512: (16, 32), 513: (19, 27)}[int(name[6:])]
        lo, hi = _box_of_cells((0.0, -0.2), n_x, n_z, 0.05)
        c.update(bbox_min=lo, bbox_max=hi, spacing=0.05, objects=[levels(12, (40, 80, 160))], thresholds=np.array([0.2, 0.3, 0.4], F))
    elif name == "yaw_1":
        c.update(angle_delta=7.0, thresholds=np.array([0.2, 0.3, 0.4], F))
    elif name == "yaw_2":
        c.update(angle_delta=3.5, thresholds=np.array([0.2, 0.3, 0.4], F))
    elif name == "inside_out":
        c.update(bbox_min=np.array([1.0, 0.0, 0.0], F), bbox_max=np.array([0.5, 0.6, 1.2], F))     # length -0.5 <= -2 spacings
    elif name == "chunk":
        # 100 x 66 cells of 1.5 cm, all of them over the floor: the poses before 65 535 and the 465 after it all score, so a
        # chunk that lands in the wrong place shows
        lo, hi = _box_of_cells((0.05, 0.1), 100, 66, 0.015)
        c.update(bbox_min=lo, bbox_max=hi, spacing=0.015, objects=[levels(13, (9, 18, 36))], thresholds=np.array([0.25, 0.3, 0.35], F))
    elif name == "ties":
        c.update(thresholds=np.array([-1.0, -1.0, -1.0], F))     # permissive; the test replaces them by tie_thresholds
    elif name == "negative":
        c.update(thresholds=np.array([-0.5, 0.4, 0.5], F), bbox_min=np.array([-0.5, 0.0, -0.5], F))
    elif name == "zero":
        c.update(thresholds=np.zeros(3, F), bbox_min=np.array([-0.5, 0.0, -0.5], F))
    elif name == "four_levels":
        c.update(objects=[levels(14, (40, 300, 600, 1200))], thresholds=np.array([0.25, 0.3, 0.4, 0.5], F))
    elif name == "repeated":
        lv = levels(11, (300, 600, 1200))
        c.update(objects=[[lv[0], lv[1], lv[1]]], thresholds=np.array([0.3, 0.4, 0.45], F))
    elif name == "batch":
        # ragged sizes in one call.  `floating` hangs 2 m up in its own frame: nothing is proposed at level 0.  `hollow` has no
        # points at its middle level: every proposal becomes -1 there and level 2 has nothing to score.  `big` has a thin lip (it
        # proposes near the instances only: a short list), `mid` a thick one (every cell on the floor proposes: a long one).
        objs = [levels(21, (9, 18, 36), lip=0.3), levels(22, (40, 80, 160), lift=2.0), levels(23, (600, 900, 1200), lip=0.4),
                levels(24, (3000, 3000, 3000), lip=0.1), levels(25, (200, 0, 400), lip=0.4)]
        c.update(objects=objs, names=("tiny", "floating", "mid", "big", "hollow"), spacing=0.08, angle_delta=3.5,
                 thresholds=np.array([0.25, 0.3, 0.35], F))
    else:
        raise KeyError(name)
    c["scene_pos"], c["scene_nor"] = scene
    c["plan"] = tuple(len(t) for t in R.grid_plan(c["bbox_min"], c["bbox_max"], c["spacing"], c["angle_delta"]))
    return c


def args_of(c, thresholds=None):
    thr = c["thresholds"] if thresholds is None else np.asarray(thresholds, F)
    return (c["bbox_min"], c["bbox_max"], c["spacing"], c["angle_delta"], c["height"], thr, c["radius"], c["max_n_neigh"])


def cascade(c, score_fn, o=0, thresholds=None):
    """R.cascade of object o of the case over score_fn( level, poses ) -> float32 scores."""
    a = args_of(c, thresholds)
    return R.cascade(score_fn, len(a[5]), *a[:6])


def oracle_scorer(oracle, c, o=0, log=None):
    """score_fn of object o over the oracle's alignment score; log (a list) receives (level, poses, scores)."""
    grid = oracle.grid_create(c["scene_pos"], 0.05)

    def score(l, P):
        pos, nor = c["objects"][o][l]
        s = oracle.alignment_scores(c["scene_pos"], c["scene_nor"], pos, nor, P, c["max_n_neigh"], scene_grid=grid) if len(P) else np.zeros(0, F)
        if log is not None:
            log.append((l, np.array(P, F), s.copy()))
        return s
    return score


def tie_thresholds(c, score_fn, o=0):
    """Per level the median of the scores > 0 that the level meets under thresholds that drop nothing: a score that occurs.  With
    it as the threshold, strict > drops exactly the entries that equal it (and those below).  Later levels are scored under the
    earlier levels' tie thresholds, so the entries they tie with are entries they meet.  (A batch is scored once: the scorer is
    asked again only for poses it has not seen.)"""
    thr = np.full(len(c["thresholds"]), -1.0, F)
    seen = {}
    for l in range(len(thr)):
        log = []

        def fn(k, P):
            key = (k, np.asarray(P, F).tobytes())
            if key not in seen:
                seen[key] = np.asarray(score_fn(k, P), F)
            log.append((k, seen[key]))
            return seen[key]
        cascade(c, fn, o, thr)
        s = [s for k, s in log if k == l][0]
        if l == 0:
            s = R.cell_best(s.reshape(-1, c["plan"][2]), -1.0)[1]
        s = np.sort(s[s > 0])
        thr[l] = s[len(s) // 2]
    return thr


def cells_of(c, poses):
    """The grid cell (x-outer, z-inner) of every listed pose, from its translation."""
    ox, oz, _ = R.grid_plan(c["bbox_min"], c["bbox_max"], c["spacing"], c["angle_delta"])
    tx, tz = c["bbox_min"][0] + ox, c["bbox_min"][2] + oz
    ix, iz = np.searchsorted(tx, poses[:, 12]), np.searchsorted(tz, poses[:, 14])
    assert (tx[ix] == poses[:, 12]).all() and (tz[iz] == poses[:, 14]).all()
    return ix * len(oz) + iz


def undecided_cells(c, s0, threshold):
    """Cells that propose under the oracle's level-0 scores s0 (n_cells, n_yaw) and whose runner-up rotation is within
    2 * SCORE_TOL of the best: the device may pick the other one."""
    s = np.where(np.isnan(s0), -np.inf, s0.astype(np.float64))
    if s.shape[1] < 2:
        return np.zeros(0, np.int64), int((s.max(axis=1) > threshold).sum()) if s.size else 0
    top = np.sort(s, axis=1)[:, -2:]
    proposing = top[:, 1] > threshold
    return np.flatnonzero(proposing & (top[:, 1] - top[:, 0] < 2 * SCORE_TOL)), int(proposing.sum())
