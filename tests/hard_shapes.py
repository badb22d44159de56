"""Deterministic hostile shapes for the voxel overlap, the non-maximum suppression and the arrangement kernels (rs_isect.hip,
rs_arrange.hip).  NumPy only, seeded, no device.  Every cloud is an integer lattice times one fp32 step (the centre of cell c of
a grid whose fattened margin holds m cells is ( 2 ( c - m ) + 1 ) * ( voxel / 2 )), so the same bytes come out on any machine;
tests/golden/isect_hard.npz stores each cloud's length and CRC, not the cloud.

A CASE is one call of rs_hip_overlap_factors: shapes [(boundary, extent)], pairs (shape_a, pose_a, shape_b, pose_b), one voxel and
one (voxelize_inside, normalize_by_smaller); `expect` is "ok", "capacity" (a line of more than 4096 cells) or "outside".  The extent
cloud sets the grid: with res = ceil( ( hi - lo + 0.6 ) / voxel ) + 1 an extent of ( T - 1.5 ) * voxel - 0.6 gives T cells."""
import functools
import zlib

import numpy as np

F = np.float32
I16 = np.eye(4, dtype=F).ravel()
# cos / sin of k * 2 pi / 10 as float32 literals (no libm at test time)
_C = [1.0, 0.80901699, 0.30901699, -0.30901699, -0.80901699, -1.0, -0.80901699, -0.30901699, 0.30901699, 0.80901699]
_S = [0.0, 0.58778525, 0.95105652, 0.95105652, 0.58778525, 0.0, -0.58778525, -0.95105652, -0.95105652, -0.58778525]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, F).tobytes()) & 0xFFFFFFFF


def pose(k=0, t=(0.0, 0.0, 0.0)):
    """Column-major 4x4: rotation about y by k * 2 pi / 10, then the translation t."""
    c, s = F(_C[k % 10]), F(_S[k % 10])
    m = np.zeros(16, F)
    m[0], m[2], m[8], m[10], m[5], m[15] = c, -s, s, c, 1.0, 1.0
    m[12:15] = np.asarray(t, F)
    return m


def shift(cx=0, cy=0, cz=0, voxel=0.1, k=0):
    """A pose that moves by whole cells."""
    return pose(k, (F(cx) * F(voxel), F(cy) * F(voxel), F(cz) * F(voxel)))


def margin(voxel):
    return int(round(0.3 / voxel))


def centres(cells, voxel):
    """float32 [n, 3]: the centres of integer cells [n, 3] (x, y, z) of a grid whose extent cloud begins at 0."""
    c = np.asarray(cells, np.int64).reshape(-1, 3)
    return ((2 * (c - margin(voxel)) + 1).astype(F) * F(F(voxel) * F(0.5))).astype(F)


def extent(res, voxel, n=2):
    """An extent cloud of n points (n = 1: the origin alone) whose grid has `res` = (x, y, z) cells."""
    e = np.array([(t - 1.5) * float(F(voxel)) - 0.6 for t in res], np.float64)
    assert n == 1 or (e > 0).all(), res
    pts = [np.zeros(3, F)] + ([e.astype(F)] if n > 1 else [])
    for j in range(max(0, n - 2)):                      # fillers strictly inside the box: the lane loop of the box kernel
        pts.append((e * ((j % 61) + 1) / 64.0).astype(F))
    return np.stack(pts).astype(F)


def with_corners(e):
    """The extent cloud plus all eight corners of its box: a rotation about y then keeps every boundary point inside the box of
    the rotated extent (the two opposite corners alone do not)."""
    lo, hi = e.min(0), e.max(0)
    return np.concatenate([e, np.stack(np.meshgrid(*[[lo[a], hi[a]] for a in range(3)], indexing="ij"), -1).reshape(-1, 3)]).astype(F)


def shell(lo, hi):
    """The surface cells of the integer box [lo, hi] (inclusive), in a fixed order."""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    g = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    return g[((g == lo) | (g == hi)).any(1)]


def without_face(cells, axis, value):
    return cells[cells[:, axis] != value]


def swap_xz(cells):
    return np.ascontiguousarray(cells[:, ::-1])


def comb(n_teeth, span=5):
    """Two plates at z = 1 and z = span, teeth at x = 2, 4, ... between them: along x the parity flips on every free cell."""
    xs = np.arange(2, 2 + 2 * n_teeth, 2)
    g = np.stack(np.meshgrid(np.arange(1, 2 * n_teeth + 3), np.arange(1, span + 1), np.arange(1, span + 1), indexing="ij"), -1).reshape(-1, 3)
    plate = (g[:, 2] == 1) | (g[:, 2] == span)
    teeth = np.isin(g[:, 0], xs)
    return g[plate | teeth]


class Case:
    def __init__(self, name, family, shapes, pairs, voxel=0.1, inside=1, by_smaller=0, expect="ok", reference=True):
        self.name, self.family, self.shapes, self.voxel, self.inside, self.by_smaller, self.expect = name, family, shapes, F(voxel), inside, by_smaller, expect
        self.reference = reference and expect == "ok"          # False: pinned by the restatement alone
        self.ia = np.array([p[0] for p in pairs], np.int32)
        self.ib = np.array([p[2] for p in pairs], np.int32)
        self.pose_a = np.stack([p[1] for p in pairs]).astype(F)
        self.pose_b = np.stack([p[3] for p in pairs]).astype(F)

    def __len__(self):
        return len(self.ia)

    def crcs(self):
        return np.array([[len(b), crc(b), len(e), crc(e)] for b, e in self.shapes], np.int64)


WIDTHS = (31, 32, 33, 63, 64, 65, 96, 97, 128)
SMALL = 11


def _width_shapes(t, axis, voxel=0.1):
    """(outer shell with a second shell inside it, a third shell) in a grid of t cells along `axis` (0: x, 2: z), SMALL across."""
    res = [SMALL] * 3
    res[axis] = t
    hi = np.array(res) - 2
    a = np.concatenate([shell([1, 1, 1], hi), shell([3, 3, 3], hi - 2)])
    lo_b, hi_b = np.array([2, 2, 2]), hi - 1
    lo_b[axis], hi_b[axis] = 4, t - 6
    e = extent(res, voxel)
    return (centres(a, voxel), e), (centres(shell(lo_b, hi_b), voxel), e)


def widths():
    out = []
    for axis, tag in ((0, "x"), (2, "z")):
        shapes, pairs = [], []
        for t in WIDTHS:
            s = len(shapes)
            shapes += list(_width_shapes(t, axis))
            pairs += [(s, I16, s + 1, I16), (s + 1, I16, s, shift(0, 1, 0))]
        out.append(Case(f"widths_{tag}", "widths", shapes, pairs))
        for t, expect in ((4096, "ok"), (4097, "capacity")):
            out.append(Case(f"widths_{tag}{t}", "widths", list(_width_shapes(t, axis)), [(0, I16, 1, I16)], expect=expect))
    return out


def seams():
    out = []
    res = (100, 9, 9)
    e = extent(res, 0.1)
    cells = [shell([2, 1, 1], [97, 7, 7])]                       # the partner of every other shape
    for w in (30, 31, 32, 33, 62, 63, 64, 65):
        cells.append(shell([w, 2, 2], [w + 24, 6, 6]))           # low wall on cell w: BOUNDARY to FREE forwards at w | w + 1
        cells.append(shell([w - 24, 2, 2], [w, 6, 6]))           # high wall on cell w: the same backwards, FREE to BOUNDARY forwards
    for w in (31, 63):                                           # two adjacent walls across the seam: BOUNDARY to BOUNDARY
        cells.append(np.concatenate([shell([w, 2, 2], [w + 24, 6, 6]), shell([w + 1, 2, 2], [w + 25, 6, 6])]))
        cells.append(np.concatenate([shell([w - 24, 2, 2], [w, 6, 6]), shell([w - 23, 2, 2], [w + 1, 6, 6])]))
    cells.append(np.concatenate([shell([2, 1, 1], [97, 7, 7]), shell([31, 3, 3], [64, 5, 5])]))        # shell in shell: in, out, in
    cells.append(without_face(shell([20, 2, 2], [70, 6, 6]), 0, 70))     # the scan directions disagree along x
    cells.append(without_face(shell([20, 2, 2], [70, 6, 6]), 2, 6))      # ... and along z
    for axis, tag in ((0, "x"), (2, "z")):
        cc = cells if axis == 0 else [swap_xz(c) for c in cells]
        ee = e if axis == 0 else np.ascontiguousarray(e[:, ::-1])
        shapes = [(centres(c, 0.1), ee) for c in cc]
        pairs = []
        for s in range(1, len(shapes)):
            pairs += [(s, I16, 0, I16), (s, I16, s, shift(1, 0, 0) if s % 2 else shift(0, 0, 1))]
        out.append(Case(f"seams_{tag}", "seams", shapes, pairs))
    for axis, tag in ((0, "x"), (2, "z")):
        shapes = []
        for n_teeth in (47, 48, 63, 64):
            c = comb(n_teeth)
            r = (2 * n_teeth + 4, 9, 9)
            ee = extent(r, 0.1)
            if axis == 2:
                c, ee = swap_xz(c), np.ascontiguousarray(ee[:, ::-1])
            shapes.append((centres(c, 0.1), ee))
        pairs = [(s, I16, s, I16) for s in range(4)] + [(s, I16, (s + 1) % 4, I16) for s in range(4)] + [(s, I16, s, shift(1, 0, 1)) for s in range(4)]
        out.append(Case(f"comb_{tag}", "seams", shapes, pairs))
    return out


def edges():
    out = []
    # boundary beyond the extent cloud, inside the 0.3 m margin (15 cells at 2 cm): cell 0 and the last cell of x lines, z lines and y
    t = 40
    e = extent((t, t, t), 0.02)
    full = centres(shell([0, 0, 0], [t - 1, t - 1, t - 1]), 0.02)
    low = centres(shell([0, 0, 0], [20, 25, 31]), 0.02)
    high = centres(shell([9, 14, 8], [t - 1, t - 1, t - 1]), 0.02)
    out.append(Case("edges_margin", "edges", [(full, e), (low, e), (high, e)], [(0, I16, 1, I16), (1, I16, 2, I16), (2, I16, 0, I16), (0, I16, 0, I16)], voxel=0.02))
    # boundary counts around the block size, extent counts around the wave size
    res = (20, 12, 12)
    surface = shell([1, 1, 1], [18, 10, 10])
    shapes = [(centres(surface[:n], 0.1), extent(res, 0.1)) for n in (1, 64, 65, 255, 256, 257)]
    shapes += [(centres(surface, 0.1), extent(res, 0.1, n)) for n in (63, 64, 65)]
    pairs = [(s, I16, (s + 1) % len(shapes), I16) for s in range(len(shapes))] + [(s, I16, s, I16) for s in range(len(shapes))]
    out.append(Case("edges_counts", "edges", shapes, pairs))
    one = (centres(shell([1, 1, 1], [5, 5, 5]), 0.1), extent((7, 7, 7), 0.1, 1))              # an extent cloud of one point
    out.append(Case("edges_extent1", "edges", [one], [(0, I16, 0, I16)]))
    # an empty boundary: counts 0; with normalize_by_smaller the denominator is 0 and the overlap 1.0f
    empty = (np.zeros((0, 3), F), extent(res, 0.1))
    out.append(Case("edges_empty", "edges", [empty, shapes[-1]], [(0, I16, 1, I16), (1, I16, 0, I16), (0, I16, 0, I16)], by_smaller=1))
    # boxes touching with equality on z: the second extent begins exactly where the first one ends
    ez = extent(res, 0.1)
    tz = pose(0, (0.0, 0.0, ez[1, 2]))
    out.append(Case("edges_touch_z", "edges", [(centres(shell([3, 3, 3], [15, 8, 7]), 0.1), ez)], [(0, I16, 0, tz), (0, tz, 0, I16)]))
    return out


def plane_bytes(res, inside=1):
    return int((int(res[0]) + 31) // 32 * int(res[1]) * int(res[2]) * 4 * (4 if inside else 2))


ROUTES_NAMED = 1          # the pair whose planes set the exact-fit budget of the "routes" case


def routes():
    """One call of 40 pairs at 5 cm: disjoint, LDS route, global route, LDS, disjoint, ... of two shapes."""
    small = (centres(np.concatenate([shell([6, 6, 6], [25, 20, 22]), shell([10, 9, 9], [20, 15, 15])]), 0.05), with_corners(extent((33, 28, 30), 0.05, 9)))
    big = (centres(np.concatenate([shell([6, 6, 6], [70, 30, 40]), shell([31, 10, 10], [64, 20, 33])]), 0.05), with_corners(extent((78, 38, 48), 0.05, 70)))
    rng = np.random.default_rng(41)
    far = shift(2000, 0, 0, 0.05)
    pairs = []
    for k in range(40):
        kind = ("disjoint", "lds", "global", "lds")[k % 4]
        i, j = (int(v) for v in rng.integers(-4, 5, 2))
        if kind == "disjoint":
            pairs.append((k % 2, shift(i, 0, j, 0.05), (k // 2) % 2, far))
        elif kind == "lds":
            pairs.append((0, I16, 0, shift(i, 0, j, 0.05)))
        else:
            pairs.append((k % 8 // 4, shift(i, 0, j, 0.05), 1, shift(j, 0, i, 0.05, k % 3)))
    return [Case("routes", "routes", [small, big], pairs, voxel=0.05)]


def nms_list():
    """~60 proposals of a shell whose walls sit on the word seam: dict(shape, centroid, poses, scores, dist_threshold, decider)."""
    cells = np.concatenate([shell([3, 3, 3], [62, 32, 10]), shell([31, 5, 5], [32, 30, 8])])       # walls on cells 31 | 32 when unmoved
    boundary = centres(cells, 0.1)
    ext = np.concatenate([centres(shell([3, 3, 3], [62, 32, 10])[::37], 0.1), centres([[3, 3, 3], [62, 32, 10]], 0.1)])
    centroid = np.array([F(3.0), F(1.5), F(0.35)], F)
    rng = np.random.default_rng(43)
    poses, scores = [], []
    for i in range(60):
        k = 0 if i % 5 else int(rng.integers(0, 10))
        cx, cz = (int(v) for v in rng.integers(-40, 41, 2)) if i % 3 == 0 else (int(rng.integers(-14, 15)), int(rng.integers(-3, 4)))
        poses.append(shift(cx, 0, cz, 0.1, k))
        scores.append(F(rng.integers(1, 12)) * F(0.25))                  # equal in groups: the first index wins
    poses, scores = np.stack(poses).astype(F), np.array(scores, F)
    scores[7] = F(10.0)                                                  # the first keep
    scores[20:23] = [np.nextafter(F(0.01), F(0)), F(0.01), np.nextafter(F(0.01), F(1))]
    poses[20:23] = [shift(70, 0, 60), shift(-70, 0, 60), shift(70, 0, -60)]          # far from everything: the score alone decides
    # the decider: second in score, turned by 3/10 of a turn and put about half a metre from the first keep's centroid, where its
    # overlap with the first keep is small: with dist_threshold = that distance's own fp32 value, `<` keeps it and `<=` would not
    cen7 = poses[7][12:15] + centroid
    turned = np.array([_C[3] * centroid[0] + _S[3] * centroid[2], centroid[1], -_S[3] * centroid[0] + _C[3] * centroid[2]])
    t = np.round((cen7 - turned) / 0.1).astype(int)
    poses[11] = shift(t[0] + 3, 0, t[2] + 4, 0.1, 3)
    scores[11] = F(9.0)
    return dict(shape=(boundary, ext), centroid=centroid, poses=poses, scores=scores, decider=(7, 11))


def centroid_distance(centroid, pose_a, pose_b):
    """The fp32 distance of the two transformed centroids, in rs_hip_nms's operations."""
    def x(m):
        return np.array([m[r] * centroid[0] + m[4 + r] * centroid[1] + m[8 + r] * centroid[2] + F(1.0) * m[12 + r] for r in range(3)], F)
    d = x(np.asarray(pose_a, F)) - x(np.asarray(pose_b, F))
    return np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2], dtype=F)


def random_pairs(n_pairs=200, seed=47):
    """Seeded unions of 2 to 5 shells under rotations about y by multiples of 2 pi / 10 and lattice translations: one Case per voxel."""
    rng = np.random.default_rng(seed)
    out = []
    for voxel in (0.05, 0.1):
        shapes = []
        for _ in range(8):
            cc, corners = [], []
            for _ in range(int(rng.integers(2, 6))):
                lo = rng.integers(0, 10, 3)
                hi = lo + rng.integers(2, 14, 3)
                cc.append(shell(lo, hi))
                corners.append(np.stack(np.meshgrid(*[[lo[a], hi[a]] for a in range(3)], indexing="ij"), -1).reshape(-1, 3))
            b = centres(np.concatenate(cc), voxel)
            shapes.append((b, np.concatenate([b[::11], centres(np.concatenate(corners), voxel)])))
        pairs = []
        for _ in range(n_pairs // 2):
            a, b = (int(v) for v in rng.integers(0, len(shapes), 2))
            i, j, p, q = (int(v) for v in rng.integers(-8, 9, 4))
            pairs.append((a, shift(i, 0, j, voxel, int(rng.integers(0, 10))), b, shift(i + p, 0, j + q, voxel, int(rng.integers(0, 10)))))
        out.append(Case(f"random_{voxel}", "random", shapes, pairs, voxel=voxel, inside=1, by_smaller=int(voxel == 0.1)))
    return out


def fixture_cases():
    """Every family but "random", in the fixture's order."""
    return widths() + seams() + edges() + routes()


def nan_case():
    """A boundary cloud with one NaN point: refused by the kernel's own in-bounds check."""
    res = (20, 12, 12)
    b = centres(shell([1, 1, 1], [18, 10, 10]), 0.1)
    bad = b.copy()
    bad[100, 1] = np.nan
    e = extent(res, 0.1)
    return Case("nan", "edges", [(b, e), (bad, e)], [(0, I16, 0, I16), (0, I16, 1, I16), (0, I16, 0, I16)], expect="outside", reference=False)


# ------------------------------------------------------------------------------------------
# arrangements: a box of 2 m, candidates for rs_hip_coverage_extensions and proposals for rs_hip_scene_saliency
# ------------------------------------------------------------------------------------------

ARR_BMIN, ARR_BMAX = np.zeros(3, F), np.full(3, 2.0, F)
ARR_VOXELS = (0.05, 0.15)


def arr_res(voxel):
    """isect_grid3d_init's resolution of the box, in its float operations."""
    return np.ceil(((ARR_BMAX + F(0.3)) - (ARR_BMIN - F(0.3))) / F(voxel)).astype(np.int64) + 1


def arrangement(voxel, cell0=True):
    """dict(scene, objects, base, cands, names): the hostile candidates of one voxel size over the box [0, 2]^3 (grid origin -0.3: 6
    margin cells at 5 cm, 2 at 15 cm).  Scene-active cells: a slab of the grid (y below two thirds); the base covers a block of it.
    cell0 = False leaves cell (0, 0, 0) without a finite scene point: only a non-finite scene point taken for cell 0 would light it."""
    res = arr_res(voxel)
    n = int(res[0])
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    active = g[(g[:, 1] < 2 * n // 3) & ((g[:, 0] >= 1) | (g[:, 2] == 0))]      # (most of x = 0 and the upper third are scene-inactive)
    # cell0: cell 0 is scene-ACTIVE by a finite point, so a candidate's NaN that became cell 0 would count there.  not cell0: the
    # scene's own non-finite points are the only ones that could light cell 0, and they light nothing.
    if not cell0:
        active = active[active.any(1)]
    scene = np.concatenate([centres(active, voxel), np.array([[np.nan, np.nan, np.nan], [np.inf, 0.5, 0.5], [0.5, -np.inf, np.nan]], F)])
    base_block = g[(g[:, 0] >= n // 2) & (g[:, 0] < n // 2 + 4) & (g[:, 1] < 4) & (g[:, 2] < n)]
    objects, cands, names = [centres(base_block, voxel)], [], []

    def add(name, pts, p=I16):
        objects.append(np.ascontiguousarray(pts, F).reshape(-1, 3))
        cands.append((len(objects) - 1, np.asarray(p, F)))
        names.append(name)

    three = np.array([[2, 2, 2], [3, 2, 2], [2, 3, 2]])
    spread = np.array([[1, 0, 0], [n - 1, 2 * n // 3 - 1, n - 1], [n // 3, n // 3, n // 3]])      # far apart: the sub-box is most of the grid
    for k in (1, 255, 256, 257, 5000):
        idx = np.arange(k) % 3 if k >= 3 else np.zeros(k, int)
        add(f"three_cells_{k}", centres(three[idx], voxel))
        add(f"spread_cells_{k}", centres(spread[idx], voxel))
    add("off_grid", centres(three, voxel) + F(50.0))
    add("inside_base", centres(base_block[::3], voxel))
    add("scene_inactive", centres(g[(g[:, 1] >= 2 * n // 3)][::5], voxel))
    add("empty", np.zeros((0, 3), F))
    add("non_finite", np.array([[np.nan, np.nan, np.nan], [np.inf, 0.5, 0.5], [-np.inf, 0.5, 0.5], [0.5, np.nan, 0.5], [np.nan, np.inf, -np.inf]], F))
    rod_len = min(n - 2, 2 * n // 3 - 1)
    add("rod", centres(np.stack([np.arange(1, 1 + rod_len)] * 3, 1), voxel))
    # a plate across y and z, longer along z: an index that took the sub-box's y extent for its z extent would fold distinct cells together
    add("plate_yz", centres(np.stack(np.meshgrid([3], np.arange(5, 10), np.arange(5, n - 1), indexing="ij"), -1).reshape(-1, 3), voxel))
    # points exactly on cell faces and on the grid's outer faces, and one ulp to either side: floorf of exactly 0 and of exactly res
    step = F(voxel)
    k = np.arange(0, n + 1)
    face = (F(-0.3) + k.astype(F) * step).astype(F)
    face = np.concatenate([face, np.nextafter(face, F(-100)), np.nextafter(face, F(100))])
    add("faces_x", np.stack([face, np.full(len(face), centres([[2, 2, 2]], voxel)[0, 1]), np.full(len(face), centres([[2, 2, 2]], voxel)[0, 2])], 1))
    add("faces_y", np.stack([np.full(len(face), centres([[2, 2, 2]], voxel)[0, 0]), face, np.full(len(face), centres([[2, 2, 2]], voxel)[0, 2])], 1))
    add("faces_z", np.stack([np.full(len(face), centres([[2, 2, 2]], voxel)[0, 0]), np.full(len(face), centres([[2, 2, 2]], voxel)[0, 1]), face], 1))
    return dict(voxel=F(voxel), res=res, scene=scene, objects=objects, base=[(0, I16, 0)], cands=cands, names=names)


def saliency_case(voxel, finite_in_cell0=False):
    """Proposals and a scene for rs_hip_scene_saliency: a static proposal listed BEFORE the dynamic one whose cells it clears, wall and
    floor points in lit cells, class -1 with wall_idx -1, and an object with NaN, +inf and -inf points plus a NaN scene point."""
    res = arr_res(voxel)
    n = int(res[0])
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    dyn = centres(g[(g[:, 0] >= 2) & (g[:, 0] < 12) & (g[:, 1] < 6) & (g[:, 2] >= 2) & (g[:, 2] < 12)], voxel)
    sta = centres(g[(g[:, 0] >= 8) & (g[:, 0] < 14) & (g[:, 1] < 3) & (g[:, 2] >= 2) & (g[:, 2] < 12)], voxel)
    wild = np.array([[np.nan, np.nan, np.nan], [np.inf, 0.5, 0.5], [-np.inf, 0.5, 0.5], [0.5, np.nan, 0.5], [0.5, 0.5, np.inf], [np.nan, np.inf, -np.inf]], F)
    if finite_in_cell0:
        wild = np.concatenate([wild, centres([[0, 0, 0]], voxel)])
    objects = [dyn, sta, wild, np.full((3, 3), np.nan, F)]
    # the static proposal comes first in the list; with a finite point in cell 0 a static cloud of NaN points must not clear that cell
    prop_obj = np.array([1, 0, 2] + ([3] if finite_in_cell0 else []), np.int32)
    prop_static = np.array([1, 0, 0] + ([1] if finite_in_cell0 else []), np.int32)
    prop_pose = np.stack([I16] * len(prop_obj)).astype(F)
    scene = centres(g[::7], voxel)
    cls = (np.arange(len(scene)) % 4 - 1).astype(np.int32)              # -1, 0, 1 (wall), 2 (floor)
    scene = np.concatenate([scene, np.array([[np.nan, np.nan, np.nan], [np.nan, 0.5, 0.5], [np.inf, np.inf, np.inf]], F), centres([[0, 0, 0]], voxel)])
    cls = np.concatenate([cls, np.array([0, 0, 0, 0], np.int32)])
    return dict(voxel=F(voxel), objects=objects, prop_obj=prop_obj, prop_pose=prop_pose, prop_static=prop_static, scene=scene.astype(F), cls=cls)


ARR_CASES = [(voxel, cell0) for voxel in ARR_VOXELS for cell0 in (True, False)]


def arr_key(kind, voxel, cell0):
    """The prefix of one case's arrays in tests/golden/arrange_hard.npz: kind "cov" (arrangement) or "sal" (saliency_case)."""
    return f"{kind}_{int(round(voxel * 100)):03d}_{int(cell0)}_"


def cloud_crcs(scene, objects):
    """int64 [1 + n, 2]: (length, CRC) of the scene cloud, then of every object's cloud — what arrange_hard.npz stores of them."""
    return np.array([[len(p), crc(p)] for p in [scene] + list(objects)], np.int64)


@functools.lru_cache(maxsize=None)
def arrangement_expectations(voxel, cell0=True):
    """Computed once per case and shared: leave the arrays unchanged.  The hostile candidates at one voxel size with what tests/ao_restate.py makes of them: (case, scene grid, base_agree, fresh,
    agree, scores, live sub-box bytes per candidate).  The counts and score bits are also in arrange_hard.npz, from the reference;
    the sub-box bytes (the route of a candidate) are the restatement's alone: the reference has no sub-boxes."""
    import ao_restate as R
    a = arrangement(voxel, cell0)
    grid = R.scene_grid(ARR_BMIN, ARR_BMAX, voxel, a["scene"], None, 0.0)
    base_agree, fresh, agree, scores = R.extensions(grid, ARR_BMIN, ARR_BMAX, voxel, a["objects"], a["base"], a["cands"])
    need = [R.live_box_bytes(grid, ARR_BMIN, ARR_BMAX, voxel, a["objects"], a["base"], c) for c in a["cands"]]
    return a, grid, base_agree, fresh, agree, scores, need
