"""Seeded clouds on which a grid search is easy to get subtly wrong, and a numpy brute-force radius search to hold the searches to.

Each family is a dict:
  points, normals (n, 3) float32     the searched cloud
  queries (4096, 3) float32           4095 and 4096 of them sit on either side of the rows' wave/tiled switch
  radius                              the rows' search radius
  grid_radius                         what the oracle's grid is built with (cell = 2 * grid_radius >= radius, so the reference's
                                      512-bin cap never truncates a candidate set)
  obj, poses, T0                      an object cut from the cloud in its own frame, 8 score poses that spread it over the whole
                                      box, and an ICP start pose near where it was cut (two_far: the two points themselves)
Small enough that brute force over every query and point takes seconds.

Rows follow the reference's grid_scan_bin (msh_hash_grid.h:826-862, oracle/rs_oracle.c): v = p - q in float32,
d² = vx*vx + vy*vy + vz*vz evaluated left to right, a point is in when d² < (float)((double)r * r) (strict), rows ascend by
(d², index).
"""
import numpy as np

NQ = 4096
FAMILIES = ("offset_1e3", "offset_1e4", "negative", "planar", "collinear", "contrast", "lattice", "outside", "two_far")


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _room(seed):
    from rescan_amd import synth
    s = synth.make_scene(seed=seed, width=1.6, depth=1.6, height=0.8, density=1500, objects=("chair",))
    return s["points"].astype(np.float32), s["normals"].astype(np.float32)


def _near(rng, pts, n, sigma):
    """n queries: cloud points moved by N(0, sigma), plus a tenth uniform over the box grown by 2 sigma."""
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    m = n // 10
    a = pts[rng.integers(0, len(pts), n - m)] + rng.normal(0.0, sigma, (n - m, 3))
    b = rng.uniform(lo - 2 * sigma, hi + 2 * sigma, (m, 3))
    q = np.concatenate([a, b]).astype(np.float32)
    return q[rng.permutation(len(q))]


def _object_and_poses(rng, pts, nor, centre, reach=0.25):
    """The cloud's points within `reach` of `centre`, in a frame centred on their mean (so a pose's translation carries the
    magnitude of the coordinates); 8 poses spread over the box (corners and middle, small rotations) plus an ICP start pose."""
    from rescan_amd import synth
    sel = np.nonzero(np.linalg.norm(pts.astype(np.float64) - centre, axis=1) < reach)[0][:600]
    c = pts[sel].astype(np.float64).mean(axis=0)
    local = (pts[sel].astype(np.float64) - c).astype(np.float32)
    I4 = np.eye(4, dtype=np.float32).ravel()
    lo, hi = pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64)
    poses = []
    for t in range(8):
        w = rng.uniform(0.0, 1.0, 3) if t >= 2 else np.full(3, float(t))      # lo corner, hi corner, then random
        P = synth.perturbed_pose(I4, rng, 0.1, 0.0).reshape(4, 4).copy()
        P[3, :3] = (lo + w * (hi - lo)).astype(np.float32)
        poses.append(P.ravel())
    P = np.eye(4, dtype=np.float32); P[3, :3] = c.astype(np.float32)
    poses[2] = P.ravel()                                                     # the object where it was cut: high scores
    T0 = synth.perturbed_pose(P.ravel(), rng, 0.03, 0.01)
    return dict(pos=local, nor=np.ascontiguousarray(nor[sel])), np.stack(poses).astype(np.float32), T0


def make(name, seed=0):
    rng = np.random.default_rng([seed, FAMILIES.index(name)])
    f = dict(name=name, radius=0.05, grid_radius=0.05, normals=None, obj=None, poses=None, T0=None)
    if name in ("offset_1e3", "offset_1e4", "negative"):
        pts, nor = _room(11 + FAMILIES.index(name))
        if name == "negative":
            off = -(pts.max(axis=0).astype(np.float64) + np.array([0.37, 0.011, 2.5]))
        else:
            mag = 1e3 if name == "offset_1e3" else 1e4
            off = np.array([mag + 0.3, -mag - 0.7, mag * 0.5 + 0.1]) * np.array([1, 1, -1])   # +x, -y, -z
        pts = (pts.astype(np.float64) + off).astype(np.float32)
        q = _near(rng, pts, NQ, 0.02)
        centre = pts[rng.integers(len(pts))]
    elif name == "planar":
        n = 12000
        pts = np.zeros((n, 3), np.float32)
        pts[:, :2] = rng.uniform(-1.0, 1.0, (n, 2))
        pts[:, 2] = np.float32(0.3)
        nor = np.tile(np.float32([0.0, 0.0, 1.0]), (n, 1))
        q = _near(rng, pts, NQ, 0.02)
        centre = np.array([0.1, -0.2, 0.3])
    elif name == "collinear":
        n = 6000
        pts = np.zeros((n, 3), np.float32)
        pts[:, 0] = rng.uniform(-3.0, 3.0, n)
        pts[:, 1] = np.float32(-0.5); pts[:, 2] = np.float32(1.25)
        nor = np.tile(np.float32([0.0, 1.0, 0.0]), (n, 1))
        q = _near(rng, pts, NQ, 0.02)
        centre = np.array([0.4, -0.5, 1.25])
    elif name == "contrast":
        dense = rng.uniform(0.0, 0.02, (50000, 3)) + np.array([1.3, 0.7, 2.1])
        sparse = rng.uniform(0.0, 4.0, (5000, 3))
        pts = np.concatenate([dense, sparse]).astype(np.float32)
        pts = pts[rng.permutation(len(pts))]
        nor = _unit(rng, len(pts))
        q = np.concatenate([_near(rng, pts[:len(pts)], NQ - 1024, 0.02),
                            (np.array([1.31, 0.71, 2.11]) + rng.normal(0, 0.02, (1024, 3)))]).astype(np.float32)
        q = q[rng.permutation(len(q))]
        centre = np.array([1.31, 0.71, 2.11])
    elif name == "lattice":
        s = 0.125                                        # spacing = radius = the oracle's cell; exact in binary
        g = np.stack(np.meshgrid(np.arange(20), np.arange(16), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
        pts = (g * s + np.array([0.5, -1.0, 0.25])).astype(np.float32)
        nor = np.tile(np.float32([0.0, 0.0, 1.0]), (len(pts), 1))
        nodes = pts[rng.integers(0, len(pts), NQ // 2)]
        half = (pts[rng.integers(0, len(pts), NQ - NQ // 2)] + np.float32(s / 2) * rng.integers(-1, 2, (NQ - NQ // 2, 3)))
        q = np.concatenate([nodes, half]).astype(np.float32)
        q = q[rng.permutation(len(q))]
        f.update(radius=s, grid_radius=s / 2)
        centre = pts[rng.integers(len(pts))]
    elif name == "outside":
        pts, nor = _room(31)
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        r = 0.05
        out = []
        for a in range(3):
            for side in (-1, 1):
                # 0.5, 1, 1.5 and 2.5 cells of the oracle's grid (cell = r) and of the device grids (cell = 2r: the k-NN grid,
                # rs_knn.hip, and the rows' cell2r layout), and 100 m
                for dist in (0.5 * r, 1.0 * r, 1.5 * r, 2.0 * r, 2.5 * r, 3.0 * r, 5.0 * r, 100.0):
                    b = pts[rng.integers(0, len(pts), 32)].astype(np.float64)
                    b[:, a] = (lo[a] - dist) if side < 0 else (hi[a] + dist)
                    out.append(b)
        out.append(np.array([lo - 0.5 * r, hi + 0.5 * r, [lo[0] - r, hi[1] + r, lo[2] - r], lo - 100.0, hi + 100.0]))
        out = np.concatenate(out)
        q = np.concatenate([out, _near(rng, pts, NQ - len(out), 0.02)]).astype(np.float32)
        q = q[rng.permutation(len(q))]
        q[NQ // 2] = np.nan                             # no point is within the radius of a NaN query (d² < r² is false)
        f.update(radius=r, grid_radius=r / 2)           # oracle cell = r
        centre = pts[rng.integers(len(pts))]
    elif name == "two_far":
        pts = np.array([[0.25, -0.5, 0.125], [31.0, 17.5, -23.0]], np.float32)
        nor = np.float32([[0.0, 0.0, 1.0], [0.6, 0.8, 0.0]])
        q = np.concatenate([pts[rng.integers(0, 2, NQ - 256)] + rng.normal(0, 0.03, (NQ - 256, 3)),
                            rng.uniform(pts.min(axis=0), pts.max(axis=0), (256, 3))]).astype(np.float32)
        centre = None
    else:
        raise KeyError(name)
    f.update(points=np.ascontiguousarray(pts, np.float32), normals=np.ascontiguousarray(nor, np.float32),
             queries=np.ascontiguousarray(q, np.float32))
    if centre is not None:
        f["obj"], f["poses"], f["T0"] = _object_and_poses(rng, f["points"], f["normals"], np.asarray(centre, np.float64))
    elif name == "two_far":
        # the two points are the object: scores and correspondences of a cloud that is almost all empty grid
        I4 = np.eye(4, dtype=np.float32)
        f["obj"] = dict(pos=pts.copy(), nor=nor.copy())
        poses = []
        for t in np.linspace(0.0, 1.0, 8):
            P = I4.copy(); P[3, :3] = (t * 0.04 - 0.02, 0.01, -t * 0.02); poses.append(P.ravel())
        f["poses"] = np.stack(poses).astype(np.float32); f["T0"] = poses[3].copy()
    return f


def d2_rows(points, queries):
    """Float32 dist² of every (query, point) pair in the reference's expression order: (queries, points)."""
    v = points[None, :, :] - queries[:, None, :]
    return v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]


def radius_sq(radius):
    return np.float32(np.float64(np.float32(radius)) * np.float64(np.float32(radius)))


def brute_rows(points, queries, radius, k, chunk=64):
    """(d², idx, n, total, within): the k nearest points with d² < r² per query, ascending by (d², index), rows zero past n;
    `within` is the full count inside the radius."""
    points = np.ascontiguousarray(points, np.float32); queries = np.ascontiguousarray(queries, np.float32)
    nq = len(queries)
    r2 = radius_sq(radius)
    D = np.zeros((nq, k), np.float32); I = np.zeros((nq, k), np.int32)
    n = np.zeros(nq, np.int64); within = np.zeros(nq, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, nq, chunk):
            d2 = d2_rows(points, queries[c0:c0 + chunk])
            hit = d2 < r2
            for r in range(len(d2)):
                j = np.nonzero(hit[r])[0]
                within[c0 + r] = len(j)
                dj = d2[r, j]
                if len(j) > k:                      # keep everything up to the k-th distance (ties included), then order
                    kth = np.partition(dj, k - 1)[k - 1]
                    keep = dj <= kth
                    j, dj = j[keep], dj[keep]
                o = np.lexsort((j, dj))[:k]
                n[c0 + r] = len(o)
                D[c0 + r, :len(o)] = dj[o]; I[c0 + r, :len(o)] = j[o]
    return D, I, n, int(n.sum()), within


def truncate(rows, k):
    """The brute-force rows of a smaller k (a prefix of the (d², index)-ordered rows)."""
    D, I, n, _, within = rows
    nk = np.minimum(n, k)
    D, I = D[:, :k].copy(), I[:, :k].copy()
    past = np.arange(k)[None, :] >= nk[:, None]
    D[past] = 0.0; I[past] = 0
    return D, I, nk, int(nk.sum()), within


def assert_rows(want, got, points, queries):
    """`got` = (d², idx, n, total) is a correct answer where `want` is the brute force: counts and total equal, distance rows
    identical bit for bit, and every returned index is a distinct point whose own float d² is the distance in its slot.  Indices
    may differ from `want` only among exactly equal distances, including ties across the k-th slot, which
    conftest.rows_equal_up_to_ties cannot see (the reference's heap keeps an arbitrary one of them)."""
    wd, wi, wn, wt = want[:4]
    gd, gi, gn, gt = got[:4]
    gn = np.asarray(gn, np.int64)
    assert int(gt) == int(wt)
    bad = np.nonzero(gn != wn)[0]
    assert not len(bad), f"{len(bad)} counts differ, first query {bad[0]}: {gn[bad[0]]} vs {wn[bad[0]]}"
    k = wd.shape[1]
    valid = np.arange(k)[None, :] < wn[:, None]
    bad = np.nonzero((gd.view(np.uint32) != wd.view(np.uint32)) & valid)
    assert not len(bad[0]), f"{len(bad[0])} distances differ, first at query {bad[0][0]} slot {bad[1][0]}"
    r, c = np.nonzero(valid & (gi != wi))
    if len(r):
        j = gi[r, c]
        assert ((j >= 0) & (j < len(points))).all()
        v = points[j] - queries[r]
        own = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
        assert (own.view(np.uint32) == gd[r, c].view(np.uint32)).all(), "an index differs and its own d² is not its slot's"
        for q in np.unique(r):
            row = gi[q, :gn[q]]
            assert len(np.unique(row)) == len(row), f"query {q}: an index appears twice"
    return len(r)


def queries_with_counts(points, radius, centre, targets, per_target, seed=0, t_range=(0.0, 0.2)):
    """Queries on rays out of `centre` (the contrast family's dense cube) with exactly `target` points within `radius`, for every
    target: each ray is bisected in its float32 query position until brute_rows' count hits the target.  Rays where the count
    jumps over the target are dropped.  Returns (queries, counts)."""
    rng = np.random.default_rng(seed)
    points = np.ascontiguousarray(points, np.float32)
    near = points[np.linalg.norm(points.astype(np.float64) - centre, axis=1) < t_range[1] + 2 * radius]
    r2 = radius_sq(radius)

    def count(q):
        return int((d2_rows(near, q[None, :])[0] < r2).sum())

    out, got = [], []
    for target in targets:
        found = 0
        for _ in range(8 * per_target):
            if found == per_target:
                break
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            lo, hi = t_range                                    # count(lo) >= target > count(hi)
            q = None
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                qm = (centre + d * mid).astype(np.float32)
                c = count(qm)
                if c == target:
                    q = qm
                    break
                lo, hi = (mid, hi) if c > target else (lo, mid)
            if q is not None:
                out.append(q); got.append(target); found += 1
    return np.array(out, np.float32).reshape(-1, 3), np.array(got, np.int64)


def surface_poses(f, n_poses, reach=1.0, cap=4000, seed=0):
    """A larger object cut from the family's cloud around a few of its points, and n_poses poses that keep it ON the surface it
    came from (shifts up to 3 cm, turns up to 0.05 rad): every object point then has scene points near the edge of the radius
    on all sides, which is where a search that culls by cell faces can lose one.  Returns (obj, poses)."""
    from rescan_amd import synth
    rng = np.random.default_rng([seed, 77])
    pts, nor = f["points"], f["normals"]
    centre = pts[rng.integers(len(pts))].astype(np.float64)
    sel = np.nonzero(np.linalg.norm(pts.astype(np.float64) - centre, axis=1) < reach)[0][:cap]
    c = pts[sel].astype(np.float64).mean(axis=0)
    obj = dict(pos=(pts[sel].astype(np.float64) - c).astype(np.float32), nor=np.ascontiguousarray(nor[sel]))
    P = np.eye(4, dtype=np.float32); P[3, :3] = c.astype(np.float32)
    poses = [P.ravel()] + [synth.perturbed_pose(P.ravel(), rng, 0.05, 0.03) for _ in range(n_poses - 1)]
    return obj, np.stack(poses).astype(np.float32)
