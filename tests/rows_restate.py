"""Numpy restatements of the three consumers that sit on the rows primitives -- the level builder, the neighbourhood graph and
label transfer -- and the hostile inputs they are run on.  tests/test_hard_rows_cpu.py holds every restatement to the CPU oracle
(oracle/rs_oracle.c); tests/test_gpu_hard_rows.py holds the device to the restatements.  Plain module, no pytest.

All distances are float32 in the reference's expression (hard_clouds.d2_rows): v = p - q, d² = vx*vx + vy*vy + vz*vz left to right,
a point is within the radius when d² < (float)((double)r * r), strictly.

Ties.  Where the reference's answer is an accident of its heap the restatements say so instead of choosing:
  edge_bounds   per point the neighbours that MUST be in its K-row (strictly nearer than the K-th distance) and those that MAY be
                (at most the K-th distance): a row with an exact tie across its K-th slot has may != must;
  label_chain   takes the lowest index among equidistant nearest object points and COUNTS the decisions in which another choice
                among them would have changed the gate's outcome (`tie_dependent`), next to the decisions that met a tie at all
                (`tied`).
"""
import itertools

import numpy as np

import hard_clouds as hc


# ---- level builder --------------------------------------------------------------------------------------------------------

def _pairs_within(points, radius):
    """Index pairs (i < j) with float32 d² < r²: a k-d tree in float64 gives a superset (radius grown by 0.1 %, far above the
    float32 rounding of d²), the exact float32 test decides."""
    from scipy.spatial import cKDTree
    P = np.ascontiguousarray(points, np.float32)
    if len(P) < 2:
        return np.zeros((0, 2), np.int64)
    pr = cKDTree(P.astype(np.float64)).query_pairs(float(radius) * 1.001 + 1e-7, output_type="ndarray").astype(np.int64)
    v = P[pr[:, 1]] - P[pr[:, 0]]
    d2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    return pr[d2 < hc.radius_sq(radius)]


def level_samples(points, radius, stats=None):
    """rs_pointcloud__compute_level_poisson restated: walk the points in index order, a point is a sample iff no earlier sample
    lies within the radius.  Returns (sample indices, increasing; the largest number of points within the radius of any point,
    itself included).  The reference's own search keeps max_n_neigh points, so the restatement is the reference's answer only
    while that count stays at or below max_n_neigh: the caller asserts it.
    stats (a dict, optional) receives avg_later -- the average number of later neighbours, which picks the device's frontier
    kernel -- and depth: the number of rounds of the dependence order (a sample is decided one round after the last of its
    earlier neighbours was covered, a covered point one round after its first earlier sample)."""
    n = len(points)
    pr = _pairs_within(points, radius)
    a = np.concatenate([pr[:, 0], pr[:, 1]]); b = np.concatenate([pr[:, 1], pr[:, 0]])
    o = np.argsort(a, kind="stable")
    a, b = a[o], b[o]
    start = np.searchsorted(a, np.arange(n + 1))
    is_sample = np.zeros(n, bool); rnd = np.zeros(n, np.int64)
    for i in range(n):
        nb = b[start[i]:start[i + 1]]
        e = nb[nb < i]
        if not len(e):
            is_sample[i] = True; rnd[i] = 1
            continue
        s = e[is_sample[e]]
        if len(s):
            rnd[i] = rnd[s].min() + 1
        else:
            is_sample[i] = True; rnd[i] = rnd[e].max() + 1
    if stats is not None:
        stats["avg_later"] = len(pr) / max(n, 1)
        stats["depth"] = int(rnd.max()) if n else 0
    within = int((start[1:] - start[:-1]).max()) + 1 if n else 0
    return np.nonzero(is_sample)[0].astype(np.int32), within


def within_count(points, query, radius):
    """Number of points within the radius of one query point (brute force)."""
    return int((hc.d2_rows(np.ascontiguousarray(points, np.float32), np.ascontiguousarray(query, np.float32)[None, :])[0]
                < hc.radius_sq(radius)).sum())


# ---- neighbourhood graph ----------------------------------------------------------------------------------------------------

def graph_radius(radius_sq):
    """rspf_compute_neighborhood's search radius: the double sqrt of the float radius², narrowed to float."""
    return np.float32(np.sqrt(np.float64(np.float32(radius_sq))))


def edge_key(a, b, n):
    a = np.asarray(a, np.int64); b = np.asarray(b, np.int64)
    return np.maximum(a, b) * n + np.minimum(a, b)


def edges(D, I, nn, n):
    """The reference's edge list from K-rows of a self-search (rs_pointcloud_filters.cpp:696-714): rows i ascending, every entry
    (i, j) of row i is offered under the undirected key, the first insertion of a key wins.  Self-edges (i, i) are part of it.
    Returns (idx1, idx2) ascending by key."""
    K = I.shape[1]
    valid = np.arange(K)[None, :] < np.asarray(nn)[:, None]
    a = np.repeat(np.arange(n, dtype=np.int64), K).reshape(n, K)[valid]
    b = I[valid].astype(np.int64)
    key = edge_key(a, b, n)
    o = np.argsort(key, kind="stable")                       # offers are generated in row order: stable = first insertion first
    key, a, b = key[o], a[o], b[o]
    first = np.ones(len(key), bool); first[1:] = key[1:] != key[:-1]
    return a[first].astype(np.int32), b[first].astype(np.int32)


def _within_sorted(points, radius):
    """Every directed pair (i, j), i == j included, with float32 d² < r², ordered by (i, d², j): (row, col, d², row starts);
    None for a cloud so dense that the pairs run into the tens of millions."""
    from scipy.spatial import cKDTree
    P = np.ascontiguousarray(points, np.float32)
    n = len(P)
    tree = cKDTree(P.astype(np.float64))
    if tree.count_neighbors(tree, float(radius) * 1.001 + 1e-7) > 4_000_000:
        return None
    pr = _pairs_within(P, radius)
    row = np.concatenate([pr[:, 0], pr[:, 1], np.arange(n)]); col = np.concatenate([pr[:, 1], pr[:, 0], np.arange(n)])
    v = P[col] - P[row]
    d2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    o = np.lexsort((col, d2, row))
    row, col, d2 = row[o], col[o], d2[o]
    return row, col, d2, np.searchsorted(row, np.arange(n + 1))


def edge_bounds(points, radius, K, cache=None):
    """Per point i, as arrays of directed keys i * n + j: `may` -- the j at most i's K-th distance (no correct K-row holds
    anything else) -- and `must` -- the j every correct K-row holds: all of `may` when there are at most K of them, else the j
    strictly nearer than the K-th distance.  Both limited to d² < r².  Third result: the rows with an exact tie across the
    K-th slot (more than K `may`).  cache: a dict that keeps the sorted pairs for another K."""
    if cache is None:
        cache = {}
    if "within" not in cache:
        cache["within"] = _within_sorted(points, radius)
    n = len(points)
    inf = np.float32(np.inf)
    if cache["within"] is not None:
        row, col, d2, start = cache["within"]
        cnt = start[1:] - start[:-1]
        kth = np.full(n, inf, np.float32)
        full = cnt > K
        kth[full] = d2[start[:-1][full] + K - 1]
        ma = d2 <= kth[row]
        tied = np.bincount(row[ma], minlength=n) > K
        mu = np.where(tied[row], d2 < kth[row], ma)
        key = row * n + col
        return key[mu], key[ma], np.nonzero(tied)[0]
    P = np.ascontiguousarray(points, np.float32)
    r2 = hc.radius_sq(radius)
    must, may, tied = [], [], []
    for c0 in range(0, n, 64):                                                       # dense: chunks of the full distance matrix
        d2 = hc.d2_rows(P, P[c0:c0 + 64])
        hit = d2 < r2
        dm = np.where(hit, d2, inf)
        kth = np.full(len(d2), inf, np.float32)
        if n > K:
            kth = np.where(hit.sum(axis=1) > K, np.partition(dm, K - 1, axis=1)[:, K - 1], kth).astype(np.float32)
        ma = hit & (dm <= kth[:, None])
        t = ma.sum(axis=1) > K
        mu = np.where(t[:, None], hit & (dm < kth[:, None]), ma)
        r, c = np.nonzero(mu); must.append((r + c0).astype(np.int64) * n + c)
        r, c = np.nonzero(ma); may.append((r + c0).astype(np.int64) * n + c)
        tied.append(np.nonzero(t)[0] + c0)
    return np.concatenate(must), np.concatenate(may), np.concatenate(tied)


def edge_inputs(points, normals, a, b):
    """An edge's own d² (float32 from its two points, candidate minus query) and normal dot (float32, left to right)."""
    P = np.ascontiguousarray(points, np.float32); N = np.ascontiguousarray(normals, np.float32)
    v = P[b] - P[a]
    d2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    na, nb = N[a], N[b]
    dot = na[:, 0] * nb[:, 0] + na[:, 1] * nb[:, 1] + na[:, 2] * nb[:, 2]
    return d2, dot


def edge_costs(oracle, d2, dot, radius_sq=0.0025, dist_exp=15.0, angle_exp=16.0):
    """oracle.edge_cost over arrays (the reference's pow / powf from the host libm)."""
    import ctypes as C
    f = oracle.lib.orc_edge_cost
    f.restype = C.c_float; f.argtypes = [C.c_float] * 5
    rep = itertools.repeat
    out = list(map(f, d2.tolist(), dot.tolist(), rep(float(np.float32(radius_sq))), rep(float(dist_exp)), rep(float(angle_exp))))
    return np.array(out, np.float32)


# ---- label transfer ---------------------------------------------------------------------------------------------------------

def gate_tmin(gate):
    """The smallest float32 dot in [0, 1] that passes the reference's label gate (acosf(|dot|) < 70 degrees), by bisection over
    the float's bit patterns on `gate` (oracle.label_gate)."""
    lo, hi = np.float32(0.0).view(np.uint32), np.float32(1.0).view(np.uint32)     # gate(lo) false, gate(hi) true
    lo, hi = int(lo), int(hi)
    assert not gate(0.0) and gate(1.0)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if gate(float(np.uint32(mid).view(np.float32))):
            hi = mid
        else:
            lo = mid
    return np.uint32(hi).view(np.float32)


def xform(m, v, w):
    """msh_mat4_vec3_mul in float32: m0*x + m4*y + m8*z + w*m12, left to right (m column-major, 16 floats)."""
    m = np.ascontiguousarray(m, np.float32).ravel(); v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    w = np.float32(w)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([m[c] * x + m[4 + c] * y + m[8 + c] * z + w * m[12 + c] for c in range(3)], axis=1).astype(np.float32)


def unit(v):
    """msh_vec3_normalize: 1.0f / sqrtf(x*x + y*y + z*z), then three multiplies (a zero vector becomes NaN)."""
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        inv = np.float32(1.0) / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        return (v * inv[:, None]).astype(np.float32)


def dot3(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def nearest(obj_pos, q, chunk=2048):
    """Per query the smallest float32 d² over all object points, the lowest index that has it, and how many have it."""
    obj_pos = np.ascontiguousarray(obj_pos, np.float32)
    n = len(q)
    dmin = np.zeros(n, np.float32); idx = np.zeros(n, np.int64); tied = np.zeros(n, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, n, chunk):
            d2 = hc.d2_rows(obj_pos, q[c0:c0 + chunk])
            i = np.argmin(d2, axis=1)
            m = d2[np.arange(len(d2)), i]
            dmin[c0:c0 + chunk] = m; idx[c0:c0 + chunk] = i; tied[c0:c0 + chunk] = (d2 == m[:, None]).sum(axis=1)
    return dmin, idx, tied


def label_chain(scene_pos, scene_nor, placements, labels, min_dists, label_base, tmin, inverse, cache=None, first=0):
    """rs_pointcloud_filters.cpp:738-778 over `placements` -- dicts of pose (16 floats, column-major), pos, nor, radius -- on
    the running (labels, min_dists), which it updates in place; placement k writes label label_base + k + 1.  `inverse` is the
    reference's 4x4 inverse (oracle.mat4_inverse).  cache: a dict that keeps each placement's brute-force nearest points under
    first + k (they do not depend on the radius or on the running state).  Returns (tied, tie_dependent)."""
    scene_pos = np.ascontiguousarray(scene_pos, np.float32); scene_nor = np.ascontiguousarray(scene_nor, np.float32)
    n_tied = n_dep = 0
    for k, pl in enumerate(placements):
        pose = np.ascontiguousarray(pl["pose"], np.float32).ravel()
        key = first + k
        if cache is not None and key in cache:
            dmin, idx, tied, q = cache[key]
        else:
            q = xform(inverse(pose), scene_pos, 1.0)
            dmin, idx, tied = nearest(pl["pos"], q)
            if cache is not None:
                cache[key] = dmin, idx, tied, q
        r2 = hc.radius_sq(pl["radius"])
        cand = (dmin < r2) & (dmin < min_dists)                                   # found, and strictly closer than the running minimum
        j = np.nonzero(cand)[0]
        n1 = unit(xform(pose.reshape(4, 4).T.ravel(), scene_nor[j], 0.0))         # the pose's transpose on the scene normal
        onor = np.ascontiguousarray(pl["nor"], np.float32)
        with np.errstate(invalid="ignore"):
            d = np.abs(dot3(n1, unit(onor[idx[j]])))
            ok = (d >= tmin) & (d <= np.float32(1.0))
            for t in np.nonzero(tied[j] > 1)[0]:                                  # would another of the tied points gate differently?
                n_tied += 1
                d2 = hc.d2_rows(np.ascontiguousarray(pl["pos"], np.float32), q[j[t]][None, :])[0]
                others = np.nonzero(d2 == dmin[j[t]])[0]
                dd = np.abs(dot3(n1[t][None, :], unit(onor[others])))
                oo = (dd >= tmin) & (dd <= np.float32(1.0))
                if oo.any() != oo.all():
                    n_dep += 1
        win = j[ok]
        min_dists[win] = dmin[win]
        labels[win] = label_base + k + 1
    return n_tied, n_dep


def arrangement(scene_pos, scene_nor, objects, placements, radius, prioritize_static, unlabelled_class_idx, tmin, inverse, cache=None):
    """rspf_arrangement_to_labels (:780-869).  objects: dicts of pos, nor, class_idx, is_static; placements: dicts of pose,
    object_idx, uidx.  Returns dict(labels, min_dists, order, class_ids, instance_ids, tied, tie_dependent)."""
    n = len(scene_pos)
    labels = np.zeros(n, np.int8); mind = np.full(n, 1e9, np.float32)
    key = np.array([(objects[p["object_idx"]]["is_static"] << 10) | objects[p["object_idx"]]["class_idx"] for p in placements], np.int64)
    order = np.argsort(key, kind="stable").astype(np.int32)                       # :823-827 (glibc's qsort is a stable merge sort)
    stat = [objects[placements[i]["object_idx"]]["is_static"] for i in order]
    first_static = next((k for k, s in enumerate(stat) if s), 0)                   # :830-835, 0 when there is none
    r1 = np.float32(radius)
    r2 = r1 if prioritize_static else np.float32(1.5) * r1                        # :845

    def chain(k0, k1, r):
        pl = [dict(pose=placements[i]["pose"], pos=objects[placements[i]["object_idx"]]["pos"],
                   nor=objects[placements[i]["object_idx"]]["nor"], radius=r) for i in order[k0:k1]]
        return label_chain(scene_pos, scene_nor, pl, labels, mind, k0, tmin, inverse, cache, first=k0)

    t1 = chain(0, first_static, r1)                                               # :837-839
    if prioritize_static:
        mind[:] = np.float32(1e9)                                                 # :841-844
    t2 = chain(first_static, len(placements), r2)                                 # :846-848
    cls = np.full(n, unlabelled_class_idx, np.int32); inst = np.full(n, 1024, np.int32)      # :851-869
    lab = np.nonzero(labels)[0]
    if len(lab):
        who = order[labels[lab].astype(np.int64) - 1]
        cls[lab] = [objects[placements[i]["object_idx"]]["class_idx"] for i in who]
        inst[lab] = [placements[i]["uidx"] for i in who]
    return dict(labels=labels, min_dists=mind, order=order, class_ids=cls, instance_ids=inst, tied=t1[0] + t2[0],
                tie_dependent=t1[1] + t2[1])


def sorted_radii(objects, placements, radius, prioritize_static=False):
    """The sorted order of an arrangement and each sorted placement's radius (what a caller of the placement loop passes)."""
    key = np.array([(objects[p["object_idx"]]["is_static"] << 10) | objects[p["object_idx"]]["class_idx"] for p in placements], np.int64)
    order = np.argsort(key, kind="stable")
    stat = [objects[placements[i]["object_idx"]]["is_static"] for i in order]
    first_static = next((k for k, s in enumerate(stat) if s), 0)
    r1 = np.float32(radius)
    r2 = r1 if prioritize_static else np.float32(1.5) * r1
    return order, [r1 if k < first_static else r2 for k in range(len(order))]


# ---- inputs -----------------------------------------------------------------------------------------------------------------

LEVEL_FAMILIES = tuple(f for f in hc.FAMILIES if f != "contrast")
EDGE_TIE_FREE = ("offset_1e3", "negative", "planar", "lattice", "outside", "two_far", "contrast9000")
EDGE_TIED = ("offset_1e4", "collinear")
EDGE_K = 8
EDGE_R2 = 0.0025

_CACHE = {}


def family(name):
    if name not in _CACHE:
        _CACHE[name] = hc.make(name)
    return _CACHE[name]


def sorted_collinear():
    """The collinear family sorted by x: every point's earlier neighbours are all on one side, dependence chains hundreds deep."""
    p = family("collinear")["points"]
    return np.ascontiguousarray(p[np.argsort(p[:, 0], kind="stable")])


def raster_planar():
    """The planar family in raster order: rows of 1 cm in y, x ascending inside a row."""
    p = family("planar")["points"]
    row = np.floor(p[:, 1].astype(np.float64) / 0.01).astype(np.int64)
    return np.ascontiguousarray(p[np.lexsort((p[:, 0], row))])


def lattice(shape=(24, 20, 12), spacing=0.0625, origin=(0.5, -1.0, 0.25), shuffled=False):
    """An exact lattice (spacing and origin exact in binary): at radius 2 * spacing the (±2, 0, 0) neighbours have d² == r²."""
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    p = (g * spacing + np.array(origin)).astype(np.float32)
    if shuffled:
        p = p[np.random.default_rng(5).permutation(len(p))]
    return np.ascontiguousarray(p)


def repeated(with_normals=False):
    """The first 3000 points of offset_1e4, quantised to 2^-10 m, each three times, shuffled: coincident triples."""
    f = family("offset_1e4")
    p = (np.round(f["points"][:3000].astype(np.float64) * 1024.0) / 1024.0).astype(np.float32)
    o = np.random.default_rng(6).permutation(9000)
    pts = np.ascontiguousarray(np.repeat(p, 3, axis=0)[o])
    if with_normals:
        return pts, np.ascontiguousarray(np.repeat(f["normals"][:3000], 3, axis=0)[o])
    return pts


def contrast_subset():
    """9000 points of the contrast family, index order kept: (points, normals)."""
    f = family("contrast")
    sel = np.sort(np.random.default_rng(0).permutation(len(f["points"]))[:9000])
    return np.ascontiguousarray(f["points"][sel]), np.ascontiguousarray(f["normals"][sel])


def level_extra_inputs():
    """name -> (points, levels) beyond the families themselves."""
    return {"collinear_sorted": (sorted_collinear(), (1, 2, 4)), "planar_raster": (raster_planar(), (1, 2, 4)),
            "repeated": (repeated(), (1, 2, 4))}


def edge_input(name):
    """(points, normals) of a neighbourhood-graph input: a family, the contrast subset or the repeated-point cloud."""
    if name == "contrast9000":
        return contrast_subset()
    if name == "repeated":
        return repeated(with_normals=True)
    f = family(name)
    return f["points"], f["normals"]


def degenerate_normals(normals):
    """Every fourth normal zero, every fifth flipped, every seventh scaled by 2 (in that order of precedence)."""
    nor = np.array(normals, np.float32, copy=True)
    i = np.arange(len(nor))
    nor[i % 7 == 0] *= np.float32(2.0)
    nor[i % 5 == 0] *= np.float32(-1.0)
    nor[i % 4 == 0] = 0.0
    return nor


def zero_normals(scene_nor, objects):
    """Every eleventh scene normal and every ninth normal of every object set to zero: (scene normals, objects)."""
    sn = np.array(scene_nor, np.float32, copy=True)
    sn[::11] = 0.0
    out = []
    for o in objects:
        nor = np.array(o["nor"], np.float32, copy=True)
        nor[::9] = 0.0
        out.append(dict(o, nor=nor))
    return sn, out


def zero_normal_survivors(base, cache, scene_nor):
    """Which scene points must come out of the zero_normals run exactly as out of the run `base` with intact normals (whose
    brute-force nearest points are in `cache`): those whose own normal is intact and whose label, if any, was won on an object
    point whose normal is intact.  Zeroing a normal only turns gate passes into failures, so an earlier placement that now fails
    leaves the running minimum no smaller and a later one that failed before still fails: label and min_dist stay.  Every other
    labelled point loses that label (its own or its winner's dot is NaN).  Returns the boolean mask."""
    keep = np.asarray(scene_nor).any(axis=1)
    for lab in np.unique(base["labels"]):
        if lab:
            sel = np.nonzero(base["labels"] == lab)[0]
            keep[sel] &= cache[int(lab) - 1][1][sel] % 9 != 0        # label = sorted position + 1; zero_normals zeroes every ninth
    return keep


def cluster(m, radius, seed=0):
    """m points inside a ball of diameter radius / 2: every point has all m within `radius`."""
    rng = np.random.default_rng([seed, m])
    v = rng.normal(size=(m, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.ascontiguousarray((v * (rng.uniform(0, 1, (m, 1)) ** (1 / 3)) * (radius / 4.0) + np.array([0.3, -0.2, 0.7])).astype(np.float32))


def six_placements(f, seed=3):
    """The arrangement every family is labelled with: six placements of the family's cut object, in arrangement order
      0 a perturbed pose near the cut        1 the cut pose         2 every second object point at the cut pose again (a
      cross-placement tie on d²: the strict < keeps the earlier label)    3 outside the cloud's low corner (misses everything)
      4 a far perturbation                   5 a static copy at the cut pose (second pass, 1.5 * radius)
    with classes chosen so that the reference's sort changes the order (4, 0, 1, 2, 3, 5; 1 and 2 share a key).
    Returns (objects, placements)."""
    from rescan_amd import synth
    rng = np.random.default_rng(seed)
    o = f["obj"]
    cut = f["poses"][2] if f["name"] != "two_far" else np.eye(4, dtype=np.float32).ravel()
    half = dict(pos=np.ascontiguousarray(o["pos"][::2]), nor=np.ascontiguousarray(o["nor"][::2]))
    objects = [dict(pos=o["pos"], nor=o["nor"], class_idx=2, is_static=0), dict(pos=o["pos"], nor=o["nor"], class_idx=3, is_static=0),
               dict(class_idx=3, is_static=0, **half), dict(pos=o["pos"], nor=o["nor"], class_idx=7, is_static=0),
               dict(pos=o["pos"], nor=o["nor"], class_idx=1, is_static=0), dict(pos=o["pos"], nor=o["nor"], class_idx=0, is_static=1)]
    miss = np.eye(4, dtype=np.float32)
    miss[3, :3] = (f["points"].min(axis=0).astype(np.float64) - np.abs(o["pos"]).max() - 0.4).astype(np.float32)
    poses = [synth.perturbed_pose(cut, rng, 0.03, 0.01), cut, cut, miss.ravel(), synth.perturbed_pose(cut, rng, 0.3, 0.1), cut]
    placements = [dict(pose=np.ascontiguousarray(p, np.float32).ravel(), object_idx=k, uidx=100 + 7 * k) for k, p in enumerate(poses)]
    return objects, placements


def tiny_scenes(f, n):
    """Index sets of n scene points of a family: its first n points, and the n nearest the pose its object was cut at."""
    cut = f["poses"][2][12:15].astype(np.float64)
    near = np.argsort(np.linalg.norm(f["points"].astype(np.float64) - cut, axis=1), kind="stable")
    return np.arange(n), near[:n]


SHELL_RADIUS = 0.0625
SHELL_SHIFT = (1e4 + 0.3, -1e4 - 0.7, -5e3 + 0.1)


def shell(shifted=False):
    """One object point with normal +z and a scene around it at the edge of the radius: along the six axes and the eight
    diagonals at d = r (on the axes d² == r² exactly: excluded), at nextafter(r, 0) (included) and at 1.5 r, and on each of the
    six sides a block of 64 points more than r beyond the object's box (a wave of the scene cloud that misses the object's
    grid).  All normals +z.  shifted: pose and scene moved by the same float32 translation of about 1e4 m, where a coordinate
    step is 2^-10 m: nextafter(r, 0) would round back onto r, so the inner ring sits at r - 2^-9.
    Returns (scene_pos, scene_nor, object dict, pose)."""
    r = np.float32(SHELL_RADIUS)
    dirs = [np.eye(3)[a] * s for a in range(3) for s in (1.0, -1.0)]
    dirs += [np.array([sx, sy, sz]) / np.sqrt(3.0) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    rng = np.random.default_rng(9)
    pts = []
    inner = np.float32(r - 2.0 ** -9) if shifted else np.nextafter(r, np.float32(0.0))     # the next coordinate below r that survives the shift
    for d in (r, inner, np.float32(1.5) * r):
        pts += [(np.float64(d) * u).astype(np.float32) for u in dirs]
    pts = [np.array(pts, np.float32)]
    for a in range(3):
        for s in (1.0, -1.0):
            b = rng.uniform(-0.02, 0.02, (64, 3))
            b[:, a] = s * rng.uniform(1.2 * float(r), 3.0 * float(r), 64)
            pts.append(b.astype(np.float32))
    scene = np.concatenate(pts)
    pose = np.eye(4, dtype=np.float32)
    if shifted:
        t = np.array(SHELL_SHIFT, np.float32)
        scene = (scene + t[None, :]).astype(np.float32)
        pose[3, :3] = t
    nor = np.tile(np.float32([0.0, 0.0, 1.0]), (len(scene), 1))
    obj = dict(pos=np.zeros((1, 3), np.float32), nor=np.float32([[0.0, 0.0, 1.0]]), class_idx=4, is_static=0)
    return np.ascontiguousarray(scene), nor, obj, pose.ravel()


def lattice_ties():
    """Exact cross-object ties: the lattice family's points as the object (constant normals), its nodes plus half-spacing points,
    moved by a translation that is exact in binary, as the scene; radius = the spacing, so a half-spacing point has 2, 4 or 8
    equidistant nearest nodes and a node at the spacing itself (d² == r²) is excluded.  Returns (scene_pos, scene_nor, object,
    pose, radius)."""
    f = family("lattice")
    t = np.float32([2.0, -0.5, 0.25])
    q = f["queries"][:2048]
    scene = (q + t[None, :]).astype(np.float32)
    assert ((scene.astype(np.float64) - q.astype(np.float64)) == t.astype(np.float64)).all()          # exact
    nor = np.tile(np.float32([0.0, 0.6, 0.8]), (len(scene), 1))
    obj = dict(pos=f["points"], nor=np.tile(np.float32([0.0, 0.0, 1.0]), (len(f["points"]), 1)), class_idx=1, is_static=0)
    pose = np.eye(4, dtype=np.float32); pose[3, :3] = t
    return np.ascontiguousarray(scene), nor, obj, pose.ravel(), f["radius"]


def cap_arrangement(n_plc):
    """n_plc placements of 8-point objects over the first 2000 points of the negative family: placement k is scene points
    [8 k, 8 k + 8) in a frame centred on their mean, posed back where they came from, so each placement labels at least its own
    points.  Returns (scene_pos, scene_nor, objects, placements)."""
    f = family("negative")
    pts, nor = np.ascontiguousarray(f["points"][:2000]), np.ascontiguousarray(f["normals"][:2000])
    objects, placements = [], []
    for k in range(n_plc):
        sel = slice(8 * k, 8 * k + 8)
        c = pts[sel].astype(np.float64).mean(axis=0)
        objects.append(dict(pos=(pts[sel].astype(np.float64) - c).astype(np.float32), nor=np.ascontiguousarray(nor[sel]), class_idx=k % 5, is_static=0))
        P = np.eye(4, dtype=np.float32); P[3, :3] = c.astype(np.float32)
        placements.append(dict(pose=P.ravel(), object_idx=k, uidx=k))
    return pts, nor, objects, placements
