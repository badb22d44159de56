"""Seeded clouds on which the index build (rescan_amd/csrc/rs_buildplan.h, rs_build.hip, rs_cloud_api.hip: cloud_create_impl) is easy to get wrong without
any search noticing, in the style of tests/hard_clouds.py, whose families are reused as they are.

A family is a dict: name, points (n, 3) float32, normals (n, 3) float32 or None, cells: the cell sizes it is built with (LAYOUTS unless
the family is about one explicit cell).  The reference is tests/build_restate.py.
"""
import numpy as np

import hard_clouds as hc

F = np.float32
FLT_MAX = np.finfo(np.float32).max
R = 0.05                                                   # the radius the layouts `2r` and `0.4r` are named after
LAYOUTS = (("auto", -1.0), ("2r", 2 * R), ("0.4r", 0.4 * R), ("brute", 0.0))

SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097)
SHAPES = ("blob", "stones", "clusters")
CELL_EDGES = ("cell_edges", "lattice_0p1")
HOSTILE = ("one_pinf", "one_ninf", "both_inf", "axis_nan", "all_nonfinite", "coincident", "zeros_denormals", "extent_1e-40",
           "far_1e10", "far_1e30", "flt_max", "fine_cell")
CLUSTER_MAX = 70


def _rng(*key):
    return np.random.default_rng([17] + [int(k) for k in key])


def cluster_sizes(n):
    """1, 2, .. 70, 1, 2, .. cut at n points"""
    out, k = [], 0
    while sum(out) < n:
        out.append(min(1 + k % CLUSTER_MAX, n - sum(out))); k += 1
    return out


def shape(name, n):
    """blob: dense, every tile is full.  stones: neighbours 0.5 m apart on a line (in a shuffled order): every tile has one point
    and the chain the pointer doubling covers has n nodes.  clusters: tight clusters of 1 .. 70 points on a 0.75 m lattice, so the
    tile lengths follow the cluster sizes, cut at 64 and across the 64-point blocks of k_build_tile_next."""
    rng = _rng(SHAPES.index(name), n)
    if name == "blob":
        p = rng.uniform(0.0, 0.05, (n, 3)) + np.array([1.0, -2.0, 0.5])
    elif name == "stones":
        p = np.zeros((n, 3)); p[:, 0] = 0.5 * rng.permutation(n); p[:, 1] = 0.25; p[:, 2] = -1.0
    elif name == "clusters":
        sizes = cluster_sizes(n)
        side = int(np.ceil(len(sizes) ** (1.0 / 3.0))) if sizes else 1
        cen = np.array([(k % side, (k // side) % side, k // (side * side)) for k in range(len(sizes))], np.float64).reshape(-1, 3) * 0.75
        p = np.concatenate([cen[k] + rng.uniform(0.0, 1e-4, (m, 3)) for k, m in enumerate(sizes)]) if sizes else np.zeros((0, 3))
        p = p[rng.permutation(n)]
    else:
        raise KeyError(name)
    return dict(name=f"{name}_{n}", points=np.ascontiguousarray(p, F).reshape(-1, 3), normals=None, cells=LAYOUTS)


def extent_pair(limit, axis, ulps):
    """two points whose separation on one axis is `limit` (ulps = 0) or that many float32 steps more; the other axes coincide"""
    d = F(limit)
    for _ in range(ulps):
        d = np.nextafter(d, F(np.inf))
    p = np.zeros((2, 3), F)
    p[1, axis] = d
    assert F(p[1, axis] - p[0, axis]) == d
    return p


def _box(rng, n=1000):
    return rng.uniform(0.0, 5.0, (n, 3)).astype(F)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def make(name):
    fams = CELL_EDGES + HOSTILE
    rng = _rng(100 + fams.index(name))
    cells, nor = LAYOUTS, None
    if name == "cell_edges":
        # on k * 0.25, one float32 step either side, and on the box maximum (where the cell is clamped to dim - 1); the box minimum is
        # one step above 0.25, which the subtraction loses for the larger coordinates: their fp32 cell is one above the exact one
        k = rng.integers(2, 21, (1000, 3)).astype(F) * F(0.25)
        step = rng.integers(-1, 2, (1000, 3))
        p = np.where(step < 0, np.nextafter(k, F(-np.inf)), np.where(step > 0, np.nextafter(k, F(np.inf)), k)).astype(F)
        p[0] = np.nextafter(F(0.25), F(np.inf)); p[1] = np.nextafter(F(5.0), F(np.inf)); p[2] = (p[0, 0], p[1, 1], F(2.5))
        cells = (("0.25", 0.25),)
    elif name == "lattice_0p1":
        # k * 0.1f: floorf((v - min) * inv_cell) lands on k for some points and on k - 1 for others
        p = rng.integers(0, 40, (1000, 3)).astype(F) * F(0.1)
        p[0] = 0.0; p[1] = F(39) * F(0.1)
        cells = (("0.1", 0.1),)
    elif name == "one_pinf":
        p = _box(rng); p[7, 0] = np.inf
    elif name == "one_ninf":
        p = _box(rng); p[11, 1] = -np.inf
    elif name == "both_inf":
        p = _box(rng); p[7, 0] = np.inf; p[11, 1] = -np.inf; p[13] = (np.inf, -np.inf, np.nan); p[500, 2] = -np.inf; p[501, 2] = np.inf
    elif name == "axis_nan":
        p = _box(rng); p[:, 2] = np.nan
    elif name == "all_nonfinite":
        p = _box(rng)
        bad = np.array([np.nan, np.inf, -np.inf], F)
        p[np.arange(1000), rng.integers(0, 3, 1000)] = bad[rng.integers(0, 3, 1000)]
        p[:8] = bad[rng.integers(0, 3, (8, 3))]
    elif name == "coincident":
        p = np.tile(F([1.25, -0.75, 3.0]), (1000, 1))
    elif name == "zeros_denormals":
        vals = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 1e-3, 0.01], F)
        p = vals[rng.integers(0, len(vals), (1000, 3))]
    elif name == "extent_1e-40":
        p = np.array([0.0, 1e-40], F)[rng.integers(0, 2, (1000, 3))] + F(0.0)
        p[0] = 0.0; p[1] = F(1e-40)
    elif name in ("far_1e10", "far_1e30"):
        p = _box(rng); p[3, 0] = F(1e10 if name == "far_1e10" else 1e30)
    elif name == "flt_max":
        p = _box(rng); p[3, 0] = FLT_MAX; p[4, 0] = -FLT_MAX; p[5, 1] = FLT_MAX; p[6] = (-FLT_MAX, FLT_MAX, F(1.0))
    elif name == "fine_cell":
        p = _box(rng)
        cells = (("0.001", 0.001),)                                       # 5000^3 cells: the coarsening loop
    else:
        raise KeyError(name)
    if name in ("one_pinf", "coincident", "far_1e10", "cell_edges"):
        nor = _unit(rng, len(p))
    return dict(name=name, points=np.ascontiguousarray(p, F), normals=nor, cells=cells)


def from_hc(name):
    f = hc.make(name)
    return dict(name="hc_" + name, points=f["points"], normals=f["normals"], cells=LAYOUTS)


def all_families(sizes=True, hard_clouds=True):
    """every family as (name, maker): shapes at every size, the cell edges, the non-finite and far clouds, tests/hard_clouds.py's"""
    out = []
    if sizes:
        out += [(f"{s}_{n}", (lambda s=s, n=n: shape(s, n))) for s in SHAPES for n in SIZES]
    out += [(k, (lambda k=k: make(k))) for k in CELL_EDGES + HOSTILE]
    if hard_clouds:
        out += [("hc_" + k, (lambda k=k: from_hc(k))) for k in hc.FAMILIES]
    return out


def finite_rows(p):
    return np.isfinite(p).all(axis=1)


def float64_cells(p, mn, cell, dims):
    """the cell of every coordinate in exact arithmetic on the float32 inputs (what fp32 rounding is compared with)"""
    c = np.floor((p.astype(np.float64) - mn.astype(np.float64)[None, :]) / np.float64(F(cell)))
    return np.clip(c, 0, dims[None, :] - 1).astype(np.int64)
