"""The cooperative ICP kernels (k_icp_corr_coop<2|4|8>) enumerate a shell once per workgroup: one row table of NW x 64 cell rows in
shared memory, one candidate stream over it dealt to the waves in chunks of 64 (rs_search.h: sweep_stream; rs_rowtable.h).  They
must return the bits they returned when every wave walked the shell in batches of 64 rows.

Which kernel a launch takes is latched at the library's first use, so every ROUTE below runs in a fresh child process (a new python
running this file as a script, under its own time limit) that writes what it computed to an .npz; the tests compare.  The children
run one after the other, and after one that failed none is started.

1. the table's own edges (CASES) against the numpy brute force below, which tests/test_coop_stream_cpu.py holds to the oracle:
   the nearest gated candidate, accepted iff fewer than 16 candidates precede it in (d², index).  Every case is built on a grid
   whose cell rows and stream length follow from its construction (grid_case), and the CPU test asserts them from the grid
   arithmetic: the search box of ANY subset of the queries covers the whole grid in y and z and, in x, exactly the placed points.
2. six warm iterations of tests/test_gpu_switches.py's pair (second shells that exclude the first, lanes that start from nothing in a
   warm call) and the nine icp_* golden calls: pose, error and iteration count bit-identical on all routes, to the default route of
   this process and to the fixtures."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

I4 = np.eye(4, dtype=np.float32).ravel()
R = np.float32(0.1)
MA = np.float32(np.deg2rad(60.0))
K = 16
N_ITER = 6
WHAT = ("c_pts1", "c_nor1", "c_pts2", "c_nor2", "weights")
PREFETCH = (1, 2, 3)             # chunks a wave may have in flight (RS_COOP_PREFETCH): streams of NW x 64 x d candidates end a ring exactly

# route -> environment of its child.  Launches of this size go straight to the cooperative kernel by default (every tile gets a
# workgroup); RS_HIP_COOP_ALL_BELOW=0 runs phase A first and queues what it hands off.
ROUTES = {}
for _nw in (2, 4, 8):
    ROUTES[f"coop{_nw}_all"] = {"RS_HIP_COOP_WAVES": str(_nw), "RS_HIP_COOP_ALL_BELOW": "1000000"}
    ROUTES[f"coop{_nw}_queue"] = {"RS_HIP_COOP_WAVES": str(_nw), "RS_HIP_COOP_ALL_BELOW": "0"}

UP = np.float32([0.0, 0.0, 1.0])
DOWN = np.float32([0.0, 0.0, -1.0])          # dot = -1 with UP: never passes the gate
EXTENT = 0.09                                # of the grid in y and z: less than the radius, so every query's reach covers all of it
PIN_X = -0.3                                 # two points far outside every query's reach in x pin the grid's corner and its size
X_SPAN = 0.01                                # the placed points and the queries lie in x in [0, X_SPAN]


# ---- cases on a grid of known rows ---------------------------------------------------------------------------------------------

def grid_case(h, d, placed, queries, normals=None):
    """A target whose grid has exactly h x d (y,z) cell rows of cubic cells of EXTENT / max(h, d), and whose whole-box sweep — from any
    query inside it — holds exactly the points of `placed`: a list of (row, count) or (row, points-in-the-unit-cell), row = z h + y
    as the sweep numbers them.  Returns the case and what it claims: dict(cell, rows, stream)."""
    s = EXTENT / max(h, d)
    pts = [[PIN_X, 0.0, 0.0], [PIN_X, (h - 0.5) * s, (d - 0.5) * s]]
    rng = np.random.default_rng(h * 1000 + d + len(placed))
    for row, what in placed:
        y, z = row % h, row // h
        assert 0 <= z < d, (row, h, d)
        u = rng.uniform(0.25, 0.75, (what, 3)) if np.isscalar(what) else np.asarray(what, np.float64)
        pts.extend(np.stack([u[:, 0] * X_SPAN, (y + u[:, 1]) * s, (z + u[:, 2]) * s], 1))
    tgt = np.asarray(pts, np.float32)
    nor = np.tile(UP, (len(tgt), 1)) if normals is None else np.concatenate([np.tile(UP, (2, 1)), np.asarray(normals, np.float32)])
    q = np.asarray(queries, np.float64)
    src = np.stack([q[:, 0] * X_SPAN, q[:, 1] * h * s, q[:, 2] * d * s], 1).astype(np.float32)
    return dict(src=src, src_nor=np.tile(UP, (len(src), 1)), tgt=tgt, tgt_nor=np.ascontiguousarray(nor, np.float32),
                cell=np.float32(s), rows=h * d, stream=len(tgt) - 2, h=h, d=d)


def _queries(rng, n, near=None):
    """n queries in the unit box, uniform — and, in front, copies of `near` (unit-box points) moved by a hair: they match those points"""
    q = rng.uniform(0.02, 0.98, (n, 3))
    if near is not None and len(near):
        q[:len(near)] = np.clip(np.asarray(near)[:n] + rng.normal(0.0, 1e-4, (min(n, len(near)), 3)), 0.0, 1.0)
    return q


# rows of one table and one row next to it, for 2, 4 and 8 waves: h x d
ROW_SHAPES = {127: (127, 1), 128: (64, 2), 129: (43, 3), 255: (85, 3), 256: (128, 2), 257: (257, 1), 511: (73, 7), 512: (256, 2), 513: (57, 9)}
STREAMS = sorted({0, 1, 63, 64, 65} | {nw * 64 * d + e for nw in (2, 4, 8) for d in PREFETCH for e in (-1, 0, 1)})


def make_cases():
    rng = np.random.default_rng(1701)
    cases = {}
    # whole-box sweeps of NW 64 - 1, NW 64 and NW 64 + 1 cell rows: a third of the rows occupied, in runs, ~1500 candidates; queries all
    # over the box, the first of them at the stream's last and first candidates
    for rows, (h, d) in ROW_SHAPES.items():
        occupied = [r for r in range(rows) if (r // 5) % 3 == 0 or r == rows - 1]
        placed = [(r, int(rng.integers(1, 8))) for r in occupied]
        ends = [((0.5, (r % h + 0.5) / h, (r // h + 0.5) / d)) for r in (occupied[-1], occupied[0], occupied[len(occupied) // 2])]
        cases[f"rows_{rows}"] = grid_case(h, d, placed, _queries(rng, 128, ends))
    # streams of 0, 1, 63, 64, 65 and NW 64 d - 1 / + 0 / + 1 candidates over 128 rows (one table for every NW)
    for n in STREAMS:
        cnt = np.bincount(rng.integers(0, 128, n), minlength=128)
        cases[f"stream_{n}"] = grid_case(64, 2, [(r, int(c)) for r, c in enumerate(cnt) if c], _queries(rng, 64))
    # the only candidates in the table's last row (of 512: the last entry of the last block at 8 waves, of a later super-batch at 2
    # and 4), and in the first row of a later wave's block
    for row in (511, 64, 128, 448):
        cases[f"only_row_{row}"] = grid_case(256, 2, [(row, 40)], _queries(rng, 64, [(0.5, (row % 256 + 0.5) / 256, (row // 256 + 0.5) / 2)]))
    # a tile outside the grid, within reach of it: queries 0.05 m below the grid in y
    c = grid_case(128, 2, [(r, 3) for r in range(0, 256, 2)], _queries(rng, 64))
    c["src"][:, 1] = np.float32(-0.05) + c["src"][:, 1] * np.float32(0.1)
    c["rows"] = c["stream"] = None              # (its sweep is clipped at the grid's face: no claim about its rows)
    cases["outside_within_reach"] = c
    # 15 / 16 / 17 candidates closer than the only gated one, the closer ones in the rows on both sides of every table edge of a shell
    # of 1152 rows (127 | 128, 255 | 256, 511 | 512, 1023 | 1024), the queries 1 m apart in x.  Distances: the query sits mid-row
    # range in y, the closer ones at the y ends (~0.045 m), the gated one 0.08 m away in x.
    h, d = 128, 9
    s = EXTENT / h
    edge_rows = [127, 128, 255, 256, 511, 512, 1023, 1024]
    tgt, nor, src = [], [], []
    for qi, n_closer in enumerate((15, 16, 17)):
        q = np.array([float(qi), 64.0 * s, 4.5 * s])
        src.append(q)
        for k in range(n_closer):
            row = edge_rows[k % len(edge_rows)]
            u = rng.uniform(0.25, 0.75, 3)
            tgt.append([q[0] + (u[0] - 0.5) * 0.004, (row % h + u[1]) * s, (row // h + u[2]) * s]); nor.append(DOWN)
        tgt.append(q + np.array([0.08, 0.0, 0.0])); nor.append(UP)
    pins = [[PIN_X, 0.0, 0.0], [PIN_X, (h - 0.5) * s, (d - 0.5) * s]]
    cases["rank_15_16_17"] = dict(src=np.asarray(src, np.float32), src_nor=np.tile(UP, (3, 1)), tgt=np.asarray(pins + tgt, np.float32),
                                  tgt_nor=np.ascontiguousarray([UP, UP] + nor, np.float32), cell=np.float32(s), rows=h * d, stream=len(tgt), h=h, d=d)
    # one sweep of more than two tables' worth of rows at any NW: cells of r / 16, a cloud all around the queries; one normal in
    # sixteen passes the gate, so that the nearest gated candidate has about sixteen before it: rank passes run and go both ways
    tgt = rng.uniform(0.0, 0.4, (4000, 3)).astype(np.float32)
    tn = np.where(rng.uniform(size=(4000, 1)) < 1.0 / 16.0, UP, DOWN).astype(np.float32)
    src = rng.uniform(0.16, 0.24, (192, 3)).astype(np.float32)
    cases["cells_r16"] = dict(src=src, src_nor=np.tile(UP, (len(src), 1)), tgt=tgt, tgt_nor=tn, cell=np.float32(float(R) / 16.0), rows=None, stream=None)
    return cases


def axis_cells(lo, hi, r, gmin, cell, dim):
    """rs_search.h's axis_range in its own float32 arithmetic: cells of one axis within r of [lo, hi], clipped to the grid"""
    f = np.float32
    inv = f(1.0) / f(cell)
    a = np.floor((f(lo) - f(r) - f(gmin)) * inv - f(0.01))
    b = np.floor((f(hi) + f(r) - f(gmin)) * inv + f(0.01))
    a = min(max(a, f(0.0)), f(16777216.0)); b = min(max(b, f(-1.0)), f(16777216.0))
    c0, c1 = int(a), min(int(b), dim - 1)
    return (c0, c1) if c1 >= c0 else (c0, -1)


def grid_of(c):
    """(min corner, dims) as the library lays the target's grid out: rs_buildplan.h (bp_table_dims)"""
    mn, mx = c["tgt"].min(0), c["tgt"].max(0)
    dims = [int(np.floor((float(mx[a]) - float(mn[a])) / float(c["cell"]))) + 1 for a in range(3)]
    return mn, dims


def brute_find_corrs(c, radius=R, k=K):
    """The reference's rule restated on all pairs (identity poses): rows of the sources that have a correspondence, and the target's index."""
    r2 = np.float32(np.float64(radius) * np.float64(radius))
    rows, idx = [], []
    tgt, tn = c["tgt"], c["tgt_nor"]
    for i, (q, n) in enumerate(zip(c["src"], c["src_nor"])):
        v = tgt - q
        d2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        dot = (tn[:, 0] * n[0] + tn[:, 1] * n[1]) + tn[:, 2] * n[2]
        dc = np.maximum(dot, np.float32(0.0))
        ok = (d2 < r2) & (dc >= np.float32(np.cos(np.float64(MA)))) & (dc <= np.float32(1.0))
        if not ok.any():
            continue
        cand = np.nonzero(ok)[0]
        w = cand[np.lexsort((cand, d2[cand]))[0]]
        before = (d2 < r2) & ((d2 < d2[w]) | ((d2 == d2[w]) & (np.arange(len(tgt)) < w)))
        if before.sum() < k:
            rows.append(i); idx.append(w)
    return np.asarray(rows, np.int64), np.asarray(idx, np.int64)


_CASES, _BRUTE = {}, {}


def cases():
    if not _CASES:
        _CASES.update(make_cases())
    return _CASES


def brute(name):
    """computed once per session, shared by the tests of every route"""
    if name not in _BRUTE:
        _BRUTE[name] = brute_find_corrs(cases()[name])
    return _BRUTE[name]


def assert_brute(name, got, what):
    c = cases()[name]
    rows, idx = brute(name)
    assert len(got[0]) == len(rows), (what, len(got[0]), len(rows))
    for a, b, field in zip((c["src"][rows], c["src_nor"][rows], c["tgt"][idx], c["tgt_nor"][idx]), got, WHAT):
        assert a.astype(np.float32).tobytes() == np.ascontiguousarray(b).tobytes(), (what, field)


# ---- the children ----------------------------------------------------------------------------------------------------------------

def switches_pair(capi):
    """tests/test_gpu_switches.py's pair: (source cloud, target cloud, start pose)."""
    from rescan_amd import synth
    s = synth.make_scene(seed=3, density=860.0, timestep=1)
    pos, nor = synth.make_object("table", 3 * 7919, 1125.0, 1.0, 0.0)
    src = capi.Cloud(np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(nor, np.float32), cell_size=0.1)
    tgt = capi.Cloud(s["points"], s["normals"], cell_size=0.1)
    return src, tgt, synth.perturbed_pose(s["objects"][0]["pose"], np.random.default_rng(5))


def golden_names():
    return sorted(f for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("icp_"))


def compute(capi):
    """Everything a route is asked for, as a flat dict of arrays."""
    out = {}
    for name, c in cases().items():
        oc = capi.Cloud(c["src"], c["src_nor"])
        scn = capi.Cloud(c["tgt"], c["tgt_nor"], cell_size=float(c["cell"]))
        for a, what in zip(capi.icp_find_corrs(oc, scn, I4, I4, R, MA), WHAT):
            out[f"case/{name}/{what}"] = a
        scn.close(); oc.close()
    src, tgt, T0 = switches_pair(capi)
    err, T, it = capi.icp_align(src, tgt, T0, I4, 0.1, MA, max_iter=N_ITER, fixed_iters=True)
    out["warm"] = np.frombuffer(np.float32(err).tobytes() + np.asarray(T, np.float32).tobytes() + np.int32(it).tobytes(), np.uint8)
    src.close(); tgt.close()
    sc = dict(np.load(os.path.join(HERE, "golden", "scene.npz")))
    clouds = {r: capi.Cloud(sc["points"], sc["normals"], cell_size=2 * r) for r in (0.05, 0.1)}
    clouds[0.075] = capi.Cloud(sc["points"], sc["normals"])
    objs = [capi.Cloud(sc[f"obj{i}_pos"], sc[f"obj{i}_nor"], cell_size=0.1) for i in range(int(sc["n_obj"]))]
    for fname in golden_names():
        g = dict(np.load(os.path.join(HERE, "golden", fname)))
        md = float(g["max_dist"])
        err, T, it = capi.icp_align(objs[int(g["obj"])], clouds[round(md, 3)], g["T1"], g["T2"], md, g["max_angle"])
        out[f"golden/{fname}"] = np.frombuffer(np.float32(err).tobytes() + np.asarray(T, np.float32).tobytes() + np.int32(it).tobytes(), np.uint8)
    return out


def child_main(path):
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()                  # (torch's copy of the HIP runtime first: tests/conftest.py)
    except ImportError:
        pass
    from rescan_amd import capi
    capi.init(0)
    np.savez(path, **compute(capi))


_ROUTE = {}
_FAILED = []


def route(name, tmp_path_factory):
    """The results of route `name`: its child runs once per session, under its own time limit; a failed child fails the test, and
    after a child that failed (a fault, an abort, a time limit) no further child is started."""
    if name not in _ROUTE:
        assert not _FAILED, f"not started: the child of route {_FAILED[0]} failed"
        path = str(tmp_path_factory.mktemp("coop_stream") / (name + ".npz"))
        env = {k: v for k, v in os.environ.items() if not k.startswith("RS_HIP_") or k == "RS_HIP_LIB"}
        env.update(ROUTES[name])
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), path]
        try:
            p = subprocess.run(cmd, env=env, timeout=60, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            _FAILED.append(name)
            raise
        if p.returncode != 0:
            _FAILED.append(name)
        assert p.returncode == 0, (name, p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        _ROUTE[name] = dict(np.load(path))
    return _ROUTE[name]


@pytest.fixture(scope="module")
def capi():
    from rescan_amd import capi as c
    c.init(0)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROUTES))
def test_edges_of_the_row_table(tmp_path_factory, name):
    got = route(name, tmp_path_factory)
    for cname in cases():
        assert_brute(cname, [got[f"case/{cname}/{w}"] for w in WHAT], (name, cname))


@pytest.mark.gpu
def test_all_routes_carry_the_same_bits(capi, tmp_path_factory):
    """The route this process takes by itself against the brute force, the fixtures and every child: the warm iterations and the
    golden calls carry the same bits everywhere.  None of the library's names is in the environment meanwhile."""
    saved = {k: v for k, v in os.environ.items() if k.startswith("RS_HIP_") and k != "RS_HIP_LIB"}
    for k in saved:
        del os.environ[k]
    try:
        base = compute(capi)
    finally:
        os.environ.update(saved)
    assert int(np.frombuffer(base["warm"].tobytes()[-4:], np.int32)[0]) == N_ITER
    for fname in golden_names():
        g = dict(np.load(os.path.join(HERE, "golden", fname)))
        want = np.float32(g["err"]).tobytes() + np.asarray(g["T_out"], np.float32).ravel().tobytes() + np.int32(g["iters"]).tobytes()
        assert base[f"golden/{fname}"].tobytes() == want, fname
    for cname in cases():
        assert_brute(cname, [base[f"case/{cname}/{w}"] for w in WHAT], ("default", cname))
    for name in ROUTES:
        got = route(name, tmp_path_factory)
        assert got["warm"].tobytes() == base["warm"].tobytes(), name
        for fname in golden_names():
            assert got[f"golden/{fname}"].tobytes() == base[f"golden/{fname}"].tobytes(), (name, fname)


if __name__ == "__main__":
    child_main(sys.argv[1])
