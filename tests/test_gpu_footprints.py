"""GPU: rs_hip_coverage_footprints against the restatement (tests/footprint_restate.py), cell for cell, and the unions of its
footprints (rs_hip_footprints_scores) against the REFERENCE's own counts and score bits (tests/golden/arrange_*.npz) and against
rs_hip_coverage_scores on the same arrangements; the LDS route, the slab route and both in one call, with the route counters
predicted from the sub-boxes; repeated calls and released buffers; the hostile candidates of tests/hard_shapes.py; the edges of the
compaction on a synthetic 64^3 grid; the shim.  No tolerances: every compared quantity is an integer or a float's bits."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
import ao_restate as R
import footprint_restate as FR
from test_arrange_cpu import NAMES, fixture, hard_fixture, trials
from test_footprints_cpu import HARD, hard_footprints, trial_footprints

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def capi():
    from rescan_amd import build, capi as m
    build.build()
    m.init(0)
    return m


@pytest.fixture(scope="module")
def cases(capi):
    """Per fixture: the arrays, the objects' device clouds, the coverage objects and, per trial, the restated footprints (computed
    once, shared, never modified)."""
    out = {}
    for name in NAMES:
        g = fixture(name)
        clouds = [capi.Cloud(p) for p in g["objects"]]
        pos2, q2 = np.ascontiguousarray(g["pos0"][g["sub"]]), np.ascontiguousarray(g["sal0_quality"][g["sub"]])
        cov = [capi.Coverage(g["bbox_min"], g["bbox_max"], pos2, q2, float(g[f"cov{j}_voxel"]), float(g[f"cov{j}_threshold"])) for j in range(3)]
        want = {(j, t): trial_footprints(g, j, base, cand) for j, t, pre, base, cand in trials(g)}
        out[name] = (g, clouds, cov, want)
    return out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_cells(fp, fps):
    assert fp.n_placements == len(fps) and fp.offsets.tolist() == FR.csr(fps)[0].tolist()
    for k, f in enumerate(fps):
        got = fp.cells(k)
        assert got.dtype == np.int32 and got.tolist() == f.tolist(), (k, got[:8], f[:8])


def routes(need, budget):
    return sum(b <= budget for b in need), sum(b > budget for b in need)


@pytest.mark.parametrize("name", NAMES)
def test_room_footprints_and_their_unions(capi, cases, name):
    g, clouds, covs, want = cases[name]
    low = int(g["low_lds_budget"])
    default = capi.coverage_lds_budget(-1)
    both = 0
    try:
        for j, t, pre, base, cand in trials(g):
            cov = covs[j]
            plc, fps, need = want[(j, t)]
            P = [(None if s else clouds[o], p, s) for o, p, s in plc]                  # (a static placement needs no cloud)
            nb = len(base)
            arr = [list(range(nb))] + [list(range(nb)) + [nb + k] for k in range(len(cand))]
            for budget in (default, low, 0):
                capi.coverage_lds_budget(budget)
                capi.coverage_footprint_routes(reset=True)
                fp = cov.footprints(P)
                assert capi.coverage_footprint_routes() == routes(need, budget), (j, t, budget)
                assert (fp.n_cells, fp.valid_cells) == (cov.n_cells, cov.valid_cells)
                same_cells(fp, fps)
                sc, ag = fp.scores(arr)
                assert ag[0] == int(g[pre + "base_agree"]) and bits(sc)[0] == bits(g[pre + "base_score"])[0], (j, t, budget)
                assert (ag[1:] == g[pre + "agree"]).all() and (bits(sc[1:]) == bits(g[pre + "score"])).all(), (j, t, budget)
                if budget == low and j == 0 and cand:
                    n_lds, n_slab = capi.coverage_footprint_routes()
                    assert n_slab > 0 and sum(0 < b <= low for b in need) > 0           # both routes in one call
                    both += 1
                if budget == default:
                    assert capi.coverage_footprint_routes()[1] == 0                   # 5 cm and 15 cm rooms: every sub-box fits the LDS budget
                    # the same numbers from whole arrangements on the device
                    full = [[(clouds[o], p, s) for o, p, s in (plc[m] for m in a)] for a in arr]
                    sc_full, ag_full = cov.scores(full)
                    assert (ag == ag_full).all() and (bits(sc) == bits(sc_full)).all()
                    same_cells(cov.footprints(P), fps)                                 # a second call
        assert both >= 2
        # released buffers (the slab's among them) are allocated again
        j, t, pre, base, cand = next(x for x in trials(g) if x[0] == 0 and x[4])
        plc, fps, need = want[(j, t)]
        P = [(None if s else clouds[o], p, s) for o, p, s in plc]
        capi.coverage_lds_budget(low)
        same_cells(covs[j].footprints(P), fps)
        capi.arrange_release()
        capi.arrange_release()                                                         # nothing held: still fine
        same_cells(covs[j].footprints(P), fps)
    finally:
        capi.coverage_lds_budget(default)


@pytest.mark.parametrize("voxel,cell0", HARD)
def test_hard_footprints_and_their_unions(capi, voxel, cell0):
    """The hostile candidates of tests/hard_shapes.py — 5 000 points in three cells, 255 / 256 / 257-point clouds, off the grid, empty,
    NaN and infinite points, points on cell faces, an object wholly on inactive cells — as footprints, at the default budget, at the
    rod's own sub-box (it stays in LDS), 4 bytes below (it goes to the slab) and at 0."""
    import hard_shapes as H
    hard = hard_fixture()
    a, grid, plc, fps, need = hard_footprints(voxel, cell0)
    pre = H.arr_key("cov", voxel, cell0)
    assert (hard[pre + "crc"] == H.cloud_crcs(a["scene"], a["objects"])).all()
    clouds = [capi.Cloud(p, None, 0.0) for p in a["objects"]]
    cov = capi.Coverage(H.ARR_BMIN, H.ARR_BMAX, a["scene"], None, voxel, 0.0)
    assert cov.scene_grid().tobytes() == grid.tobytes() and cov.valid_cells == int(hard[pre + "valid"])
    P = [(clouds[o], p, s) for o, p, s in plc]
    nb = len(a["base"])
    arr = [list(range(nb))] + [list(range(nb)) + [nb + k] for k in range(len(a["cands"]))]
    rod = need[nb + a["names"].index("rod")]
    default = capi.coverage_lds_budget(-1)
    try:
        for budget in (default, rod, rod - 4, 0):
            capi.coverage_lds_budget(budget)
            capi.coverage_footprint_routes(reset=True)
            fp = cov.footprints(P)
            assert capi.coverage_footprint_routes() == routes(need, budget), budget
            same_cells(fp, fps)
            sc, ag = fp.scores(arr)
            assert ag[0] == int(hard[pre + "base_agree"]) and bits(sc)[0] == bits(hard[pre + "base_score"])[0]
            assert (ag[1:] == hard[pre + "agree"]).all() and (bits(sc[1:]) == bits(hard[pre + "score"])).all(), budget
        assert routes(need, rod)[1] + 1 == routes(need, rod - 4)[1] and rod <= default
    finally:
        capi.coverage_lds_budget(default)


EDGE_BMAX = np.full(3, 2.525, F)          # 64 cells per axis at 5 cm: ceilf( ( 2.525 + 0.6 ) / 0.05 ) + 1
EDGE_ACTIVE_Y = 56                        # the scene's active cells: the solid block y < 56


def edge_placements():
    """(names, cell lists [n, 3] as (x, y, z)) of the compaction's edges on the 64^3 grid."""
    out = []
    line = lambda n: np.array([[1 + i % 16, 2, 1 + i // 16] for i in range(n)], np.int64).reshape(-1, 3)     # noqa: E731  (a 16-wide strip, row by row)
    for n in (1, 31, 32, 33, 255, 256, 257):
        out.append((f"cells_{n}", line(n)))
    out.append(("cells_0", np.array([[3, EDGE_ACTIVE_Y, 3], [9, 60, 9], [63, 63, 63]])))                       # on inactive cells only
    out.append(("run_word_boundary", np.array([[x, 5, 7] for x in range(64)])))                                # bits 0 .. 63: two full words
    out.append(("run_bit_31", np.array([[x, 5, 7] for x in range(31, 64)] + [[x, 5, 8] for x in range(31)])))  # bits 31 .. 94: a straddled word either side of a full one
    rng = np.random.default_rng(4097)

    def box(lo, ext, n_inside):
        lo, ext = np.array(lo), np.array(ext)
        inside = lo[None, :] + rng.integers(0, ext, (n_inside, 3))
        return np.concatenate([[lo], [lo + ext - 1], inside])
    out.append(("box_255_words", box((2, 1, 3), (60, 8, 17), 300)))            # 8160 bits
    out.append(("box_256_words", box((0, 9, 5), (64, 8, 16), 300)))            # 8192 bits
    out.append(("box_257_words", box((7, 20, 11), (50, 4, 41), 300)))          # 8200 bits: the last word holds 8 of them
    out.append(("box_4096_words", box((0, 3, 0), (64, 32, 64), 900)))          # 131072 bits = 16384 bytes: the LDS budget exactly
    out.append(("box_4097_words", box((5, 2, 9), (57, 46, 50), 900)))          # 131100 bits: one word more, a partial one
    out.append(("twin_a", line(40)))
    out.append(("twin_b", np.concatenate([line(40)[::-1], line(40)[::3]])))    # the same cells in another order, some of them twice
    return [n for n, _ in out], [c for _, c in out]


def test_compaction_edges(capi):
    import hard_shapes as H
    voxel = 0.05
    bmin = np.zeros(3, F)
    origin, res = R.grid_shape(bmin, EDGE_BMAX, voxel)
    assert res.tolist() == [64, 64, 64]
    g = np.stack(np.meshgrid(np.arange(64), np.arange(EDGE_ACTIVE_Y), np.arange(64), indexing="ij"), -1).reshape(-1, 3)
    scene = H.centres(g, voxel)
    grid = R.scene_grid(bmin, EDGE_BMAX, voxel, scene, None, 0.0)
    assert int(grid.sum()) == 64 * EDGE_ACTIVE_Y * 64 and grid[: 64 * 64 * EDGE_ACTIVE_Y].all()      # (y-major: the block is the first 56 planes)
    names, cells = edge_placements()
    objects = [H.centres(c, voxel) for c in cells]
    for c, pts in zip(cells, objects):                                                  # the centres fall into the cells they were made for
        assert (R.cells(origin, res, voxel, pts) == c[:, 1] * 4096 + c[:, 2] * 64 + c[:, 0]).all()
    plc = [(0, H.I16, 1)] + [(k, H.I16, 0) for k in range(len(objects))] + [(0, H.I16, 1)]     # the first and the last placement are static
    args = (grid, bmin, EDGE_BMAX, voxel, objects)
    fps = [FR.footprint(*args, p) for p in plc]
    need = [FR.footprint_box_bytes(*args, p) for p in plc]
    by = {n: (f, b) for n, f, b in zip(names, fps[1:-1], need[1:-1])}
    for n in (0, 1, 31, 32, 33, 255, 256, 257):
        assert len(by[f"cells_{n}"][0]) == n
    assert len(by["run_word_boundary"][0]) == 64 and by["run_word_boundary"][1] == 8
    assert len(by["run_bit_31"][0]) == 64 and by["run_bit_31"][1] == 16 and (np.diff(by["run_bit_31"][0]) == 1).all()
    assert [by[f"box_{w}_words"][1] for w in (255, 256, 257, 4096, 4097)] == [255 * 4, 256 * 4, 257 * 4, 16384, 16388]
    assert by["twin_a"][0].tolist() == by["twin_b"][0].tolist() and len(fps[0]) == len(fps[-1]) == 0
    clouds = [capi.Cloud(p, None, 0.0) for p in objects]
    cov = capi.Coverage(bmin, EDGE_BMAX, scene, None, voxel, 0.0)
    assert cov.scene_grid().tobytes() == grid.tobytes()
    P = [(None if s else clouds[o], p, s) for o, p, s in plc]
    default = capi.coverage_lds_budget(-1)
    assert default == 16384
    try:
        for budget in (default, 0):
            capi.coverage_lds_budget(budget)
            capi.coverage_footprint_routes(reset=True)
            fp = cov.footprints(P)
            assert capi.coverage_footprint_routes() == routes(need, budget)
            if budget == default:
                assert routes(need, budget)[1] == 1                                     # the 4 097-word box alone
            same_cells(fp, fps)
            twins = [1 + names.index("twin_a"), 1 + names.index("twin_b")]
            sc, ag = fp.scores([twins, twins[:1], list(range(len(P)))])
            assert ag[0] == ag[1] == 40 and ag[2] == len(np.unique(np.concatenate(fps)))
            assert bits(sc).tolist() == bits([F(a) / F(cov.valid_cells) for a in ag]).tolist()
        capi.coverage_lds_budget(default)
        capi.coverage_footprint_routes(reset=True)
        none = cov.footprints([])
        assert none.n_placements == 0 and none.offsets.tolist() == [0] and capi.coverage_footprint_routes() == (0, 0)
        assert none.scores([[]])[1].tolist() == [0]
        only_static = cov.footprints([(None, H.I16, 1), (None, H.I16, 1)])
        assert only_static.offsets.tolist() == [0, 0, 0]
    finally:
        capi.coverage_lds_budget(default)


def test_the_shim_gives_the_same(capi, cases):
    g, clouds, covs, want = cases[NAMES[0]]
    lib = C.CDLL(os.path.join(ROOT, "rescan_amd", "librescan_dropin.so"))
    vp, i32, f = C.c_void_p, C.c_int32, C.c_float
    j, t, pre, base, cand = next(x for x in trials(g) if x[0] == 0 and x[3] and x[4])
    plc, fps, _ = want[(j, t)]
    objs = [np.ascontiguousarray(o, F) for o in g["objects"]]
    bmin, bmax = np.ascontiguousarray(g["bbox_min"], F), np.ascontiguousarray(g["bbox_max"], F)
    pos2, q2 = np.ascontiguousarray(g["pos0"][g["sub"]], F), np.ascontiguousarray(g["sal0_quality"][g["sub"]], F)
    lib.rsd_coverage_create.restype = vp
    lib.rsd_coverage_create.argtypes = [vp, vp, f, vp, vp, i32, f]
    lib.rsd_coverage_destroy.argtypes = [vp]
    mk = lib.rsd_coverage_footprints; mk.restype = vp; mk.argtypes = [vp, vp, vp, vp, vp, i32]
    score = lib.rsd_footprints_score; score.restype = f; score.argtypes = [vp, vp, i32]
    lib.rsd_footprints_destroy.argtypes = [vp]
    h = lib.rsd_coverage_create(bmin.ctypes.data, bmax.ctypes.data, float(g[f"cov{j}_voxel"]), pos2.ctypes.data, q2.ctypes.data, len(pos2), float(g[f"cov{j}_threshold"]))
    assert h
    ptr = (vp * len(plc))(*[None if s else objs[o].ctypes.data for o, _, s in plc])
    n = np.array([len(objs[o]) for o, _, _ in plc], np.int32)
    poses = np.ascontiguousarray([np.asarray(p, F).ravel() for _, p, _ in plc], F)
    stat = np.array([s for _, _, s in plc], np.int32)
    fh = mk(h, C.addressof(ptr), n.ctypes.data, poses.ctypes.data, stat.ctypes.data, len(plc))
    assert fh
    native = covs[j].footprints([(None if s else clouds[o], p, s) for o, p, s in plc])
    nb = len(base)
    arr = [list(range(nb))] + [list(range(nb)) + [nb + k] for k in range(len(cand))]
    sc, _ = native.scores(arr)
    members = [np.array(a, np.int32) for a in arr]
    got = np.array([score(fh, m.ctypes.data, len(m)) for m in members], F)
    assert (bits(got) == bits(sc)).all() and bits(got)[0] == bits(g[pre + "base_score"])[0] and (bits(got[1:]) == bits(g[pre + "score"])).all()
    lib.rsd_footprints_destroy(fh)
    lib.rsd_coverage_destroy(h)
