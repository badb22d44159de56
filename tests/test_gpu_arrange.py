"""GPU: rs_hip_scene_saliency and rs_hip_coverage_extensions against the reference's own numbers (tests/golden/arrange_*.npz,
tools/arrange_fixture), byte for byte and bit for bit: saliency grid and qualities; every candidate's count and score bits, also
against rs_hip_coverage_scores on base + candidate computed here; the LDS route and the global-slab route; two consecutive calls;
and the same through the shim's rsd_scene_saliency / rsd_coverage_extensions; the hostile cases of tests/hard_shapes.py against
arrange_hard.npz.  No tolerances: every compared quantity is an integer,
a 0 / 1 float or a float whose bits the reference fixes."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from test_arrange_cpu import NAMES, fixture, hard_fixture, trials

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
    """Per fixture: the arrays, the objects' device clouds (shared by every test, never modified) and the coverage objects."""
    out = {}
    for name in NAMES:
        g = fixture(name)
        clouds = [capi.Cloud(p) for p in g["objects"]]
        pos2, q2 = np.ascontiguousarray(g["pos0"][g["sub"]]), np.ascontiguousarray(g["sal0_quality"][g["sub"]])
        cov = [capi.Coverage(g["bbox_min"], g["bbox_max"], pos2, q2, float(g[f"cov{j}_voxel"]), float(g[f"cov{j}_threshold"])) for j in range(3)]
        out[name] = (g, clouds, cov)
    return out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("name", NAMES)
def test_saliency_is_the_references(capi, cases, name):
    g, clouds, _ = cases[name]
    for j in range(2):
        args = (g["bbox_min"], g["bbox_max"], clouds, g["prop_obj"], g["prop_pose"], g["prop_static"], g["pos0"], g["class0"], int(g["wall_idx"]), int(g["floor_idx"]))
        quality, grid = capi.scene_saliency(*args, voxel_size=g[f"sal{j}_voxel"], want_grid=True)
        assert grid.tobytes() == g[f"sal{j}_grid"].tobytes()
        assert quality.tobytes() == g[f"sal{j}_quality"].tobytes()
        again = capi.scene_saliency(*args, voxel_size=g[f"sal{j}_voxel"])
        assert again.tobytes() == quality.tobytes()
    # no proposals: an unlit grid, every quality 0
    q, grid = capi.scene_saliency(g["bbox_min"], g["bbox_max"], [], [], np.zeros((0, 16), F), [], g["pos0"], g["class0"], 1, 2, want_grid=True)
    assert not grid.any() and not q.any()


@pytest.mark.parametrize("name", NAMES)
def test_extensions_are_the_references(capi, cases, name):
    g, clouds, covs = cases[name]
    low = int(g["low_lds_budget"])
    default = capi.coverage_lds_budget(-1)
    try:
        for j, t, pre, base, cand in trials(g):
            cov = covs[j]
            assert cov.scene_grid().tobytes() == g[f"cov{j}_grid"].tobytes() and cov.valid_cells == int(g[f"cov{j}_valid"])
            b = [(clouds[o], p, s) for o, p, s in base]
            c = [(clouds[o], p) for o, p in cand]
            capi.coverage_lds_budget(default)
            capi.coverage_extension_routes(reset=True)
            sc, ag, ba = cov.extensions(b, c)
            assert capi.coverage_extension_routes() == (len(c), 0)             # 5 cm and 15 cm rooms: every sub-box fits the LDS budget
            assert ba == int(g[pre + "base_agree"])
            assert (ag == g[pre + "agree"]).all() and (bits(sc) == bits(g[pre + "score"])).all(), (j, t)
            # the parent's only way to the same numbers: whole arrangements base + [candidate k]
            sc_full, ag_full = cov.scores([b + [(cl, p, 0)] for cl, p in c]) if c else (np.zeros(0, F), np.zeros(0, np.int32))
            assert (ag == ag_full).all() and (bits(sc) == bits(sc_full)).all()
            sc_b, ag_b = cov.scores([b])
            assert ag_b[0] == ba and bits(sc_b)[0] == bits(g[pre + "base_score"])[0]
            # a second call, then the lowered budget (the partition and other large sub-boxes on the slab), then the slab alone
            sc2, ag2, ba2 = cov.extensions(b, c)
            assert (ag2 == ag).all() and (bits(sc2) == bits(sc)).all() and ba2 == ba
            for budget in (low, 0):
                capi.coverage_lds_budget(budget)
                capi.coverage_extension_routes(reset=True)
                sc3, ag3, ba3 = cov.extensions(b, c)
                n_lds, n_slab = capi.coverage_extension_routes()
                assert (ag3 == ag).all() and (bits(sc3) == bits(sc)).all() and ba3 == ba, (j, t, budget)
                assert n_lds + n_slab == len(c)
                if c and cov.valid_cells and budget == low and t == 0 and j == 0:
                    assert n_slab > 0 and n_lds > 0                            # both routes in one call
                if budget == 0:
                    assert n_slab == int((ag > ba).sum())                      # (a candidate without a live cell needs no sub-box at all)
    finally:
        capi.coverage_lds_budget(default)


def test_released_buffers_are_allocated_again(capi, cases):
    """rs_hip_arrange_release hands the thread's buffers back (the slab route's among them); the next calls give the same bits."""
    g, clouds, covs = cases[NAMES[0]]
    j, t, pre, base, cand = next(x for x in trials(g) if x[4] and covs[x[0]].valid_cells)
    b = [(clouds[o], p, s) for o, p, s in base]
    c = [(clouds[o], p) for o, p in cand]
    args = (g["bbox_min"], g["bbox_max"], clouds, g["prop_obj"], g["prop_pose"], g["prop_static"], g["pos0"], g["class0"], int(g["wall_idx"]), int(g["floor_idx"]))
    default = capi.coverage_lds_budget(0)
    try:
        sc, ag, ba = covs[j].extensions(b, c)
        capi.arrange_release()
        capi.arrange_release()                                                 # nothing held: still fine
        sc2, ag2, ba2 = covs[j].extensions(b, c)
        assert (ag2 == g[pre + "agree"]).all() and (ag2 == ag).all() and (bits(sc2) == bits(sc)).all() and ba2 == ba
    finally:
        capi.coverage_lds_budget(default)
    capi.arrange_release()
    assert capi.scene_saliency(*args, voxel_size=g["sal0_voxel"]).tobytes() == g["sal0_quality"].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_the_shim_gives_the_same(capi, cases, name):
    g, _, _ = cases[name]
    lib = C.CDLL(os.path.join(ROOT, "rescan_amd", "librescan_dropin.so"))
    vp, i32, f = C.c_void_p, C.c_int32, C.c_float
    objs = [np.ascontiguousarray(o, F) for o in g["objects"]]
    optr = (vp * len(objs))(*[o.ctypes.data for o in objs]); on = np.array([len(o) for o in objs], np.int32)
    sal = lib.rsd_scene_saliency; sal.restype = C.c_int
    sal.argtypes = [vp, vp, f, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, i32, vp]
    bmin, bmax = np.ascontiguousarray(g["bbox_min"], F), np.ascontiguousarray(g["bbox_max"], F)
    po, pp, ps = (np.ascontiguousarray(g[k]) for k in ("prop_obj", "prop_pose", "prop_static"))
    pos0, class0 = np.ascontiguousarray(g["pos0"], F), np.ascontiguousarray(g["class0"], np.int32)
    for j in range(2):
        q = np.full(len(pos0), 7, F)
        rc = sal(bmin.ctypes.data, bmax.ctypes.data, float(g[f"sal{j}_voxel"]), C.addressof(optr), on.ctypes.data, len(objs), po.ctypes.data, pp.ctypes.data,
                 ps.ctypes.data, len(po), pos0.ctypes.data, class0.ctypes.data, len(pos0), int(g["wall_idx"]), int(g["floor_idx"]), q.ctypes.data)
        assert rc == 0 and q.tobytes() == g[f"sal{j}_quality"].tobytes()
    lib.rsd_coverage_create.restype = vp
    lib.rsd_coverage_create.argtypes = [vp, vp, f, vp, vp, i32, f]
    lib.rsd_coverage_destroy.argtypes = [vp]
    ext = lib.rsd_coverage_extensions; ext.restype = C.c_int
    ext.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp]
    pos2, q2 = np.ascontiguousarray(pos0[g["sub"]]), np.ascontiguousarray(g["sal0_quality"][g["sub"]], F)
    for j in range(3):
        h = lib.rsd_coverage_create(bmin.ctypes.data, bmax.ctypes.data, float(g[f"cov{j}_voxel"]), pos2.ctypes.data, q2.ctypes.data, len(pos2), float(g[f"cov{j}_threshold"]))
        assert h
        for jj, t, pre, base, cand in trials(g):
            if jj != j:
                continue
            bptr = (vp * max(1, len(base)))(*[objs[o].ctypes.data for o, _, _ in base]); bn = np.array([len(objs[o]) for o, _, _ in base] or [0], np.int32)
            bp = np.ascontiguousarray(g[pre + "base_pose"], F).reshape(-1, 16); bs = np.ascontiguousarray(g[pre + "base_static"], np.int32)
            cptr = (vp * max(1, len(cand)))(*[objs[o].ctypes.data for o, _ in cand]); cn = np.array([len(objs[o]) for o, _ in cand] or [0], np.int32)
            cp = np.ascontiguousarray(g[pre + "cand_pose"], F).reshape(-1, 16)
            sc = np.full(max(1, len(cand)), 7, F)
            rc = ext(h, C.addressof(bptr), bn.ctypes.data, bp.ctypes.data if len(base) else None, bs.ctypes.data if len(base) else None, len(base),
                     C.addressof(cptr), cn.ctypes.data, cp.ctypes.data if len(cand) else None, len(cand), sc.ctypes.data)
            assert rc == 0 and (bits(sc[:len(cand)]) == bits(g[pre + "score"])).all(), (j, t)
        lib.rsd_coverage_destroy(h)


HARD = [(0.05, True), (0.05, False), (0.15, True), (0.15, False)]


@pytest.fixture(scope="module")
def hard():
    return hard_fixture()


@pytest.mark.parametrize("voxel,cell0", HARD)
def test_hard_candidates_are_the_references(capi, hard, voxel, cell0):
    """The hostile candidates of tests/hard_shapes.py (thousands of points in three cells, off the grid, inside the base, on inactive
    cells, empty, NaN and infinite coordinates, a diagonal rod whose sub-box fits the LDS budget exactly, points on cell faces and on
    the grid's outer faces) against the reference's own numbers (tests/golden/arrange_hard.npz): the scene grid — whose cloud holds
    NaN and infinite points, with cell 0 active only in the run that has a finite point there —, every count and every score bit.
    The route of every candidate is predicted from its live sub-box (tests/ao_restate.py; the reference has no sub-boxes) and
    checked against the route counters."""
    import hard_shapes as H
    a, _, _, _, _, _, need = H.arrangement_expectations(voxel, cell0)
    pre = H.arr_key("cov", voxel, cell0)
    assert (hard[pre + "crc"] == H.cloud_crcs(a["scene"], a["objects"])).all()
    want_grid = np.unpackbits(hard[pre + "grid"])[:int(a["res"].prod())]
    base_agree, agree, scores = int(hard[pre + "base_agree"]), hard[pre + "agree"], hard[pre + "score"]
    clouds = [capi.Cloud(p, None, 0.0) for p in a["objects"]]
    cov = capi.Coverage(H.ARR_BMIN, H.ARR_BMAX, a["scene"], None, voxel, 0.0)
    grid = cov.scene_grid()
    assert grid[0] == int(cell0) == want_grid[0] and cov.valid_cells == int(hard[pre + "valid"])      # a non-finite scene point lights nothing
    assert grid.tobytes() == want_grid.tobytes()
    b = [(clouds[o], p, s) for o, p, s in a["base"]]
    c = [(clouds[o], p) for o, p in a["cands"]]
    rod = need[a["names"].index("rod")]
    default = capi.coverage_lds_budget(-1)
    try:
        for budget in (default, rod, rod - 4, 0) if cell0 else (default, 0):
            capi.coverage_lds_budget(budget)
            capi.coverage_extension_routes(reset=True)
            sc, ag, ba = cov.extensions(b, c)
            assert ba == base_agree and (ag == agree).all(), (budget, [(n, int(x), int(y)) for n, x, y in zip(a["names"], ag, agree) if x != y])
            assert (bits(sc) == bits(scores)).all()
            assert capi.coverage_extension_routes() == (sum(v <= budget for v in need), sum(v > budget for v in need)), budget
            sc2, ag2, ba2 = cov.extensions(b, c)
            assert (ag2 == ag).all() and (bits(sc2) == bits(sc)).all() and ba2 == ba
        assert rod <= default and sum(v > rod for v in need) < sum(v > rod - 4 for v in need)             # exactly the budget: LDS; 4 bytes less: the slab
        # the same numbers from whole arrangements
        capi.coverage_lds_budget(default)
        sc_full, ag_full = cov.scores([b + [(cl, p, 0)] for cl, p in c])
        assert (ag_full == agree).all() and (bits(sc_full) == bits(scores)).all()
        sc_b, ag_b = cov.scores([b])
        assert ag_b[0] == base_agree and bits(sc_b)[0] == bits(hard[pre + "base_score"])[0]
    finally:
        capi.coverage_lds_budget(default)


@pytest.mark.parametrize("voxel,cell0", HARD)
def test_hard_saliency_is_the_references(capi, hard, voxel, cell0):
    """Phase order against list order, wall and floor points in lit cells, class -1 with wall_idx -1, and non-finite coordinates: a
    NaN, +inf or -inf coordinate lights, clears and reads no cell — cell 0 least of all (a device float-to-int conversion of NaN is
    0) — as the reference recorded it in tests/golden/arrange_hard.npz."""
    import hard_shapes as H
    s = H.saliency_case(voxel, cell0)
    pre = H.arr_key("sal", voxel, cell0)
    assert (hard[pre + "crc"] == H.cloud_crcs(s["scene"], s["objects"])).all()
    clouds = [capi.Cloud(p, None, 0.0) for p in s["objects"]]
    q, grid = capi.scene_saliency(H.ARR_BMIN, H.ARR_BMAX, clouds, s["prop_obj"], s["prop_pose"], s["prop_static"], s["scene"], s["cls"], -1, 2,
                                  voxel_size=voxel, want_grid=True)
    want_grid = np.unpackbits(hard[pre + "grid"])[:len(grid)]
    assert grid[0] == int(cell0) == want_grid[0], (cell0, grid[0])
    assert grid.tobytes() == want_grid.tobytes() and q.tobytes() == hard[pre + "quality"].tobytes()
    assert q[-1] == F(cell0) and (q[-4:-1] == 0).all()
