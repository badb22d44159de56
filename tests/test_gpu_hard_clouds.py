"""Every search entry point on the hostile geometry of tests/hard_clouds.py: coordinates 1e3 and 1e4 m from the origin with mixed
signs, an all-negative room, planar and collinear clouds (grids one bin thick), 50 k points in a 2 cm cube inside a sparse 4 m
one, an exact lattice with d² == r² pairs, queries outside the box on every side (and one NaN), and two points tens of metres
apart.  Test ids name the family and the entry point.

- radius rows (rs_hip_radius_search): against the numpy brute force, which tests/test_hard_clouds_cpu.py holds to the oracle;
  4095 and 4096 queries take k_rows_wave and the tiled k_rows for k < 16 under the default switch, and the contrast family's
  rows of more than 1024 points send whole calls to the storage-free k_rows;
- k-NN (rs_hip_knn_search): bit for bit against the shim's host restatement, against brute force, and against the reference's
  own msh_hash_grid_knn_search where it is defined;
- alignment scores: both routes against the oracle and against each other;
- ICP correspondences: bit for bit against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import hard_clouds as hc

pytestmark = pytest.mark.gpu

SCORE_TOL = 2e-6                                           # as tests/test_gpu_parity.py
ROWS_K = (1, 2, 3, 15, 16, 17, 63, 64, 1024)
KNN_K = (1, 2, 7, 8, 9, 17, 63, 64)                        # around RS_KNN_INSERT_BELOW (8) and not powers of two
# (family, k) where the reference's msh_hash_grid_knn_search is not defined on the cloud's own points: its walk would pass
# MAX_BIN_COUNT (256) bins and assert (msh_hash_grid.h:870, 1412) -- the dense cube leaves most shell bins empty, and two
# points with k = n leave the walk to cross the whole grid
REF_KNN_UNDEFINED = {("contrast", k) for k in KNN_K if k >= 7} | {("two_far", k) for k in KNN_K if k >= 2}


@pytest.fixture(scope="module")
def capi():
    from rescan_amd import capi
    capi.init(0)
    return capi


_FAMILY = {}


def family(name):
    """The family and its brute-force rows at k = 1024 (shorter k are prefixes), built once per module."""
    if name not in _FAMILY:
        f = hc.make(name)
        _FAMILY[name] = f, hc.brute_rows(f["points"], f["queries"], f["radius"], 1024)
    return _FAMILY[name]


def layouts(r):
    return {"cell2r": 2 * r, "fine": 0.4 * r, "auto": -1.0, "brute": 0.0}


# ---- radius rows ---------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["cell2r", "fine", "auto", "brute"])
@pytest.mark.parametrize("name", hc.FAMILIES)
def test_radius_rows(capi, name, layout):
    """rs_hip_radius_search == brute force: counts, totals and distances bit for bit, indices up to exact ties (k-th slot
    included), for every k of ROWS_K and for 4095 and 4096 queries."""
    f, full = family(name)
    r = f["radius"]
    cloud = capi.Cloud(f["points"], None, cell_size=layouts(r)[layout])
    try:
        for k in ROWS_K:
            if layout == "brute" and k > 16:
                continue
            want = hc.truncate(full, k)
            for nq in (4095, 4096):
                q = f["queries"][:nq]
                got = capi.radius_search(cloud, q, r, k)
                w = (want[0][:nq], want[1][:nq], want[2][:nq], int(want[2][:nq].sum()))
                try:
                    hc.assert_rows(w, got, f["points"], q)
                except AssertionError as e:
                    raise AssertionError(f"{name}/{layout}: k = {k}, {nq} queries: {e}") from None
    finally:
        cloud.close()


@pytest.mark.parametrize("layout", ["cell2r", "auto"])
def test_rows_with_a_full_wave_list(capi, layout):
    """k_rows_wave keeps up to 1024 hits per query in LDS (ROWS_CAP); a query with more hands the whole call to the storage-free
    k_rows.  Queries on rays out of the contrast family's dense cube with exactly 901 ... 1024 points within the radius fill the
    list without a hand-off; adding queries with exactly 1025 (and then 1026) forces one.  Every call against the brute force."""
    f, _ = family("contrast")
    r = f["radius"]
    q_in, c_in = hc.queries_with_counts(f["points"], r, np.array([1.31, 0.71, 2.11]), (901, 960, 1000, 1023, 1024), 6, seed=1)
    q_out, c_out = hc.queries_with_counts(f["points"], r, np.array([1.31, 0.71, 2.11]), (1025, 1026), 6, seed=2)
    assert len(q_in) >= 25 and (c_in == 1024).sum() >= 4 and len(q_out) >= 8 and (c_out == 1025).sum() >= 4
    cloud = capi.Cloud(f["points"], None, cell_size=layouts(r)[layout])
    try:
        for q in (q_in, np.concatenate([q_in, q_out[c_out == 1025]]), np.concatenate([q_in, q_out])):
            full = hc.brute_rows(f["points"], q, r, 1024)
            assert full[4].min() > 900 and ((full[4] > 1024).any() == (len(q) > len(q_in)))
            for k in (16, 63, 1024):
                try:
                    hc.assert_rows(hc.truncate(full, k), capi.radius_search(cloud, q, r, k), f["points"], q)
                except AssertionError as e:
                    raise AssertionError(f"{layout}: k = {k}, {len(q)} queries: {e}") from None
    finally:
        cloud.close()


# ---- k-NN ----------------------------------------------------------------------------------

def knn_queries(f, n=1024):
    q = f["queries"]
    return np.ascontiguousarray(q[np.isfinite(q).all(axis=1)][:n])


@pytest.mark.parametrize("name", hc.FAMILIES)
def test_knn(capi, name, monkeypatch):
    """rs_hip_knn_search on 1024 queries of the family (inside and outside the box), k around the insertion/bitonic switch:
    (a) identical to the shim's host restatement, rows past the counts untouched; (b) every (d², index) is that point's own
    float d², rows ascend strictly in (d², index), and no slot is nearer than the cloud's true j-th nearest.  (Rows need not be
    the exact k nearest: the reference stops one shell after it first holds k points, msh_hash_grid.h:1428-1430.)
    two_far: k <= n and 32 queries, since every such query walks most of a 13 M-bin grid."""
    import test_gpu_knn as tk
    f, _ = family(name)
    P, r = f["points"], f["radius"]
    q, ks = knn_queries(f), KNN_K
    if name == "two_far":
        q, ks = q[:32], (1, 2)
    d2_all = hc.d2_rows(P, q)
    best = np.sort(d2_all, axis=1)
    for k in ks:
        got = tk.native(P, 3, r, q, k)
        want = tk.shim_host(P, 3, r, q, k, monkeypatch)
        tk.assert_identical(got, want)
        d, i, nn, tot = got
        kk = min(k, len(P))
        assert (nn == kk).all() and tot == kk * len(q)
        i = i[:, :kk]; d = d[:, :kk]
        own = np.take_along_axis(d2_all, i.astype(np.int64), axis=1)
        assert (own.view(np.uint32) == d.view(np.uint32)).all(), f"{name}: k = {k}: a returned d² is not its point's"
        if kk > 1:
            asc = (d[:, 1:] > d[:, :-1]) | ((d[:, 1:] == d[:, :-1]) & (i[:, 1:] > i[:, :-1]))
            assert asc.all(), f"{name}: k = {k}: a row does not ascend in (d², index)"
        assert (d >= best[:, :kk]).all(), f"{name}: k = {k}: a slot is nearer than the cloud's true j-th nearest"


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                                                    "libref.so")),
                    reason="oracle/_ref/libref.so (the reference compiled in place) not built")
@pytest.mark.parametrize("name", hc.FAMILIES)
def test_knn_vs_reference(capi, name):
    """rs_hip_knn_search against the reference's own msh_hash_grid_knn_search (oracle/_ref/libref.so) on 256 of the cloud's own
    points, for every k where the reference is defined: counts, totals and distances equal, indices up to exact ties."""
    import test_gpu_knn as tk
    f, _ = family(name)
    P, r = f["points"], f["radius"]
    ref = tk._bind(C.CDLL(tk.REF_LIB))
    q = np.ascontiguousarray(P[np.random.default_rng(1).permutation(len(P))[:256]])
    checked = 0
    for k in KNN_K:
        if (name, k) in REF_KNN_UNDEFINED or k > len(P):
            continue
        want = tk.by_name(ref, P, 3, r, q, k)
        got = tk.native(P, 3, r, q, k)
        hc.assert_rows(want, got, P, q)
        checked += 1
    assert checked >= 1


# ---- alignment scores ----------------------------------------------------------------------

@pytest.mark.parametrize("name", hc.FAMILIES)
def test_scores(capi, oracle, name):
    """Both score routes (object space, scene space) against the oracle within SCORE_TOL and against each other bit for bit, the
    object posed over the whole box (corners, random, where it was cut), scene cells 0.1 and auto."""
    f, _ = family(name)
    o = f["obj"]
    want = oracle.alignment_scores(f["points"], f["normals"], o["pos"], o["nor"], f["poses"], 64)
    oc = capi.Cloud(o["pos"], o["nor"], cell_size=0.1)
    for cell in (0.1, -1.0):
        scn = capi.Cloud(f["points"], f["normals"], cell_size=cell)
        prev = capi.score_scene_space_from(1 << 60)
        try:
            a = capi.alignment_scores(oc, scn, f["poses"], 0.1, 64)
            capi.score_scene_space_from(0)
            b = capi.alignment_scores(oc, scn, f["poses"], 0.1, 64)
        finally:
            capi.score_scene_space_from(prev)
        scn.close()
        assert np.abs(a.astype(np.float64) - want).max() < SCORE_TOL, (name, cell, a, want)
        assert (a.view(np.uint32) == b.view(np.uint32)).all(), (name, cell, a, b)
    assert want.max() > 0.5                                   # the pose where the object was cut scores


@pytest.mark.parametrize("name", ["offset_1e4", "offset_1e3"])
def test_scene_space_scores_far_from_the_origin(capi, oracle, name):
    """The scene-space route (k_score_scene, the default for large batches) culls each cell row by a reach re-derived from cell
    faces (sweep_shell: sqrtf(rem)); 1e4 m out a face coordinate rounds by up to half an ulp, 2^-11 m.  A piece of
    the room scored at 96 poses that keep it on its own surface, scene cells from 0.1 down to 0.025 (the x-range slack of
    axis_range, 0.01 cell, is then below that rounding): both routes bit for bit, and the oracle within SCORE_TOL."""
    f, _ = family(name)
    obj, poses = hc.surface_poses(f, 96)
    assert len(obj["pos"]) >= 2500
    want = oracle.alignment_scores(f["points"], f["normals"], obj["pos"], obj["nor"], poses, 64)
    assert want.min() > 0.3
    oc = capi.Cloud(obj["pos"], obj["nor"], cell_size=0.1)
    for cell in (0.1, -1.0, 0.05, 0.04, 0.025):
        scn = capi.Cloud(f["points"], f["normals"], cell_size=cell)
        prev = capi.score_scene_space_from(1 << 60)
        try:
            a = capi.alignment_scores(oc, scn, poses, 0.1, 64)
            capi.score_scene_space_from(0)
            b = capi.alignment_scores(oc, scn, poses, 0.1, 64)
        finally:
            capi.score_scene_space_from(prev)
        scn.close()
        assert np.abs(a.astype(np.float64) - want).max() < SCORE_TOL, (name, cell)
        bad = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]
        assert not len(bad), (name, cell, bad, a[bad], b[bad], want[bad])


# ---- ICP correspondences -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["offset_1e3", "offset_1e4", "negative", "planar", "collinear", "contrast"])
def test_icp_find_corrs(capi, oracle, name):
    """rs_hip_icp_find_corrs against the oracle bit for bit, the object started near where it was cut, scene cells auto and 0.2."""
    f, _ = family(name)
    o = f["obj"]
    I4 = np.eye(4, dtype=np.float32).ravel()
    want = oracle.icp_find_corrs(o["pos"], o["nor"], f["points"], f["normals"], f["T0"], I4, 0.1, np.float32(np.deg2rad(60.0)))
    assert len(want[0]) > 0
    oc = capi.Cloud(o["pos"], o["nor"])
    for cell in (-1.0, 0.2):
        scn = capi.Cloud(f["points"], f["normals"], cell_size=cell)
        got = capi.icp_find_corrs(oc, scn, f["T0"], I4, 0.1, np.deg2rad(60.0))
        scn.close()
        for a, b, what in zip(want, got, ("c_pts1", "c_nor1", "c_pts2", "c_nor2", "weights")):
            assert a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all(), (name, cell, what)
