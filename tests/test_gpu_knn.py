"""msh_hash_grid_knn_search on the device: rs_hip_knn_search (rs_knn.hip) against the shim's host restatement of the reference's
traversal (KnnGrid) and against the reference's own compiled function (oracle/_ref/libref.so)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

DROPIN = os.path.join(ROOT, "rescan_amd", "librescan_dropin.so")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libref.so")
FILL = -7                                              # what a row holds past its count, before and after


class HashGrid(C.Structure):                       # msh_hash_grid_t, lib/msh/msh_hash_grid.h:248-269
    _fields_ = [("width", C.c_size_t), ("height", C.c_size_t), ("depth", C.c_size_t), ("cell_size", C.c_double),
                ("min_pt", C.c_float * 3), ("max_pt", C.c_float * 3), ("bin_table", C.c_void_p),
                ("data_buffer", C.c_void_p), ("offsets", C.c_void_p), ("_slab_size", C.c_int32),
                ("_inv_cell_size", C.c_double), ("_pts_dim", C.c_uint8), ("_num_threads", C.c_uint16),
                ("_dont_use_omp", C.c_int32), ("max_n_pts_in_bin", C.c_uint32), ("_n_pts", C.c_size_t)]


class SearchDesc(C.Structure):                     # msh_hash_grid_search_desc_t, :196-216
    _fields_ = [("query_pts", C.c_void_p), ("n_query_pts", C.c_size_t), ("distances_sq", C.c_void_p),
                ("indices", C.c_void_p), ("n_neighbors", C.c_void_p), ("radius", C.c_float),
                ("max_n_neigh", C.c_size_t), ("sort", C.c_int)]


def _bind(lib):
    for name in ("msh_hash_grid_init_3d", "msh_hash_grid_init_2d"):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = [C.POINTER(HashGrid), C.c_void_p, C.c_int32, C.c_float]
    lib.msh_hash_grid_term.restype = None
    lib.msh_hash_grid_term.argtypes = [C.POINTER(HashGrid)]
    lib.msh_hash_grid_knn_search.restype = C.c_size_t
    lib.msh_hash_grid_knn_search.argtypes = [C.POINTER(HashGrid), C.POINTER(SearchDesc)]
    return lib


def _lib(path):
    from rescan_amd import build
    build.build()
    return _bind(C.CDLL(path))


def by_name(lib, pts, dim, radius, q, k, sort=1):
    """msh_hash_grid_init_{dim}d + msh_hash_grid_knn_search + term through `lib` (the shim or the reference); rows past a count keep FILL."""
    pts = np.ascontiguousarray(pts, np.float32); q = np.ascontiguousarray(q, np.float32)
    hg = HashGrid()
    getattr(lib, "msh_hash_grid_init_%dd" % dim)(C.byref(hg), pts.ctypes.data, len(pts), float(radius))
    d = np.full((len(q), k), FILL, np.float32); i = np.full((len(q), k), FILL, np.int32); nn = np.zeros(len(q), np.uint64)
    sd = SearchDesc(q.ctypes.data, len(q), d.ctypes.data, i.ctypes.data, nn.ctypes.data, float(radius), k, sort)
    tot = lib.msh_hash_grid_knn_search(C.byref(hg), C.byref(sd))
    lib.msh_hash_grid_term(C.byref(hg))
    return d, i, nn.astype(np.int64), int(tot)


def shim_host(pts, dim, radius, q, k, monkeypatch):
    monkeypatch.setenv("RS_DROPIN_HOST_QUERIES", str(len(q) + 1))
    try:
        return by_name(_lib(DROPIN), pts, dim, radius, q, k)
    finally:
        monkeypatch.delenv("RS_DROPIN_HOST_QUERIES")


def native(pts, dim, radius, q, k):
    """rs_hip_knn_search through the C ABI (cloud -> knn grid), rows pre-filled with FILL."""
    from rescan_amd import capi
    capi.init(0)
    p3 = np.zeros((len(pts), 3), np.float32); p3[:, :dim] = pts
    q3 = np.zeros((len(q), 3), np.float32); q3[:, :dim] = q
    cloud = capi.Cloud(p3)
    grid = capi.KnnGrid(cloud, radius, dim)
    assert grid.geometry()[0] == capi.knn_geometry(p3, radius, dim)[0]
    d = np.full((len(q), k), FILL, np.float32); i = np.full((len(q), k), FILL, np.int32); nn = np.zeros(len(q), np.uint64)
    tot = C.c_uint64()
    rc = capi.load().rs_hip_knn_search(grid.handle, q3, len(q3), k, d, i, nn, C.byref(tot))
    assert rc == 0, capi.load().rs_hip_last_error()
    grid.close(); cloud.close()
    return d, i, nn.astype(np.int64), int(tot.value)


def assert_identical(a, b):
    (da, ia, na, ta), (db, ib, nb, tb) = a, b
    assert ta == tb and (na == nb).all()
    assert (da.view(np.uint32) == db.view(np.uint32)).all()             # every entry, the untouched FILL past the counts included
    assert (ia == ib).all()


def cloud_with_ties(rng, n, dim):
    pts = rng.uniform(0.0, 1.0, (n, dim)).astype(np.float32)
    if dim == 3:
        pts[:, 2] *= 0.5
    dup = rng.choice(n, n // 10, replace=False)
    pts[dup[: len(dup) // 2]] = pts[dup[len(dup) // 2:]]                # exact duplicates: equal distances, ties broken by index
    return pts


def queries(rng, pts, n_in=300, n_out=60):
    dim = pts.shape[1]
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    inside = pts[rng.integers(0, len(pts), n_in)] + rng.normal(0, 0.01, (n_in, dim)).astype(np.float32)
    outside = rng.uniform(lo - 0.6, hi + 0.6, (n_out, dim)).astype(np.float32)
    outside[:, 0] = np.where(rng.random(n_out) < 0.5, lo[0] - rng.uniform(0.01, 0.6, n_out), hi[0] + rng.uniform(0.01, 0.6, n_out))
    return np.concatenate([inside, outside]).astype(np.float32)


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("radius", [0.04, 0.0, -1.0])
def test_native_knn_equals_the_host_restatement(dim, radius, monkeypatch):
    """(a) k in {1, 8, 16, 32, 64}, radius > 0 and <= 0 (extent-derived cell), queries inside and outside the box, duplicated points:
    distances, indices, counts and totals identical to the shim's host route, rows past the counts untouched."""
    rng = np.random.default_rng(7 + dim)
    pts = cloud_with_ties(rng, 6000, dim)
    q = queries(rng, pts)
    for k in (1, 8, 16, 32, 64):
        want = shim_host(pts, dim, radius, q, k, monkeypatch)
        got = native(pts, dim, radius, q, k)
        assert_identical(got, want)
        assert (want[2] == k).all()


@pytest.mark.parametrize("dim", [3, 2])
def test_native_knn_on_clouds_smaller_than_k(dim, monkeypatch):
    """(a) fewer points than k: the walk visits every bin and returns every point (the reference would spin)."""
    rng = np.random.default_rng(3 + dim)
    for n, radius in ((5, 0.1), (40, 0.02), (40, 0.0), (1, 0.1)):
        pts = cloud_with_ties(rng, n, dim)
        q = queries(rng, pts, 50, 20)
        for k in (8, 64):
            want = shim_host(pts, dim, radius, q, k, monkeypatch)
            got = native(pts, dim, radius, q, k)
            assert_identical(got, want)
            assert (want[2] == min(n, k)).all()


def test_knn_k_cap_and_absurd_grid():
    """k above the cap and a grid of more than 2^26 bins are refused with their codes, not attempted."""
    from rescan_amd import capi
    capi.init(0)
    rng = np.random.default_rng(1)
    pts = rng.uniform(0, 1, (1000, 3)).astype(np.float32)
    cloud = capi.Cloud(pts)
    grid = capi.KnnGrid(cloud, 0.05)
    with pytest.raises(capi.RescanHipError, match="error -4"):
        capi.knn_search(grid, pts[:10], capi.KNN_MAX_K + 1)
    with pytest.raises(capi.RescanHipError):
        capi.KnnGrid(cloud, 1e-4)
    with pytest.raises(capi.RescanHipError, match="error -4"):
        capi.knn_geometry(pts, 1e-4)


@pytest.mark.skipif(not os.path.exists(REF_LIB), reason="oracle/_ref/libref.so (the reference compiled in place) not built")
@pytest.mark.parametrize("dim", [3, 2])
def test_device_route_matches_the_reference(dim, monkeypatch):
    """(b) the shim's device route (400 queries > RS_DROPIN_HOST_QUERIES) against the reference's own msh_hash_grid_knn_search, on
    inputs where the reference is defined (those of tests/test_dropin.py, plus k = 64): distances bit for bit, indices up to exact
    ties, counts and totals equal; sorted and unsorted calls."""
    from conftest import rows_equal_up_to_ties
    shim, ref = _lib(DROPIN), _bind(C.CDLL(REF_LIB))
    monkeypatch.delenv("RS_DROPIN_HOST_QUERIES", raising=False)
    rng = np.random.default_rng(41 + dim)
    for n, radius, k in ((20000, 0.05, 8), (20000, 0.1, 16), (3000, 0.04, 1), (50000, 0.08, 32), (50000, 0.08, 64)):
        pts = rng.uniform(0.0, 1.0, (n, dim)).astype(np.float32)
        if dim == 3:
            pts[:, 2] *= 0.5
        q = np.ascontiguousarray(pts[rng.permutation(n)[:400]] + rng.normal(0, 0.01, (400, dim)).astype(np.float32))
        q = np.clip(q, pts.min(axis=0), pts.max(axis=0)).astype(np.float32)      # inside the grid's box
        for sort in (1, 0):
            got = by_name(shim, pts, dim, radius, q, k, sort)
            want = by_name(ref, pts, dim, radius, q, k, sort)
            if not sort:                                                          # the reference leaves heap order: compare as sets
                rows = []
                for d, i, nn, t in (got, want):
                    o = np.argsort(d, axis=1, kind="stable")
                    rows.append((np.take_along_axis(d, o, axis=1), np.take_along_axis(i, o, axis=1), nn, t))
                got, want = rows
            assert got[3] == want[3]
            rows_equal_up_to_ties(want[0], want[1], want[2], got[0], got[1], got[2])
            assert (want[2] == k).all()


ROUTES = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_knn as t
lib = t._lib(t.DROPIN)
rng = np.random.default_rng(5)
for dim in (3, 2):
    pts = t.cloud_with_ties(rng, 30000, dim)
    q = t.queries(rng, pts, 2000, 100)
    for k in (4, 32):
        os.environ["RS_DROPIN_HOST_QUERIES"] = str(len(q) + 1)
        host = t.by_name(lib, pts, dim, 0.03, q, k)
        os.environ["RS_DROPIN_HOST_QUERIES"] = "4"
        dev = t.by_name(lib, pts, dim, 0.03, q, k)
        t.assert_identical(dev, host)
print("routes agree")
"""


def test_shim_device_route_equals_host_route():
    """(c) the shim's two routes give the same rows, and RS_DROPIN_STATS shows that the device route served the batched calls."""
    env = dict(os.environ, RS_DROPIN_STATS="1")
    r = subprocess.run([sys.executable, "-c", ROUTES, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "routes agree" in r.stdout
    dev = [ln for ln in r.stderr.splitlines() if "knn_search, device path" in ln]
    assert dev and int(dev[0].split("path")[1].split()[0]) == 4, r.stderr
    assert "failed" not in r.stderr, r.stderr


def test_scan_sized_knn(monkeypatch):
    """(d) ~1 M queries against a 1 M-point synthetic room, k = 8, through the shim's device route; a random 20 000-query sample
    against the host route."""
    import time
    from rescan_amd import synth
    shim = _lib(DROPIN)
    monkeypatch.delenv("RS_DROPIN_HOST_QUERIES", raising=False)
    s = synth.scene_for_point_count(1_000_000, seed=11)
    pts = np.ascontiguousarray(s["points"], np.float32)
    rng = np.random.default_rng(0)
    q = (pts + rng.normal(0, 0.005, pts.shape)).astype(np.float32)
    k, radius = 8, 0.02
    hg = HashGrid()
    shim.msh_hash_grid_init_3d(C.byref(hg), pts.ctypes.data, len(pts), radius)
    d = np.full((len(q), k), FILL, np.float32); i = np.full((len(q), k), FILL, np.int32); nn = np.zeros(len(q), np.uint64)
    sd = SearchDesc(q.ctypes.data, len(q), d.ctypes.data, i.ctypes.data, nn.ctypes.data, radius, k, 1)
    shim.msh_hash_grid_knn_search(C.byref(hg), C.byref(sd))        # (builds the device grid)
    t0 = time.perf_counter()
    tot = shim.msh_hash_grid_knn_search(C.byref(hg), C.byref(sd))
    dt = time.perf_counter() - t0
    print(f"scan-sized k-NN: {len(q)} queries x {len(pts)} points, k = {k}: {dt * 1e3:.1f} ms per call")
    assert tot == int(nn.sum())
    shim.msh_hash_grid_term(C.byref(hg))
    sample = np.sort(rng.choice(len(q), 20000, replace=False))
    want = shim_host(pts, 3, radius, q[sample], k, monkeypatch)
    got = (d[sample], i[sample], nn[sample].astype(np.int64), int(want[3]))
    assert int(nn[sample].sum()) == want[3]
    assert_identical(got, want)
