"""The device k-NN search's C ABI without a GPU: its exports, the no-device answer, and the host-side grid geometry, which must be
msh_hash_grid_knn_search's own (KnnGrid::build in rescan_amd/csrc/rs_dropin.cpp, lib/msh/msh_hash_grid.h:413-449)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "rescan_amd", "librescan_hip.so")


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def knn_grid_geometry(pts, radius):
    """KnnGrid::build's geometry restated in numpy, float32 where the reference computes in float and float64 where in double."""
    p = np.asarray(pts, np.float32)
    f32 = np.float32
    mn = np.minimum(f32(1e9), p.min(axis=0)).astype(f32) - f32(0.0001)
    mx = np.maximum(f32(-1e9), p.max(axis=0)).astype(f32) + f32(0.0001)
    ext = (mx - mn).astype(f32)
    max_dim = ext.max()
    if radius > 0.0:
        cell = 2.0 * float(f32(radius))
    else:
        cell = float(f32(max_dim / (f32(32) * np.sqrt(f32(3.0)))))
    dims = tuple(max(int(float(e) / cell + 1.0), 1) for e in ext)
    return dims, cell, mn


def test_knn_entry_points_are_exported():
    from rescan_amd import build
    build.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = set(re.findall(r" T ([a-z0-9_]+)", out))
    assert {"rs_hip_knn_grid_create", "rs_hip_knn_grid_destroy", "rs_hip_knn_grid_geometry", "rs_hip_knn_geometry",
            "rs_hip_knn_search"} <= exported
    hdr = open(os.path.join(ROOT, "include", "rescan_hip.h")).read()
    assert re.search(r"#define\s+RS_HIP_KNN_MAX_K\s+64\b", hdr)


@pytest.mark.skipif(not _no_gpu(), reason="checks the answer of a machine without a HIP device")
def test_knn_search_without_a_device():
    from rescan_amd import capi
    lib = capi.load()
    q = np.zeros((4, 3), np.float32)
    d = np.zeros((4, 8), np.float32); i = np.zeros((4, 8), np.int32); nn = np.zeros(4, np.uint64)
    tot = C.c_uint64()
    assert lib.rs_hip_knn_search(None, q, 4, 8, d, i, nn, C.byref(tot)) == -1          # RS_HIP_E_NODEVICE
    assert lib.rs_hip_knn_grid_create(None, C.c_float(0.1), 3) is None
    with pytest.raises(capi.RescanHipError):
        capi.KnnGrid(type("NoCloud", (), {"handle": None})(), 0.1)


@pytest.mark.parametrize("dim", [3, 2])
def test_knn_geometry_is_the_references(dim):
    """w, h, d, cell and the grid's origin, computed by the library on the host, equal KnnGrid's on a few boxes (2-D: points (x, y, 0))."""
    from rescan_amd import capi
    rng = np.random.default_rng(11 + dim)
    boxes = [((0.0, 0.0, 0.0), (1.0, 1.0, 0.5)), ((-3.2, 0.1, -1.0), (0.4, 2.9, 0.2)), ((10.0, 10.0, 10.0), (10.3, 17.0, 10.01)),
             ((-0.05, -0.05, -0.05), (0.05, 0.05, 0.05))]
    for lo, hi in boxes:
        pts = rng.uniform(lo, hi, (2000, 3)).astype(np.float32)
        if dim == 2:
            pts[:, 2] = 0.0
        for radius in (0.05, 0.013, 0.5, 0.0, -1.0):
            want_dims, want_cell, want_mn = knn_grid_geometry(pts, radius)
            dims, cell, mn = capi.knn_geometry(pts, radius, dim)
            assert dims == want_dims, (lo, hi, radius)
            assert cell == want_cell and (mn == want_mn).all()
            if dim == 2:
                assert dims[2] == 1


def test_knn_geometry_refuses_an_absurd_table():
    from rescan_amd import capi
    pts = np.array([[0, 0, 0], [100, 100, 100]], np.float32)
    with pytest.raises(capi.RescanHipError, match="error -4"):          # RS_HIP_E_CAPACITY: 10^12 bins
        capi.knn_geometry(pts, 0.05)
    assert capi.knn_geometry(pts, 5.0)[0] == (11, 11, 11)
