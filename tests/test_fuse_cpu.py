"""CPU: the model fusion's fixtures (tests/golden/fuse_*.npz, written by the reference's own rs_pointcloud_copy_by_ids, icp_align,
rs_pointcloud_transform and rs_pointcloud_merge: tools/fuse_fixture) are reproduced bit for bit by the NumPy restatement
(tests/fuse_restate.py); the host planner behind rs_hip_shuffle_plan gives the reference's permutation without a device; every
refusal is decided before a device is touched; the new entry points exist and fail loudly without a GPU."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
import fuse_restate as R

LIB = os.path.join(ROOT, "rescan_amd", "librescan_hip.so")
DROPIN = os.path.join(ROOT, "rescan_amd", "librescan_dropin.so")
KEYS = ("pos", "nor", "col", "radii", "qual", "cls", "inst")
E_NODEVICE, E_ARG, E_CAPACITY = -1, -2, -4
SEEDS = (12346, 1, 64321, 0xFFFFFFFF)
SYMBOLS = ("rs_hip_shuffle_plan", "rs_hip_shuffle_permutation", "rs_hip_select_by_ids", "rs_hip_merge_shuffled", "rs_hip_cloud_create_fused")


@pytest.fixture(scope="module")
def built():
    from rescan_amd import build
    build.build()


@pytest.fixture(scope="module")
def lib(built):
    lib = C.CDLL(LIB)
    lib.rs_hip_shuffle_plan.restype = C.c_int
    lib.rs_hip_shuffle_plan.argtypes = [C.c_int64, C.c_uint32, C.c_void_p]
    lib.rs_hip_shuffle_permutation.restype = C.c_int
    lib.rs_hip_shuffle_permutation.argtypes = [C.c_int64, C.c_uint32, C.c_void_p]
    lib.rs_hip_select_by_ids.restype = C.c_int
    lib.rs_hip_select_by_ids.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.rs_hip_merge_shuffled.restype = C.c_int
    lib.rs_hip_merge_shuffled.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32] + [C.c_void_p] * 3
    lib.rs_hip_last_error.restype = C.c_char_p
    return lib


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def plan(lib, n, seed=12346):
    perm = np.full(max(n, 1), -7, np.int32)
    rc = lib.rs_hip_shuffle_plan(n, seed, perm.ctypes.data)
    assert rc == 0, lib.rs_hip_last_error()
    return perm[:n]


def check_against_fixture(perm, g, n):
    assert len(perm) == n
    if f"perm_{n}" in g:
        assert (perm == g[f"perm_{n}"]).all(), n
    else:
        assert (sha(perm) == g[f"sha256_{n}"]).all(), n
        assert (perm[:256] == g[f"head_{n}"]).all() and (perm[n - 256:] == g[f"tail_{n}"]).all(), n


def test_fixtures_are_small_and_hold_the_cases():
    for name in ("perm", "chair", "wall"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"fuse_{name}.npz")) < 757075
    g = load_golden("fuse_perm.npz")
    assert g["sizes"].tolist() == [2, 3, 64, 65, 4097, 65537, 200001]
    g = load_golden("fuse_chair.npz")
    n_ext = len(g["extracted_pos"])
    assert len(np.unique(g["scan_inst"])) == 4 and 2000 <= len(g["scan_pos"]) <= 9000 and int(g["is_static"]) == 0
    assert 0 < n_ext == int((g["scan_inst"] == g["uidx"]).sum()) <= 16384 and len(g["merged_pos"]) == n_ext + len(g["model_pos"])
    # the ICP moved the pose it started from
    start = np.linalg.inv(g["pose"].astype(np.float64).reshape(4, 4).T).T.ravel()
    assert np.linalg.norm(g["xform"].astype(np.float64) - start) > 1e-3 and float(g["icp_err"]) > 0
    g = load_golden("fuse_wall.npz")
    assert int(g["is_static"]) == 1 and not (g["scan_inst"] == g["absent_uidx"]).any() and int(g["absent_n_extracted"]) == 0


def test_restatement_reproduces_the_permutations():
    g = load_golden("fuse_perm.npz")
    for n in g["sizes"].tolist():
        check_against_fixture(R.plan(n), g, n)


@pytest.mark.parametrize("name", ("chair", "wall"))
def test_restatement_reproduces_every_array(name):
    g = load_golden(f"fuse_{name}.npz")
    idx = R.select(g["scan_inst"], [int(g["uidx"])])
    for k in KEYS:
        assert R.same_bits(g["scan_" + k][idx], g["extracted_" + k]), k
    pos, nor, source = R.merge(g["extracted_pos"], g["extracted_nor"], g["xform"], g["model_pos"], g["model_nor"])
    assert R.same_bits(pos, g["merged_pos"]) and R.same_bits(nor, g["merged_nor"])
    for k in ("col", "radii", "qual", "cls"):
        assert R.same_bits(np.concatenate([g["extracted_" + k], g["model_" + k]])[source], g["merged_" + k]), k
    assert (g["merged_inst"] == g["uidx"]).all()                 # database_update.cpp:79-85
    if name == "wall":                                           # static: the pose is the inverse alone
        from rescan_amd import capi
        assert R.same_bits(capi.mat4_inverse(g["pose"]), g["xform"])
        assert len(R.select(g["scan_inst"], [int(g["absent_uidx"])])) == 0


def test_plan_gives_the_reference_permutations(lib):
    """Fails on a library without rs_hip_shuffle_plan."""
    g = load_golden("fuse_perm.npz")
    for n in g["sizes"].tolist():
        check_against_fixture(plan(lib, n), g, n)


def test_plan_agrees_with_the_restatement(lib):
    for seed in SEEDS:
        for n in (0, 1, 2, 3, 63, 64, 65):
            got, want = plan(lib, n, seed), R.plan(n, seed)
            assert (got == want).all() and (np.sort(got) == np.arange(n)).all(), (n, seed)
    assert len({plan(lib, 65, s).tobytes() for s in SEEDS}) == len(SEEDS)        # the seed matters
    from rescan_amd import capi
    assert (capi.shuffle_plan(65) == R.plan(65)).all() and len(capi.shuffle_plan(0)) == 0


def test_refusals_need_no_device(lib):
    perm = np.full(8, -7, np.int32)
    for call in (lib.rs_hip_shuffle_plan, lib.rs_hip_shuffle_permutation):
        assert call((1 << 24) + 1, 12346, perm.ctypes.data) == E_CAPACITY and b"2^24" in lib.rs_hip_last_error()
        assert call(-1, 12346, perm.ctypes.data) == E_ARG
        assert call(8, 12346, None) == E_ARG
        assert call(0, 12346, None) == 0                         # nothing to write
    assert (perm == -7).all()
    for why, n in (("capacity", (1 << 24) + 1), ("negative", -1)):
        with pytest.raises(R.Refused):
            R.plan(n)
    # a repeated id, a negative count, null arrays: before any device work
    ids = np.array([5, 9, 5], np.int32); pts = np.arange(8, dtype=np.int32); index = np.full(8, -7, np.int32); count = C.c_int64(-7)
    sel = lib.rs_hip_select_by_ids
    assert sel(pts.ctypes.data, 8, ids.ctypes.data, 3, index.ctypes.data, C.addressof(count)) == E_ARG and b"twice" in lib.rs_hip_last_error()
    assert sel(pts.ctypes.data, -1, ids.ctypes.data, 2, index.ctypes.data, C.addressof(count)) == E_ARG
    assert sel(None, 8, ids.ctypes.data, 2, index.ctypes.data, C.addressof(count)) == E_ARG
    assert sel(pts.ctypes.data, 8, ids.ctypes.data, 2, index.ctypes.data, None) == E_ARG
    assert sel(pts.ctypes.data, 8, None, 2, index.ctypes.data, C.addressof(count)) == E_ARG
    assert count.value == -7 and (index == -7).all()
    with pytest.raises(R.Refused):
        R.select(pts, ids)
    # no points or no ids: a count of 0, without a device
    assert sel(pts.ctypes.data, 0, ids.ctypes.data, 2, index.ctypes.data, C.addressof(count)) == 0 and count.value == 0
    count.value = -7
    assert sel(pts.ctypes.data, 8, None, 0, index.ctypes.data, C.addressof(count)) == 0 and count.value == 0 and (index == -7).all()
    # the merge: counts, arrays, the size of the result
    p = np.zeros((4, 3), np.float32); x = np.eye(4, dtype=np.float32).ravel(); out = np.full((8, 3), -7, np.float32)
    mrg = lib.rs_hip_merge_shuffled
    a = (p.ctypes.data, p.ctypes.data)
    assert mrg(*a, -1, x.ctypes.data, *a, 4, 12346, out.ctypes.data, out.ctypes.data, None) == E_ARG
    assert mrg(*a, 4, None, *a, 4, 12346, out.ctypes.data, out.ctypes.data, None) == E_ARG
    assert mrg(p.ctypes.data, None, 4, x.ctypes.data, *a, 4, 12346, out.ctypes.data, out.ctypes.data, None) == E_ARG       # A without normals
    assert mrg(*a, 4, x.ctypes.data, *a, 4, 12346, None, out.ctypes.data, None) == E_ARG
    assert mrg(*a, 1 << 24, x.ctypes.data, *a, 1, 12346, out.ctypes.data, out.ctypes.data, None) == E_CAPACITY
    assert mrg(None, None, 0, x.ctypes.data, None, None, 0, 12346, None, None, None) == 0                                  # an empty merge
    assert (out == -7).all()


def test_new_symbols_exist(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    for s in SYMBOLS:
        assert re.search(r" T %s\b" % s, out), s
    out = subprocess.check_output(["nm", "-D", "--defined-only", DROPIN], text=True)
    assert re.search(r" T rsd_augment_model\b", out)
    from rescan_amd import capi
    for s in SYMBOLS:
        assert s in capi.SIGNATURES, s
    for f in (capi.shuffle_plan, capi.shuffle_permutation, capi.select_by_ids, capi.merge_shuffled, capi.Cloud.fused):
        assert callable(f)


def test_new_entry_points_fail_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from rescan_amd import capi
    p = np.zeros((4, 3), np.float32)
    with pytest.raises(capi.RescanHipError, match="no HIP device"):
        capi.shuffle_permutation(8)
    with pytest.raises(capi.RescanHipError, match="no HIP device"):
        capi.select_by_ids(np.arange(8), [3])
    with pytest.raises(capi.RescanHipError, match="no HIP device"):
        capi.merge_shuffled(p, p, np.eye(4).ravel(), p, p)
    perm = np.full(8, -7, np.int32)
    assert lib.rs_hip_shuffle_permutation(8, 12346, perm.ctypes.data) == E_NODEVICE and (perm == -7).all()


def test_shim_refuses_without_a_device(built):
    d = C.CDLL(DROPIN)
    f = d.rsd_augment_model
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p] * 7 + [C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 8
    g = load_golden("fuse_wall.npz")
    outs = (C.c_void_p * 7)()
    ptrs = [C.addressof(outs) + 8 * k for k in range(7)]
    scan = [g["scan_" + k].ctypes.data for k in KEYS]; model = [g["model_" + k].ctypes.data for k in KEYS[:6]]
    pose = np.ascontiguousarray(g["pose"])
    assert f(None, *scan[1:], len(g["scan_pos"]), *model, len(g["model_pos"]), pose.ctypes.data, 1, 1, *ptrs, None) == E_ARG
    assert f(*scan, len(g["scan_pos"]), *model, len(g["model_pos"]), None, 1, 1, *ptrs, None) == E_ARG
    assert all(not outs[k] for k in range(7))
