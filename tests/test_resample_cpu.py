"""CPU: the mesh resampler's fixtures (tests/golden/resample_*.npz, written by the reference's own
rs_pointcloud_uniform_resample and msh_discrete_distribution_init: tools/resample_fixture) are reproduced bit for bit by the NumPy
restatement that computes every sample on its own (tests/resample_restate.py); the host planner behind rs_hip_resample_plan gives
the reference's sample count, total area and alias table without a device; every refusal is decided before a device is touched;
the new entry points exist."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
import hard_meshes as H
import resample_restate as R

LIB = os.path.join(ROOT, "rescan_amd", "librescan_hip.so")
DROPIN = os.path.join(ROOT, "rescan_amd", "librescan_dropin.so")
KEYS = ("pos", "nor", "col", "radii", "cls", "inst")
FULL = ("patch", "skew")
E_ARG, E_CAPACITY = -2, -4


@pytest.fixture(scope="module")
def built():
    from rescan_amd import build
    build.build()


def fixture_mesh(g):
    return {k: g["mesh_" + k] for k in KEYS + ("faces",)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


@pytest.mark.parametrize("name", FULL + ("long",))
def test_fixture_is_the_mesh_of_hard_meshes_and_small(name):
    g = load_golden(f"resample_{name}.npz")
    m = getattr(H, name)()
    for k in KEYS + ("faces",):
        assert g["mesh_" + k].dtype == m[k].dtype and (bits(g["mesh_" + k]) == bits(m[k])).all(), k
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"resample_{name}.npz")) <= 757075
    n = int(g["n_samples"])
    assert {"patch": 5000 <= n <= 7000, "skew": 2500 <= n <= 3500, "long": n > 65536}[name]


@pytest.mark.parametrize("name", FULL)
def test_restatement_reproduces_every_array(name):
    g = load_golden(f"resample_{name}.npz")
    r = R.resample(fixture_mesh(g))
    assert r["n_samples"] == int(g["n_samples"]) and bits(np.float64(r["total_area"])) == bits(g["total_area"])
    for k in KEYS + ("face",):
        assert r[k].dtype == g[k].dtype and r[k].shape == g[k].shape and (bits(r[k]) == bits(g[k])).all(), k
    _, _, prob, alias = R.plan(g["mesh_pos"], g["mesh_faces"])
    assert (bits(prob) == bits(g["prob"])).all() and (alias == g["alias"]).all()
    # windows give the same samples
    n = r["n_samples"]
    for first, count in ((0, 1), (1, 64), (n - 257, 257), (n, 0), (n // 2, 300)):
        w = R.resample(fixture_mesh(g), first, count)
        for k in KEYS + ("face",):
            assert (bits(w[k]) == bits(g[k][first:first + count])).all(), (k, first, count)


def test_fixtures_hold_the_cases():
    g = load_golden("resample_patch.npz")
    used = np.bincount(g["face"], minlength=len(g["mesh_faces"]))
    areas = R.face_areas(g["mesh_pos"], g["mesh_faces"])
    assert (areas[-2:] == 0).all() and (used[-2:] == 0).all() and (g["prob"][-2:] == 0).all()       # the two zero-area faces
    assert used[-3] > len(g["face"]) // 3                                                          # the large triangle
    r = R.resample(fixture_mesh(g))
    assert 0.3 < r["flipped"].mean() < 0.7
    g = load_golden("resample_skew.npz")
    areas = R.face_areas(g["mesh_pos"], g["mesh_faces"])
    big = int(np.argmax(areas))
    assert areas[big] > 0.99 * areas.sum() and np.log10(areas.max() / areas.min()) >= 6 and (g["alias"] == big).sum() >= 190


def test_restatement_reproduces_the_long_sequence():
    g = load_golden("resample_long.npz")
    r = R.resample(fixture_mesh(g))
    n = int(g["n_samples"])
    assert r["n_samples"] == n > 65536
    for k in KEYS + ("face",):
        assert (sha(r[k]) == g["sha256_" + k]).all(), k
        assert (bits(r[k][:256]) == bits(g["head_" + k])).all() and (bits(r[k][n - 256:]) == bits(g["tail_" + k])).all(), k
    w = R.resample(fixture_mesh(g), n - 256, 256)
    for k in KEYS + ("face",):
        assert (bits(w[k]) == bits(g["tail_" + k])).all(), k


def test_the_chosen_mesh_has_tied_weights():
    """hard_meshes.TIE_INDICES: one tie of each pair of weights among the smallest two."""
    pairs = set()
    for i in H.TIE_INDICES:
        w0, w1, w2, _ = R.weights(i, 1)
        m = min(w0[0], w1[0], w2[0])
        tied = tuple(k for k, w in enumerate((w0[0], w1[0], w2[0])) if w == m)
        assert len(tied) == 2, (i, w0, w1, w2)
        pairs.add(tied)
    assert pairs == {(1, 2), (0, 2), (0, 1)}


def plan_lib():
    lib = C.CDLL(LIB)
    f = lib.rs_hip_resample_plan
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rs_hip_last_error.restype = C.c_char_p
    return lib


def run_plan(lib, pos, faces, table=True, n_faces=None, n_vertices=None):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3); faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    n, total = C.c_int64(-7), C.c_double(-7.0)
    nf = len(faces) if n_faces is None else n_faces
    prob, alias = np.full(max(len(faces), 1), -7.0), np.full(max(len(faces), 1), -7, np.int32)
    rc = lib.rs_hip_resample_plan(pos.ctypes.data, len(pos) if n_vertices is None else n_vertices, faces.ctypes.data, nf, C.addressof(n), C.addressof(total),
                                  prob.ctypes.data if table else None, alias.ctypes.data if table else None)
    return rc, n.value, total.value, prob, alias


@pytest.mark.parametrize("name", FULL + ("long",))
def test_plan_gives_the_reference_count_area_and_alias_table(built, name):
    """Fails on a library without rs_hip_resample_plan."""
    g = load_golden(f"resample_{name}.npz")
    lib = plan_lib()
    rc, n, total, prob, alias = run_plan(lib, g["mesh_pos"], g["mesh_faces"])
    assert rc == 0, lib.rs_hip_last_error()
    assert n == int(g["n_samples"]) and bits(np.float64(total)) == bits(g["total_area"])
    assert (bits(prob) == bits(g["prob"])).all() and (alias == g["alias"]).all()
    rc, n2, total2, prob, alias = run_plan(lib, g["mesh_pos"], g["mesh_faces"], table=False)
    assert rc == 0 and n2 == n and total2 == total and (prob == -7.0).all() and (alias == -7).all()


def test_plan_agrees_with_the_restatement_on_the_other_meshes(built):
    lib = plan_lib()
    meshes = [H.triangle(k) for k in H.SMALL_COUNTS[1:]] + [H.mostly_degenerate(), H.equal_pair(), H.huge()]
    for m in meshes:
        want = R.plan(m["pos"], m["faces"])
        rc, n, total, prob, alias = run_plan(lib, m["pos"], m["faces"])
        assert rc == 0 and n == want[0] and bits(np.float64(total)) == bits(np.float64(want[1]))
        assert (bits(prob) == bits(want[2])).all() and (alias == want[3]).all()
    assert [R.plan(H.triangle(k)["pos"], H.triangle(k)["faces"])[0] for k in H.SMALL_COUNTS] == list(H.SMALL_COUNTS)
    n = R.plan(H.huge()["pos"], H.huge()["faces"])[0]
    assert (1 << 31) - (1 << 10) < n <= R.INT32_MAX
    assert (R.plan(H.equal_pair()["pos"], H.equal_pair()["faces"])[2] == 1.0).all()
    assert (R.face_areas(H.mostly_degenerate()["pos"], H.mostly_degenerate()["faces"]) == 0).sum() == 39


def refusals():
    tri = H.triangle(64)
    inf = tri["pos"].copy(); inf[1, 0] = np.inf
    far = tri["pos"].copy(); far[1, 0] = 3e38; far[2, 2] = -3e38
    big = H.huge()
    return [
        ("index past the vertices", tri["pos"], [[0, 1, 3]], None, E_ARG),
        ("negative index", tri["pos"], [[0, -1, 2]], None, E_ARG),
        ("no faces", tri["pos"], np.zeros((0, 3), np.int32), None, E_ARG),
        ("negative face count", tri["pos"], [[0, 1, 2]], -1, E_ARG),
        ("infinite vertex", inf, [[0, 1, 2]], None, E_ARG),
        ("area overflows fp32", far, [[0, 1, 2]], None, E_ARG),
        ("zero area", tri["pos"], [[0, 0, 0], [0, 1, 1]], None, E_ARG),
        ("area sum below 1e-8", tri["pos"] * np.float32(1e-3 / np.sqrt(64.5 / 6400.0) * 0.09), [[0, 1, 2]], None, E_ARG),
        ("more than 2^24 faces", tri["pos"], np.zeros(((1 << 24) + 1, 3), np.int32), None, E_CAPACITY),
        ("more than INT32_MAX samples", big["pos"] * np.float32(1.001), big["faces"], None, E_CAPACITY),
    ]


def test_refusals_need_no_device(built):
    """Each refusal of include/rescan_hip.h, through the plan and through rs_hip_uniform_resample, with nothing written."""
    lib = plan_lib()
    res = lib.rs_hip_uniform_resample
    res.restype = C.c_int
    res.argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 7
    out = np.full((64, 3), -7.0, np.float32)
    for what, pos, faces, n_faces, code in refusals():
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3); faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        try:
            R.plan(pos, faces if n_faces is None else faces[:0])
            assert False, what + ": the restatement accepts it"
        except R.Refused as e:
            assert e.code == code, what
        rc, n, total, prob, alias = run_plan(lib, pos, faces, n_faces=n_faces)
        assert rc == code and lib.rs_hip_last_error().startswith(b"resample:"), (what, rc, lib.rs_hip_last_error())
        assert n == -7 and total == -7.0 and (prob == -7.0).all() and (alias == -7).all(), what
        nf = len(faces) if n_faces is None else n_faces
        rc = res(pos.ctypes.data, None, None, None, None, None, len(pos), faces.ctypes.data, nf, 0, 1, out.ctypes.data, None, None, None, None, None, None)
        assert rc == code and (out == -7.0).all(), (what, rc)
    # the area sum that is refused is the fp32 one: just above 1e-8 passes the plan
    tri = H.triangle(64)
    ok = tri["pos"] * np.float32(1e-3 / np.sqrt(64.5 / 6400.0) * 0.11)
    assert 1e-8 < R.face_areas(ok, [[0, 1, 2]])[0] < 2e-8 and run_plan(lib, ok, [[0, 1, 2]])[:2] == (0, 0)
    # arguments of rs_hip_uniform_resample itself: pos / out_pos required, the window inside [0, n_samples]
    pos, faces = tri["pos"], tri["faces"]
    call = lambda p, o, first, count: res(p, None, None, None, None, None, 3, faces.ctypes.data, 1, first, count, o, None, None, None, None, None, None)   # noqa: E731
    assert call(None, out.ctypes.data, 0, 1) == E_ARG and call(pos.ctypes.data, None, 0, 1) == E_ARG
    for first, count in ((-1, 1), (0, -1), (0, 65), (64, 1), (65, 0), (1 << 62, 1 << 62)):
        assert call(pos.ctypes.data, out.ctypes.data, first, count) == E_ARG, (first, count)
    assert b"window" in lib.rs_hip_last_error() and (out == -7.0).all()
    # count = 0 succeeds and writes nothing, without a device
    assert call(pos.ctypes.data, out.ctypes.data, 0, 0) == 0 and call(pos.ctypes.data, out.ctypes.data, 64, 0) == 0 and (out == -7.0).all()


def test_new_symbols_exist(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    for s in ("rs_hip_resample_plan", "rs_hip_uniform_resample", "rs_hip_cloud_create_resampled", "rs_hip_cloud_points"):
        assert re.search(r" T %s\b" % s, out), s
    out = subprocess.check_output(["nm", "-D", "--defined-only", DROPIN], text=True)
    assert re.search(r" T rsd_uniform_resample\b", out)
    from rescan_amd import capi
    assert callable(capi.resample_plan) and callable(capi.uniform_resample) and callable(capi.Cloud.resampled)
    n, total, prob, alias = capi.resample_plan(H.equal_pair()["pos"], H.equal_pair()["faces"])
    assert n == 3200 and total == 0.5 and (prob == 1.0).all() and (alias == [0, 1]).all()


def test_shim_returns_the_count_without_a_device(built):
    d = C.CDLL(DROPIN)
    f = d.rsd_uniform_resample
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 6
    g = load_golden("resample_patch.npz")
    pos, faces = g["mesh_pos"], g["mesh_faces"]
    assert f(pos.ctypes.data, None, None, None, None, None, len(pos), faces.ctypes.data, len(faces), 0, None, None, None, None, None, None) == int(g["n_samples"])
    out = np.full((16, 3), -7.0, np.float32)
    assert f(pos.ctypes.data, None, None, None, None, None, len(pos), faces.ctypes.data, len(faces), 16, out.ctypes.data, None, None, None, None, None) == E_ARG
    bad = faces.copy(); bad[5, 1] = len(pos)
    assert f(pos.ctypes.data, None, None, None, None, None, len(pos), bad.ctypes.data, len(faces), 0, None, None, None, None, None, None) == E_ARG
    assert (out == -7.0).all()
