"""CPU: the vertex-normal fixtures (tests/golden/normals_*.npz, written by the reference's own rs_pointcloud__compute_normals:
tools/normals_fixture) are reproduced by the NumPy restatement (tests/normals_restate.py) bit for bit where the reference's value is
not NaN, and as NaN where it is; every refusal of rs_hip_vertex_normals and rs_hip_cloud_create_from_mesh is decided before a device
is touched, with nothing written; the new entry points and the shim's exist."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

from conftest import ROOT, load_golden
import normal_meshes as M
import normals_restate as R

LIB = os.path.join(ROOT, "rescan_amd", "librescan_hip.so")
DROPIN = os.path.join(ROOT, "rescan_amd", "librescan_dropin.so")
NAMES = ("patch", "fan", "quirks")
E_ARG = -2
Y = np.array([0.0, 1.0, 0.0], np.float32)


@pytest.fixture(scope="module")
def built():
    from rescan_amd import build
    build.build()


def orders(name):
    return (("faces", ""), ("faces_shuffled", "_shuffled")) if name == "fan" else (("faces", ""),)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_the_mesh_of_normal_meshes_and_small(name):
    g = load_golden(f"normals_{name}.npz")
    pos, faces = getattr(M, name)()
    assert g["pos"].dtype == pos.dtype and g["pos"].tobytes() == pos.tobytes() and g["faces"].dtype == faces.dtype and (g["faces"] == faces).all()
    if name == "fan":
        assert (g["faces_shuffled"] == M.fan_shuffled()[1]).all() and (np.sort(g["faces_shuffled"].ravel()) == np.sort(faces.ravel())).all()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"normals_{name}.npz")) <= 757075


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_every_array(name):
    g = load_golden(f"normals_{name}.npz")
    for fk, sfx in orders(name):
        for loader, key in ((False, "nor"), (True, "nor_loader")):
            n, c = R.vertex_normals(g["pos"], g[fk], loader)
            assert R.same_bits(n, g[key + sfx]), (name, fk, key)
            assert c.dtype == g["counts"].dtype and (c == g["counts"]).all()
        assert not np.isnan(g["nor_loader" + sfx]).any()           # with the loader's pass the compare is on all bits


def test_fixtures_hold_the_cases():
    g = load_golden("normals_fan.npz")
    a, b = g["nor"][0], g["nor_shuffled"][0]
    assert g["counts"][0] == M.FAN_FACES == 3000
    assert (a.view(np.uint32) != b.view(np.uint32)).any() and np.abs(a - b).max() < 1e-4        # the order shows in the last bits only
    assert sorted(np.nonzero(g["faces"] == 0)[1][:3]) == [0, 1, 2]                              # the hub in every corner position
    g = load_golden("normals_quirks.npz")
    n, nl = g["nor"], g["nor_loader"]
    assert (n[[0, 1, 2]] == Y).all()                               # two opposite faces: exact cancellation
    assert (n[[3, 4]] == Y).all() and (g["counts"][[3, 4]] == [7, 2]).all()       # (a,a,b), (a,b,a), (a,a,a)
    assert (n[9] == Y).all() and g["counts"][9] == 0               # no face names it
    assert np.isnan(n[10:13, 2]).all() and (n[10:13, :2] == 0).all() and (nl[10:13] == 0).all()     # overflow: infinite norm -> NaN -> zeros
    assert (n[13:16] == Y).all()                                   # a NaN coordinate fails the compare
    assert (n[16:22] == Y).all()                                   # underflow to zero; denormal products whose squares are zero
    assert not (n[22:25] == Y).all(1).any() and np.isfinite(n[22:25]).all()       # denormal squares, positive sum
    assert (g["counts"][[5, 8]] == [5, 4]).all()
    # vertex 5 pins "one t for both corners of a doubled face", vertex 8 "the count advances after the face": a restatement
    # that advances per corner gives other bits
    fn = R.face_normals(g["pos"], g["faces"])
    F = np.float32
    lerp = lambda a, b, t: t * b + (F(1.0) - t) * a                # noqa: E731
    v = np.zeros(3, F)
    for face, t in ((5, 1), (6, 2), (7, 3), (7, 4), (8, 5)):       # per corner: 1/3 then 1/4 inside face 7
        v = lerp(v, fn[face], F(1.0) / F(t))
    wrong = v / np.sqrt((v * v).sum(dtype=F))
    assert (wrong.view(np.uint32) != n[5].view(np.uint32)).any()


def test_restatement_is_quick_on_many_faces():
    pos, faces = M.grid(300, 301)
    assert len(pos) == 90300 and len(faces) == 179400 and len(pos) % 256 and len(faces) % 256
    t0 = time.perf_counter()
    n, c = R.vertex_normals(pos, faces, True)
    assert time.perf_counter() - t0 < 5.0
    assert c.max() == 6 and c.min() == 1 and c.sum() == 3 * len(faces)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6 and (np.sign(n[:, 1]) == np.sign(n[0, 1])).all() and n[0, 1] != 0      # a height field: every normal points one way


def normals_lib():
    lib = C.CDLL(LIB)
    f = lib.rs_hip_vertex_normals
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    g = lib.rs_hip_cloud_create_from_mesh
    g.restype = C.c_void_p
    g.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]
    lib.rs_hip_last_error.restype = C.c_char_p
    return lib


def test_refusals_need_no_device(built):
    """Each refusal of include/rescan_hip.h with nothing written.  Fails on a library without rs_hip_vertex_normals."""
    lib = normals_lib()
    pos, faces = M.single()
    out = np.full((4, 3), -7.0, np.float32); cnt = np.full(4, -7, np.int32)
    bad_hi = np.array([[0, 1, 3]], np.int32); bad_lo = np.array([[0, -1, 2]], np.int32)
    P, Fc, O, Cn = pos.ctypes.data, faces.ctypes.data, out.ctypes.data, cnt.ctypes.data
    cases = [
        ("null pos", (None, 3, Fc, 1, 0, O, Cn)),
        ("null faces", (P, 3, None, 1, 0, O, Cn)),
        ("null out_nor", (P, 3, Fc, 1, 0, None, Cn)),
        ("no vertices", (P, 0, Fc, 1, 0, O, Cn)),
        ("negative vertex count", (P, -3, Fc, 1, 0, O, Cn)),
        ("no faces", (P, 3, Fc, 0, 1, O, Cn)),
        ("negative face count", (P, 3, Fc, -1, 0, O, Cn)),
        ("index past the vertices", (P, 3, bad_hi.ctypes.data, 1, 0, O, Cn)),
        ("negative index", (P, 3, bad_lo.ctypes.data, 1, 1, O, Cn)),
        ("3 n_faces above INT32_MAX", (P, 3, Fc, (1 << 31) // 3 + 1, 0, O, Cn)),       # refused on the count, before a face is read
        ("n_vertices above INT32_MAX", (P, 1 << 31, Fc, 1, 0, O, Cn)),
    ]
    for what, args in cases:
        rc = lib.rs_hip_vertex_normals(*args)
        assert rc == E_ARG and lib.rs_hip_last_error().startswith(b"vertex_normals:"), (what, rc, lib.rs_hip_last_error())
        assert (out == -7.0).all() and (cnt == -7).all(), what
    # the restatement refuses the same meshes
    for f in (bad_hi, bad_lo, np.zeros((0, 3), np.int32)):
        with pytest.raises(R.Refused):
            R.vertex_normals(pos, f)
    # from_mesh: the same, and the resampler's own (a zero-area mesh), all on the host
    n = C.c_int64(-7)
    flat = np.array([[0, 0, 0], [0, 1, 1]], np.int32)
    for what, args, text in [
        ("null pos", (None, 3, Fc, 1), b"vertex_normals:"),
        ("no vertices", (P, 0, Fc, 1), b"vertex_normals:"),
        ("no faces", (P, 3, Fc, 0), b"vertex_normals:"),
        ("index past the vertices", (P, 3, bad_hi.ctypes.data, 1), b"resample: face 0 names vertex 3"),
        ("zero area", (P, 3, flat.ctypes.data, 2), b"resample: the area sum"),
    ]:
        assert lib.rs_hip_cloud_create_from_mesh(*args, -1.0, C.addressof(n)) is None, what
        assert lib.rs_hip_last_error().startswith(text) and n.value == -7, (what, lib.rs_hip_last_error())


def test_new_symbols_exist_and_the_shim_refuses_without_a_device(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    for s in ("rs_hip_vertex_normals", "rs_hip_cloud_create_from_mesh"):
        assert re.search(r" T %s\b" % s, out), s
    out = subprocess.check_output(["nm", "-D", "--defined-only", DROPIN], text=True)
    assert re.search(r" T rsd_compute_normals\b", out)
    from rescan_amd import capi
    assert callable(capi.vertex_normals) and callable(capi.Cloud.from_mesh)
    with pytest.raises(capi.RescanHipError, match="vertex_normals: face 0 names vertex 3"):
        capi.vertex_normals(M.single()[0], [[0, 1, 3]])
    d = C.CDLL(DROPIN)
    f = d.rsd_compute_normals
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    pos, faces = M.single()
    nor = np.full((3, 3), -7.0, np.float32)
    bad = np.array([[0, 1, 3]], np.int32)
    assert f(pos.ctypes.data, 3, bad.ctypes.data, 1, nor.ctypes.data) == E_ARG
    assert f(pos.ctypes.data, 3, faces.ctypes.data, 0, nor.ctypes.data) == E_ARG          # no face: the reference's loop stays
    assert f(pos.ctypes.data, 3, faces.ctypes.data, 1, None) == E_ARG
    assert (nor == -7.0).all()
