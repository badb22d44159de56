"""GPU: rs_hip_vertex_normals, rsd_compute_normals and rs_hip_cloud_create_from_mesh against the reference's fixtures
(tests/golden/normals_*.npz) and, where no recording exists, against the restatement that reproduces them (tests/normals_restate.py,
checked in tests/test_normals_cpu.py).  The comparison rule (normals_restate.same_bits): bit for bit where the reference's value is not
NaN, NaN where it is — x86 and gfx950 differ in the NaN an inf * 0 makes; with the loader's pass no NaN is left and every bit counts.
The GPU work runs in child processes, each under its own time limit; nothing here provokes a fault: every refusal is decided on the host
before a launch."""
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PRELUDE = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from rescan_amd import capi
import normal_meshes as M
import normals_restate as R
capi.init(0)
def golden(name): return dict(np.load(os.path.join(sys.argv[1], "tests", "golden", f"normals_{name}.npz")))
def orders(name): return (("faces", ""), ("faces_shuffled", "_shuffled")) if name == "fan" else (("faces", ""),)
def rows(got, want): return np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[:5]
def against_restatement(pos, faces, what):
    for loader in (False, True):
        want, wc = R.vertex_normals(pos, faces, loader)
        got, gc = capi.vertex_normals(pos, faces, loader, counts=True)
        assert R.same_bits(got, want), (what, loader, rows(got, want))
        assert (gc == wc).all(), what
        if loader: assert got.tobytes() == want.tobytes(), what
    return want
"""


def run_child(body, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


def test_fixtures_through_the_c_abi():
    run_child(r"""
for name in ("patch", "fan", "quirks"):
    g = golden(name)
    for fk, sfx in orders(name):
        for loader, key in ((False, "nor"), (True, "nor_loader")):
            got, cnt = capi.vertex_normals(g["pos"], g[fk], loader, counts=True)
            assert R.same_bits(got, g[key + sfx]), (name, fk, key, rows(got, g[key + sfx]))
            assert cnt.dtype == np.int32 and (cnt == g["counts"]).all(), (name, fk)
            if loader: assert got.tobytes() == g[key + sfx].tobytes()
            alone = capi.vertex_normals(g["pos"], g[fk], loader)                       # counts NULL
            assert alone.tobytes() == got.tobytes() or np.isnan(got).any()
g = golden("fan")
a, b = capi.vertex_normals(g["pos"], g["faces"])[0], capi.vertex_normals(g["pos"], g["faces_shuffled"])[0]
assert (a.view(np.uint32) != b.view(np.uint32)).any()          # the hub's chain is walked in face order: another order, other last bits
print("ok")
""")


def test_fixtures_through_the_shim():
    run_child(r"""
d = C.CDLL(os.path.join(sys.argv[1], "rescan_amd", "librescan_dropin.so"))
f = d.rsd_compute_normals; f.restype = C.c_int32
f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
for name in ("patch", "fan", "quirks"):
    g = golden(name)
    for fk, sfx in orders(name):
        out = np.full((len(g["pos"]), 3), -7.0, np.float32)
        assert f(g["pos"].ctypes.data, len(g["pos"]), g[fk].ctypes.data, len(g[fk]), out.ctypes.data) == 0
        assert R.same_bits(out, g["nor" + sfx]), (name, fk, rows(out, g["nor" + sfx]))
        bad = g[fk].copy(); bad[len(bad) // 2, 1] = len(g["pos"])
        assert f(g["pos"].ctypes.data, len(g["pos"]), bad.ctypes.data, len(bad), out.ctypes.data) == -2      # where the reference's loop stays
        assert R.same_bits(out, g["nor" + sfx])
print("ok")
""")


def test_sizes_that_cross_launch_boundaries():
    run_child(r"""
pos, faces = M.single()
against_restatement(pos, faces, "a single face on 3 vertices")
pos, faces = M.grid(5, 13)
assert len(pos) == 65
against_restatement(pos, faces, "65 vertices")
pos, faces = M.grid(300, 301)
assert len(pos) == 90300 and len(pos) % 256 and len(faces) % 256 and (3 * len(faces)) % 256
against_restatement(pos, faces, "a 300 x 301 grid")
pos, faces = M.ends()
assert len(pos) == 70001 > 1 << 16
w = against_restatement(pos, faces, "faces on the first and the last three of 70 001 vertices")
assert (w[3:-3] == np.array([0, 1, 0], np.float32)).all() and not (w[-3:] == np.array([0, 1, 0], np.float32)).all(1).any()
pos, faces = M.fan(hub_last=True)
assert (faces == len(pos) - 1).sum() == M.FAN_FACES
against_restatement(pos, faces, "the fan with its hub at the last vertex")
pos, faces = M.fan_shuffled(hub_last=True)
against_restatement(pos, faces, "the shuffled fan with its hub at the last vertex")
print("ok")
""")


def test_from_mesh_equals_resampled_with_the_same_normals():
    run_child(r"""
g = golden("patch")
cases = [("patch", g["pos"], g["faces"], g["nor_loader"])]
pos, faces = M.grid(300, 301)
cases.append(("grid", pos, faces, R.vertex_normals(pos, faces, True)[0]))
for what, pos, faces, nor in cases:
    assert capi.vertex_normals(pos, faces, True).tobytes() == nor.tobytes(), what
    a = capi.Cloud.from_mesh(pos, faces)
    b = capi.Cloud.resampled(pos, nor, faces)
    assert a.n == b.n > 1000, what
    assert a._pos.tobytes() == b._pos.tobytes() and a._nor.tobytes() == b._nor.tobytes(), what
    q = np.ascontiguousarray(b._pos[np.random.default_rng(5).permutation(b.n)[:512]] + np.float32(0.001))
    ra, rb = capi.radius_search(a, q, 0.03, 16), capi.radius_search(b, q, 0.03, 16)
    assert ra[3] == rb[3] > 512 and (ra[2] == rb[2]).all() and (ra[1] == rb[1]).all() and (ra[0].view(np.uint32) == rb[0].view(np.uint32)).all(), what
    # the older entry point keeps its meaning of "no normals"
    c = capi.Cloud.resampled(pos, None, faces)
    assert c.n == a.n and c._nor is None and c._pos.tobytes() == a._pos.tobytes()
print("ok")
""")


def test_two_calls_give_the_same_bytes():
    run_child(r"""
for what, (pos, faces) in (("shuffled fan", M.fan_shuffled()), ("grid", M.grid(300, 301))):
    for loader in (False, True):
        x, cx = capi.vertex_normals(pos, faces, loader, counts=True)
        y, cy = capi.vertex_normals(pos, faces, loader, counts=True)
        assert x.tobytes() == y.tobytes() and cx.tobytes() == cy.tobytes(), (what, loader)
pos, faces = M.grid(300, 301)                                    # (the fan's area would make tens of millions of samples)
a, b = capi.Cloud.from_mesh(pos, faces), capi.Cloud.from_mesh(pos, faces)
assert a.n == b.n and a._pos.tobytes() == b._pos.tobytes() and a._nor.tobytes() == b._nor.tobytes()
print("ok")
""")


def test_refusals_on_the_device_path_leave_the_library_usable():
    run_child(r"""
g = golden("patch")
capi.Cloud.from_mesh(g["pos"], g["faces"])                       # the device is up
pos, _ = M.single()
lib = capi.load()
n = C.c_int64(-7)
flat = np.array([[0, 0, 0], [0, 1, 1]], np.int32)
assert lib.rs_hip_cloud_create_from_mesh(pos.ctypes.data, 3, flat.ctypes.data, 2, -1.0, C.byref(n)) is None
assert lib.rs_hip_last_error().startswith(b"resample: the area sum") and n.value == -7
try:
    capi.Cloud.from_mesh(pos, flat); assert False
except capi.RescanHipError as e:
    assert "resample: the area sum" in str(e)
try:
    capi.vertex_normals(pos, [[0, 1, 3]]); assert False
except capi.RescanHipError as e:
    assert "names vertex 3" in str(e)
got = capi.vertex_normals(g["pos"], g["faces"], True)
assert got.tobytes() == g["nor_loader"].tobytes()
a = capi.Cloud.from_mesh(g["pos"], g["faces"])
b = capi.Cloud.resampled(g["pos"], g["nor_loader"], g["faces"])
assert a.n == b.n and a._nor.tobytes() == b._nor.tobytes()
print("ok")
""")
