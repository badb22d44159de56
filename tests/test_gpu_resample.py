"""GPU: rs_hip_uniform_resample, rsd_uniform_resample and rs_hip_cloud_create_resampled against the reference's fixtures
(tests/golden/resample_*.npz) and, where no recording exists, against the restatement that reproduces them (tests/resample_restate.py,
checked in tests/test_resample_cpu.py).  Comparisons are uint32 bit equality; one exception: an entry that is NaN in the reference (a
normal whose interpolated sum is zero) only has to be NaN on the device — x86 and gfx950 differ in the NaN they produce.
The GPU work runs in child processes, each under its own time limit; nothing here provokes a fault: every refusal is decided on the
host before a launch."""
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PRELUDE = r"""
import ctypes as C, hashlib, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from rescan_amd import capi
import hard_meshes as H
import resample_restate as R
capi.init(0)
KEYS = ("pos", "nor", "col", "radii", "cls", "inst")
OUT = dict(pos="pos", nor="nor", col="col", radii="radii", cls="class_ids", inst="instance_ids", face="face")
def golden(name): return dict(np.load(os.path.join(sys.argv[1], "tests", "golden", f"resample_{name}.npz")))
def fixture_mesh(g): return {k: g["mesh_" + k] for k in KEYS + ("faces",)}
def device(m, first=0, count=None):
    return capi.uniform_resample(m["pos"], m["faces"], m.get("nor"), m.get("col"), m.get("radii"), m.get("cls"), m.get("inst"), first, count)
def same(got, want, what):
    for k, o in OUT.items():
        if k in want:
            assert R.same_bits(got[o], want[k]), (what, k, np.flatnonzero(~(np.ascontiguousarray(got[o]).reshape(len(want[k]), -1) == np.ascontiguousarray(want[k]).reshape(len(want[k]), -1)).all(1))[:5])
def sha(a): return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)
def against_restatement(m, what, windows=None):
    n = capi.resample_plan(m["pos"], m["faces"])[0]
    want = R.resample(m)
    assert want["n_samples"] == n, what
    for first, count in windows or [(0, n)]:
        got = device(m, first, count)
        assert got["n_samples"] == n and len(got["pos"]) == count
        same(got, {k: want[k][first:first + count] for k in KEYS + ("face",)}, (what, first, count))
    return want
"""


def run_child(body, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


def test_fixtures_through_the_c_abi_whole_and_in_windows():
    run_child(r"""
for name in ("patch", "skew"):
    g = golden(name); m = fixture_mesh(g); n = int(g["n_samples"])
    got = device(m)
    assert got["n_samples"] == n
    same(got, g, name)
    for cuts in ((0, n // 2, n), (0, 257, n - 64, n)):                # two and three windows that partition the sequence
        parts = [device(m, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
        same({o: np.concatenate([p[o] for p in parts]) for o in OUT.values()}, g, (name, cuts))
g = golden("long"); m = fixture_mesh(g); n = int(g["n_samples"])
assert n > 65536
got = device(m)
for k, o in OUT.items():
    assert (sha(got[o]) == g["sha256_" + k]).all(), k
    assert R.same_bits(got[o][:256], g["head_" + k]) and R.same_bits(got[o][n - 256:], g["tail_" + k]), k
for cuts in ((0, 65536 - 3, n), (0, 1, 65536 + 1, n)):
    parts = [device(m, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    for k, o in OUT.items():
        assert (sha(np.concatenate([p[o] for p in parts])) == g["sha256_" + k]).all(), (k, cuts)
same(device(m, n - 256, 256), {k: g["tail_" + k] for k in OUT}, "long tail window")
# attributes without an input are skipped; positions alone give the same positions
only = capi.uniform_resample(m["pos"], m["faces"])
assert set(only) == {"n_samples", "pos", "face"} and (sha(only["pos"]) == g["sha256_pos"]).all()
print("ok")
""")


def test_fixtures_through_the_shim():
    run_child(r"""
d = C.CDLL(os.path.join(sys.argv[1], "rescan_amd", "librescan_dropin.so"))
f = d.rsd_uniform_resample; f.restype = C.c_int64
f.argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 6
for name in ("patch", "skew", "long"):
    g = golden(name); m = fixture_mesh(g); n = int(g["n_samples"])
    ins = [m[k].ctypes.data for k in KEYS]
    assert f(*ins, len(m["pos"]), m["faces"].ctypes.data, len(m["faces"]), 0, None, None, None, None, None, None) == n
    out = dict(pos=np.zeros((n, 3), np.float32), nor=np.zeros((n, 3), np.float32), col=np.zeros((n, 3), np.float32), radii=np.zeros(n, np.float32),
               cls=np.zeros(n, np.int32), inst=np.zeros(n, np.int32))
    assert f(*ins, len(m["pos"]), m["faces"].ctypes.data, len(m["faces"]), n, *[out[k].ctypes.data for k in KEYS]) == n
    for k in KEYS:
        if name == "long": assert (sha(out[k]) == g["sha256_" + k]).all(), k
        else: assert R.same_bits(out[k], g[k]), (name, k)
    assert f(*ins, len(m["pos"]), m["faces"].ctypes.data, len(m["faces"]), n - 1, *[out[k].ctypes.data for k in KEYS]) == -2     # capacity below the count
print("ok")
""")


def test_small_counts_and_offset_windows():
    run_child(r"""
for k in H.SMALL_COUNTS:
    m = H.triangle(k)
    n = capi.resample_plan(m["pos"], m["faces"])[0]
    assert n == k
    windows = [(0, n)] + ([(1, n - 1)] if n >= 1 else []) + [(n, 0)]
    against_restatement(m, ("triangle", k), windows)
print("ok")
""")


def test_hostile_meshes():
    run_child(r"""
w = against_restatement(H.triangle(257), "a single face")
assert (w["face"] == 0).all() and w["flipped"].any() and not w["flipped"].all()          # draws with s + t > 1, and without
m = H.mostly_degenerate()
w = against_restatement(m, "all faces but one of zero area")
assert (R.face_areas(m["pos"], m["faces"]) == 0).sum() == len(m["faces"]) - 1 and (w["face"] == 20).all()
m = H.equal_pair()
w = against_restatement(m, "two faces of equal area")
assert (capi.resample_plan(m["pos"], m["faces"])[2] == 1.0).all() and set(np.unique(w["face"])) == {0, 1}
# a zero normal sum: NaN in the reference's arithmetic, NaN on the device
m = H.triangle(65); m["nor"] = np.zeros_like(m["nor"])
w = against_restatement(m, "zero normals")
assert np.isnan(w["nor"]).all() and np.isnan(device(m)["nor"]).all()
# samples whose two smallest weights tie (the weights depend on the index alone: windows of the huge mesh around them)
m = H.huge(); plan = R.plan(m["pos"], m["faces"])
picks = set()
for i in H.TIE_INDICES:
    want = R.resample(m, i - 100, 256, plan)
    assert want["tie"][100] and want["tie"].sum() >= 1
    picks.add(int(want["pick"][100]))
    got = device(m, i - 100, 256)
    same(got, {k: want[k] for k in KEYS + ("face",)}, ("tie", i))
assert picks == {0, 1}                                  # vertex 0 wins a tie with 1 or 2, vertex 1 a tie with 2
print("ok")
""")


def test_large_indices():
    run_child(r"""
m = H.huge()
n = capi.resample_plan(m["pos"], m["faces"])[0]
assert (1 << 31) - (1 << 10) < n <= (1 << 31) - 1
plan = R.plan(m["pos"], m["faces"])
assert plan[0] == n
for first in ((1 << 16) - 128, (1 << 30) - 128, n - 256):
    want = R.resample(m, first, 256, plan)
    got = device(m, first, 256)
    assert got["n_samples"] == n
    same(got, {k: want[k] for k in KEYS + ("face",)}, ("huge", first))
assert 2 * (n - 1) >= 1 << 31                          # 2 i does not fit a signed 32-bit word: the jump runs in 64 bits
print("ok")
""")


def test_device_cloud_and_determinism():
    run_child(r"""
g = golden("patch"); m = fixture_mesh(g); n = int(g["n_samples"])
a = capi.Cloud.resampled(m["pos"], m["nor"], m["faces"])
b = capi.Cloud(g["pos"], g["nor"])
assert a.n == n == b.n and R.same_bits(a._pos, g["pos"]) and R.same_bits(a._nor, g["nor"])
q = np.ascontiguousarray(g["pos"][np.random.default_rng(3).permutation(n)[:512]] + np.float32(0.001))
ra, rb = capi.radius_search(a, q, 0.03, 16), capi.radius_search(b, q, 0.03, 16)
assert ra[3] == rb[3] > 512 and (ra[2] == rb[2]).all() and (ra[1] == rb[1]).all() and (ra[0].view(np.uint32) == rb[0].view(np.uint32)).all()
la, ia = capi.Cloud.level_of(a, 0.01, 256)
lb, ib = capi.Cloud.level_of(b, 0.01, 256)
assert la.n == lb.n and (ia == ib).all() and 0 < la.n < n
c = capi.Cloud.resampled(m["pos"], None, m["faces"])              # without normals
assert c.n == n and c._nor is None and R.same_bits(c._pos, g["pos"])
# two calls on the same mesh give equal bytes
for name in ("skew", "long"):
    m = fixture_mesh(golden(name))
    x, y = device(m), device(m)
    for o in OUT.values():
        assert x[o].tobytes() == y[o].tobytes(), (name, o)
a2 = capi.Cloud.resampled(fixture_mesh(g)["pos"], fixture_mesh(g)["nor"], fixture_mesh(g)["faces"])
assert a2._pos.tobytes() == a._pos.tobytes() and a2._nor.tobytes() == a._nor.tobytes()
print("ok")
""")
