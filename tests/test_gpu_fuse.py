"""GPU: rs_hip_shuffle_permutation, rs_hip_select_by_ids, rs_hip_merge_shuffled, rs_hip_cloud_create_fused and rsd_augment_model
against the reference's fixtures (tests/golden/fuse_*.npz) and, where no recording exists, against the host plan and the restatement
that reproduce them (tests/fuse_restate.py, checked in tests/test_fuse_cpu.py).  Comparisons are uint32 bit equality.
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
import fuse_restate as R
capi.init(0)
KEYS = ("pos", "nor", "col", "radii", "qual", "cls", "inst")
def golden(name): return dict(np.load(os.path.join(sys.argv[1], "tests", "golden", f"fuse_{name}.npz")))
def sha(a): return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)
def attributes(g, info):
    # the merged cloud's other arrays, through scan_index / source and the device gather
    names = ("col", "radii", "qual", "cls")
    ext = capi.gather_attributes(info["scan_index"], [g["scan_" + k] for k in names])
    both = [np.concatenate([e, g["model_" + k]]) for e, k in zip(ext, names)]
    out = dict(zip(names, capi.gather_attributes(info["source"], both)))
    out["inst"] = np.full(len(info["source"]), g["uidx"], np.int32)
    return out
def check_row(g, cloud, info):
    n_ext = len(g["extracted_pos"])
    assert info["n_extracted"] == n_ext and cloud.n == n_ext + len(g["model_pos"])
    assert (info["scan_index"] == R.select(g["scan_inst"], [int(g["uidx"])])).all()
    assert R.same_bits(g["scan_pos"][info["scan_index"]], g["extracted_pos"])
    assert R.same_bits(info["xform"], g["xform"]), (info["xform"], g["xform"])
    assert (info["source"] == R.plan(cloud.n)).all()
    assert R.same_bits(cloud._pos, g["merged_pos"]) and R.same_bits(cloud._nor, g["merged_nor"])
    got = attributes(g, info)
    for k in ("col", "radii", "qual", "cls", "inst"):
        assert R.same_bits(got[k], g["merged_" + k]), k
    level, _ = capi.Cloud.level_of(cloud, 0.01, 256)             # voxel_size[1], 1024 * 1 / 4 (rs_pointcloud.h:145,995)
    assert level.n == int(g["level_counts"][1]) and cloud.n == int(g["level_counts"][0])
"""


def run_child(body, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


def test_permutation_equals_the_host_plan_and_the_fixtures():
    run_child(r"""
g = golden("perm")
for seed in (12346, 977):
    for n in (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4097, 65535, 65537, 200001):
        got, want = capi.shuffle_permutation(n, seed), capi.shuffle_plan(n, seed)
        assert got.shape == want.shape and (got == want).all(), (n, seed, np.flatnonzero(got != want)[:5])
for n in g["sizes"].tolist():
    got = capi.shuffle_permutation(n)
    if f"perm_{n}" in g:
        assert (got == g[f"perm_{n}"]).all(), n
    else:
        assert (sha(got) == g[f"sha256_{n}"]).all() and (got[:256] == g[f"head_{n}"]).all() and (got[n - 256:] == g[f"tail_{n}"]).all(), n
# a small size after a large one (the workspace keeps its larger buffers), and the same call twice
assert (capi.shuffle_permutation(65) == capi.shuffle_plan(65)).all()
assert capi.shuffle_permutation(200001).tobytes() == capi.shuffle_permutation(200001).tobytes()
print("ok")
""")


def test_select_keeps_the_input_order():
    run_child(r"""
def run_edge(n):
    # a run of matches across the last wave, block or 65 536 boundary below n
    for e in (65536, 256, 64):
        if e < n: return np.arange(max(0, e - 6), min(n, e + 7))
    return np.arange(max(0, n - 3), n)
for ids in ([7], [7, -2, 40]):
    other = np.array([5, 8, 41, -3], np.int32)
    for n in (0, 1, 64, 65, 257, 70001):
        masks = dict(all=np.ones(n, bool), none=np.zeros(n, bool), alternating=np.arange(n) % 2 == 0, run=np.isin(np.arange(n), run_edge(n)))
        if n == 70001:
            masks["last"] = np.arange(n) == n - 1
        for what, m in masks.items():
            pts = np.where(m, np.array(ids, np.int32)[np.arange(n) % len(ids)], other[np.arange(n) % len(other)]).astype(np.int32)
            got, want = capi.select_by_ids(pts, ids), R.select(pts, ids)
            assert (want == np.flatnonzero(m)).all() and got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), (len(ids), n, what)
print("ok")
""")


def test_merge_is_the_reference_merge():
    run_child(r"""
g = golden("chair")
pos, nor, source = capi.merge_shuffled(g["extracted_pos"], g["extracted_nor"], g["xform"], g["model_pos"], g["model_nor"])
assert R.same_bits(pos, g["merged_pos"]) and R.same_bits(nor, g["merged_nor"])
n = len(pos)
assert (source == R.plan(n)).all() and (source == capi.shuffle_permutation(n)).all()
# one side empty, and a single point
E = np.zeros((0, 3), np.float32)
for a, b in ((E, g["model_pos"][:300]), (g["extracted_pos"][:257], E), (g["extracted_pos"][:1], E), (E, g["model_pos"][:1])):
    an = g["extracted_nor"][:len(a)]; bn = g["model_nor"][:len(b)]
    got = capi.merge_shuffled(a, an, g["xform"], b, bn)
    want = R.merge(a, an, g["xform"], b, bn)
    for x, y in zip(got, want):
        assert R.same_bits(x, y), (len(a), len(b))
got = capi.merge_shuffled(E, E, g["xform"], E, E)
assert all(len(x) == 0 for x in got)
# another seed gives another order of the same points
p2, n2, s2 = capi.merge_shuffled(g["extracted_pos"], g["extracted_nor"], g["xform"], g["model_pos"], g["model_nor"], seed=977)
w2 = R.merge(g["extracted_pos"], g["extracted_nor"], g["xform"], g["model_pos"], g["model_nor"], seed=977)
assert R.same_bits(p2, w2[0]) and R.same_bits(n2, w2[1]) and (s2 == w2[2]).all() and (s2 != source).any()
print("ok")
""")


def test_whole_row_dynamic_placement():
    run_child(r"""
g = golden("chair")
scan = capi.Cloud(g["scan_pos"], g["scan_nor"]); model = capi.Cloud(g["model_pos"], g["model_nor"])
cloud, info = capi.Cloud.fused(scan, g["scan_inst"], int(g["uidx"]), model, g["pose"], refine=True, max_dist=float(g["max_dist"]), max_angle=float(g["max_angle"]))
assert np.float32(info["icp_err"]).view(np.uint32) == g["icp_err"].view(np.uint32), (info["icp_err"], g["icp_err"])
check_row(g, cloud, info)
# the same call again gives the same bytes
again, info2 = capi.Cloud.fused(scan, g["scan_inst"], int(g["uidx"]), model, g["pose"])
assert again._pos.tobytes() == cloud._pos.tobytes() and info2["xform"].tobytes() == info["xform"].tobytes()
print("ok")
""")


def test_whole_row_static_placement_and_absent_id():
    run_child(r"""
g = golden("wall")
scan = capi.Cloud(g["scan_pos"], g["scan_nor"]); model = capi.Cloud(g["model_pos"], g["model_nor"])
cloud, info = capi.Cloud.fused(scan, g["scan_inst"], int(g["uidx"]), model, g["pose"], refine=False)
assert info["icp_err"] == 0.0
check_row(g, cloud, info)
none, info = capi.Cloud.fused(scan, g["scan_inst"], int(g["absent_uidx"]), model, g["pose"], refine=False)
assert none is None and info["n_extracted"] == 0 and len(info["source"]) == 0 and capi.load().rs_hip_last_error() == b""
none, info = capi.Cloud.fused(scan, g["scan_inst"], int(g["absent_uidx"]), model, g["pose"], refine=True)
assert none is None and info["n_extracted"] == 0
print("ok")
""")


def test_shim_returns_the_merged_arrays():
    run_child(r"""
d = C.CDLL(os.path.join(sys.argv[1], "rescan_amd", "librescan_dropin.so"))
libc = C.CDLL(None); libc.free.argtypes = [C.c_void_p]
f = d.rsd_augment_model; f.restype = C.c_int64
f.argtypes = [C.c_void_p] * 7 + [C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 8
TYPES = dict(pos=(np.float32, 3), nor=(np.float32, 3), col=(np.float32, 3), radii=(np.float32, 1), qual=(np.float32, 1), cls=(np.int32, 1), inst=(np.int32, 1))
def call(g, uidx):
    outs = (C.c_void_p * 7)(); x = np.zeros(16, np.float32)
    n = f(*[g["scan_" + k].ctypes.data for k in KEYS], len(g["scan_pos"]), *[g["model_" + k].ctypes.data for k in KEYS[:6]], len(g["model_pos"]),
          np.ascontiguousarray(g["pose"]).ctypes.data, int(uidx), int(g["is_static"]), *[C.addressof(outs) + 8 * k for k in range(7)], x.ctypes.data)
    arrays = {}
    for k, key in enumerate(KEYS):
        if outs[k]:
            t, w = TYPES[key]
            a = np.ctypeslib.as_array(C.cast(outs[k], C.POINTER(C.c_float if t == np.float32 else C.c_int32)), shape=(n * w,)).copy()
            arrays[key] = a.reshape(n, 3) if w == 3 else a
            libc.free(outs[k])
    return n, x, arrays
for name in ("chair", "wall"):
    g = golden(name)
    n, x, arrays = call(g, g["uidx"])
    assert n == len(g["merged_pos"]) and R.same_bits(x, g["xform"])
    for key in KEYS:
        assert R.same_bits(arrays[key], g["merged_" + key]), (name, key)
n, x, arrays = call(g, g["absent_uidx"])
assert n == 0 and not arrays
print("ok")
""")
