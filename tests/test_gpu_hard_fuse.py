"""GPU: the fuse row on hostile inputs.  k_fuse_merge under every transform of tests/hard_fuse.py (underflow, overflow, -0, Inf and
NaN) on points with +-0, subnormal, Inf and NaN coordinates, against the reference's recorded rs_pointcloud_transform
(tests/golden/fuse_hostile.npz); the same through Cloud.fused(..., refine=False), the device-cloud route of fuse_load, for the
transforms whose merged cloud stays finite (that route indexes the merged points); the device permutation against the host plan at
every small size, at odd seeds and once at 2^24; the selection with the extreme ids.  Comparisons are integer equality or uint32 bit
equality; where both sides are NaN the payload is not compared (a processor's default NaN carries no information).  That
rs_hip_shuffle_permutation refuses 2^24 + 1 with -4 before any launch is asserted in tests/test_fuse_cpu.py, without a device.
The GPU work runs in child processes, each under its own time limit."""
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PRELUDE = r"""
import os, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from rescan_amd import capi
import fuse_restate as R
import hard_fuse as H
capi.init(0)
F = np.float32
g = dict(np.load(os.path.join(sys.argv[1], "tests", "golden", "fuse_hostile.npz")))
def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    nan = np.isnan(a)
    return a.shape == b.shape and bool((nan == np.isnan(b)).all()) and bool((R.bits(a)[~nan] == R.bits(b)[~nan]).all())
def where_not(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return np.flatnonzero(((R.bits(a) != R.bits(b)) & ~(np.isnan(a) & np.isnan(b))).any(axis=1))[:5]
"""


def run_child(body, *args, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT, *args], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


def test_merge_under_every_hostile_transform():
    run_child(r"""
for tag, pts in (("", H.points()), ("finite_", H.points(finite=True))):
    assert same(pts["a_pos"], g[tag + "a_pos"]) and same(pts["a_nor"], g[tag + "a_nor"])
    plan = R.plan(H.N_A + H.N_B)
    for name, x in H.transforms().items():
        pos, nor, source = capi.merge_shuffled(pts["a_pos"], pts["a_nor"], x, pts["b_pos"], pts["b_nor"])
        assert (source == plan).all(), (tag, name)
        want_pos = np.concatenate([g[f"{tag}{name}_pos"], pts["b_pos"]])[plan]          # the reference's own transform of A; B as it is
        want_nor = np.concatenate([g[f"{tag}{name}_nor"], pts["b_nor"]])[plan]
        assert same(pos, want_pos), (tag, name, "positions", where_not(pos, want_pos))
        assert same(nor, want_nor), (tag, name, "normals", where_not(nor, want_nor))
        w = R.merge(pts["a_pos"], pts["a_nor"], x, pts["b_pos"], pts["b_nor"])
        assert same(pos, w[0]) and same(nor, w[1]) and (source == w[2]).all(), (tag, name, "restatement")
# what would not show otherwise: the zero normals under the -0 matrix come out +0 (without the w * m[12] term they would be -0)
pts = H.points()
pos, nor, source = capi.merge_shuffled(pts["a_pos"], pts["a_nor"], H.transforms()["negzero"], pts["b_pos"], pts["b_nor"])
zero = np.flatnonzero((pts["a_nor"] == 0).all(axis=1) & ~np.signbit(pts["a_nor"]).any(axis=1))
out_at = np.flatnonzero(np.isin(source, zero))
assert len(out_at) >= 1 and (nor[out_at] == 0).all() and not np.signbit(nor[out_at]).any()
# and the subnormal results of the 1e-20 scale are kept
pos, nor, source = capi.merge_shuffled(pts["a_pos"], pts["a_nor"], H.transforms()["tiny"], pts["b_pos"], pts["b_nor"])
from_a = source < H.N_A
assert ((pos[from_a] != 0) & (np.abs(pos[from_a]) < np.finfo(F).tiny)).sum() >= 20
print("ok")
""")


def test_device_cloud_route_under_the_finite_transforms():
    run_child(r"""
pts = H.points(finite=True)
rng = np.random.default_rng(7)
n_other = 300
# the scan: the 257 points that carry the id, in their order, among 300 others
n = H.N_A + n_other
slot = np.sort(rng.choice(n, H.N_A, replace=False))
scan_pos = rng.uniform(-1, 1, (n, 3)).astype(F); scan_nor = np.tile(np.array([0, 1, 0], F), (n, 1)); ids = rng.choice(np.array([0, 1, 2, 9], np.int32), n).astype(np.int32)
scan_pos[slot] = pts["a_pos"]; scan_nor[slot] = pts["a_nor"]; ids[slot] = 7
scan = capi.Cloud(scan_pos, scan_nor); model = capi.Cloud(pts["b_pos"], pts["b_nor"])
for name in H.FINITE:
    pose = H.transforms()[name]
    cloud, info = capi.Cloud.fused(scan, ids, 7, model, pose, refine=False)
    assert info["n_extracted"] == H.N_A and (info["scan_index"] == slot).all() and info["icp_err"] == 0.0, name
    assert R.same_bits(info["xform"], capi.mat4_inverse(pose)), name
    want = R.merge(pts["a_pos"], pts["a_nor"], info["xform"], pts["b_pos"], pts["b_nor"])
    assert (info["source"] == want[2]).all(), name
    assert same(cloud._pos, want[0]), (name, "positions", where_not(cloud._pos, want[0]))
    assert same(cloud._nor, want[1]), (name, "normals", where_not(cloud._nor, want[1]))
    if name == "identity":                                # inverse( identity ) is the identity: the reference's own arrays
        assert R.same_bits(info["xform"], pose)
        assert same(cloud._pos, np.concatenate([g["finite_identity_pos"], pts["b_pos"]])[want[2]])
        assert same(cloud._nor, np.concatenate([g["finite_identity_nor"], pts["b_nor"]])[want[2]])
    # the same transform through the host-array route
    got = capi.merge_shuffled(pts["a_pos"], pts["a_nor"], info["xform"], pts["b_pos"], pts["b_nor"])
    assert same(got[0], cloud._pos) and same(got[1], cloud._nor), name
    cloud.close()
print("ok")
""")


def test_permutation_equals_the_host_plan_at_every_small_size():
    run_child(r"""
for seed in range(16):
    for n in range(131):
        got, want = capi.shuffle_permutation(n, seed), capi.shuffle_plan(n, seed)
        assert got.shape == want.shape == (n,) and (got == want).all(), (n, seed, np.flatnonzero(got != want)[:5])
for seed in (0, 1, 0x7fffffff, 0xffffffff):
    for n in (4097, 65537):
        got, want = capi.shuffle_permutation(n, seed), capi.shuffle_plan(n, seed)
        assert (got == want).all() and (np.sort(got) == np.arange(n)).all(), (n, seed, np.flatnonzero(got != want)[:5])
assert (capi.shuffle_plan(130, 3) == R.plan(130, 3)).all() and (capi.shuffle_plan(4097, 0xffffffff) == R.plan(4097, 0xffffffff)).all()
print("ok")
""")


def test_permutation_at_two_to_the_24():
    """n = 2^24 is the largest size the library takes and the one where (float)i stops being exact.  One measured run on an MI355X:
    host plan 0.11 s, device permutation with its download 0.05 s, the whole test 0.5 s (profiles/r19/gpu_tests.txt); the limit of
    30 s leaves room for a cold start of the child and a slower host."""
    out = run_child(r"""
n = 1 << 24
t0 = time.time(); want = capi.shuffle_plan(n); t1 = time.time(); got = capi.shuffle_permutation(n); t2 = time.time()
assert got.shape == want.shape == (n,)
bad = np.flatnonzero(got != want)
assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
print(f"host plan {t1 - t0:.2f} s, device permutation {t2 - t1:.2f} s")
print("ok")
""", limit=30)
    print(out)


def test_select_with_the_extreme_ids():
    run_child(r"""
EXTREME = np.array([-2147483648, -1, 0, 2147483647], np.int32)
near = np.array([-2147483647, -2, 1, 2147483646, 5], np.int32)
rng = np.random.default_rng(3)
for n in (1, 64, 65, 257, 2049):
    pts = rng.choice(np.concatenate([EXTREME, near]), n).astype(np.int32)
    for ids in (EXTREME, EXTREME[::-1], EXTREME[:1], EXTREME[3:], np.concatenate([EXTREME, near[:2]])):
        got, want = capi.select_by_ids(pts, ids), R.select(pts, ids)
        assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), (n, ids.tolist())
        assert (want == np.flatnonzero(np.isin(pts, ids))).all()
print("ok")
""")
