"""GPU: the whole arrangement in one call — rs_hip_shuffle_permutations, rs_hip_merge_shuffled_multi, rs_hip_cloud_fuse_arrangement and
rsd_augment_models — against the reference's recorded loop (tests/golden/fuse_arrangement.npz), against the single-placement calls
they replace, and, where no recording exists, against the host plan and the restatement (tests/fuse_restate.py).  Comparisons are
integer equality or uint32 bit equality (NaN payloads apart, as in tests/test_gpu_hard_fuse.py); the one pose above the reference-order
ICP's 16 384 points is held to the project's 1e-4 bar.  The GPU work runs in child processes, each under its own time limit; nothing
here provokes a fault: every bad input is refused on the host."""
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PRELUDE = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from rescan_amd import capi, synth
import fuse_restate as R
import hard_fuse as H
capi.init(0)
F = np.float32
KEYS = ("pos", "nor", "col", "radii", "qual", "cls", "inst")
def golden(name): return dict(np.load(os.path.join(sys.argv[1], "tests", "golden", f"fuse_{name}.npz")))
def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    nan = np.isnan(a)
    return a.shape == b.shape and bool((nan == np.isnan(b)).all()) and bool((R.bits(a)[~nan] == R.bits(b)[~nan]).all())
def arrangement(g):
    # the fixture's placements for Cloud.fuse_arrangement, and the scan
    scan = capi.Cloud(g["scan_pos"], g["scan_nor"])
    pls = []
    for p in range(len(g["uidx"])):
        frm = int(g["model_from"][p])
        pls.append(dict(uidx=int(g["uidx"][p]), pose=g["poses"][p], refine=not int(g["is_static"][p]), model_from=frm,
                        model=capi.Cloud(g[f"p{p}_model_pos"], g[f"p{p}_model_nor"]) if frm < 0 else None))
    return scan, pls
def as_one(g):
    # fuse_chair / fuse_wall as an arrangement of one
    return dict(uidx=int(g["uidx"]), pose=g["pose"], refine=not int(g["is_static"]), model=capi.Cloud(g["model_pos"], g["model_nor"]))
def same_result(a, b):
    (ca, ia), (cb, ib) = a, b
    assert (ca is None) == (cb is None) and ia["n_extracted"] == ib["n_extracted"]
    assert (ia["scan_index"] == ib["scan_index"]).all() and ia["source"].shape == ib["source"].shape and (ia["source"] == ib["source"]).all()
    if ca is None: return
    assert R.same_bits(ia["xform"], ib["xform"]) and F(ia["icp_err"]).view(np.uint32) == F(ib["icp_err"]).view(np.uint32)
    assert ca.n == cb.n and R.same_bits(ca._pos, cb._pos) and R.same_bits(ca._nor, cb._nor)
"""


def run_child(body, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


def test_segmented_permutation_equals_the_host_plan_slice_by_slice():
    run_child(r"""
BASE = (1, 1, 2, 1, 3, 63, 64, 65, 1, 255, 256, 257, 2, 4097)
rng = np.random.default_rng(5)
ORDERS = [BASE,                                                      # a size-1 placement first
          BASE[::-1],                                                # ... and last
          (4097, 1, 257, 256, 1, 65, 1, 64, 63, 3, 2, 255, 2, 1),    # ... and between the two large ones
          tuple(rng.permutation(BASE).tolist()),
          (64, 192, 256, 1, 511, 64),                                # offsets exactly on 64, 256, 512, 513, 1024
          (5, 0, 1, 0, 0, 7, 0),                                     # empty placements, also first in line and last
          (0, 1), (1,), (0,), (2,), (4097,), ()]
plans = {}
def plan(n, seed):
    if (n, seed) not in plans: plans[(n, seed)] = capi.shuffle_plan(n, seed)
    return plans[(n, seed)]
def check(sizes, seed):
    got = capi.shuffle_permutations(sizes, seed)
    assert got.dtype == np.int32 and got.shape == (sum(sizes),), sizes
    at = 0
    for p, n in enumerate(sizes):
        assert (got[at:at + n] == plan(n, seed)).all(), (sizes, seed, p, n, np.flatnonzero(got[at:at + n] != plan(n, seed))[:5])
        at += n
    return got
for seed in (12346, 977):
    for sizes in ORDERS:
        check(sizes, seed)
# P = 1 is the single call's permutation
for n in (1, 2, 65, 4097):
    assert (capi.shuffle_permutations([n]) == capi.shuffle_permutation(n)).all(), n
# a short list after a long one (the workspace keeps its larger buffers), and the same call twice
long = check((70001, 1, 30000), 12346)
check((1, 3, 1), 12346); check((2,), 977)
assert capi.shuffle_permutations((70001, 1, 30000)).tobytes() == long.tobytes()
print("ok")
""")


def test_segmented_merge_keeps_every_placement_to_its_own_transform():
    run_child(r"""
g = golden("hostile")
pts, X = H.points(), H.transforms()
E = np.zeros((0, 3), F)
a_pos, a_nor, b_pos, b_nor = pts["a_pos"], pts["a_nor"], pts["b_pos"], pts["b_nor"]
# (name of the transform, A, B): the hostile transforms side by side, boundaries inside a wave (1, 17, 30 ...), n_a = 0 and n_b = 0
parts = [("identity", (a_pos, a_nor), (b_pos, b_nor)), ("negzero", (a_pos, a_nor), (b_pos, b_nor)), ("tiny", (a_pos[:1], a_nor[:1]), (E, E)),
         ("inf_nan", (a_pos, a_nor), (b_pos, b_nor)), ("huge", (E, E), (b_pos[:17], b_nor[:17])), ("tiny", (a_pos, a_nor), (b_pos, b_nor)),
         ("rotation", (a_pos[:30], a_nor[:30]), (b_pos[:3], b_nor[:3])), ("inf_nan", (a_pos[:65], a_nor[:65]), (E, E)),
         ("negzero", (E, E), (E, E)), ("translation", (a_pos[:2], a_nor[:2]), (b_pos[:1], b_nor[:1])), ("identity", (E, E), (b_pos, b_nor)),
         ("huge", (a_pos, a_nor), (b_pos, b_nor))]
for seed in (12346, 977):
    got = capi.merge_shuffled_multi([(a[0], a[1], X[name], b[0], b[1]) for name, a, b in parts], seed)
    assert len(got) == len(parts)
    for k, (name, a, b) in enumerate(parts):
        one = capi.merge_shuffled(a[0], a[1], X[name], b[0], b[1], seed)
        want = R.merge(a[0], a[1], X[name], b[0], b[1], seed)
        assert (got[k][2] == one[2]).all() and (got[k][2] == want[2]).all(), (k, name, "source")
        for what, x, y, z in (("positions", got[k][0], one[0], want[0]), ("normals", got[k][1], one[1], want[1])):
            assert same(x, y), (k, name, seed, what, "the single call")
            assert same(x, z), (k, name, seed, what, "the restatement")
        if len(a[0]) == H.N_A and len(b[0]) == H.N_B:                # the reference's own transform of A; B as it is
            assert same(got[k][0], np.concatenate([g[f"{name}_pos"], b[0]])[want[2]]), (k, name, "recorded positions")
            assert same(got[k][1], np.concatenate([g[f"{name}_nor"], b[1]])[want[2]]), (k, name, "recorded normals")
# the neighbours differ: a lane that read the transform next door would show
ident, negz = got[0], got[1]
assert not same(ident[0], negz[0])
assert capi.merge_shuffled_multi([]) == []
print("ok")
""")


def test_whole_call_against_the_reference_loop():
    run_child(r"""
g = golden("arrangement")
scan, pls = arrangement(g)
res = capi.Cloud.fuse_arrangement(scan, g["scan_inst"], pls, max_dist=float(g["max_dist"]), max_angle=float(g["max_angle"]))
assert len(res) == 5
shapes = []
for p, (cloud, info) in enumerate(res):
    uidx, frm = int(g["uidx"][p]), int(g["model_from"][p])
    model = shapes[frm] if frm >= 0 else {k: g[f"p{p}_model_{k}"] for k in KEYS}
    assert info["n_extracted"] == int(g["n_extracted"][p]), p
    if p == 2:                                                     # a uidx no scan point carries
        assert cloud is None and info["n_extracted"] == 0 and len(info["source"]) == 0 and len(info["scan_index"]) == 0
        shapes.append(model)
        continue
    assert (info["scan_index"] == R.select(g["scan_inst"], [uidx])).all(), p
    assert R.same_bits(info["xform"], g[f"p{p}_xform"]), (p, info["xform"], g[f"p{p}_xform"])
    assert F(info["icp_err"]).view(np.uint32) == g[f"p{p}_icp_err"].view(np.uint32), (p, info["icp_err"], g[f"p{p}_icp_err"])
    assert cloud.n == len(g[f"p{p}_merged_pos"]) and (info["source"] == R.plan(cloud.n)).all(), p
    assert R.same_bits(cloud._pos, g[f"p{p}_merged_pos"]) and R.same_bits(cloud._nor, g[f"p{p}_merged_nor"]), p
    names = ("col", "radii", "qual", "cls")
    ext = capi.gather_attributes(info["scan_index"], [g["scan_" + k] for k in names])
    merged = dict(zip(names, capi.gather_attributes(info["source"], [np.concatenate([e, model[k]]) for e, k in zip(ext, names)])))
    merged["inst"] = np.full(cloud.n, uidx, np.int32)
    for k in names + ("inst",):
        assert R.same_bits(merged[k], g[f"p{p}_merged_{k}"]), (p, k)
    shapes.append(merged)
# the dependent placement merged the chair's MERGED cloud: with the chair's own model it would be smaller
assert res[4][0].n == res[4][1]["n_extracted"] + res[0][0].n != res[4][1]["n_extracted"] + pls[0]["model"].n
# the same call again gives the same bytes
again = capi.Cloud.fuse_arrangement(scan, g["scan_inst"], pls, max_dist=float(g["max_dist"]), max_angle=float(g["max_angle"]))
for a, b in zip(res, again): same_result(a, b)
print("ok")
""")


def test_whole_call_against_the_single_call():
    run_child(r"""
g = golden("arrangement")
scan, pls = arrangement(g)
kw = dict(max_dist=float(g["max_dist"]), max_angle=float(g["max_angle"]))
res = capi.Cloud.fuse_arrangement(scan, g["scan_inst"], pls, **kw)
shapes = []
for p, pl in enumerate(pls):
    model = pl["model"] if pl["model_from"] < 0 else shapes[pl["model_from"]]          # the earlier result, fed as the model
    one = capi.Cloud.fused(scan, g["scan_inst"], pl["uidx"], model, pl["pose"], refine=pl["refine"], **kw)
    same_result(res[p], one)
    shapes.append(one[0] if one[0] is not None else model)
# a chain through a placement that extracted nothing, and the same object placed twice: 0 <- 1 (absent uidx) <- 2, 0 <- 3
chair = pls[0]
chain = [chair, dict(uidx=99, pose=g["poses"][2], model_from=0), dict(uidx=int(g["uidx"][3]), pose=g["poses"][3], model_from=1),
         dict(uidx=chair["uidx"], pose=g["poses"][4], model_from=0, refine=False)]
res = capi.Cloud.fuse_arrangement(scan, g["scan_inst"], chain, **kw)
assert res[1][0] is None and res[1][1]["n_extracted"] == 0
first = capi.Cloud.fused(scan, g["scan_inst"], chair["uidx"], chair["model"], chair["pose"], **kw)
same_result(res[0], first)
same_result(res[2], capi.Cloud.fused(scan, g["scan_inst"], chain[2]["uidx"], first[0], chain[2]["pose"], **kw))
same_result(res[3], capi.Cloud.fused(scan, g["scan_inst"], chair["uidx"], first[0], chain[3]["pose"], refine=False, **kw))
# the single-placement fixtures as arrangements of one
for name in ("chair", "wall"):
    f = golden(name)
    s1 = capi.Cloud(f["scan_pos"], f["scan_nor"]); one = as_one(f)
    (cloud, info), = capi.Cloud.fuse_arrangement(s1, f["scan_inst"], [one])
    same_result((cloud, info), capi.Cloud.fused(s1, f["scan_inst"], one["uidx"], one["model"], one["pose"], refine=one["refine"]))
    assert R.same_bits(cloud._pos, f["merged_pos"]) and R.same_bits(cloud._nor, f["merged_nor"]) and R.same_bits(info["xform"], f["xform"]), name
    if name == "wall":
        (none, info), = capi.Cloud.fuse_arrangement(s1, f["scan_inst"], [dict(one, uidx=int(f["absent_uidx"]))])
        assert none is None and info["n_extracted"] == 0
assert capi.Cloud.fuse_arrangement(scan, g["scan_inst"], []) == []
print("ok")
""")


def test_a_placement_above_the_reference_order_icp():
    """About 20 k extracted points: beyond 16 384 the library's ICP is within 1e-4 of the reference-order pose, not bit-identical to
    it, so xform is held to that bar against the single call and the merged arrays to the merge under the xform returned."""
    run_child(r"""
s = synth.make_scene(seed=29, width=2.4, depth=2.4, height=0.6, density=15500.0, objects=("chair",))
o = s["objects"][0]
ids = s["instance_idx"]
n_ext = int((ids == o["uidx"]).sum())
assert 17000 <= n_ext <= 30000, n_ext
scan = capi.Cloud(s["points"], s["normals"]); model = capi.Cloud(o["pos"], o["nor"])
pose = synth.perturbed_pose(o["pose"], np.random.default_rng(3))
wall = dict(uidx=1, pose=np.eye(4, dtype=F).ravel(), refine=False, model=model)       # a static neighbour in the same round
res = capi.Cloud.fuse_arrangement(scan, ids, [wall, dict(uidx=o["uidx"], pose=pose, model=model)])
cloud, info = res[1]
one, info1 = capi.Cloud.fused(scan, ids, o["uidx"], model, pose)
assert info["n_extracted"] == n_ext == info1["n_extracted"] and (info["scan_index"] == info1["scan_index"]).all()
d = float(np.linalg.norm(info["xform"].astype(np.float64) - info1["xform"].astype(np.float64)))
print("xform against the single call, Frobenius:", d)
assert d < 1e-4, d
idx = info["scan_index"]
want = R.merge(s["points"][idx], s["normals"][idx], info["xform"], o["pos"], o["nor"])
assert (info["source"] == want[2]).all() and R.same_bits(cloud._pos, want[0]) and R.same_bits(cloud._nor, want[1])
same_result(res[0], capi.Cloud.fused(scan, ids, 1, model, wall["pose"], refine=False))
print("ok")
""")


def test_more_instances_than_the_split_takes_are_refused():
    run_child(r"""
n = 4097
rng = np.random.default_rng(1)
pos = rng.uniform(0, 1, (n, 3)).astype(F); nor = np.tile(np.array([0, 1, 0], F), (n, 1))
scan = capi.Cloud(pos, nor); model = capi.Cloud(pos[:50], nor[:50])
try:
    capi.Cloud.fuse_arrangement(scan, np.arange(n, dtype=np.int32), [dict(uidx=5, pose=np.eye(4), model=model)])
    raise SystemExit("not refused")
except capi.RescanHipError as e:
    assert "error -4" in str(e) and "4096" in str(e), e
res = capi.Cloud.fuse_arrangement(scan, np.arange(n, dtype=np.int32) % 4096, [dict(uidx=0, pose=np.eye(4), model=model, refine=False)])
assert res[0][1]["n_extracted"] == 2 and res[0][0].n == 52
# a scan or a model without normals
bare = capi.Cloud(pos[:50])
for sc, md in ((bare, model), (scan, bare)):
    try:
        capi.Cloud.fuse_arrangement(sc, np.zeros(sc.n, np.int32), [dict(uidx=0, pose=np.eye(4), model=md)])
        raise SystemExit("not refused")
    except capi.RescanHipError as e:
        assert "error -2" in str(e) and "normals" in str(e), e
print("ok")
""")


def test_shim_returns_what_the_single_calls_return():
    run_child(r"""
g = golden("arrangement")
d = C.CDLL(os.path.join(sys.argv[1], "rescan_amd", "librescan_dropin.so"))
libc = C.CDLL(None); libc.free.argtypes = [C.c_void_p]
one = d.rsd_augment_model; one.restype = C.c_int64
one.argtypes = [C.c_void_p] * 7 + [C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 8
many = d.rsd_augment_models; many.restype = C.c_int32
many.argtypes = [C.c_void_p] * 7 + [C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_void_p] * 2 + [C.c_void_p] * 3 + [C.c_void_p] * 7 + [C.c_void_p, C.c_void_p]
TYPES = dict(pos=(F, 3), nor=(F, 3), col=(F, 3), radii=(F, 1), qual=(F, 1), cls=(np.int32, 1), inst=(np.int32, 1))
def take(ptrs, n):
    arrays = {}
    for key, ptr in zip(KEYS, ptrs):
        t, w = TYPES[key]
        a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float if t == F else C.c_int32)), shape=(n * w,)).copy()
        arrays[key] = a.reshape(n, 3) if w == 3 else a
        libc.free(ptr)
    return arrays
P = len(g["uidx"])
scan = [g["scan_" + k].ctypes.data for k in KEYS]
frm = np.ascontiguousarray(g["model_from"]); uidx = np.ascontiguousarray(g["uidx"]); static = np.ascontiguousarray(g["is_static"]); poses = np.ascontiguousarray(g["poses"])
models = [(C.c_void_p * P)(*[g[f"p{p}_model_{k}"].ctypes.data if frm[p] < 0 else None for p in range(P)]) for k in KEYS[:6]]
n_model = np.array([len(g[f"p{p}_model_pos"]) if frm[p] < 0 else 0 for p in range(P)], np.int32)
outs = [(C.c_void_p * P)() for _ in range(7)]; out_n = np.full(P, -7, np.int64); xforms = np.zeros((P, 16), F)
rc = many(*scan, len(g["scan_pos"]), P, *[C.addressof(m) for m in models], n_model.ctypes.data, frm.ctypes.data, poses.ctypes.data, uidx.ctypes.data,
          static.ctypes.data, *[C.addressof(o) for o in outs], out_n.ctypes.data, xforms.ctypes.data)
assert rc == 0, rc
shapes = []
for p in range(P):
    model = shapes[frm[p]] if frm[p] >= 0 else {k: g[f"p{p}_model_{k}"] for k in KEYS}
    so = (C.c_void_p * 7)(); x = np.zeros(16, F)
    n = one(*scan, len(g["scan_pos"]), *[model[k].ctypes.data for k in KEYS[:6]], len(model["pos"]), poses[p].ctypes.data, int(uidx[p]), int(static[p]),
            *[C.addressof(so) + 8 * k for k in range(7)], x.ctypes.data)
    assert n == out_n[p], (p, n, out_n[p])
    if n == 0:
        assert p == 2 and all(not o[p] for o in outs)
        shapes.append(model)
        continue
    want = take([so[k] for k in range(7)], n); got = take([o[p] for o in outs], n)
    assert R.same_bits(x, xforms[p]) and R.same_bits(x, g[f"p{p}_xform"]), p
    for k in KEYS:
        assert R.same_bits(got[k], want[k]) and R.same_bits(got[k], g[f"p{p}_merged_{k}"]), (p, k)
    shapes.append(want)
print("ok")
""")
