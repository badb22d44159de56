"""GPU: rs_hip_plane_votes, rs_hip_detect_planes, rs_hip_gather_plane_inliers, rs_hip_relabel_walls_and_floors and the three rsd_*
plane calls against the reference's fixtures (tests/golden/planes_*.npz) and, where no recording exists, against the restatement
that reproduces them (tests/planes_restate.py, checked in tests/test_planes_cpu.py).  Every comparison is exact.
The GPU work runs in child processes, each under its own time limit; nothing here provokes a fault: every refusal is decided on the
host before a launch."""
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
import planes_restate as R
capi.init(0)
F = np.float32
TILE = 1024                                              # PLANE_TILE of rs_planes.hip
def golden(name): return dict(np.load(os.path.join(sys.argv[1], "tests", "golden", f"planes_{name}.npz")))
def rounds_of(g, prefix):
    return [{k: g[f"{prefix}r{r}_{k}"] for k in ("idx", "normal", "valid", "counts", "best", "mask_before", "mask_after") if f"{prefix}r{r}_{k}" in g}
            for r in range(int(g[prefix + "n_rounds"]))]
def refused(code, what, f, *a, **k):
    try:
        f(*a, **k)
    except capi.RescanHipError as e:
        assert f"error {code}:" in str(e) and what in str(e), str(e)
        return True
    return False
def scene(n, seed):
    # n points of three slabs (a floor and two walls, 2 cm thick) and clutter, so that counts spread from 0 to about n / 3
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, 1, (n, 3)); k = np.arange(n) % 4
    pos[k == 0, 1] *= 0.02; pos[k == 1, 0] *= 0.02; pos[k == 2, 2] *= 0.02
    return pos.astype(F)
def hyps(pos, h, seed):
    # h hypotheses from triples of pos; every 7th triple repeats a point (NaN), every 5th fails a made-up up test
    rng = np.random.default_rng(seed)
    n = len(pos)
    if n == 0:
        c = rng.uniform(0, 1, (h, 3)).astype(F); nn = rng.normal(0, 1, (h, 3)); nn = (nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(F)
    else:
        idx = rng.integers(0, n, (h, 3)).astype(np.int32); idx[::7, 2] = idx[::7, 0]
        c, nn = R.hypotheses(pos, idx)
    valid = (np.arange(h) % 5 != 3).astype(np.uint8)
    return c, nn, valid
def check_votes(n, h, seed, mask=None, dist=0.01):
    pos = scene(n, seed); mask = np.ones(n, np.uint8) if mask is None else mask
    c, nn, valid = hyps(pos, h, seed + 1)
    want = R.votes(pos, mask, c, nn, dist)
    got = capi.plane_votes(pos, mask, c, nn, dist)
    assert got.dtype == np.int32 and got.shape == (h,) and (got == want).all(), (n, h, np.flatnonzero(got != want)[:5])
    got = capi.plane_votes(pos, mask, c, nn, dist, valid)
    assert (got == np.where(valid != 0, want, 0)).all(), (n, h, "valid")
    if n:
        assert (np.isnan(nn).any(axis=1) & (want == 0)).sum() >= (h + 6) // 7 and (n < 63 or h < 63 or want.max() > 0)
    return pos, mask, c, nn, want
N_CANDS = (0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 70001)
"""


def run_child(body, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


def test_votes_equal_the_recorded_counts_of_every_round():
    run_child(r"""
g = golden("room")
pos = g["pos"]
for form in (0, 1):
    capi.plane_votes_form(form)
    for k, b in enumerate(rounds_of(g, "")):
        c = pos[b["idx"][:, 0]]
        got = capi.plane_votes(pos, b["mask_before"], c, b["normal"], g["dist_threshold"])
        assert (got == b["counts"]).all(), (form, k, np.flatnonzero(got != b["counts"])[:5])
        got = capi.plane_votes(pos, b["mask_before"], c, b["normal"], g["dist_threshold"], b["valid"])
        assert (got == np.where(b["valid"] != 0, b["counts"], 0)).all(), (form, k)
assert capi.plane_votes_form(0) == 1
print("ok")
""")


def test_votes_every_candidate_count_at_257_hypotheses():
    run_child(r"""
for form in (0, 1):
    capi.plane_votes_form(form)
    for n in N_CANDS:
        check_votes(n, 257, 100 + n)
capi.plane_votes_form(0)
# masks: none, alternating, the last point only; the candidates are what the mask keeps
n = 2 * TILE + 1
pos = scene(n, 7); c, nn, valid = hyps(pos, 257, 8)
for what, m in (("none", np.zeros(n, np.uint8)), ("alternating", (np.arange(n) % 2).astype(np.uint8)), ("last", (np.arange(n) == n - 1).astype(np.uint8)),
                ("one tile", (np.arange(n) < TILE).astype(np.uint8))):
    got, want = capi.plane_votes(pos, m, c, nn, 0.01, valid), R.votes(pos, m, c, nn, 0.01, valid)
    assert (got == want).all() and got.max() <= int(m.sum()) and (what in ("none", "last") or got.max() > 0), what
# a small call after a large one (the workspace keeps its larger buffers), and the same call twice
check_votes(70001, 257, 3); check_votes(65, 63, 4)
pos = scene(5000, 5); c, nn, valid = hyps(pos, 2500, 6)
assert capi.plane_votes(pos, np.ones(5000, np.uint8), c, nn, 0.01, valid).tobytes() == capi.plane_votes(pos, np.ones(5000, np.uint8), c, nn, 0.01, valid).tobytes()
print("ok")
""")


def test_votes_every_candidate_count_at_5000_hypotheses():
    run_child(r"""
for n in N_CANDS:
    check_votes(n, 5000, 200 + n)
print("ok")
""")


def test_votes_every_hypothesis_count_at_one_tile_plus_one():
    run_child(r"""
for form in (0, 1):
    capi.plane_votes_form(form)
    for h in (1, 63, 64, 65, 255, 256, 257, 2500, 5000):
        check_votes(TILE + 1, h, 300 + h)
capi.plane_votes_form(0)
assert len(capi.plane_votes(scene(10, 1), np.ones(10, np.uint8), np.zeros((0, 3), F), np.zeros((0, 3), F), 0.01)) == 0
print("ok")
""")


def test_detect_planes_reproduces_the_room_and_its_whole_trace():
    run_child(r"""
g = golden("room")
cloud = capi.Cloud(g["pos"], g["nor"])
got = cloud.detect_planes(float(g["dot_threshold"]), float(g["dist_threshold"]), int(g["count_threshold"]), trace=True)
assert R.same_bits(got["centers"], g["centers"]) and R.same_bits(got["normals"], g["normals"]) and (got["n_inliers"] == g["n_inliers"]).all()
assert got["n_floors"] == int(g["n_floors"]) and got["n_walls"] == int(g["n_walls"])
t, want = got["trace"], rounds_of(g, "")
assert t["n_rounds"] == len(want)
assert (t["mask_before"][0] == g["floor_mask"]).all() and (t["mask_before"][1] == g["wall_mask"]).all()
for k, b in enumerate(want):
    h = len(b["idx"])
    assert t["n_iters"][k] == h and (t["idx"][k, :h] == b["idx"]).all() and (t["valid"][k, :h] == b["valid"]).all(), k
    assert (t["counts"][k, :h] == np.where(b["valid"] != 0, b["counts"], 0)).all() and t["best"][k] == int(b["best"]), k
    assert (t["mask_before"][k] == b["mask_before"]).all() and (t["mask_after"][k] == b["mask_after"]).all(), k
# the reference's call is the default; the same call again gives the same bytes, with the other form of the votes kernel too
capi.plane_votes_form(1)
again = capi.detect_planes(cloud)
capi.plane_votes_form(0)
assert again["centers"].tobytes() == got["centers"].tobytes() and again["normals"].tobytes() == got["normals"].tobytes() and (again["n_inliers"] == got["n_inliers"]).all()
# more models than the caller has room for
assert refused(-4, "capacity", capi.detect_planes, cloud, capacity=2)
print("ok")
""")


def test_detect_planes_keeps_the_quirks_and_refuses_the_empty_pop():
    run_child(r"""
g = golden("quirks")
for p in ("a_", "c_", "d_", "e_"):
    cloud = capi.Cloud(g[p + "pos"], g[p + "nor"])
    got = cloud.detect_planes(float(g[p + "dot_threshold"]), float(g[p + "dist_threshold"]), int(g[p + "count_threshold"]), trace=True)
    assert R.same_bits(got["centers"], g[p + "centers"]) and R.same_bits(got["normals"], g[p + "normals"]) and (got["n_inliers"] == g[p + "n_inliers"]).all(), p
    assert got["n_floors"] == int(g[p + "n_floors"]) and got["n_walls"] == int(g[p + "n_walls"]), p
    t, want = got["trace"], rounds_of(g, p)
    assert t["n_rounds"] == len(want), p
    for k, b in enumerate(want):
        h = len(b["idx"])
        assert (t["idx"][k, :h] == b["idx"]).all() and (t["valid"][k, :h] == b["valid"]).all() and t["best"][k] == int(b["best"]), (p, k)
        assert (t["counts"][k, :h] == np.where(b["valid"] != 0, b["counts"], 0)).all(), (p, k)
        assert (t["mask_before"][k] == b["mask_before"]).all() and (t["mask_after"][k] == b["mask_after"]).all(), (p, k)
# (a): the pop took the floor; (b): nothing to pop
assert int(g["a_n_floors"]) == 1 and len(g["a_centers"]) == 0
cloud = capi.Cloud(g["b_pos"], g["b_nor"])
assert refused(-2, "pop an empty", cloud.detect_planes, float(g["b_dot_threshold"]), float(g["b_dist_threshold"]), int(g["b_count_threshold"]))
# no floor candidate at all, one wall candidate: refused before a hypothesis is drawn
flat = capi.Cloud(g["b_pos"], np.tile(np.array([1, 0, 0], F), (len(g["b_pos"]), 1)))
assert refused(-2, "uninitialised", flat.detect_planes)
nor = np.tile(np.array([0, 1, 0], F), (len(g["b_pos"]), 1)); nor[5] = (1, 0, 0)
assert refused(-2, "never end", capi.Cloud(g["b_pos"], nor).detect_planes)
print("ok")
""")


def test_gather_and_relabel_reproduce_the_fixture_and_the_restatement():
    run_child(r"""
g = golden("gather")
M = {k: g["model_" + k] for k in ("center", "normal", "axes", "extends", "valid", "up_dot")}
clouds = {k: capi.Cloud(g[k + "_pos"], g[k + "_nor"]) for k in ("l0", "l1")}
for name, cl, cv, ce in (("plain", "l0", False, False), ("checked", "l1", True, True)):
    got = capi.gather_plane_inliers(clouds[cl], M["center"], M["normal"], M["axes"], M["extends"], M["valid"], float(g[name + "_dot_threshold"]),
                                    float(g[name + "_dist_threshold"]), cv, ce)
    o = g[name + "_offsets"]
    for m in range(4):
        assert got[m].dtype == np.int32 and (got[m] == g[name + "_index"][o[m]:o[m + 1]]).all(), (name, m)
ids = (int(g["floor_idx"]), int(g["wall_idx"]), int(g["unlabelled_idx"]))
cls, inst = capi.relabel_walls_and_floors(clouds["l1"], M["center"], M["normal"], M["axes"], M["extends"], M["valid"], M["up_dot"], *ids,
                                          g["class_before"], g["instance_before"])
assert (cls == g["class_after"]).all() and (inst == g["instance_after"]).all()
# other sizes and model sets against the restatement: points of the fixture's room, repeated and shifted along the planes
rng = np.random.default_rng(11)
for n in (70001, 257, 65, 64, 1, 0):
    k = np.arange(n) % len(g["l1_pos"])
    pos = (g["l1_pos"][k] + (rng.uniform(-0.02, 0.02, (n, 3)) * [1, 0.2, 1])).astype(F); nor = g["l1_nor"][k]
    cloud = capi.Cloud(pos, nor)
    cls0 = rng.choice(np.array([0, 0, 1, 2, 5], np.int32), n).astype(np.int32); inst0 = rng.choice(np.array([3, 1023, 1024, 2000], np.int32), n).astype(np.int32)
    for what, sel, valid in (("all", slice(0, 4), M["valid"]), ("one", slice(0, 1), M["valid"]), ("none", slice(0, 0), M["valid"]), ("invalid", slice(0, 4), np.zeros(4, np.int8))):
        m = {key: M[key][sel] for key in M}; v = valid[sel]
        for dot, dist, cv, ce in ((0.8, 0.05, False, False), (0.0, 0.05, True, True), (0.8, 0.033, False, True)):
            got = capi.gather_plane_inliers(cloud, m["center"], m["normal"], m["axes"], m["extends"], v, dot, dist, cv, ce)
            want = R.gather(pos, nor, m["center"], m["normal"], m["axes"], m["extends"], v, dot, dist, cv, ce)
            assert len(got) == len(want) and all((a == b).all() and a.shape == b.shape for a, b in zip(got, want)), (n, what, dot, cv, ce)
        got = capi.relabel_walls_and_floors(cloud, m["center"], m["normal"], m["axes"], m["extends"], v, m["up_dot"], *ids, cls0, inst0)
        want = R.relabel(pos, nor, m["center"], m["normal"], m["axes"], m["extends"], v, m["up_dot"], *ids, cls0, inst0)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), (n, what)
        if what == "all" and n >= 257:
            assert (got[0] != cls0).any() and (got[1] != inst0).any()
print("ok")
""")


def test_shim_gives_the_same_arrays_from_host_pointers():
    run_child(r"""
d = C.CDLL(os.path.join(sys.argv[1], "rescan_amd", "librescan_dropin.so"))
libc = C.CDLL(None); libc.free.argtypes = [C.c_void_p]
vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
d.rsd_detect_floor_and_walls.restype = i32
d.rsd_detect_floor_and_walls.argtypes = [vp, vp, i64, f32, f32, i64, i32, vp, vp, vp, vp, vp]
d.rsd_gather_model_inliers.restype = i64
d.rsd_gather_model_inliers.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, i32, f32, f32, i32, i32, vp, vp]
d.rsd_relabel_walls_and_floors.restype = C.c_int
d.rsd_relabel_walls_and_floors.argtypes = [vp, vp, i64] + [vp] * 6 + [i32] * 4 + [vp, vp]
g = golden("room")
c = np.zeros((64, 3), F); nn = np.zeros((64, 3), F); k = np.zeros(64, np.int64); nf, nw = i32(), i32()
m = d.rsd_detect_floor_and_walls(g["pos"].ctypes.data, g["nor"].ctypes.data, len(g["pos"]), 0.8, 0.033, 250, 64, c.ctypes.data, nn.ctypes.data, k.ctypes.data,
                                 C.addressof(nf), C.addressof(nw))
assert m == len(g["centers"]) and R.same_bits(c[:m], g["centers"]) and R.same_bits(nn[:m], g["normals"]) and (k[:m] == g["n_inliers"]).all()
assert nf.value == int(g["n_floors"]) and nw.value == int(g["n_walls"])
q = golden("quirks")
assert d.rsd_detect_floor_and_walls(q["b_pos"].ctypes.data, q["b_nor"].ctypes.data, len(q["b_pos"]), 0.8, 0.033, 250, 64, c.ctypes.data, nn.ctypes.data,
                                    k.ctypes.data, C.addressof(nf), C.addressof(nw)) == -2
g = golden("gather")
M = {key: np.ascontiguousarray(g["model_" + key]) for key in ("center", "normal", "axes", "extends", "valid", "up_dot")}
for name, cl, cv, ce in (("plain", "l0", 0, 0), ("checked", "l1", 1, 1)):
    index = vp(); offsets = np.zeros(5, np.int64)
    total = d.rsd_gather_model_inliers(g[cl + "_pos"].ctypes.data, g[cl + "_nor"].ctypes.data, len(g[cl + "_pos"]), M["center"].ctypes.data, M["normal"].ctypes.data,
                                       M["axes"].ctypes.data, M["extends"].ctypes.data, M["valid"].ctypes.data, 4, float(g[name + "_dot_threshold"]),
                                       float(g[name + "_dist_threshold"]), cv, ce, C.addressof(index), offsets.ctypes.data)
    assert total == len(g[name + "_index"]) and (offsets == g[name + "_offsets"]).all(), name
    got = np.ctypeslib.as_array(C.cast(index, C.POINTER(C.c_int32)), shape=(total,)).copy(); libc.free(index)
    assert (got == g[name + "_index"]).all(), name
cls, inst = g["class_before"].copy(), g["instance_before"].copy()
rc = d.rsd_relabel_walls_and_floors(g["l1_pos"].ctypes.data, g["l1_nor"].ctypes.data, len(g["l1_pos"]), M["center"].ctypes.data, M["normal"].ctypes.data,
                                    M["axes"].ctypes.data, M["extends"].ctypes.data, M["valid"].ctypes.data, M["up_dot"].ctypes.data, 4,
                                    int(g["floor_idx"]), int(g["wall_idx"]), int(g["unlabelled_idx"]), cls.ctypes.data, inst.ctypes.data)
assert rc == 0 and (cls == g["class_after"]).all() and (inst == g["instance_after"]).all()
print("ok")
""")
