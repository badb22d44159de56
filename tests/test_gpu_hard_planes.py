"""GPU: the plane kernels on the hostile inputs of tests/hard_planes.py.  rs_hip_plane_votes on every vote family in both kernel forms,
with and without `valid`, under three masks; rs_hip_detect_planes on the probe room and on every tie cloud, whole trace; the gather
and the relabel on the normal-dot band, the quad edges and the label corner cases at five cloud sizes; the shim's three plane calls.
Every expectation is the reference's recording (tests/golden/planes_hostile.npz) where one exists, otherwise the restatement
(tests/planes_restate.py) that tests/test_hard_planes_cpu.py pins to those recordings.  Every comparison is exact.  After each
vote family the counts are also compared with what the other orders of evaluation would give (hard_planes.variant_votes): a failure
there names the arithmetic the kernel took.  The GPU work runs in child processes, each under its own time limit; nothing here
provokes a fault: the inputs are hostile to the arithmetic, not to the addressing."""
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
import hard_planes as H
capi.init(0)
F = np.float32
g = dict(np.load(os.path.join(sys.argv[1], "tests", "golden", "planes_hostile.npz")))
def recorded(prefix):
    # the fixture's detection in the shape of R.detect's result (counts 0 where the up test failed, as the kernel leaves them)
    rounds = []
    for r in range(int(g[prefix + "n_rounds"])):
        b = {k: g[f"{prefix}r{r}_{k}"] for k in ("idx", "valid", "counts", "best", "mask_before", "mask_after")}
        b["counts"] = np.where(b["valid"] != 0, b["counts"], 0); b["best"] = int(b["best"])
        rounds.append(b)
    return dict(centers=g[prefix + "centers"], normals=g[prefix + "normals"], n_inliers=g[prefix + "n_inliers"], n_floors=int(g[prefix + "n_floors"]),
                n_walls=int(g[prefix + "n_walls"]), rounds=rounds)
def check_detection(got, want, what):
    assert R.same_bits(got["centers"], want["centers"]) and R.same_bits(got["normals"], want["normals"]), what
    assert (got["n_inliers"] == want["n_inliers"]).all() and got["n_floors"] == want["n_floors"] and got["n_walls"] == want["n_walls"], what
    t = got["trace"]
    assert t["n_rounds"] == len(want["rounds"]), (what, t["n_rounds"])
    for k, b in enumerate(want["rounds"]):
        h = len(b["idx"])
        assert t["n_iters"][k] == h and (t["idx"][k, :h] == b["idx"]).all() and (t["valid"][k, :h] == b["valid"]).all(), (what, k)
        bad = np.flatnonzero(t["counts"][k, :h] != b["counts"])
        assert len(bad) == 0, (what, k, "counts", bad[:5], t["counts"][k, bad[:5]], b["counts"][bad[:5]])
        assert t["best"][k] == b["best"], (what, k, "best", int(t["best"][k]), b["best"])
        assert (t["mask_before"][k] == b["mask_before"]).all(), (what, k, "mask_before")
        bad = np.flatnonzero(t["mask_after"][k] != b["mask_after"])
        assert len(bad) == 0, (what, k, "mask_after", bad[:5])
def both_forms(f):
    for form in (0, 1):
        capi.plane_votes_form(form)
        f(form)
    assert capi.plane_votes_form(0) == 1
"""


def run_child(body, *args, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT, *args], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


@pytest.mark.parametrize("family", ("band", "band_3m", "far", "exact", "special"))
def test_votes_on_the_family(family):
    run_child(r"""
OTHERS = dict(band=("fma", "pre", "other"), band_3m=("fma", "pre", "other"), far=("pre",), exact=(), special=())[sys.argv[2]]
for c in H.VOTE_FAMILIES[sys.argv[2]]():
    name, thr = c["name"], c["dist_threshold"]
    assert c["pos"].shape == (2 * 1024 + 1, 3) and c["center"].shape == (257, 3)
    masks = H.vote_masks(c)
    want = {m: R.votes(c["pos"], mask, c["center"], c["normal"], thr) for m, mask in masks.items()}
    if name == "exact":                                  # the one expectation that does not come from the restatement
        want = {m: (c["inlier"] & mask.astype(bool)[None]).sum(axis=1).astype(np.int32) for m, mask in masks.items()}
    t = H.trimmed(c)
    def run(form):
        for m, mask in H.vote_masks(t).items():          # the reference's own counts on the recorded subset
            got = capi.plane_votes(t["pos"], mask, t["center"], t["normal"], thr)
            bad = np.flatnonzero(got != g[f"votes_{name}_counts_{m}"])
            assert len(bad) == 0, (name, form, m, "recorded", bad[:5], got[bad[:5]], g[f"votes_{name}_counts_{m}"][bad[:5]])
        for m, mask in masks.items():
            got = capi.plane_votes(c["pos"], mask, c["center"], c["normal"], thr)
            bad = np.flatnonzero(got != want[m])
            assert got.dtype == np.int32 and len(bad) == 0, (name, form, m, bad[:5], got[bad[:5]], want[m][bad[:5]])
            got = capi.plane_votes(c["pos"], mask, c["center"], c["normal"], thr, c["valid"])
            assert (got == np.where(c["valid"] != 0, want[m], 0)).all(), (name, form, m, "valid")
        # which arithmetic: the counts each other order of evaluation would give are not the kernel's
        got = capi.plane_votes(c["pos"], masks["all"], c["center"], c["normal"], thr)
        other = H.variant_votes(c)
        assert (other["plain"] == want["all"]).all()
        for k in OTHERS:
            assert (got != other[k]).any(), f"{name}, form {form}: the kernel's counts are those of the '{k}' arithmetic"
        if name == "special_subnormal":
            assert (got != H.flushed_votes(c)).all(), "the kernel's counts are those of a flush to zero"
    both_forms(run)
    print(name, int(want["all"].max()), flush=True)
print("ok")
""", family)


def test_detect_planes_on_the_probe_room():
    run_child(r"""
want = recorded("room_")
cloud = capi.Cloud(g["room_pos"], g["room_nor"])
def run(form):
    got = cloud.detect_planes(float(g["room_dot_threshold"]), float(g["room_dist_threshold"]), int(g["room_count_threshold"]), trace=True)
    t = got["trace"]
    bad = np.flatnonzero(t["mask_before"][0] != g["room_floor_mask"])
    assert len(bad) == 0, ("floor mask", form, bad[:5], g["room_nor"][bad[:5]])
    bad = np.flatnonzero(t["mask_before"][1] != g["room_wall_mask"])
    assert len(bad) == 0, ("wall mask", form, bad[:5], g["room_nor"][bad[:5]])
    check_detection(got, want, ("room", form))
both_forms(run)
# what the room is for: the probes sit on the masks' edges, and k_plane_remove decided the band points with their own model
probes, band = g["room_probes"], g["room_band"]
assert g["room_floor_mask"][probes].any() and g["room_wall_mask"][probes].any() and not np.isfinite(g["room_nor"][probes]).all()
removed = (want["rounds"][1]["mask_before"] == 1) & (want["rounds"][1]["mask_after"] == 0)
assert 40 <= removed[band].sum() <= len(band) - 40
print("ok")
""")


@pytest.mark.parametrize("name", ("t3", "t4", "t5_late", "t5_last"))
def test_detect_planes_on_the_tie_cloud(name):
    run_child(r"""
c = H.tie_clouds((sys.argv[2],))[0]
want = R.detect(c["pos"], c["nor"], 0.8, 0.033, c["count_threshold"])
if c["name"] == "t3":                                    # the reference's own detection of this one
    assert R.same_bits(c["pos"], g["tie_pos"]) and R.same_bits(c["nor"], g["tie_nor"])
    rec = recorded("tie_")
    assert len(rec["rounds"]) == len(want["rounds"]) and all((a["counts"] == b["counts"]).all() and a["best"] == b["best"] for a, b in zip(rec["rounds"], want["rounds"]))
    want = rec
cloud = capi.Cloud(c["pos"], c["nor"])
def run(form):
    got = cloud.detect_planes(0.8, 0.033, c["count_threshold"], trace=True)
    t = got["trace"]
    for k, b in enumerate(want["rounds"]):               # best and its count first: what the tie clouds are for
        assert t["best"][k] == b["best"], (c["name"], form, k, int(t["best"][k]), b["best"])
        if b["best"] >= 0:
            assert t["counts"][k, b["best"]] == b["counts"][b["best"]] == b["counts"].max(), (c["name"], form, k)
    check_detection(got, want, (c["name"], form))
both_forms(run)
if c["first"] is not None:
    assert want["rounds"][1]["best"] == c["first"]["index"] >= 256
print("ok")
""", name)


@pytest.mark.parametrize("family", ("dot_band", "quad_edges", "labels"))
def test_gather_and_relabel_on_the_family(family):
    run_child(r"""
name = sys.argv[2]
def lists_equal(got, want, what):
    assert len(got) == len(want), what
    for m, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.int32 and a.shape == b.shape and (a == b).all(), (what, m, len(a), len(b))
changed = 0
for n, order in ((1, None), (64, None), (65, None), (257, None), (257, "reverse"), (2049, None)):
    c = H.GATHER_FAMILIES[name](n, order=order); M = c["models"]
    cloud = capi.Cloud(c["pos"], c["nor"])
    for dot, dist, cv, ce in H.GATHER_PARAMS:
        got = capi.gather_plane_inliers(cloud, M["center"], M["normal"], M["axes"], M["extends"], M["valid"], dot, dist, cv, ce)
        want = R.gather(c["pos"], c["nor"], M["center"], M["normal"], M["axes"], M["extends"], M["valid"], dot, dist, cv, ce)
        lists_equal(got, want, (name, n, order, dot, dist, cv, ce))
        if n == 257 and order is None and (dot, dist, ce) in ((0.8, 0.05, False), (0.0, 0.05, True)):          # the reference's own lists
            p = f"gather_{name}_" + ("checked" if ce else "plain")
            o = g[p + "_offsets"]
            lists_equal(got, [g[p + "_index"][o[m]:o[m + 1]] for m in range(len(o) - 1)], (name, "recorded", ce))
    got = capi.relabel_walls_and_floors(cloud, M["center"], M["normal"], M["axes"], M["extends"], M["valid"], M["up_dot"], *c["ids"], c["cls"], c["inst"])
    want = R.relabel(c["pos"], c["nor"], M["center"], M["normal"], M["axes"], M["extends"], M["valid"], M["up_dot"], *c["ids"], c["cls"], c["inst"])
    if n == 257 and order is None:
        assert (c["cls"] == g[f"gather_{name}_class_before"]).all() and (c["inst"] == g[f"gather_{name}_instance_before"]).all()
        want = (g[f"gather_{name}_class_after"], g[f"gather_{name}_instance_after"])
    bad = np.flatnonzero((got[0] != want[0]) | (got[1] != want[1]))
    assert len(bad) == 0, (name, n, order, "relabel", bad[:5], c["nor"][bad[:5]])
    changed += int((got[0] != c["cls"]).sum() + (got[1] != c["inst"]).sum())
    cloud.close()
assert changed > 100
print("ok")
""", family)


def test_shim_plane_calls_on_hostile_cases():
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
# the detection of the tie cloud
c = np.zeros((64, 3), F); nn = np.zeros((64, 3), F); k = np.zeros(64, np.int64); nf, nw = i32(), i32()
pos, nor = np.ascontiguousarray(g["tie_pos"]), np.ascontiguousarray(g["tie_nor"])
m = d.rsd_detect_floor_and_walls(pos.ctypes.data, nor.ctypes.data, len(pos), float(g["tie_dot_threshold"]), float(g["tie_dist_threshold"]),
                                 int(g["tie_count_threshold"]), 64, c.ctypes.data, nn.ctypes.data, k.ctypes.data, C.addressof(nf), C.addressof(nw))
assert m == len(g["tie_centers"]) >= 2 and R.same_bits(c[:m], g["tie_centers"]) and R.same_bits(nn[:m], g["tie_normals"]) and (k[:m] == g["tie_n_inliers"]).all()
assert nf.value == int(g["tie_n_floors"]) and nw.value == int(g["tie_n_walls"])
# the checked gather of the quad edges
p = "gather_quad_edges_"
M = {key: np.ascontiguousarray(g[p + "model_" + key]) for key in ("center", "normal", "axes", "extends", "valid", "up_dot")}
pos, nor = np.ascontiguousarray(g[p + "pos"]), np.ascontiguousarray(g[p + "nor"])
nm = len(M["center"])
index = vp(); offsets = np.zeros(nm + 1, np.int64)
total = d.rsd_gather_model_inliers(pos.ctypes.data, nor.ctypes.data, len(pos), M["center"].ctypes.data, M["normal"].ctypes.data, M["axes"].ctypes.data,
                                   M["extends"].ctypes.data, M["valid"].ctypes.data, nm, 0.0, 0.05, 1, 1, C.addressof(index), offsets.ctypes.data)
assert total == len(g[p + "checked_index"]) > 0 and (offsets == g[p + "checked_offsets"]).all()
got = np.ctypeslib.as_array(C.cast(index, C.POINTER(C.c_int32)), shape=(total,)).copy(); libc.free(index)
assert (got == g[p + "checked_index"]).all()
# the relabel of the label corner cases
p = "gather_labels_"
M = {key: np.ascontiguousarray(g[p + "model_" + key]) for key in ("center", "normal", "axes", "extends", "valid", "up_dot")}
pos, nor = np.ascontiguousarray(g[p + "pos"]), np.ascontiguousarray(g[p + "nor"])
cls, inst = g[p + "class_before"].copy(), g[p + "instance_before"].copy()
rc = d.rsd_relabel_walls_and_floors(pos.ctypes.data, nor.ctypes.data, len(pos), M["center"].ctypes.data, M["normal"].ctypes.data, M["axes"].ctypes.data,
                                    M["extends"].ctypes.data, M["valid"].ctypes.data, M["up_dot"].ctypes.data, len(M["center"]), *H.IDS, cls.ctypes.data, inst.ctypes.data)
assert rc == 0 and (cls == g[p + "class_after"]).all() and (inst == g[p + "instance_after"]).all() and (cls != g[p + "class_before"]).any()
print("ok")
""")
