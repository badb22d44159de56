"""GPU: what the host runtime shared by the units with entry points of their own (rs_host.h: Buf, ProfSpan, fail) can get wrong and
no other test pins — a workspace buffer that grows between two calls of one thread, the profiling spans a call books, and a unit's
next call after a refusal.  Every comparison is exact: against the project's host-side counterpart of the call (the shim's KnnGrid,
tests/isect_restate.py, tests/resample_restate.py, rs_hip_shuffle_plan, numpy, tests/planes_restate.py) or, for the coverage
extensions, against the same call made first after rs_hip_arrange_release.
Each test runs in one child process under its own time limit, so that the thread's workspaces start empty whatever ran before;
nothing here provokes a fault or a HIP error: every refusal is one of arguments.
The second half does the same for the host units of the C ABI proper: of the five, rs_api.hip holds the runtime state and the other
four (rs_cloud_api.hip, rs_icp_api.hip, rs_score.hip, rs_rows_api.hip: DevBuf, ProfScope) a workspace each: calls of different units
alternate while their buffers grow,
against the committed fixtures with the parity suite's own comparisons (tests/test_gpu_parity.py)."""
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
import isect_restate as I
import planes_restate as P
import resample_restate as R
from test_gpu_knn import DROPIN, _bind, by_name
capi.init(0)
F = np.float32
SMALL, LARGE = 64, 4096                  # Buf grows by 25 % + 256 bytes: a call 64 times larger frees and allocates again
rng = np.random.default_rng(20)

def same(got, want):
    got, want = list(got), list(want)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (k, g.dtype, w.dtype, g.shape, w.shape)

def pose(angle, t):
    # column-major: a rotation about y, then the translation t
    c, s = F(np.cos(angle)), F(np.sin(angle))
    return np.array([c, 0, -s, 0,  0, 1, 0, 0,  s, 0, c, 0,  t[0], t[1], t[2], 1], F)

# ---- k-NN rows: n queries against one grid; the shim's KnnGrid answers on the host ----
knn_pts = rng.uniform(0, 1, (2000, 3)).astype(F)
knn_q = rng.uniform(-0.05, 1.05, (LARGE, 3)).astype(F)
KNN_R, KNN_K = 0.05, 8
knn_cloud = capi.Cloud(knn_pts)
knn_grid = capi.KnnGrid(knn_cloud, KNN_R)
def knn_call(n):
    d, i, nn, tot = capi.knn_search(knn_grid, knn_q[:n], KNN_K)
    return d, i, nn, np.int64(tot)
def knn_want(n):
    os.environ["RS_DROPIN_HOST_QUERIES"] = str(n + 1)
    try:
        d, i, nn, tot = by_name(_bind(C.CDLL(DROPIN)), knn_pts, 3, KNN_R, knn_q[:n], KNN_K)
    finally:
        del os.environ["RS_DROPIN_HOST_QUERIES"]
    past = np.arange(KNN_K)[None, :] >= nn[:, None]              # (the shim leaves a row as it was past its count, capi.knn_search zeroes it)
    d[past] = 0; i[past] = 0
    return d, i, nn, np.int64(tot)

# ---- voxel overlap: n pairs of one shape, 64 distinct pairs repeated; isect_restate answers per distinct pair ----
g = np.linspace(-1, 1, 7)
u, v = (a.ravel() for a in np.meshgrid(g, g))
faces = [np.stack(np.roll([u, v, np.full_like(u, s)], r, axis=0), axis=1) for r in range(3) for s in (-1, 1)]
shell = (np.concatenate(faces) * np.array([0.2, 0.15, 0.25])).astype(F)             # the surface of a 0.4 x 0.3 x 0.5 box
isect_shape = (capi.Cloud(shell), capi.Cloud(shell))
PA = np.stack([pose(rng.uniform(0, 3), rng.uniform(-0.05, 0.05, 3)) for _ in range(SMALL)])
PB = np.stack([pose(rng.uniform(0, 3), rng.uniform(-0.35, 0.35, 3)) for _ in range(SMALL)])
isect_distinct = []
def isect_call(n):
    k = np.arange(n) % SMALL
    z = np.zeros(n, np.int32)
    return capi.overlap_factors([isect_shape], z, PA[k].reshape(-1, 16), z, PB[k].reshape(-1, 16), 0.1, True, False)
def isect_want(n):
    if not isect_distinct:
        isect_distinct.extend(I.overlap((shell, shell), PA[j], (shell, shell), PB[j], 0.1, True, False) for j in range(SMALL))
    k = np.arange(n) % SMALL
    ov = np.array([isect_distinct[j][0] for j in k], F).reshape(n)
    cnt = np.array([isect_distinct[j][1] for j in k], np.int32).reshape(n, 3)
    return ov, cnt

# ---- mesh resampling: t triangles of area 0.005 (64 samples each), a window of the sequence; resample_restate answers ----
def mesh_of(t):
    r = np.random.default_rng(100 + t)
    a = r.uniform(0, 1, (t, 3))
    pos = np.stack([a, a + [0.1, 0, 0], a + [0, 0.1, 0]], axis=1).reshape(-1, 3).astype(F)
    nor = r.normal(0, 1, (3 * t, 3)); nor = (nor / np.linalg.norm(nor, axis=1, keepdims=True)).astype(F)
    return dict(pos=pos, nor=nor, cls=r.integers(0, 9, 3 * t).astype(np.int32), faces=np.arange(3 * t, dtype=np.int32).reshape(t, 3))
MESH = {t: mesh_of(t) for t in (2, 64)}
mesh_whole = {}
def mesh_call(s):
    t, first, count = s
    m = MESH[t]
    o = capi.uniform_resample(m["pos"], m["faces"], nor=m["nor"], class_ids=m["cls"], first=first, count=count)
    return o["pos"], o["nor"], o["class_ids"], o["face"], np.int64(o["n_samples"])
def mesh_want(s):
    t, first, count = s
    if t not in mesh_whole:
        mesh_whole[t] = R.resample(MESH[t])
    w = mesh_whole[t]
    count = w["n_samples"] - first if count is None else count
    cut = slice(first, first + count)
    return w["pos"][cut], w["nor"][cut], w["cls"][cut], w["face"][cut], np.int64(w["n_samples"])

# ---- the shuffle's permutation of n elements; rs_hip_shuffle_plan is the reference's loop on the host ----
def perm_call(n): return [capi.shuffle_permutation(n)]
def perm_want(n): return [capi.shuffle_plan(n)]

# ---- selection by ids among n points; numpy answers ----
point_ids = rng.integers(0, 6, LARGE).astype(np.int32)
IDS = np.array([1, 4], np.int32)
def select_call(n): return [capi.select_by_ids(point_ids[:n], IDS)]
def select_want(n): return [np.flatnonzero(np.isin(point_ids[:n], IDS)).astype(np.int32)]

# ---- plane votes of h hypotheses over n points; planes_restate answers ----
plane_pos = rng.uniform(0, 1, (LARGE, 3)); plane_pos[::2, 1] *= 0.02; plane_pos = plane_pos.astype(F)
plane_active = (np.arange(LARGE) % 5 != 4).astype(np.uint8)
plane_c = rng.uniform(0, 1, (256, 3)); plane_c[::2, 1] = 0.01; plane_c = plane_c.astype(F)
plane_n = rng.normal(0, 0.2, (256, 3)); plane_n[:, 1] += 1; plane_n = (plane_n / np.linalg.norm(plane_n, axis=1, keepdims=True)).astype(F)
def votes_call(s): return [capi.plane_votes(plane_pos[:s[0]], plane_active[:s[0]], plane_c[:s[1]], plane_n[:s[1]], 0.02)]
def votes_want(s): return [P.votes(plane_pos[:s[0]], plane_active[:s[0]], plane_c[:s[1]], plane_n[:s[1]], 0.02)]

# ---- coverage extensions: n candidates (one small object, n poses) on a base of three placements ----
cov_scene = rng.uniform(0, 2, (3000, 3)).astype(F)
cov = capi.Coverage(np.zeros(3, F), np.full(3, 2, F), cov_scene, None, 0.1)
cov_obj = capi.Cloud(rng.uniform(-0.2, 0.2, (40, 3)).astype(F))
cov_base = [(cov_obj, pose(rng.uniform(0, 3), rng.uniform(0.3, 1.7, 3)), 0) for _ in range(3)]
cov_cand = [(cov_obj, pose(rng.uniform(0, 3), rng.uniform(0.1, 1.9, 3))) for _ in range(LARGE)]
def cov_call(n):
    sc, ag, ba = cov.extensions(cov_base, cov_cand[:n])
    return sc, ag, np.int64(ba)

# unit -> (call, host-side counterpart or None, the sizes: small, large, one, none)
UNITS = dict(
    knn_search=(knn_call, knn_want, (SMALL, LARGE, 1, 0)),
    overlap_factors=(isect_call, isect_want, (SMALL, LARGE, 1, 0)),
    uniform_resample=(mesh_call, mesh_want, ((2, 0, None), (64, 0, None), (2, 5, 1), (2, 0, 0))),
    shuffle_permutation=(perm_call, perm_want, (SMALL, LARGE, 1, 0)),
    select_by_ids=(select_call, select_want, (SMALL, LARGE, 1, 0)),
    plane_votes=(votes_call, votes_want, ((SMALL, 8), (LARGE, 256), (1, 1), (0, 8))),
    extensions=(cov_call, None, (SMALL, LARGE, 1, 0)),
)

def refused(code, what, f, *a, **k):
    try:
        f(*a, **k)
    except capi.RescanHipError as e:
        assert f"error {code}:" in str(e) and what in str(e), str(e)
        return True
    return False
"""


def run_child(body, limit=120, prelude=PRELUDE):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", prelude + body, ROOT], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


def test_regrowth_keeps_results():
    """small, large (every buffer of the unit is freed and allocated again), one element, none, small again: the last equals the
    first bit for bit and every call equals its host-side counterpart; the n + 1 flags and ranks of a selection of one point are
    where an off-by-one of Buf::ensure would show."""
    run_child(r"""
assert mesh_want((64, 0, None))[4] > 4 * mesh_want((2, 0, None))[4]
for name, (call, want, (small, large, one, none)) in UNITS.items():
    first = call(small)
    big = call(large)
    single = call(one)
    nothing = call(none)
    again = call(small)
    same(again, first)
    if want is not None:
        for s, got in ((small, first), (large, big), (one, single), (none, nothing)):
            same(got, want(s))
    if name == "extensions":
        cov_big = big
    print(name, "regrown")
# the coverage extensions have no host-side counterpart: the large call again, first in a released workspace
capi.arrange_release()
same(cov_call(LARGE), cov_big)
assert cov_big[1].max() > cov_big[2] and len(set(cov_big[1].tolist())) > 8           # (candidates that add cells, and not all the same number)
print("ok")
""")


def test_spans_are_booked_as_before():
    """One call per unit under rs_hip_profile_enable: the spans each name books, with a finite time.  A span left open, closed
    twice or widened over another changes a count."""
    print(run_child(r"""
# spans per call, taken from the parent commit (hand-paired api_prof_begin / api_prof_end) by running this body on its library
BOOKED = dict(plane_compact=1, plane_votes=1, plane_best=0, plane_gather_flags=0, plane_scatter=0, plane_relabel=0,
              fuse_select=1, fuse_permutation=1, fuse_merge=0, mesh_sample=1, isect=2, saliency=0, coverage=1)
for name, (call, want, (small, large, one, none)) in UNITS.items():
    if name != "knn_search":                       # (rs_knn.hip books no span)
        call(small)                                # outside the profile: buffers, first launches
capi.profile_reset()
capi.profile_enable(True)
try:
    for name in ("plane_votes", "select_by_ids", "shuffle_permutation", "uniform_resample", "overlap_factors", "extensions"):
        call, want, sizes = UNITS[name]
        got = call(sizes[0])
        if want is not None:
            same(got, want(sizes[0]))
    read = {k: capi.profile_read(k) for k in BOOKED}
finally:
    capi.profile_enable(False)
print(read)
for k, (n, ms) in read.items():
    assert n == BOOKED[k], (k, n, BOOKED[k])
    assert np.isfinite(ms) and ms >= 0.0 and (n > 0 or ms == 0.0), (k, ms)
# with the profile off again nothing more is booked
UNITS["select_by_ids"][0](SMALL)
assert capi.profile_read("fuse_select")[0] == BOOKED["fuse_select"]
print("ok")
"""))


def test_a_refusal_leaves_the_unit_usable():
    """A refused call — of arguments only, some refused before any device work, some after launches and a read-back — and then the
    valid call of before: the same bits."""
    run_child(r"""
before = {name: call(sizes[0]) for name, (call, want, sizes) in UNITS.items()}
lib = capi.load()
# refused before the unit touches the device
assert refused(-2, "twice", capi.select_by_ids, point_ids[:SMALL], [3, 5, 3])
n_big = (1 << 24) + 1
counts = np.zeros(8, np.int32)
rc = lib.rs_hip_plane_votes(None, n_big, None, plane_c.ctypes.data, plane_n.ctypes.data, None, 8, 0.02, counts.ctypes.data)
assert rc == -2 and not counts.any(), (rc, lib.rs_hip_last_error())
one = np.zeros(3, F); act = np.ones(1, np.uint8)
rc = lib.rs_hip_plane_votes(one.ctypes.data, n_big, act.ctypes.data, plane_c.ctypes.data, plane_n.ctypes.data, None, 8, 0.02, counts.ctypes.data)
assert rc == -4 and b"2^24" in lib.rs_hip_last_error() and not counts.any(), (rc, lib.rs_hip_last_error())
m2 = MESH[2]
assert refused(-2, "window", capi.uniform_resample, m2["pos"], m2["faces"], first=0, count=10 ** 6)
# refused once the device is ready: k above the limit
assert refused(-4, "RS_HIP_KNN_MAX_K", capi.knn_search, knn_grid, knn_q[:SMALL], capi.KNN_MAX_K + 1)
# refused after both launches and the read-back: a boundary point outside the grid of the extent clouds
far = capi.Cloud(np.concatenate([shell, [[3.0, 0, 0]]]).astype(F))
z = np.zeros(2, np.int32)
near = np.stack([pose(0.0, (0, 0, 0)), pose(0.0, (0.1, 0, 0))])
assert refused(-2, "pair 1", capi.overlap_factors, [isect_shape, (far, isect_shape[1])], [0, 0], near[[0, 0]], [0, 1], near[[1, 1]], 0.1, True, False)
# refused after the flags, their scan and the read-back of the offsets: more inliers than the caller's capacity
flat = plane_pos[:SMALL].copy(); flat[:, 1] = 0.0
up = np.tile(np.array([0, 1, 0], F), (SMALL, 1))
floor = capi.Cloud(flat, up)
c0, n0 = np.zeros((1, 3), F), np.array([[0, 1, 0]], F)
inliers = capi.gather_plane_inliers(floor, c0, n0)
assert len(inliers) == 1 and (inliers[0] == np.arange(SMALL)).all()
index = np.zeros(1, np.int32); offsets = np.full(2, -1, np.int64)
rc = lib.rs_hip_gather_plane_inliers(floor.handle, c0.ctypes.data, n0.ctypes.data, None, None, None, 1, 0.8, 0.05, 0, 0, index.ctypes.data, 1, offsets.ctypes.data)
assert rc == -4 and b"capacity" in lib.rs_hip_last_error() and (offsets == -1).all() and index[0] == 0, (rc, lib.rs_hip_last_error())
same(capi.gather_plane_inliers(floor, c0, n0), inliers)
for name, (call, want, sizes) in UNITS.items():
    same(call(sizes[0]), before[name])
print("ok")
""")


# ---- the host units of the C ABI with a workspace (clouds, ICP, scores, rows): every step IS a case of tests/test_gpu_parity.py, called on its fixture ----
API_PRELUDE = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from rescan_amd import capi
import test_gpu_parity as TP                     # its test functions are called as they are: no comparison is restated here
from conftest import coverage_case, label_case, load_golden
from oracle.pyoracle import LEVEL_VOXEL, level_max_n_neigh
capi.init(0)
F = np.float32
sd = load_golden("scene.npz")                    # (conftest.gscene, which is a fixture and cannot be called here)
gscene = dict(points=sd["points"], normals=sd["normals"],
              objects=[dict(pos=sd[f"obj{i}_pos"], nor=sd[f"obj{i}_nor"], pose=sd["obj_pose"][i], class_idx=int(sd["obj_class"][i]),
                            uidx=int(sd["obj_uidx"][i])) for i in range(int(sd["n_obj"]))])
pts, nor = gscene["points"], gscene["normals"]
clouds = {r: capi.Cloud(pts, nor, cell_size=2 * r) for r in (0.05, 0.1)}              # test_gpu_parity.scene_clouds
clouds[0.075] = capi.Cloud(pts, nor)
objs = [capi.Cloud(o["pos"], o["nor"], cell_size=0.1) for o in gscene["objects"]]
scene_clouds = (clouds, objs)

# the parity case, then the call's bits (what a repeated call is compared with)
def scores(fname, scene_route=False):
    (TP.test_scores_scene_space_route_vs_golden if scene_route else TP.test_scores_vs_golden)(capi, scene_clouds, fname + ".npz")
    g = load_golden(fname + ".npz")
    prev = capi.score_scene_space_from(0) if scene_route else None
    try:
        return [capi.alignment_scores(objs[int(g["obj"])], clouds[cell], g["poses"], 0.1, int(g["k"])) for cell in (0.05, 0.1)]
    finally:
        if scene_route:
            capi.score_scene_space_from(prev)

def icp(fname):
    TP.test_icp_align_vs_golden(capi, gscene, scene_clouds, fname + ".npz")
    g = load_golden(fname + ".npz")
    md = float(g["max_dist"])
    err, T, iters = capi.icp_align(objs[int(g["obj"])], clouds[round(md, 3)], g["T1"], g["T2"], md, g["max_angle"])
    return [T, F(err), np.int32(iters)]

def rows(fname):
    TP.test_rows_vs_golden(capi, gscene, fname + ".npz")
    g = load_golden(fname + ".npz")
    return list(capi.radius_search(clouds[0.05], g["query"], float(g["radius"]), int(g["k"]))[:3])

def coverage_objects():
    d, cobjs, static, arrangements = coverage_case(gscene)
    cov = capi.Coverage(d["bbox_min"], d["bbox_max"], pts, d["quality"], 0.05, 0.5)
    cc = [capi.Cloud(p, np.zeros_like(p)) for p in cobjs]
    return cov, [[(cc[k], pose, static[k]) for k, pose in plc] for plc in arrangements]

def same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (k, g.dtype, w.dtype, g.shape, w.shape)
"""


# (as tests/conftest.py: torch initialises its copy of the HIP runtime before librescan_hip.so loads the system's)
TORCH_FIRST = r"""
import torch
torch.cuda.init()
"""


def test_api_units_regrow_next_to_each_other():
    """One thread, one sequence: score, ICP, score, rows, edges, rows, level, labels, coverage, the estimator entry point, rows, score
    (through the scene-space route), ICP — the units that shared buffers before each had a workspace of its own (queue / queue_count:
    ICP and score; rd2 / ridx / rnn: rows and edges; the tile buffer: rows and the estimator entry point; lvl_samples: level and
    labels) alternate, and the later call of a unit is the larger or the same.  Every result is its fixture's as the parity suite
    demands; a repeated call returns the bits of its first occurrence."""
    run_child(r"""
s1 = scores("scores_chair1_k32")
i1 = icp("icp_chair1_refine")
scores("scores_table0_k64")
r1 = rows("rows_k8_r005")
TP.test_neighborhood_vs_golden(capi, gscene)                      # (neighborhood_obj0 and the other three)
rows("rows_k64_r010")
TP.test_level_builder_vs_golden(capi, gscene)
TP.test_level_cloud_built_on_the_device(capi, None, gscene)       # (level gather -> cloud construction, across two units)
TP.test_labels_vs_golden(capi, gscene, scene_clouds, "labels_mixed.npz")
TP.test_coverage_vs_golden(capi, gscene)
from oracle.pyoracle import Oracle
TP.test_icp_estimate_vs_oracle(capi, Oracle(), gscene)
same(rows("rows_k8_r005"), r1)
same(scores("scores_chair1_k32", scene_route=True), s1)
same(icp("icp_chair1_refine"), i1)
print("ok")
""", prelude=API_PRELUDE)


def test_label_state_outlives_calls_of_other_units():
    """Two partials of the placement loop written to device memory (rs_hip_label_partial_device returns without a synchronisation,
    its placements still uploading from the unit's pinned block), a score call and a rows call in between, then the ordered fold:
    the labels and distances of rs_hip_assign_labels over the same placements, exactly (labels_ties: every distance tie of the
    fixture is decided by the order)."""
    run_child(r"""
d, lobjs, plcs = label_case(gscene, "labels_ties.npz")
oc = [capi.Cloud(o["pos"], o["nor"], cell_size=0.1) for o in lobjs]
scene = clouds[0.05]
ns, n = scene.n, len(plcs)
order = [int(k) for k in d["order"]]
poses = np.stack([plcs[k]["pose"] for k in order]); pobj = [oc[plcs[k]["object_idx"]] for k in order]
first_static = next((k for k, oi in enumerate(order) if lobjs[plcs[oi]["object_idx"]]["is_static"]), 0)
radii = [0.05 if k < first_static else np.float32(1.5) * np.float32(0.05) for k in range(n)]
want_l = np.zeros(ns, np.int8); want_m = np.full(ns, 1e9, F)
capi.assign_labels(scene, poses, pobj, radii, want_l, want_m)
assert (want_l == d["labels"]).all() and (want_m == d["min_dists"]).all()          # (the fixture's, too: test_labels_vs_golden's sharded route)
assert len(set(want_l.tolist())) > 3
# per part: min_dists float32[ns], then labels int8[ns] (rescan_amd/dist.py's layout)
stride = (5 * ns + 255) // 256 * 256
dev = torch.empty(2 * stride, dtype=torch.uint8, device="cuda")
half = n // 2
for r, (p0, p1) in enumerate(((0, half), (half, n))):
    base = dev.data_ptr() + r * stride
    capi.label_partial_device(scene, poses[p0:p1], pobj[p0:p1], radii[p0:p1], p0, base, base + 4 * ns)
scores("scores_chair1_k32")
rows("rows_k8_r005")
mo = np.array([r * stride // 4 for r in range(2)], np.int64); lo = np.array([r * stride + 4 * ns for r in range(2)], np.int64)
got_l, got_m = capi.fold_label_partials_device(dev.data_ptr(), mo, lo, ns, query_order_of=scene)
assert got_l.tobytes() == want_l.tobytes() and got_m.tobytes() == want_m.tobytes()
print("ok")
""", prelude=TORCH_FIRST + API_PRELUDE)


def test_api_spans_are_booked_as_before():
    """One call per moved entry point under rs_hip_profile_enable, the profile reset in between: the names each books and how often.
    A ProfScope that lost its launch in the move, or a span now booked by two units, changes a count."""
    print(run_child(r"""
# spans per call, taken from the parent commit (one rs_api.hip, one workspace) by running this body on its library
BOOKED = dict(
    alignment_scores=dict(nn_score=1),
    assign_labels=dict(nn_label=1),
    radius_search=dict(nn_rows=1),
    compute_neighborhood=dict(nn_rows=1, edges=1),
    level_samples=dict(level_neighbours=2, level_rounds=1),
    coverage_scores=dict(coverage=1),
    icp_align=dict(nn_icp=7, icp_moments=7),
)
NAMES = ("nn_score", "nn_label", "label_fold", "nn_rows", "edges", "level_neighbours", "level_rounds", "coverage", "nn_icp", "icp_moments")
gs, gr, gi = (load_golden(f + ".npz") for f in ("scores_chair1_k32", "rows_k64_r010", "icp_chair1_refine"))
d, lobjs, plcs = label_case(gscene, "labels_ties.npz")
oc = [capi.Cloud(o["pos"], o["nor"], cell_size=0.1) for o in lobjs]
cov, batch = coverage_objects()
lab = np.zeros(len(pts), np.int8); mind = np.full(len(pts), 1e9, F)
bare = capi.Cloud(pts, None)
md = float(gi["max_dist"])
CALLS = dict(
    alignment_scores=lambda: capi.alignment_scores(objs[int(gs["obj"])], clouds[0.1], gs["poses"], 0.1, int(gs["k"])),
    assign_labels=lambda: capi.assign_labels(clouds[0.05], np.stack([p["pose"] for p in plcs]), [oc[p["object_idx"]] for p in plcs], [0.05] * len(plcs), lab, mind),
    radius_search=lambda: capi.radius_search(clouds[0.05], gr["query"], float(gr["radius"]), int(gr["k"])),
    compute_neighborhood=lambda: capi.compute_neighborhood(objs[0]),
    level_samples=lambda: capi.level_samples(bare, LEVEL_VOXEL[2], level_max_n_neigh(2)),
    coverage_scores=lambda: cov.scores(batch),
    icp_align=lambda: capi.icp_align(objs[int(gi["obj"])], clouds[round(md, 3)], gi["T1"], gi["T2"], md, gi["max_angle"]),
)
for call in CALLS.values():
    call()                                         # outside the profile: buffers, first launches
read = {}
capi.profile_enable(True)
try:
    for name, call in CALLS.items():
        capi.profile_reset()
        call()
        read[name] = {k: capi.profile_read(k) for k in NAMES}
finally:
    capi.profile_enable(False)
print({name: {k: v[0] for k, v in r.items() if v[0]} for name, r in read.items()})
for name, r in read.items():
    for k, (n, ms) in r.items():
        assert n == BOOKED[name].get(k, 0), (name, k, n)
        assert np.isfinite(ms) and ms >= 0.0 and (n > 0 or ms == 0.0), (name, k, ms)
print("ok")
""", prelude=API_PRELUDE))
