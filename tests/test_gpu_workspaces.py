"""GPU: what the host runtime shared by the units with entry points of their own (rs_host.h: Buf, ProfSpan, fail) can get wrong and
no other test pins — a workspace buffer that grows between two calls of one thread, the profiling spans a call books, and a unit's
next call after a refusal.  Every comparison is exact: against the project's host-side counterpart of the call (the shim's KnnGrid,
tests/isect_restate.py, tests/resample_restate.py, rs_hip_shuffle_plan, numpy, tests/planes_restate.py) or, for the coverage
extensions, against the same call made first after rs_hip_arrange_release.
Each test runs in one child process under its own time limit, so that the thread's workspaces start empty whatever ran before;
nothing here provokes a fault or a HIP error: every refusal is one of arguments."""
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


def run_child(body, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True)
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
