"""GPU: rs_hip_propose_poses, rs_hip_cell_best, rs_hip_verify_marks and rsd_propose_poses against the reference's own lists
(tests/golden/propose_*.npz, written by mgs__propose_poses_at_level and mgs_propose_poses: tools/propose_fixture) and against the
cascade composed on the host over capi.alignment_scores with the restated bookkeeping (tests/propose_restate.py) — what the library
could do before the search existed.  Every comparison is exact.  Where a case equals the composed cascade but not the fixture, the
difference is the scorer's (its sums are not the reference's order), not the search's; the assertion says which of the two failed.
The GPU work runs in child processes, each under its own time limit; nothing here provokes a fault: every refusal is decided on the
host."""
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PRELUDE = r"""
import ctypes as C, os, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from rescan_amd import capi
import propose_restate as R
capi.init(0)
F = np.float32
def golden(name): return dict(np.load(os.path.join(sys.argv[1], "tests", "golden", f"propose_{name}.npz")))
def clouds_of(g, static=False):
    scene = capi.Cloud(g["scene_pos"], g["scene_nor"])
    which = [o for o in range(int(g["n_objects"])) if static or not int(g[f"obj{o}_static"])]      # the caller leaves static objects out
    objs = [[capi.Cloud(g[f"obj{o}_l{l}_pos"], g[f"obj{o}_l{l}_nor"]) for l in range(3)] for o in which]
    return scene, which, objs
def args_of(g, r=0, n_levels=3):
    return (g["bbox"][:3], g["bbox"][3:], g[f"run{r}_spacing"], g[f"run{r}_angle_delta"], g["height"], g["thresholds"][:n_levels], g["radius"], int(g["max_n_neigh"]))
def native(g, scene, objs, r=0, n_levels=3, **kw):
    return capi.propose_poses([o[:n_levels] for o in objs], scene, *args_of(g, r, n_levels), **kw)
def composed(g, scene, levels, r=0, n_levels=3):
    a = args_of(g, r, n_levels)
    return R.cascade(lambda l, P: capi.alignment_scores(levels[l], scene, P, a[6], a[7]), n_levels, *a[:6])
def same(a, b): return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
def refused(code, f, *a, **k):
    try:
        f(*a, **k)
    except capi.RescanHipError as e:
        assert f"error {code}:" in str(e), str(e)
        return True
    return False
"""


def run_child(body, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


@pytest.mark.parametrize("case", ("room", "wide", "floor", "empty"))
def test_lists_equal_the_references_and_the_composed_cascade(case):
    """Counts, poses and scores of every run of the case; the trace's counts are the recorded storage's."""
    run_child(r"""
g = golden(sys.argv[2])
scene, which, objs = clouds_of(g)
for r in range(int(g["n_runs"])):
    t0 = time.perf_counter(); got, tr = native(g, scene, objs, r, trace=True); t_native = time.perf_counter() - t0
    ox, oz, yaw = capi.pose_grid_plan(g["bbox"][:3], g["bbox"][3:], g[f"run{r}_spacing"], g[f"run{r}_angle_delta"])
    n_grid = len(ox) * len(oz) * len(yaw)
    for k, o in enumerate(which):
        want = (g[f"run{r}_obj{o}_final_poses"], g[f"run{r}_obj{o}_final_scores"])
        t0 = time.perf_counter(); cp, cs, ctrace, _ = composed(g, scene, objs[k], r); t_comp = time.perf_counter() - t0
        vs_cascade, vs_fixture = same(got[k], (cp, cs)), same(got[k], want)
        print(f"{sys.argv[2]} run {r} object {o}: {n_grid} grid poses, {len(got[k][1])} proposals (fixture {len(want[1])}); equals cascade {vs_cascade}, equals fixture {vs_fixture}; "
              f"call {t_native * 1e3:.1f} ms (all objects), composed {t_comp * 1e3:.1f} ms")
        assert vs_cascade, "the search differs from the cascade composed over alignment_scores: the search's fault"
        assert vs_fixture, "the search equals the composed cascade but not the reference's lists: the scorer's difference, not the search's"
        s = [g[f"run{r}_obj{o}_s{j}"] for j in range(3)]
        assert tr["n_proposed"][k] == len(s[0])
        assert tr["n_scored"][k].tolist() == [n_grid, int((s[0] > 0).sum()), int((s[1] > 0).sum())], tr["n_scored"][k]
        assert tr["n_kept"][k].tolist() == [int((x > 0).sum()) for x in s], tr["n_kept"][k]
        assert [(a, b) for a, b in ctrace] == list(zip(tr["n_scored"][k].tolist(), tr["n_kept"][k].tolist()))
print("ok")
""".replace("sys.argv[2]", repr(case)))


def test_cell_best_on_hand_made_scores():
    run_child(r"""
nan = np.nan
def check(scores, thr):
    scores = np.asarray(scores, F)
    got, want = capi.cell_best(scores, thr), R.cell_best(scores, thr)
    for a, b, name in zip(got, want, ("best_yaw", "best_score", "keep")):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, scores.shape, np.flatnonzero(a != b)[:5])
    return got
by, bs, keep = check([[0.3, 0.5, 0.5, 0.2], [0.5, 0.3, 0.5, 0.5]], 0.25)
assert by.tolist() == [1, 0] and keep.tolist() == [0, 1]                               # equal maxima: the first yaw wins
by, bs, keep = check([[nan, 0.4, nan, 0.3], [nan, nan, nan, nan], [0.2, nan, 0.6, nan]], 0.25)
assert by.tolist() == [1, -1, 2] and bs.tolist() == [F(0.4), 0.0, F(0.6)] and keep.tolist() == [0, -1, 1]        # a NaN never wins
by, bs, keep = check([[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [-1.0, 0.0, -0.5]], 0.25)
assert by.tolist() == [-1, -1, -1] and not np.signbit(bs).any() and keep.tolist() == [-1, -1, -1]                 # all zeros and -0.0
by, bs, keep = check([[0.25, 0.1], [np.nextafter(F(0.25), F(1)), 0.1], [0.1, 0.25]], 0.25)
assert keep.tolist() == [-1, 0, -1]                                                   # best == threshold: not kept
by, bs, keep = check([[0.3], [0.2], [nan], [0.9]], 0.25)
assert by.tolist() == [0, 0, -1, 0] and keep.tolist() == [0, -1, -1, 1]               # n_yaw = 1
by, bs, keep = check([[0.0, 0.0]], -0.5)
assert by.tolist() == [-1] and keep.tolist() == [0]                                   # (a negative threshold proposes without a rotation, :217-241)
rng = np.random.default_rng(3)
for n_cells in (1, 63, 64, 65, 4097):                                                 # the scan's seams; order kept
    for n_yaw in (1, 10):
        s = rng.random((n_cells, n_yaw)).astype(F) * F(0.5)
        s[rng.random((n_cells, n_yaw)) < 0.1] = nan
        s[::7] = np.minimum(s[::7], F(0.2))                                           # scattered cells that propose nothing
        by, bs, keep = check(s, 0.25)
        k = keep[keep >= 0]
        assert (k == np.arange(len(k))).all() and (n_cells < 63 or (0 < len(k) < n_cells))
assert len(capi.cell_best(np.zeros((0, 10), F), 0.25)[0]) == 0
print("ok")
""")


def test_verify_marks_on_hand_made_scores():
    run_child(r"""
nan = np.nan
old = np.array([0.5, 0.3, -1.0, 0.0, -0.0, 0.7, 0.9, 1e-7, nan, 0.6], F)
new = np.array([0.36, 0.35, 0.9, 0.9, 0.9, nan, 0.2, 0.5, 0.9, np.nextafter(F(0.35), F(1))], F)
got = capi.verify_marks(old, new, 0.35)
want = R.verify_marks(old, new, 0.35)
assert got.tobytes() == want.tobytes(), (got, want)
# scores <= 0 (and a NaN, which is not > 0) untouched; equality with the threshold gives -1; NaN gives -1
assert got[2] == -1 and got[3] == 0 and np.signbit(got[4]) and np.isnan(got[8]) and got[1] == -1 and got[5] == -1 and got[6] == -1
assert got[0] == F(0.36) and got[7] == F(0.5) and got[9] == new[9]
rng = np.random.default_rng(4)
for n in (1, 255, 256, 257, 5000):
    old = np.where(rng.random(n) < 0.3, F(-1), rng.random(n).astype(F)).astype(F); new = rng.random(n).astype(F)
    assert capi.verify_marks(old, new, 0.4).tobytes() == R.verify_marks(old, new, 0.4).tobytes()
assert len(capi.verify_marks(np.zeros(0, F), np.zeros(0, F), 0.4)) == 0
print("ok")
""")


def test_batches_sizes_and_release():
    """An object alone gives what it gives inside a batch of three; a smaller call after a larger one gives what a fresh call gives."""
    run_child(r"""
g = golden("room")
scene, which, objs = clouds_of(g, static=True)              # three objects: for this test the static one is searched too
assert len(objs) == 3
batch = native(g, scene, objs)
for k in range(3):
    alone = native(g, scene, [objs[k]])
    assert same(alone[0], batch[k]), k
f = golden("floor"); fscene, _, fobjs = clouds_of(f)
e = golden("empty"); escene, _, eobjs = clouds_of(e)
capi.propose_release()
fresh = dict(room=native(g, scene, objs[:1]), floor=native(f, fscene, fobjs, 1, trace=True), empty=native(e, escene, eobjs, trace=True))
capi.propose_release(); capi.propose_release()             # nothing held the second time: still fine
big = native(g, scene, objs)                                # larger (three objects, 22 x 18 cells) ...
small = native(f, fscene, fobjs, 1, trace=True)             # ... then smaller (one object, 11 x 11 cells)
assert same(small[0][0], fresh["floor"][0][0]) and all((small[1][k] == fresh["floor"][1][k]).all() for k in small[1])
none = native(e, escene, eobjs, trace=True)                 # ... then a call that proposes nothing: no stale counts
assert len(none[0][0][1]) == 0 and all((none[1][k] == fresh["empty"][1][k]).all() for k in none[1]) and none[1]["n_proposed"][0] == 0
again = native(g, scene, objs[:1])
assert same(again[0], fresh["room"][0]) and same(again[0], big[0])
print("ok")
""")


def test_capacity_and_edge_cases():
    run_child(r"""
g = golden("room")
scene, which, objs = clouds_of(g)
full = native(g, scene, objs)
need = [len(s) for _, s in full]
assert min(need) > 1
# a capacity that is too small: E_CAPACITY, the needed counts, arrays untouched
lib = capi.load()
a = args_of(g)
lo, hi, thr = np.ascontiguousarray(a[0], F), np.ascontiguousarray(a[1], F), np.ascontiguousarray(a[5], F)
handles = (C.c_void_p * 6)(*[c.handle for o in objs for c in o])
cap = max(need) - 1
counts = np.full(2, -7, np.int32); poses = np.full((2, cap, 16), -7, F); scores = np.full((2, cap), -7, F)
rc = lib.rs_hip_propose_poses(handles, 2, 3, scene.handle, lo.ctypes.data, hi.ctypes.data, float(a[2]), float(a[3]), float(a[4]), thr.ctypes.data,
                              float(a[6]), a[7], cap, counts.ctypes.data, poses.ctypes.data, scores.ctypes.data, None)
assert rc == -4 and counts.tolist() == need and (poses == -7).all() and (scores == -7).all(), (rc, counts)
assert refused(-4, native, g, scene, objs, capacity=cap)
exact = native(g, scene, objs, capacity=max(need))
assert all(same(x, y) for x, y in zip(exact, full))
# no objects
assert native(g, scene, []) == []
# a level cloud of 0 points: at level 0 nothing is proposed; at a later level the proposals become -1 (0 / 0 is NaN, :156)
empty = capi.Cloud(np.zeros((0, 3), F), np.zeros((0, 3), F))
got, tr = native(g, scene, [[empty, objs[0][1], objs[0][2]], [objs[0][0], empty, objs[0][2]], [objs[0][0], objs[0][1], empty]], trace=True)
assert len(got[0][1]) == 0 and tr["n_proposed"].tolist() == [0, need[0], need[0]]
assert got[1][0].tobytes() == full[0][0].tobytes() and (got[1][1] == -1).all() and tr["n_scored"][1].tolist()[2] == 0
s1 = g[f"run0_obj{which[0]}_s1"]
assert got[2][0].tobytes() == full[0][0].tobytes() and (got[2][1] == np.where(s1 > 0, F(-1), s1)).all()
# one level: the grid search alone
one = native(g, scene, objs, n_levels=1)
for k, o in enumerate(which):
    assert same(one[k], (g[f"run0_obj{o}_poses"], g[f"run0_obj{o}_s0"])), k
    cp, cs, _, _ = composed(g, scene, objs[k], n_levels=1)
    assert same(one[k], (cp, cs))
two = native(g, scene, objs, n_levels=2)
for k, o in enumerate(which):
    assert same(two[k], (g[f"run0_obj{o}_poses"], g[f"run0_obj{o}_s1"])), k
five = [o + o[:2] for o in objs]                            # n_levels outside 1..4: refused on the host
assert refused(-2, capi.propose_poses, five, scene, a[0], a[1], a[2], a[3], a[4], np.full(5, 0.3, F), a[6], a[7])
# the shim on host arrays equals the native call
dropin = C.CDLL(os.path.join(sys.argv[1], "rescan_amd", "librescan_dropin.so"))
dropin.rsd_propose_poses.restype = C.c_int
dropin.rsd_propose_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
P = [np.ascontiguousarray(g[f"obj{o}_l{l}_pos"]) for o in which for l in range(3)]; N = [np.ascontiguousarray(g[f"obj{o}_l{l}_nor"]) for o in which for l in range(3)]
pp = (C.c_void_p * 6)(*[x.ctypes.data for x in P]); nn = (C.c_void_p * 6)(*[x.ctypes.data for x in N]); cnt = np.array([len(x) for x in P], np.int32)
cap = max(need); counts = np.zeros(2, np.int32); poses = np.zeros((2, cap, 16), F); scores = np.zeros((2, cap), F)
sp, sn = np.ascontiguousarray(g["scene_pos"]), np.ascontiguousarray(g["scene_nor"])
rc = dropin.rsd_propose_poses(pp, nn, cnt.ctypes.data, 2, 3, sp.ctypes.data, sn.ctypes.data, len(sp), lo.ctypes.data, hi.ctypes.data, float(a[2]), float(a[3]), float(a[4]),
                              thr.ctypes.data, float(a[6]), a[7], cap, counts.ctypes.data, poses.ctypes.data, scores.ctypes.data)
assert rc == 0 and counts.tolist() == need
assert all(same((poses[k, :need[k]], scores[k, :need[k]]), full[k]) for k in range(2))
print("ok")
""")


def test_alignment_scores_keep_their_bits_after_the_split():
    """rs_hip_alignment_scores is now a shell around the device core the search calls: the bench workload's 256 poses (the case of
    tests/golden/bench_seed11.npz) still give the fixture's scores, and the two routes still give each other's bits."""
    run_child(r"""
import hashlib
import bench
g = dict(np.load(os.path.join(sys.argv[1], "tests", "golden", "bench_seed11.npz")))
t0 = time.perf_counter()
w = bench.build_workload(int(g["n_points"]), seed=int(g["seed"]), knn="hash")
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
assert sha(w["score_poses"]) == str(g["in_sha"][6]), "the generator no longer produces the poses the fixture was made for"
sc = capi.alignment_scores(w["obj_score"], w["scan1"], w["score_poses"], 0.1, 64)
prev = capi.score_scene_space_from(0)
other = capi.alignment_scores(w["obj_score"], w["scan1"], w["score_poses"], 0.1, 64)
capi.score_scene_space_from(prev)
want = g["scores"].astype(F)
print(f"{len(sc)} poses, {int((sc.view(np.uint32) != want.view(np.uint32)).sum())} differ in bits from the fixture, max abs {np.abs(sc.astype(np.float64) - want).max():.3e}; workload and calls {time.perf_counter() - t0:.1f} s")
assert len(sc) >= 256 and sc.tobytes() == other.tobytes()
assert sc.tobytes() == want.tobytes()
print("ok")
""", limit=300)
