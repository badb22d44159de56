"""Times the pose search on one GPU against the cascade composed on the host, in one process:

    python tools/propose_timing.py [--repeats 200] [--once]

  (a) rs_hip_propose_poses: tables, grid poses, scores, per-cell best, compaction and the later levels on the device
  (b) the same cascade composed on the host over rs_hip_alignment_scores — what the library offered before the search existed: the
      grid's poses enumerated once and kept (so (b) does not pay the enumeration again), uploaded with every call, the scores read
      back, per-cell best / threshold / survivor list in vectorised NumPy, the survivors uploaded again per level.

The scene is a synth room of the bench's size (BASELINE.json configs[1]: about 10^6 points), searched at its level 1; a chair and a
table at levels 4, 3, 2; the reference's constants.  Both forms go through ctypes with their arguments packed once, are warmed up,
checked to give identical lists, and then timed interleaved (a, b, a, b, ..) with a host clock around the synchronous calls.
Reported: median and interquartile range per form.  --once: one call of each form after the warm-up and no timing, for a
kernel trace (rocprofv3 --kernel-trace --stats -- python tools/propose_timing.py --once).
The level-0 score kernel is the same in both forms and dominates both; nothing here measures a kernel improvement."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F = np.float32
LEVEL_VOXEL = (0.005, 0.01, 0.02, 0.04, 0.08)              # lib/rs/rs_pointcloud.h:145
THRESHOLDS = np.array([0.25, 0.35, 0.40], F)
SPACING, DELTA = F(0.10), F(np.float64(6.2831853072) / np.float64(F(10.0)))
RADIUS, K = F(0.1), 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--points", type=int, default=1_000_000)
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()              # torch's copy of the HIP runtime first (tests/conftest.py)
    except Exception:
        pass
    from rescan_amd import capi, synth
    import propose_restate as R
    capi.init(0)
    lib = capi.load()
    s = synth.scene_for_point_count(a.points, seed=11)
    base = capi.Cloud(s["points"], s["normals"])
    scene, _ = capi.Cloud.level_of(base, LEVEL_VOXEL[1], 256)
    lo, hi = s["points"].min(0).astype(F), s["points"].max(0).astype(F)
    objs = []
    for kind, seed in (("chair", 101), ("table", 102)):
        p, n = synth.make_object(kind, seed)
        b = capi.Cloud(p, n)
        objs.append([capi.Cloud.level_of(b, LEVEL_VOXEL[l], 1024 * l // 4)[0] for l in (4, 3, 2)])
    ox, oz, yaw = capi.pose_grid_plan(lo, hi, SPACING, DELTA)
    n_cells, n_yaw = len(ox) * len(oz), len(yaw)
    print(f"scene: {base.n} points, level 1 {scene.n}; box {hi[0] - lo[0]:.2f} x {hi[2] - lo[2]:.2f} m: {len(ox)} x {len(oz)} cells x {n_yaw} yaws = {n_cells * n_yaw} "
          f"level-0 poses per object ({n_cells * n_yaw * 64 / 1e6:.2f} MB as matrices); objects (levels 4, 3, 2): "
          + ", ".join("/".join(str(c.n) for c in o) for o in objs) + " points")

    # (a) packed once
    handles = (C.c_void_p * 6)(*[c.handle for o in objs for c in o])
    cap = n_cells
    counts, poses, scores = np.zeros(2, np.int32), np.zeros((2, cap, 16), F), np.zeros((2, cap), F)
    tr = dict(n_scored=np.zeros((2, 3), np.int32), n_kept=np.zeros((2, 3), np.int32), n_proposed=np.zeros(2, np.int32))
    trace = capi.ProposeTrace(tr["n_scored"].ctypes.data, tr["n_kept"].ctypes.data, tr["n_proposed"].ctypes.data)
    args_a = (handles, 2, 3, scene.handle, lo.ctypes.data, hi.ctypes.data, float(SPACING), float(DELTA), 0.0, THRESHOLDS.ctypes.data, float(RADIUS), K, cap,
              counts.ctypes.data, poses.ctypes.data, scores.ctypes.data)

    def form_a(with_trace=False):
        rc = lib.rs_hip_propose_poses(*args_a, C.byref(trace) if with_trace else None)
        assert rc == 0, lib.rs_hip_last_error()
        return [(poses[o, :counts[o]].copy(), scores[o, :counts[o]].copy()) for o in range(2)]

    # (b) the grid's poses enumerated once
    P = np.ascontiguousarray(R.grid_poses(lo, 0.0, ox, oz, yaw))
    s0 = np.zeros(len(P), F)

    def score(cloud, X, out):
        rc = lib.rs_hip_alignment_scores(cloud.handle, scene.handle, X, len(X), float(RADIUS), K, out)
        assert rc == 0, lib.rs_hip_last_error()

    def form_b():
        out = []
        for o in objs:
            score(o[0], P, s0)
            sc = np.where(np.isnan(s0), F(-np.inf), s0).reshape(n_cells, n_yaw)
            arg = sc.argmax(1)                                           # the first of equal maxima
            best = np.maximum(sc[np.arange(n_cells), arg], F(0.0))
            cells = np.flatnonzero(best > THRESHOLDS[0])
            lp, ls = np.ascontiguousarray(P[cells * n_yaw + arg[cells]]), best[cells].copy()
            for l in (1, 2):
                act = np.flatnonzero(ls > 0)
                if len(act):
                    X, new = np.ascontiguousarray(lp[act]), np.zeros(len(act), F)
                    score(o[l], X, new)
                    ls[act] = np.where(new > THRESHOLDS[l], new, F(-1.0))
            m = np.abs(ls) > F(0.000001)
            out.append((lp[m], ls[m]))
        return out

    for _ in range(3):
        ra, rb = form_a(True), form_b()
    for o in range(2):
        assert ra[o][0].tobytes() == rb[o][0].tobytes() and ra[o][1].tobytes() == rb[o][1].tobytes(), "the two forms differ"
    print("both forms give identical lists; per object and level, poses scored " + str(tr["n_scored"].tolist()) + ", still > 0 after the level "
          + str(tr["n_kept"].tolist()) + ", proposals " + str(tr["n_proposed"].tolist()) + ", final lists " + str(counts.tolist()))
    if a.once:
        form_a(); form_b()
        capi.synchronize()
        print("once: one call of each form after the warm-up")
        return
    ta, tb = [], []
    for _ in range(max(200, a.repeats)):
        t0 = time.perf_counter(); form_a(); t1 = time.perf_counter(); form_b(); t2 = time.perf_counter()
        ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1))
    for name, t in (("(a) rs_hip_propose_poses, 2 objects, 3 levels", ta), ("(b) host-composed cascade over rs_hip_alignment_scores", tb)):
        q1, q2, q3 = np.percentile(t, [25, 50, 75])
        print(f"{name}: median {q2:.3f} ms, interquartile range {q1:.3f} .. {q3:.3f} ms ({q3 - q1:.3f}), min {min(t):.3f}, {len(t)} interleaved repeats")
    d = np.array(tb) - np.array(ta)
    q1, q2, q3 = np.percentile(d, [25, 50, 75])
    print(f"(b) - (a) per pair of neighbouring calls: median {q2:.3f} ms, interquartile range {q1:.3f} .. {q3:.3f} ms")
    capi.profile_enable(True); capi.profile_reset()
    form_a()
    capi.synchronize()
    print("one call of (a) by the library's event spans: " + ", ".join(f"{n} {capi.profile_read(n)[1]:.3f} ms in {capi.profile_read(n)[0]} spans" for n in ("nn_score", "pose_search")))
    capi.profile_enable(False)


if __name__ == "__main__":
    main()
