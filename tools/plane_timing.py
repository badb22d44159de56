"""Times the plane stage (rs_planes.hip) on the GPU: one 5 000-hypothesis wall round by stage, the two forms of the votes kernel, the
whole rs_hip_detect_planes, the inlier gather at a level-0 size and the relabel at a level-1 size.

    python tools/plane_timing.py [--out profiles/r11/plane_timing.txt]

Every step is a child process under its own `timeout`; the first step that fails ends the run.  Each figure is the median of
REPEATS timed calls after WARMUP untimed ones: a host clock around work that ends in a device synchronisation, or, for a kernel,
the library's event spans (rs_hip_profile_enable).  The cases are seeded; tools/plane_fixture/gen.py --time runs the reference on
the same detect call."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPEATS = 2, 7
STEPS = (("round", 300), ("forms", 300), ("detect", 300), ("gather", 300), ("relabel", 300))
F = np.float32


def room(n_target, seed):
    """A synth room with three objects scaled to about n_target points."""
    from rescan_amd import synth
    s = synth.scene_for_point_count(n_target, seed=seed)
    return np.ascontiguousarray(s["points"], F), np.ascontiguousarray(s["normals"], F)


def detect_case():
    """The level-2-like cloud of the detect call: about 10^5 points."""
    return room(100_000, 61)


def models_of(det):
    """The detected planes as gather / relabel models: axes from the normal the way rspf__refine_plane_models orients them, generous
    extends, all valid."""
    m = len(det["centers"])
    axes = np.zeros((m, 9), F); ext = np.tile(np.array([50, 50, -50, -50], F), (m, 1)); up = det["normals"][:, 1].copy()
    for k, n in enumerate(det["normals"].astype(np.float64)):
        a1 = np.array([0, 0, 1.0]) if n[1] > 0.8 else np.array([0, 1.0, 0])
        a0 = np.cross(a1, n); a0 /= np.linalg.norm(a0)
        a1 = np.cross(a0, n); a1 /= np.linalg.norm(a1)
        axes[k] = np.concatenate([a0, a1, n])
    return dict(centers=det["centers"], normals=det["normals"], axes=axes, extends=ext, valid=np.ones(m, np.int8), up=up)


def median_ms(f):
    for _ in range(WARMUP):
        f()
    t = []
    for _ in range(REPEATS):
        t0 = time.perf_counter(); f(); t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def span_ms(capi, name, f):
    """Median per-call device time of the span `name` over REPEATS calls of f."""
    for _ in range(WARMUP):
        f()
    t = []
    for _ in range(REPEATS):
        capi.profile_reset(); f(); capi.synchronize()
        n, ms = capi.profile_read(name)
        t.append(ms / max(n, 1))
    return float(np.median(t))


def step(name):
    from rescan_amd import capi
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import planes_restate as R
    capi.init(0)
    if name in ("round", "forms", "detect"):
        pos, nor = detect_case()
        n = len(pos)
        _, wall = R.candidate_masks(nor, 0.8)
    if name == "round":
        t_plan = median_ms(lambda: capi.plane_hypotheses(pos, wall, 5000, 1))
        idx, c, nn = capi.plane_hypotheses(pos, wall, 5000, 1)
        valid = (R.absf(R.up_dot(nn)) < (F(1) - F(0.8))).astype(np.uint8)
        capi.profile_enable(True)
        call = lambda: capi.plane_votes(pos, wall, c, nn, 0.033, valid)
        t_votes, t_compact = span_ms(capi, "plane_votes", call), span_ms(capi, "plane_compact", call)
        capi.profile_enable(False)
        t_call = median_ms(call)
        print(f"one wall round, {n} points, {int(wall.sum())} candidates, 5000 hypotheses ({int(valid.sum())} pass the up test): host table + draws + "
              f"hypotheses {t_plan:.2f} ms | compaction (flags, scan, scatter) {t_compact:.3f} ms | k_plane_votes {t_votes:.3f} ms | "
              f"rs_hip_plane_votes from host arrays (uploads of points, mask and hypotheses, kernels, download of counts) {t_call:.2f} ms")
    elif name == "forms":
        idx, c, nn = capi.plane_hypotheses(pos, wall, 5000, 1)
        capi.profile_enable(True)
        out = []
        for form in (0, 1):
            capi.plane_votes_form(form)
            out.append(span_ms(capi, "plane_votes", lambda: capi.plane_votes(pos, wall, c, nn, 0.033)))
        capi.plane_votes_form(0)
        print(f"k_plane_votes, {int(wall.sum())} candidates x 5000 hypotheses: LDS tile {out[0]:.3f} ms | wave-uniform global loads {out[1]:.3f} ms")
    elif name == "detect":
        cloud = capi.Cloud(pos, nor)
        t = median_ms(lambda: capi.detect_planes(cloud))
        det = capi.detect_planes(cloud, trace=True)
        tr = det["trace"]
        plan = 0.0
        for k in range(tr["n_rounds"]):
            t0 = time.perf_counter(); capi.plane_hypotheses(pos, tr["mask_before"][k], int(tr["n_iters"][k]), int(k > 0)); plan += 1e3 * (time.perf_counter() - t0)
        capi.profile_enable(True); capi.profile_reset(); capi.detect_planes(cloud); capi.synchronize()
        spans = {s: capi.profile_read(s)[1] for s in ("plane_votes", "plane_compact", "plane_best")}
        capi.profile_enable(False)
        print(f"rs_hip_detect_planes( 0.8, 0.033, 250, 2500, 5000 ), {n} points: {t:.1f} ms for {tr['n_rounds']} rounds ({det['n_floors']} floor + {det['n_walls']} walls, "
              f"inliers {det['n_inliers'].tolist()}); of it the host planner {plan:.1f} ms (timed apart, same masks), k_plane_votes {spans['plane_votes']:.2f} ms, "
              f"compaction {spans['plane_compact']:.2f} ms, k_plane_best {spans['plane_best']:.2f} ms; the rest is transfers (mask down, hypotheses up, "
              f"best and counts down), synchronisations and the positions' one download")
    elif name in ("gather", "relabel"):
        pos, nor = detect_case()
        det = capi.detect_planes(capi.Cloud(pos, nor))
        M = models_of(det)
        big_pos, big_nor = room(1_000_000 if name == "gather" else 300_000, 62)
        cloud = capi.Cloud(big_pos, big_nor)
        if name == "gather":
            f = lambda: capi.gather_plane_inliers(cloud, M["centers"], M["normals"], M["axes"], M["extends"], M["valid"], 0.8, 0.05, False, False)
            lists = f()
            print(f"rs_hip_gather_plane_inliers, {cloud.n} points x {len(lists)} models, {sum(len(x) for x in lists)} inliers: {median_ms(f):.2f} ms "
                  f"(flags, one scan, scatter, download; the Python wrapper's retry with a larger index array included)")
        else:
            rng = np.random.default_rng(63)
            cls = rng.choice(np.array([0, 0, 1, 2, 5], np.int32), cloud.n).astype(np.int32); inst = rng.choice(np.array([3, 1024, 2000], np.int32), cloud.n).astype(np.int32)
            f = lambda: capi.relabel_walls_and_floors(cloud, M["centers"], M["normals"], M["axes"], M["extends"], M["valid"], M["up"], 2, 1, 0, cls, inst)
            got = f()
            print(f"rs_hip_relabel_walls_and_floors, {cloud.n} points x {len(M['centers'])} models, {int((got[0] != cls).sum() + (got[1] != inst).sum())} ids rewritten: "
                  f"{median_ms(f):.2f} ms (upload and download of both id arrays included)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        return step(a.step)
    lines = []
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True)
        if r.returncode != 0:
            print(f"{name}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            sys.exit(1)
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
