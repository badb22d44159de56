"""Times the model fusion (rs_fuse.hip) on the GPU: the shuffle's permutation made by the host plan (upload included) against the
device's, and the whole rs_hip_cloud_create_fused for an object-sized dynamic placement and a scan-sized static one.

    python tools/fuse_timing.py [--out profiles/r10/fuse_timing.txt]

Every step is a child process under its own `timeout`; the first step that fails ends the run.  Each figure is the median of
REPEATS timed calls after WARMUP untimed ones, a host clock around work that ends in a device synchronisation.  The cases are
seeded; tools/fuse_fixture/gen.py --time runs the reference on the same two placements."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPEATS = 2, 7
STEPS = (("perm_100000", 120), ("perm_1000000", 120), ("perm_16777216", 300), ("dynamic", 300), ("static", 300))


def plane(rng, n, density=6400.0):
    """n points of a square patch of the plane x = 0 (normal +x, slightly noisy), at `density` points per square metre."""
    side = np.sqrt(n / density)
    pos = np.zeros((n, 3)); pos[:, 1:] = rng.uniform(0.0, side, (n, 2)); pos[:, 0] = rng.normal(0.0, 0.001, n)
    nor = np.zeros((n, 3)); nor[:, 0] = 1.0; nor += rng.normal(0.0, 0.02, (n, 3))
    nor /= np.linalg.norm(nor, axis=1, keepdims=True)
    return pos.astype(np.float32), nor.astype(np.float32)


def dynamic_case(n_target=50_000):
    """A chair of about n_target scan points over a chair model of about as many (two samplings of the same surfaces), on a floor patch
    that carries another id; the placement's pose is the true one, perturbed."""
    from rescan_amd import synth
    base = len(synth.make_object("chair", 5, 1200.0)[0])
    density = 1200.0 * n_target / base
    model_pos, model_nor = synth.make_object("chair", 5, density)
    sp, sn = synth.make_object("chair", 6, density)
    pose = synth.pose_matrix(0.7, (1.0, 0.0, 1.2))
    rng = np.random.default_rng(10)
    floor_pos, floor_nor = plane(rng, 4000, 1000.0)
    scan_pos = np.concatenate([synth.apply_pose(pose, sp), floor_pos[:, [1, 0, 2]]]).astype(np.float32)
    scan_nor = np.concatenate([synth.apply_pose(pose, sn, False), floor_nor[:, [1, 0, 2]]]).astype(np.float32)
    ids = np.concatenate([np.full(len(sp), 3), np.zeros(len(floor_pos))]).astype(np.int32)
    order = rng.permutation(len(ids))
    return dict(scan_pos=scan_pos[order], scan_nor=scan_nor[order], scan_ids=ids[order], uidx=3, model_pos=model_pos, model_nor=model_nor,
                pose=synth.perturbed_pose(pose, rng), refine=1)


def static_case(n=1_000_000):
    """A wall of n scan points over a wall model of n points; static, so no ICP."""
    from rescan_amd import synth
    rng = np.random.default_rng(11)
    scan_pos, scan_nor = plane(rng, n)
    model_pos, model_nor = plane(rng, n)
    return dict(scan_pos=scan_pos, scan_nor=scan_nor, scan_ids=np.ones(n, np.int32), uidx=1, model_pos=model_pos, model_nor=model_nor,
                pose=synth.pose_matrix(0.3, (0.5, 0.0, 0.2)), refine=0)


def median_ms(f):
    for _ in range(WARMUP):
        f()
    ts = []
    for _ in range(REPEATS):
        t = time.perf_counter(); f(); ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts))


def step_perm(n):
    import torch
    from rescan_amd import capi
    capi.init(0)
    host = capi.shuffle_plan(n)
    assert (capi.shuffle_permutation(n) == host).all()
    dev = torch.empty(n, dtype=torch.int32, device="cuda")

    def plan_and_upload():
        dev.copy_(torch.from_numpy(capi.shuffle_plan(n))); torch.cuda.synchronize()
    a = median_ms(plan_and_upload)
    b = median_ms(lambda: capi.shuffle_permutation(n))          # (ends in the download of the array and a synchronisation)
    print(f"permutation n = {n}: host plan + upload {a[0]:.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}) | "
          f"device, download included {b[0]:.3f} ms (min {b[1]:.3f}, max {b[2]:.3f})", flush=True)


def step_fused(case, name):
    from rescan_amd import capi
    capi.init(0)
    scan = capi.Cloud(case["scan_pos"], case["scan_nor"]); model = capi.Cloud(case["model_pos"], case["model_nor"])

    def call():
        c, info = capi.Cloud.fused(scan, case["scan_ids"], case["uidx"], model, case["pose"], refine=case["refine"])
        n = (info["n_extracted"], c.n); c.close()
        return n
    n_ext, n = call()
    capi.fuse_seconds(False)
    whole = median_ms(call)
    capi.fuse_seconds(True)
    laps = []
    for _ in range(REPEATS):
        call(); laps.append(capi.fuse_seconds(True))
    capi.fuse_seconds(False)
    lap = 1e3 * np.median(np.array(laps), axis=0)
    print(f"fused {name}: {n_ext} extracted of {scan.n} scan points + {model.n} model points = {n}: whole call {whole[0]:.3f} ms "
          f"(min {whole[1]:.3f}, max {whole[2]:.3f}), the host copy of the merged points included", flush=True)
    print(f"fused {name}, a synchronisation after every stage: extraction {lap[0]:.3f} | ICP {lap[1]:.3f} | permutation {lap[2]:.3f} | "
          f"merge {lap[3]:.3f} | index build {lap[4]:.3f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step:
        if a.step.startswith("perm_"):
            return step_perm(int(a.step[5:]))
        return step_fused(dynamic_case() if a.step == "dynamic" else static_case(), a.step)
    lines = []
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True)
        sys.stdout.write(r.stdout); sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            print(f"step {name} ended with status {r.returncode}: stopping", flush=True)
            sys.exit(1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/fuse_timing.py: median of {REPEATS} calls after {WARMUP} warm-up calls\n" + "".join(lines))


if __name__ == "__main__":
    main()
