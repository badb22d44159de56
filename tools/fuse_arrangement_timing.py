"""Times the whole arrangement in one call (rs_hip_cloud_fuse_arrangement) against the route it replaces, one
rs_hip_cloud_create_fused per placement, on the same inputs:

  (a) 8 and 16 dynamic object-sized placements (a chair of about 50 k scan points over a model of about as many, each with its own
      instance id and pose) in a scan of about 1 M points;
  (b) the same plus two static placements of 500 k scan points over 500 k model points each (walls; no ICP).

    python tools/fuse_arrangement_timing.py [--out profiles/r24/fuse_arrangement_timing.txt]

The protocol is tools/fuse_timing.py's: every case is a child process under its own `timeout`, the first that fails ends the run; each
figure is the median of REPEATS timed calls after WARMUP untimed ones, a host clock around work that ends in a device
synchronisation.  The two routes are interleaved: one call of the one, one of the other, and so on.  Both go through the C ABI with
arrays allocated beforehand, ask for source and scan_index, and destroy the clouds they make inside the timed span; neither copies
the merged points to the host.  The stage split comes from rs_hip_fuse_seconds, which both routes feed (a synchronisation after every
stage, so its laps add up to more than the whole call)."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WARMUP, REPEATS = 2, 7
CASES = (("a8", 600), ("a16", 600), ("b8", 600), ("b16", 600))
STAGES = ("extraction", "ICP", "permutation", "merge", "index builds")


def make_case(n_objects, n_walls, n_scan=1_000_000, n_object=50_000, n_wall=500_000):
    from rescan_amd import synth
    import fuse_timing as T
    rng = np.random.default_rng([12, n_objects, n_walls])
    base = len(synth.make_object("chair", 5, 1200.0)[0])
    density = 1200.0 * n_object / base
    pos, nor, ids, placements = [], [], [], []
    for k in range(n_objects):
        model_pos, model_nor = synth.make_object("chair", 100 + k, density)
        sp, sn = synth.make_object("chair", 200 + k, density)
        pose = synth.pose_matrix(0.4 * k, (2.0 * (k % 4) + 1.0, 0.0, 2.0 * (k // 4) + 1.0))
        pos.append(synth.apply_pose(pose, sp)); nor.append(synth.apply_pose(pose, sn, False)); ids.append(np.full(len(sp), 3 + k))
        placements.append(dict(uidx=3 + k, pose=synth.perturbed_pose(pose, rng), refine=1, model=(model_pos, model_nor)))
    for k in range(n_walls):
        wp, wn = T.plane(rng, n_wall); mp, mn = T.plane(rng, n_wall)
        wp = wp + np.array([-1.0 - k, 0, 0], np.float32)
        pos.append(wp); nor.append(wn); ids.append(np.full(n_wall, 1 + k))
        placements.append(dict(uidx=1 + k, pose=synth.pose_matrix(0.0, (-1.0 - k, 0.0, 0.0)), refine=0, model=(mp, mn)))
    n_floor = max(n_scan - sum(len(p) for p in pos[:n_objects]), 1000)
    fp, fn = T.plane(rng, n_floor, n_floor / 81.0)                  # a 9 m x 9 m floor under the objects, id 0
    pos.append(fp[:, [1, 0, 2]]); nor.append(fn[:, [1, 0, 2]]); ids.append(np.zeros(n_floor))
    pos = np.concatenate(pos).astype(np.float32); nor = np.concatenate(nor).astype(np.float32); ids = np.concatenate(ids).astype(np.int32)
    order = rng.permutation(len(ids))
    return dict(scan_pos=pos[order], scan_nor=nor[order], scan_ids=np.ascontiguousarray(ids[order]), placements=placements)


def run_case(name):
    from rescan_amd import capi
    capi.init(0)
    lib = capi.load()
    case = make_case(int(name[1:]), 2 if name[0] == "b" else 0)
    scan = capi.Cloud(case["scan_pos"], case["scan_nor"])
    ids = case["scan_ids"]
    pls = case["placements"]
    P = len(pls)
    models = [capi.Cloud(*pl["model"]) for pl in pls]
    n_ext = [int((ids == pl["uidx"]).sum()) for pl in pls]
    sources = [np.zeros(n_ext[p] + models[p].n, np.int32) for p in range(P)]; indices = [np.zeros(scan.n, np.int32) for _ in range(P)]
    poses = [np.ascontiguousarray(pl["pose"], np.float32).ravel() for pl in pls]
    max_angle = float(np.float32(10.0 * 0.005555555556 * np.pi))
    recs = (capi.FusePlacement * P)(); outs = (capi.FuseResult * P)()
    for p, pl in enumerate(pls):
        recs[p].uidx = pl["uidx"]; recs[p].refine = pl["refine"]; recs[p].model_from = -1; recs[p].model = models[p].handle
        recs[p].pose[:] = poses[p].tolist()
        outs[p].source = sources[p].ctypes.data; outs[p].scan_index = indices[p].ctypes.data
    got = {}

    def one_call():
        rc = lib.rs_hip_cloud_fuse_arrangement(scan.handle, ids.ctypes.data, C.addressof(recs), P, 0.05, max_angle, -1.0, C.addressof(outs))
        assert rc == 0, lib.rs_hip_last_error()
        got["one"] = [(int(outs[p].n_extracted), bytes(outs[p].xform), sources[p][:64].tobytes()) for p in range(P)]
        for p in range(P):
            lib.rs_hip_cloud_destroy(outs[p].cloud)

    def p_calls():
        res = []
        for p, pl in enumerate(pls):
            x = np.zeros(16, np.float32); err = C.c_float(); n = C.c_int64()
            h = lib.rs_hip_cloud_create_fused(scan.handle, ids.ctypes.data, pl["uidx"], models[p].handle, poses[p].ctypes.data, pl["refine"], 0.05, max_angle, -1.0,
                                              x.ctypes.data, C.byref(err), sources[p].ctypes.data, indices[p].ctypes.data, C.byref(n))
            assert h, lib.rs_hip_last_error()
            res.append((n.value, x.tobytes(), sources[p][:64].tobytes()))
            lib.rs_hip_cloud_destroy(h)
        got["many"] = res

    capi.fuse_seconds(False)
    times = {"one": [], "many": []}
    for k in range(WARMUP + REPEATS):
        for route, f in (("many", p_calls), ("one", one_call)) if k % 2 else (("one", one_call), ("many", p_calls)):
            t = time.perf_counter(); f(); dt = time.perf_counter() - t
            if k >= WARMUP:
                times[route].append(dt)
    same_pose = sum(a[1] == b[1] for a, b in zip(got["one"], got["many"]))
    assert all(a[0] == b[0] and a[2] == b[2] for a, b in zip(got["one"], got["many"]))
    laps = {}
    for route, f in (("one", one_call), ("many", p_calls)):
        capi.fuse_seconds(True)
        rows = []
        for _ in range(REPEATS):
            f(); rows.append(capi.fuse_seconds(True))
        capi.fuse_seconds(False)
        laps[route] = 1e3 * np.median(np.array(rows), axis=0)
    ms = {r: 1e3 * np.array(v) for r, v in times.items()}
    what = f"{name}: {P} placements ({sum(pl['refine'] for pl in pls)} dynamic), scan {scan.n} points, extracted {min(n_ext)} .. {max(n_ext)}, merged {sum(n_ext) + sum(m.n for m in models)} points in all"
    print(what)
    for route, label in (("one", "one call (rs_hip_cloud_fuse_arrangement)"), ("many", f"{P} calls (rs_hip_cloud_create_fused)  ")):
        print(f"  {label}: median {np.median(ms[route]):8.3f} ms (min {ms[route].min():.3f}, max {ms[route].max():.3f}) | with a synchronisation after every stage: "
              + " | ".join(f"{s} {v:.3f}" for s, v in zip(STAGES, laps[route])) + " ms")
    a, b = ms["one"], ms["many"]
    verdict = "faster beyond both ranges" if a.max() < b.min() else ("slower beyond both ranges" if a.min() > b.max() else "the ranges overlap")
    print(f"  one call / {P} calls by the medians: {np.median(a) / np.median(b):.3f} ({verdict}); xform bit-equal between the routes for {same_pose} of {P} placements", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.case:
        return run_case(a.case)
    lines = []
    for name, limit in CASES:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", name], capture_output=True, text=True)
        sys.stdout.write(r.stdout); sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            print(f"case {name} ended with status {r.returncode}: stopping", flush=True)
            sys.exit(1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/fuse_arrangement_timing.py: median of {REPEATS} calls after {WARMUP} warm-up calls, the two routes interleaved\n" + "".join(lines))


if __name__ == "__main__":
    main()
