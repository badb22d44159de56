"""Times the scan-to-objects split (rs_split.hip) on the GPU, on a room of the bench's size
(synth.scene_for_point_count( 1_000_000, seed=11 ), level 0):

  (a) rs_hip_scan_to_objects and rs_hip_cloud_split_objects, whole and by stage (table, partition, chains, transform, index builds)
  (b) what the library offered before: rs_hip_select_by_ids once per instance — against the one-pass rs_hip_split_by_instance
      (table plus partition) on the same ids.  THE CLAIM ON TRIAL: the one pass is faster by more than twice the larger
      interquartile range
  (c) rs_hip_split_plan on the host
  (d) the share of addends the chains took one by one; the chains alone in both forms (a wave per chain with order-free steps; a
      lone lane per chain), whose time is the longest chain's
  (e) both routes of the partition

    python tools/split_timing.py [--out profiles/r21/split_timing.txt]

Every step is a child process under its own `timeout`; the first step that fails ends the run.  Synchronous C ABI calls timed with
the host clock, arguments packed once; after WARMUP untimed rounds, REPEATS rounds in which the variants of a step take turns
(interleaved); medians and interquartile ranges.  tools/split_fixture/gen.py --time runs the reference on the same room."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPEATS = 2, 9
STEPS = (("partition", 300), ("objects", 400), ("chains", 300), ("plan", 300))


def room(n=1_000_000):
    from rescan_amd import synth
    s = synth.scene_for_point_count(n, seed=11)
    return dict(pos=s["points"], nor=s["normals"], cls=s["class_idx"].astype(np.int32), inst=s["instance_idx"].astype(np.int32),
                static=np.array([synth.CLASS_IDX[k] for k in synth.STATIC_CLASSES], np.int32))


def interleaved(variants, repeats=REPEATS, warmup=WARMUP):
    """variants: name -> callable.  Returns name -> (median ms, interquartile range ms)."""
    ts = {k: [] for k in variants}
    for r in range(warmup + repeats):
        for k, f in variants.items():
            t = time.perf_counter(); f(); dt = time.perf_counter() - t
            if r >= warmup:
                ts[k].append(1e3 * dt)
    return {k: (float(np.median(v)), float(np.percentile(v, 75) - np.percentile(v, 25))) for k, v in ts.items()}


def fmt(r):
    return " | ".join(f"{k} {m:.3f} ms (IQR {q:.3f})" for k, (m, q) in r.items())


def packed(capi, n, room_for, points):
    k = C.c_int32()
    a = dict(inst_ids=np.zeros(room_for, np.int32), counts=np.zeros(room_for, np.int64), first=np.zeros(room_for, np.int64), offsets=np.zeros(room_for + 1, np.int64),
             order=np.zeros(n, np.int32), class_of=np.zeros(room_for, np.int32), is_static=np.zeros(room_for, np.int32), sums=np.zeros((room_for, 3)),
             centroids=np.zeros((room_for, 3), np.float32), xforms=np.zeros((room_for, 16), np.float32), poses=np.zeros((room_for, 16), np.float32))
    if points:
        a["out_pos"] = np.zeros((n, 3), np.float32); a["out_nor"] = np.zeros((n, 3), np.float32)
    return k, a, capi.SplitOut(n_instances=C.addressof(k), **{key: v.ctypes.data for key, v in a.items()})


def step_partition():
    from rescan_amd import capi
    capi.init(0)
    lib = capi.load()
    s = room(); ids = s["inst"]; n = len(ids)
    inst = capi.instance_table(ids)[0]
    index = np.zeros(n, np.int32); count = C.c_int64(); one = np.zeros(1, np.int32)
    out_inst = np.zeros(4096, np.int32); off = np.zeros(4097, np.int64); order = np.zeros(n, np.int32); k = C.c_int32()

    def select_each():
        for v in inst:
            one[0] = v
            assert lib.rs_hip_select_by_ids(ids.ctypes.data, n, one.ctypes.data, 1, index.ctypes.data, C.byref(count)) == 0

    def one_pass():
        assert lib.rs_hip_split_by_instance(ids.ctypes.data, n, out_inst.ctypes.data, off.ctypes.data, order.ctypes.data, C.byref(k)) == 0

    def one_pass_sort():
        before = capi.split_lds_ranks(0)
        try:
            one_pass()
        finally:
            capi.split_lds_ranks(before)

    def table_only():
        assert lib.rs_hip_instance_table(ids.ctypes.data, n, out_inst.ctypes.data, None, None, C.byref(k)) == 0
    r = interleaved({"(b) select_by_ids per instance": select_each, "one pass, LDS route": one_pass, "(e) one pass, sort route": one_pass_sort, "table alone": table_only})
    print(f"partition, {n} points, {len(inst)} instances (uploads and the download of order included): {fmt(r)}", flush=True)
    (mb, qb), (ma, qa) = r["(b) select_by_ids per instance"], r["one pass, LDS route"]
    holds = mb - ma > 2.0 * max(qa, qb)
    print(f"claim: the one-pass partition is faster than one select per instance by more than twice the larger interquartile range: "
          f"{mb:.3f} - {ma:.3f} = {mb - ma:.3f} ms against 2 x {max(qa, qb):.3f} ms: {'HOLDS' if holds else 'DOES NOT HOLD'}", flush=True)


def step_objects():
    from rescan_amd import capi
    capi.init(0)
    lib = capi.load()
    s = room(); n = len(s["pos"])
    ins = (s["pos"].ctypes.data, s["nor"].ctypes.data, s["cls"].ctypes.data, s["inst"].ctypes.data)
    k, a, out = packed(capi, n, 4096, True)
    k2, a2, out2 = packed(capi, n, 4096, False)
    scan = capi.Cloud(s["pos"], s["nor"])
    handles = (C.c_void_p * 4096)()

    def arrays():
        assert lib.rs_hip_scan_to_objects(*ins, n, s["static"].ctypes.data, len(s["static"]), C.addressof(out)) == 0

    def clouds():
        assert lib.rs_hip_cloud_split_objects(scan.handle, s["cls"].ctypes.data, s["inst"].ctypes.data, s["static"].ctypes.data, len(s["static"]), -1.0,
                                              C.addressof(handles), C.addressof(out2)) == 0
        for j in range(k2.value):
            lib.rs_hip_cloud_destroy(handles[j])
    capi.split_seconds(False)
    r = interleaved({"(a) scan_to_objects": arrays, "(a) cloud_split_objects": clouds}, repeats=5)
    print(f"objects, {n} points, {k.value} instances ({int(a['is_static'][:k.value].sum())} static): {fmt(r)}", flush=True)
    print(f"(d) addends the chains took one by one: {capi.split_chains_sequential()} of {3 * n}", flush=True)
    for name, f in (("scan_to_objects", arrays), ("cloud_split_objects", clouds)):
        capi.split_seconds(True)
        laps = []
        for _ in range(5):
            f(); laps.append(capi.split_seconds(True))
        capi.split_seconds(False)
        lap = 1e3 * np.median(np.array(laps), axis=0)
        print(f"(a) {name}, a synchronisation after every stage: table {lap[0]:.3f} | partition {lap[1]:.3f} | chains {lap[2]:.3f} | "
              f"transform and copies {lap[3]:.3f} | index builds {lap[4]:.3f} ms (uploads are in the first stage that waits for them)", flush=True)


def step_chains():
    from rescan_amd import capi
    capi.init(0)
    lib = capi.load()
    s = room(); n = len(s["pos"])
    inst, off, order = capi.split_by_instance(s["inst"])
    sums = np.zeros((len(inst), 3)); longest = int(np.diff(off).max())

    def call():
        assert lib.rs_hip_segment_centroids(s["pos"].ctypes.data, n, order.ctypes.data, off.ctypes.data, len(inst), sums.ctypes.data, None) == 0

    def lone():
        before = capi.split_chains_form(1)
        try:
            call()
        finally:
            capi.split_chains_form(before)

    def empty():                                                      # the same uploads with chains of no addends: what the copies cost
        z = np.zeros(len(off), np.int64)
        assert lib.rs_hip_segment_centroids(s["pos"].ctypes.data, n, order.ctypes.data, z.ctypes.data, len(inst), sums.ctypes.data, None) == 0
    r = interleaved({"block steps": call, "a lone lane per chain": lone, "the upload of positions alone": empty}, repeats=5, warmup=1)
    print(f"(d) chains alone, {len(inst)} instances, the longest {longest} points (the upload of positions and order included): {fmt(r)}", flush=True)


def step_plan():
    from rescan_amd import capi
    lib = capi.load()
    s = room(); n = len(s["pos"])
    ins = (s["pos"].ctypes.data, s["nor"].ctypes.data, s["cls"].ctypes.data, s["inst"].ctypes.data)
    k, a, out = packed(capi, n, 4096, True)

    def plan():
        assert lib.rs_hip_split_plan(*ins, n, s["static"].ctypes.data, len(s["static"]), C.addressof(out)) == 0
    r = interleaved({"(c) split_plan on the host": plan}, repeats=5, warmup=1)
    print(f"plan, {n} points, {k.value} instances: {fmt(r)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step:
        return dict(partition=step_partition, objects=step_objects, chains=step_chains, plan=step_plan)[a.step]()
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
            f.write(f"tools/split_timing.py: medians and interquartile ranges of interleaved timed rounds after warm-up rounds\n" + "".join(lines))


if __name__ == "__main__":
    main()
