"""msh_hash_grid_knn_search at scan size: ~1 M queries (the points, jittered by 5 mm) against a 1 M-point synthetic room, radius 0.02
(the reference's grid: 4 cm bins), k in {1, 8, 32, 64}.  Queries per second of the shim's device route (librescan_dropin.so, host
arrays in and out, the device grid already built), of the native entry point rs_hip_knn_search on a resident grid, and of the shim's
host route (KnnGrid, one thread) on a 50 000-query sample.

  python tools/knn_timing.py                  the table
  python tools/knn_timing.py --rocprof DIR    the device calls again in a child process under rocprofv3 --kernel-trace --stats
                                              (output in DIR), and the average k_knn kernel time per k from its kernel statistics"""
import ctypes as C, csv, glob, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

KS = (1, 8, 32, 64)
RADIUS = 0.02
HOST_SAMPLE = 50_000


def workload():
    from rescan_amd import synth
    s = synth.scene_for_point_count(1_000_000, seed=11)
    pts = np.ascontiguousarray(s["points"], np.float32)
    q = (pts + np.random.default_rng(0).normal(0, 0.005, pts.shape)).astype(np.float32)
    return pts, q


def device_calls(pts, q, repeat):
    """(k, seconds per shim call, seconds per native call) per k; the shim's first call (device grid build) is not timed."""
    from rescan_amd import capi
    from test_gpu_knn import HashGrid, SearchDesc, _lib, DROPIN
    capi.init(0)
    shim = _lib(DROPIN)
    os.environ.pop("RS_DROPIN_HOST_QUERIES", None)
    hg = HashGrid()
    shim.msh_hash_grid_init_3d(C.byref(hg), pts.ctypes.data, len(pts), RADIUS)
    cloud = capi.Cloud(pts)
    grid = capi.KnnGrid(cloud, RADIUS)
    out = []
    for k in KS:
        d = np.zeros((len(q), k), np.float32); i = np.zeros((len(q), k), np.int32); nn = np.zeros(len(q), np.uint64)
        sd = SearchDesc(q.ctypes.data, len(q), d.ctypes.data, i.ctypes.data, nn.ctypes.data, RADIUS, k, 1)
        shim.msh_hash_grid_knn_search(C.byref(hg), C.byref(sd))
        ts = []
        for _ in range(repeat):
            t = time.perf_counter(); shim.msh_hash_grid_knn_search(C.byref(hg), C.byref(sd)); ts.append(time.perf_counter() - t)
        tot = C.c_uint64(); lib = capi.load()
        tn = []
        for _ in range(repeat):
            t = time.perf_counter(); lib.rs_hip_knn_search(grid.handle, q, len(q), k, d, i, nn, C.byref(tot)); tn.append(time.perf_counter() - t)
        out.append((k, float(np.median(ts)), float(np.median(tn))))
    shim.msh_hash_grid_term(C.byref(hg))
    return out


def host_calls(pts, q):
    from test_gpu_knn import HashGrid, SearchDesc, _lib, DROPIN
    shim = _lib(DROPIN)
    sq = np.ascontiguousarray(q[np.random.default_rng(1).choice(len(q), HOST_SAMPLE, replace=False)])
    os.environ["RS_DROPIN_HOST_QUERIES"] = str(len(sq) + 1)
    hg = HashGrid()
    shim.msh_hash_grid_init_3d(C.byref(hg), pts.ctypes.data, len(pts), RADIUS)
    out = {}
    for k in KS:
        d = np.zeros((len(sq), k), np.float32); i = np.zeros((len(sq), k), np.int32); nn = np.zeros(len(sq), np.uint64)
        sd = SearchDesc(sq.ctypes.data, len(sq), d.ctypes.data, i.ctypes.data, nn.ctypes.data, RADIUS, k, 1)
        t = time.perf_counter(); shim.msh_hash_grid_knn_search(C.byref(hg), C.byref(sd)); out[k] = time.perf_counter() - t
    shim.msh_hash_grid_term(C.byref(hg))
    os.environ.pop("RS_DROPIN_HOST_QUERIES")
    return out


def main():
    if "--device-only" in sys.argv:
        pts, q = workload()
        device_calls(pts, q, 3)
        return
    if "--rocprof" in sys.argv:
        outdir = sys.argv[sys.argv.index("--rocprof") + 1]
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "knn", "--", sys.executable, os.path.abspath(__file__), "--device-only"]
        print(" ".join(cmd[:-3] + ["python", "tools/knn_timing.py", "--device-only"]), flush=True)
        subprocess.run(cmd, check=True, timeout=900)
        files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            sys.exit("no kernel_stats.csv under " + outdir)
        for row in csv.DictReader(open(files[0])):
            if "knn" in row["Name"]:
                print(f"{row['Name'][:60]:60s} calls {int(row['Calls']):4d}  average {float(row['AverageNs']) / 1e6:8.3f} ms  "
                      f"min {float(row['MinNs']) / 1e6:8.3f} ms  max {float(row['MaxNs']) / 1e6:8.3f} ms")
        # per k: every search call launches k_knn once per chunk of queries (rs_hip_knn_search: ~32 MB of rows per chunk); 7 calls per k
        trace = glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True)
        if trace:
            rows = [r for r in csv.DictReader(open(trace[0])) if r["Kernel_Name"].split("(")[0].endswith("k_knn")]
            rows.sort(key=lambda r: int(r["Start_Timestamp"]))
            nq = len(workload()[1])
            at = 0
            for k in KS:
                chunks = -(-nq // max(1024, (32 << 20) // (8 * k)))
                part = rows[at:at + 7 * chunks]; at += 7 * chunks
                ns = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in part)
                print(f"k = {k:2d}: k_knn {ns / 7 / 1e6:8.3f} ms per ~1 M-query call ({chunks} launch(es) per call, {len(part)} launches traced)")
        return
    pts, q = workload()
    print(f"{len(q)} queries x {len(pts)} points, radius {RADIUS} (the reference's grid: {2 * RADIUS} m bins), host arrays in and out")
    host = host_calls(pts, q)
    for k, t_shim, t_nat in device_calls(pts, q, 5):
        qh = HOST_SAMPLE / host[k]
        print(f"k = {k:2d}: device (shim) {t_shim * 1e3:8.2f} ms/call {len(q) / t_shim / 1e6:7.2f} Mq/s | native {t_nat * 1e3:8.2f} ms/call "
              f"{len(q) / t_nat / 1e6:7.2f} Mq/s | host (KnnGrid, {HOST_SAMPLE} sample) {qh / 1e6:7.3f} Mq/s | device / host {len(q) / t_shim / qh:7.1f}x")


if __name__ == "__main__":
    main()
