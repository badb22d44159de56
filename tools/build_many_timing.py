"""Times the batched index build (capi.Cloud.many, rs_hip_cloud_create_many) against one capi.Cloud per cloud, on rescan_amd/synth.py
objects sampled to a given number of points:

    K = 1, 4, 16, 64, 1024 clouds  x  1 000, 50 000, 500 000 points per cloud (1024 x 500 000 is beyond memory and skipped)

    python tools/build_many_timing.py [--out profiles/r25/build_many_timing.txt]

Per case, after WARMUP untimed rounds, REPEATS rounds in which the two routes take turns (interleaved, one process); medians and
interquartile ranges of the host clock around the create calls (synchronous C ABI) and, separately, around the destroy calls; then the
laps of rs_hip_cloud_build_seconds per route.  Every size is a child process under its own `timeout`; the first that fails ends the run.
The last line per size says whether the batch beat the single builds at K = 16 (the rule of rs_hip_cloud_many_single_above's default:
the median is lower and the interquartile ranges do not overlap the other way)."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPEATS = 1, 7
KS = (1, 4, 16, 64, 1024)
SIZES = ((1_000, 300), (50_000, 600), (500_000, 900))          # (points per cloud, time limit of the step in seconds)
TOO_LARGE = 200_000_000                                         # points in one batch


def objects(n):
    """the four synth objects, each sampled to exactly n points (a denser surface for more points, then a random subset)"""
    from rescan_amd import synth
    out = []
    for k, kind in enumerate(synth.OBJECT_MAKERS):
        density = synth.DENSITY
        while True:
            p, q = synth.make_object(kind, 100 + k, density=density)
            if len(p) >= n:
                break
            density *= max(1.5, 1.2 * n / len(p))
        keep = np.sort(np.random.default_rng(k).choice(len(p), n, replace=False))
        out.append((np.ascontiguousarray(p[keep]), np.ascontiguousarray(q[keep])))
    return out


def stats(v):
    return float(np.median(v)), float(np.percentile(v, 75) - np.percentile(v, 25))


def step(n):
    from rescan_amd import capi
    capi.init(0)
    capi.cloud_many_single_above(2 ** 31 - 1)          # every size through the batch: the default of this setter is what is being measured
    objs = objects(n)
    verdict = None
    for K in KS:
        if K * n > TOO_LARGE:
            print(f"n = {n:7d}  K = {K:5d}: skipped, {K * n} points are beyond memory", flush=True)
            continue
        pairs = [objs[k % len(objs)] for k in range(K)]

        def many():
            t0 = time.perf_counter(); clouds = capi.Cloud.many(pairs); t1 = time.perf_counter()
            for c in clouds:
                c.close()
            return t1 - t0, time.perf_counter() - t1

        def singles():
            t0 = time.perf_counter(); clouds = [capi.Cloud(p, q) for p, q in pairs]; t1 = time.perf_counter()
            for c in clouds:
                c.close()
            return t1 - t0, time.perf_counter() - t1
        routes = {"many": many, "singles": singles}
        ts = {k: [] for k in routes}
        laps = {}
        repeats = REPEATS if K * n <= 20_000_000 else 3
        for r in range(WARMUP + repeats):
            for k, f in routes.items():
                capi.cloud_build_seconds(True)
                dt = f()
                if r >= WARMUP:
                    ts[k].append([1e3 * x for x in dt])
                    laps.setdefault(k, []).append(capi.cloud_build_seconds(True)[0])
        res = {k: (stats([a for a, _ in v]), stats([b for _, b in v])) for k, v in ts.items()}
        (mm, mq), (sm, sq) = res["many"][0], res["singles"][0]
        print(f"n = {n:7d}  K = {K:5d}: create many {mm:9.3f} ms (IQR {mq:.3f}) | singles {sm:9.3f} ms (IQR {sq:.3f}) | x{sm / mm:5.2f}"
              f" || destroy many {res['many'][1][0]:8.3f} ms (IQR {res['many'][1][1]:.3f}) | singles {res['singles'][1][0]:8.3f} ms (IQR {res['singles'][1][1]:.3f})", flush=True)
        for k in routes:
            lap = 1e3 * np.median(np.array(laps[k]), axis=0)
            print(f"             laps, {k:7s}: host copy {lap[0]:.3f} | upload + bounds {lap[1]:.3f} | cell index {lap[2]:.3f} | Hilbert order + tiles {lap[3]:.3f} ms", flush=True)
        if K == 16:
            verdict = mm + mq / 2 < sm - sq / 2              # (the ranges taken as centred on their medians)
    print(f"n = {n:7d}: at K = 16 the batch {'beats' if verdict else 'DOES NOT beat'} the single builds", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step:
        return step(a.step)
    lines = []
    for n, limit in SIZES:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", str(n)], capture_output=True, text=True)
        sys.stdout.write(r.stdout); sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            print(f"step {n} ended with status {r.returncode}: stopping", flush=True)
            sys.exit(1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/build_many_timing.py: medians and interquartile ranges of interleaved timed rounds after a warm-up round\n" + "".join(lines))


if __name__ == "__main__":
    main()
