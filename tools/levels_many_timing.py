"""Times the batched level builder (capi.Cloud.levels_many, rs_hip_cloud_create_levels_many) against the composed route, a loop of
capi.Cloud.level_of over the same bases and levels, on the GPU:

    16 bases of 1 000 points | 16 bases of 50 000 points | 1 base of 1 000 000 points | 2 bases of 1 000 000 points
    each on levels 1-4 and on levels (4, 3, 2) alone

    python tools/levels_many_timing.py [--out profiles/r27/levels_many_timing.txt] [--lib rescan_amd/librescan_hip_<tag>.so]

A base is a gently curved sheet sampled uniformly at 10 000 points per square metre, in random order: about 3 points within level 1's
radius and about 200 within level 4's, as a level-0 model of the reference has, and every level's cap holds.  Per case, after WARMUP
untimed turns, ROUNDS rounds of REPEATS turns in which the two routes alternate in one process; per round the median and the range of
the host clock around the calls (synchronous C ABI; the clouds are destroyed outside the clock).  Then, with profiling on, the laps of
both routes from the library's own spans.  Every size is a child process under its own `timeout`; the first that fails ends the run.

--lib: the library the children load (RS_HIP_LIB).  A base above rs_levels.h's SINGLE_ABOVE takes the single call's path inside the
one call, so what the batch itself does at 1 000 000 points shows only in a library built with a larger constant
(tools/variant.sh <tag> -DRS_LEVELS_SINGLE_ABOVE=<points>); the output names the library it ran."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, ROUNDS, REPEATS = 1, 3, 5
SIZES = ((16, 1_000, 300), (16, 50_000, 600), (1, 1_000_000, 900), (2, 1_000_000, 900))       # (bases, points per base, time limit in seconds)
LEVEL_SETS = ((1, 2, 3, 4), (4, 3, 2))
VOXEL = (0.005, 0.01, 0.02, 0.04, 0.08)                         # rs_pointcloud.h:148
DENSITY = 10_000.0                                              # points per square metre


def cap_of(level):
    m = int(np.float32(1024) * (np.float32(level) / np.float32(4)))      # rs_pointcloud.h:995-996
    return m if m else 256


def sheet(n, seed):
    """n points of a curved sheet of n / DENSITY square metres with unit normals, in random order"""
    rng = np.random.default_rng(seed)
    side = float(np.sqrt(n / DENSITY))
    x, y = rng.uniform(0, side, n), rng.uniform(0, side, n)
    z = 0.05 * np.sin(3.0 * x + seed) * np.cos(2.0 * y)
    nor = np.stack([-0.15 * np.cos(3.0 * x + seed) * np.cos(2.0 * y), 0.10 * np.sin(3.0 * x + seed) * np.sin(2.0 * y), np.ones(n)], 1)
    nor /= np.linalg.norm(nor, axis=1, keepdims=True)
    return np.ascontiguousarray(np.stack([x, y, z], 1), np.float32), np.ascontiguousarray(nor, np.float32)


SPANS = {"one call": ("levels_neighbours", "levels_rounds", "levels_samples", "levels_build"),
         "composed": ("level_neighbours", "level_rounds")}


def step(K, n):
    from rescan_amd import capi
    capi.init(0)
    print(f"library {os.path.relpath(os.environ.get('RS_HIP_LIB', capi.LIB_PATH), ROOT)}", flush=True)
    bases = [capi.Cloud(*sheet(n, 7 + k)) for k in range(K)]
    for numbers in LEVEL_SETS:
        levels = [(VOXEL[lv], cap_of(lv)) for lv in numbers]

        def one_call():
            t0 = time.perf_counter(); made = capi.Cloud.levels_many(bases, levels); dt = time.perf_counter() - t0
            sizes = [[c.n for c, _ in row] for row in made]
            for row in made:
                for c, _ in row:
                    c.close()
            return dt, sizes

        def composed():
            t0 = time.perf_counter(); made = [[capi.Cloud.level_of(b, r, cap) for r, cap in levels] for b in bases]; dt = time.perf_counter() - t0
            sizes = [[c.n for c, _ in row] for row in made]
            for row in made:
                for c, _ in row:
                    c.close()
            return dt, sizes
        routes = {"one call": one_call, "composed": composed}
        for _ in range(WARMUP):
            a, b = one_call()[1], composed()[1]
            assert a == b, "the two routes made levels of different sizes"
        head = f"{K:2d} x {n:7d} points, levels {numbers}"
        wins = 0
        for rnd in range(ROUNDS):
            ts = {k: [] for k in routes}
            for r in range(REPEATS):
                for k, f in (list(routes.items()) if r % 2 == 0 else list(routes.items())[::-1]):
                    ts[k].append(1e3 * f()[0])
            m = {k: float(np.median(v)) for k, v in ts.items()}
            wins += m["one call"] < m["composed"]
            print(f"{head}, round {rnd + 1}: one call {m['one call']:9.3f} ms ({min(ts['one call']):.3f} .. {max(ts['one call']):.3f}) | "
                  f"composed {m['composed']:9.3f} ms ({min(ts['composed']):.3f} .. {max(ts['composed']):.3f}) | x{m['composed'] / m['one call']:5.2f}", flush=True)
        print(f"{head}: the one call's median is below the composed route's in {wins} of {ROUNDS} rounds", flush=True)
        # the laps, in turns of their own: profiling costs host time
        capi.profile_enable(True)
        for k, f in routes.items():
            capi.profile_reset(); capi.cloud_build_seconds(True)
            t0 = time.perf_counter(); f(); capi.synchronize()
            laps = {s: capi.profile_read(s) for s in SPANS[k]}
            build = 1e3 * float(np.sum(capi.cloud_build_seconds(True)[0]))
            text = " | ".join(f"{s} {ms:.3f} ms in {cnt} spans" for s, (cnt, ms) in laps.items())
            print(f"{head}: laps, {k}: {text} | index build (host clock of its stages) {build:.3f} ms", flush=True)
        capi.profile_enable(False)
    for b in bases:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, nargs=2)
    ap.add_argument("--only", type=int, nargs=2, action="append", help="bases and points of a size to run (default: all)")
    ap.add_argument("--lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step:
        return step(*a.step)
    env = dict(os.environ)
    if a.lib:
        env["RS_HIP_LIB"] = os.path.abspath(a.lib)
    lines = []
    for K, n, limit in SIZES:
        if a.only and [K, n] not in a.only:
            continue
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", str(K), str(n)], capture_output=True, text=True, env=env)
        sys.stdout.write(r.stdout); sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            print(f"step {K} x {n} ended with status {r.returncode}: stopping", flush=True)
            sys.exit(1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("tools/levels_many_timing.py: per round the median (and range) of interleaved timed turns after a warm-up turn\n" + "".join(lines))


if __name__ == "__main__":
    main()
