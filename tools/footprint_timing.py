"""Times of the coverage term as the simulated-annealing loop would ask for it, on the room of tests/golden/scene.npz at 5 cm (the
inputs of tools/arrange_timing.py): 256 candidate placements plus 8 base placements, and a fixed, seeded list of 25 000 arrangements
of 8 placements, each differing from its predecessor by one or two swapped members — the loop's shape, not its actions.

  (a) rs_hip_coverage_footprints over the 264 placements, once: the whole call on the host clock, its kernels by ProfSpan
      ("footprints"), the placements per route;
  (b) the 25 000 arrangements through rs_hip_footprints_scores, one arrangement per call;
  (c) the same 25 000 through rs_hip_coverage_scores, one arrangement per call: what the library offered the loop before.

(b) and (c) must agree bit for bit on every arrangement before anything is timed.  Both are called through the C ABI with their
arguments packed once.  They run in interleaved blocks of --block arrangements; per form the block times give the median and the
interquartile range per arrangement and, scaled, per 25 000.  The claim on trial: (a) + (b) is below (c) by more than twice the
larger interquartile range.  The outcome is written down either way.

    python tools/footprint_timing.py [--arrangements 25000] [--block 500] [--repeats 20] [--reference-us US] [--out profiles/r18/footprint_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rescan_amd import capi  # noqa: E402
import arrange_timing  # noqa: E402
import footprint_restate as FR  # noqa: E402

F = np.float32


def arrangement_list(n_arr, n_plc, size, seed):
    """int32 [n_arr, size]: distinct members per arrangement; each row swaps one or two members of the row before for placements not in it."""
    rng = np.random.default_rng(seed)
    cur = rng.choice(n_plc, size, replace=False)
    out = np.zeros((n_arr, size), np.int32)
    for a in range(n_arr):
        prev = cur.copy()
        slots = rng.choice(size, int(rng.integers(1, 3)), replace=False)
        for slot in slots:
            new = int(rng.integers(0, n_plc))
            while new in cur or new in prev:
                new = int(rng.integers(0, n_plc))
            cur[slot] = new
        out[a] = cur
    return out


def quartiles(x):
    x = np.asarray(x)
    return float(np.median(x)), float(np.percentile(x, 75) - np.percentile(x, 25))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arrangements", type=int, default=25000)
    ap.add_argument("--block", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=20, help="timed repetitions of the footprint call")
    ap.add_argument("--reference-us", type=float, default=None, help="context only: the reference's own coverage score per arrangement on some CPU, microseconds")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    capi.init(0)
    lib = capi.load()
    pts, lo, hi, objs, base, cand, _ = arrange_timing.inputs()
    clouds = [capi.Cloud(o) for o in objs]
    cov = capi.Coverage(lo, hi, pts, None, 0.05)
    plc = [(o, p, 0) for o, p in cand] + list(base)                                 # 256 candidates, then the 8 base placements
    P = [(clouds[o], p, s) for o, p, s in plc]
    n = len(P)
    arr = arrangement_list(a.arrangements, n, 8, 1806)
    # arguments packed once
    objs_c = (C.c_void_p * n)(*[x[0].handle for x in P])
    poses = np.ascontiguousarray([np.asarray(x[1], F).ravel() for x in P], F)
    stat = np.zeros(n, np.int32)

    def footprints():
        h = lib.rs_hip_coverage_footprints(cov.handle, C.addressof(objs_c), poses.ctypes.data, stat.ctypes.data, n)
        assert h, lib.rs_hip_last_error()
        return h
    capi.coverage_footprint_routes(reset=True)
    fh = footprints()                                                                 # warm-up, and the handle (b) scores with
    n_lds, n_slab = capi.coverage_footprint_routes()
    fp = capi.Footprints(fh)                                                          # (owns the handle from here on)
    grid = cov.scene_grid()
    want = [FR.footprint(grid, lo, hi, 0.05, objs, p) for p in plc]
    assert all(fp.cells(k).tolist() == want[k].tolist() for k in range(n)), "the footprints disagree with the restatement"
    need = np.array([FR.footprint_box_bytes(grid, lo, hi, 0.05, objs, p) for p in plc])
    sizes = np.diff(fp.offsets)

    # (c)'s arguments per arrangement: pointers into arrays made once
    first2 = np.array([0, 8], np.int32)
    stat8 = np.zeros(8, np.int32)
    obj_rows = [(C.c_void_p * 8)(*[P[m][0].handle for m in row]) for row in arr]
    pose_rows = np.ascontiguousarray(poses[arr.ravel()].reshape(len(arr), 8 * 16))
    sc_b, ag_b = np.zeros(len(arr), F), np.zeros(len(arr), np.int32)
    sc_c, ag_c = np.zeros(len(arr), F), np.zeros(len(arr), np.int32)
    mem_p, first_p = arr.ctypes.data, first2.ctypes.data
    scb_p, agb_p, scc_p, agc_p, pose_p, stat_p = sc_b.ctypes.data, ag_b.ctypes.data, sc_c.ctypes.data, ag_c.ctypes.data, pose_rows.ctypes.data, stat8.ctypes.data
    f_scores, c_scores = lib.rs_hip_footprints_scores, lib.rs_hip_coverage_scores
    c_scores.argtypes = [C.c_void_p] * 5 + [C.c_int32] + [C.c_void_p] * 2           # (raw addresses: no array checks inside the timed loop)
    obj_p = [C.addressof(o) for o in obj_rows]

    def run_b(i0, i1):
        for i in range(i0, i1):
            f_scores(fh, mem_p + 32 * i, first_p, 1, scb_p + 4 * i, agb_p + 4 * i)

    def run_c(i0, i1):
        for i in range(i0, i1):
            c_scores(cov.handle, obj_p[i], pose_p + 512 * i, stat_p, first_p, 1, scc_p + 4 * i, agc_p + 4 * i)
    blocks = [(i, min(i + a.block, len(arr))) for i in range(0, len(arr), a.block)]
    for b in blocks:                                                                  # the check, and the warm-up of both
        run_b(*b); run_c(*b)
    assert (ag_b == ag_c).all() and (sc_b.view(np.uint32) == sc_c.view(np.uint32)).all(), "the two routes disagree"
    t_b, t_c = [], []
    for b in blocks:                                                                  # interleaved blocks
        t0 = time.perf_counter(); run_b(*b); t1 = time.perf_counter(); run_c(*b); t2 = time.perf_counter()
        t_b.append((t1 - t0) / (b[1] - b[0])); t_c.append((t2 - t1) / (b[1] - b[0]))
    assert (ag_b == ag_c).all() and (sc_b.view(np.uint32) == sc_c.view(np.uint32)).all()
    # the empty ctypes loop, for context: what of (b) is the caller's own overhead
    noop = lib.rs_hip_coverage_lds_budget
    t0 = time.perf_counter()
    for i in range(a.block):
        noop(-1)
    t_call = (time.perf_counter() - t0) / a.block

    # (a): the call, repeated; then once more under the profiler for the kernels' own time
    t_a = []
    for _ in range(a.repeats):
        t0 = time.perf_counter(); h = footprints(); t_a.append(time.perf_counter() - t0)
        lib.rs_hip_footprints_destroy(h)
    capi.profile_enable(True)
    capi.profile_reset(); lib.rs_hip_footprints_destroy(footprints()); k_a = capi.profile_read("footprints")
    capi.profile_reset(); run_c(0, 100); k_c = capi.profile_read("coverage")
    capi.profile_enable(False)

    n_arr = len(arr)
    (mb, qb), (mc, qc), (ma, qa) = quartiles(t_b), quartiles(t_c), quartiles(t_a)
    total_new, total_old = ma + n_arr * mb, n_arr * mc
    spread = n_arr * max(qb, qc)
    holds = total_old - total_new > 2.0 * spread
    changed = (arr[1:, None, :] != arr[:-1, :, None]).all(1).sum(1) if n_arr > 1 else np.zeros(1)
    lines = [f"footprint timing, {lib.rs_hip_version().decode()}",
             f"room: {len(pts)} scan points, grid {cov.res.tolist()} at 0.05 = {cov.n_cells} cells, {cov.valid_cells} valid; objects of {[len(o) for o in objs]} points",
             f"placements: 256 candidates + 8 base = {n}; footprints hold {int(sizes.min())}-{int(sizes.max())} cells (median {int(np.median(sizes))}, {int(sizes.sum())} in all); "
             f"sub-boxes 0-{int(need.max())} B (median {int(np.median(need))} B)",
             f"arrangements: {n_arr} of 8 placements, seeded; {int(changed.min())}-{int(changed.max())} members differ from the arrangement before; "
             f"agreeing cells {int(ag_b.min())}-{int(ag_b.max())}; every count and every score bit equal on both routes, checked before and after timing",
             "host clock around synchronous C ABI calls made from Python (ctypes), arguments packed once",
             f"(a) rs_hip_coverage_footprints, {n} placements, {a.repeats} calls after one warm-up:",
             f"      whole call      median {1e3 * ma:8.3f} ms   iqr {1e3 * qa:.3f} ms   min {1e3 * min(t_a):.3f}   max {1e3 * max(t_a):.3f}",
             f"      kernels         {k_a[1]:.3f} ms in {k_a[0]} spans (k_footprint<LDS>, k_footprint_pack; k_footprint<slab> and a second pack when a placement overflows)",
             f"      routes          {n_lds} LDS, {n_slab} slab",
             f"(b) rs_hip_footprints_scores, one arrangement per call, {len(blocks)} blocks of {a.block}, interleaved with (c):",
             f"      per arrangement median {1e6 * mb:8.3f} us   iqr {1e6 * qb:.3f} us      per {n_arr}: {1e3 * n_arr * mb:10.2f} ms   iqr {1e3 * n_arr * qb:.2f} ms",
             f"      (for scale: a one-argument ctypes call of the same library that only reads a setting takes {1e6 * t_call:.3f} us here)",
             "(c) rs_hip_coverage_scores, one arrangement per call (upload, plane clear, launch, blocking read-back each):",
             f"      per arrangement median {1e6 * mc:8.3f} us   iqr {1e6 * qc:.3f} us      per {n_arr}: {1e3 * n_arr * mc:10.2f} ms   iqr {1e3 * n_arr * qc:.2f} ms",
             f"      kernels         {k_c[1] / max(1, k_c[0]) * 1e3:.1f} us per arrangement ({k_c[0]} spans)",
             f"claim: (a) + (b) = {1e3 * total_new:.2f} ms against (c) = {1e3 * total_old:.2f} ms per {n_arr} arrangements; difference {1e3 * (total_old - total_new):.2f} ms, "
             f"twice the larger interquartile range {1e3 * 2 * spread:.2f} ms: the claim {'HOLDS' if holds else 'DOES NOT HOLD'} (ratio {total_old / total_new:.1f})"]
    if a.reference_us is not None:
        lines.append(f"context only (a CPU of another host, one thread, not this measurement): the reference's rsao__compute_scene_coverage_score takes {a.reference_us:.1f} us per arrangement "
                     f"(tools/arrange_fixture/gen.py --time), {1e-3 * a.reference_us * n_arr:.1f} ms per {n_arr}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
