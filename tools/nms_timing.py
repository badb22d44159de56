"""Time of rs_hip_nms for one object with 64, 256 and 1024 proposals (a chair: the level-1 / level-3 clouds and the centroid of
tests/golden/nms_chair.npz; proposals from rescan_amd.synth.nms_proposals( 7, n, span = 1.5 ), the inputs for which
tools/nms_fixture/gen.py prints the reference's CPU time).  Reports, per list: milliseconds per call (median of --repeats
after a warm-up call), pairs evaluated on the device, pairs settled without (cheap tests, disjoint boxes), rounds, kept
proposals, and the summed time of the "isect" kernels.  No oracle is involved.

    python tools/nms_timing.py [--repeats 5] [--out profiles/r07/nms_timing.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rescan_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    capi.init(0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "nms_chair.npz"))
    shape = (capi.Cloud(g["boundary"], None, 0.0), capi.Cloud(g["extent"], None, 0.0))
    lines = [f"rs_hip_nms, chair ({len(g['boundary'])} level-1 points, {len(g['extent'])} level-3 points), dist_threshold 0.2, {capi.load().rs_hip_version().decode()}",
             "proposals  ms/call  pairs_evaluated  pairs_skipped  rounds  kept  isect_kernels_ms  isect_launches"]
    for n in (64, 256, 1024):
        poses, scores = synth.nms_proposals(7, n, span=1.5)
        capi.nms(shape, g["centroid"], poses, scores, 0.2)                      # warm-up: buffers, code objects
        times = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            marks, keep, rounds = capi.nms(shape, g["centroid"], poses, scores, 0.2)
            times.append(time.perf_counter() - t0)
        capi.isect_pairs(reset=True)
        capi.profile_enable(True); capi.profile_reset()
        capi.nms(shape, g["centroid"], poses, scores, 0.2)
        launches, ms = capi.profile_read("isect")
        capi.profile_enable(False)
        ev, sk = capi.isect_pairs()
        lines.append(f"{n:9d}  {1e3 * float(np.median(times)):7.2f}  {ev:15d}  {sk:13d}  {rounds:6d}  {len(keep):4d}  {ms:16.2f}  {launches:14d}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
