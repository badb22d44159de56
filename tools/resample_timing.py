"""Time of the mesh resampler on a mesh of about 1 M vertices and 2 M faces (tests/hard_meshes.py: big(), ~1.1 M samples — the
mesh for which tools/resample_fixture/gen.py --time prints the reference's CPU time).  Recorded, not asserted.  Reports, as the
median of --repeats calls after a warm-up call:
  host plan           rs_hip_resample_plan with the alias table (areas, sums, the stack loop) — part of every call below
  k_mesh_sample       the kernel, from the library's event timing, for positions + normals (the cloud path) and for all attributes
  cloud index         the index build of the sampled cloud (rs_hip_cloud_build_seconds: host arrays, upload + bounds, cell index, Hilbert order + tiles)
  upload + rest       Cloud.resampled minus the three above: packing the 48-byte records, the three uploads, the points' copy to the host
  Cloud.resampled     the whole call
  uniform_resample    all six attributes to host arrays, the whole call
No oracle is involved.

    python tools/resample_timing.py [--repeats 5] [--out profiles/r09/resample_timing.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rescan_amd import capi  # noqa: E402
import hard_meshes as H  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    capi.init(0)
    m = H.big()
    med = lambda v: 1e3 * float(np.median(v))        # noqa: E731
    plan, whole, kern, index, attrs, kern_all = [], [], [], [], [], []
    for r in range(a.repeats + 1):
        t0 = time.perf_counter(); n = capi.resample_plan(m["pos"], m["faces"])[0]; t_plan = time.perf_counter() - t0
        capi.cloud_build_seconds(reset=True)
        capi.profile_enable(True); capi.profile_reset()
        t0 = time.perf_counter(); c = capi.Cloud.resampled(m["pos"], m["nor"], m["faces"]); t_whole = time.perf_counter() - t0
        _, ms = capi.profile_read("mesh_sample")
        secs, _ = capi.cloud_build_seconds()
        capi.profile_reset()
        t0 = time.perf_counter()
        capi.uniform_resample(m["pos"], m["faces"], m["nor"], m["col"], m["radii"], m["cls"], m["inst"])
        t_attrs = time.perf_counter() - t0
        _, ms_all = capi.profile_read("mesh_sample")
        capi.profile_enable(False)
        assert c.n == n
        c.close()
        if r:                                         # the first round warms buffers and code objects up
            plan.append(t_plan); whole.append(t_whole); kern.append(ms * 1e-3); index.append(sum(secs)); attrs.append(t_attrs); kern_all.append(ms_all * 1e-3)
    rest = [w - p - k - i for w, p, k, i in zip(whole, plan, kern, index)]
    lines = [f"mesh resampler, {len(m['pos'])} vertices, {len(m['faces'])} faces, {n} samples, {capi.load().rs_hip_version().decode()}, median of {a.repeats} calls, ms",
             f"host plan (areas, sums, alias table)            {med(plan):9.2f}",
             f"k_mesh_sample, positions + normals              {med(kern):9.3f}",
             f"k_mesh_sample, all attributes + face            {med(kern_all):9.3f}",
             f"cloud index (bounds, cells, Hilbert, tiles)     {med(index):9.2f}",
             f"upload + rest (records, uploads, host copy)     {med(rest):9.2f}",
             f"Cloud.resampled, whole call                     {med(whole):9.2f}",
             f"uniform_resample to host arrays, whole call     {med(attrs):9.2f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
