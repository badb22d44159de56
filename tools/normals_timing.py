"""Time of the vertex normals on the mesh of tools/resample_timing.py (tests/hard_meshes.py: big(), about 1 M vertices and 2 M faces).
Recorded, not asserted: the call did not exist before.  After a warm-up round, --repeats rounds; each round runs, in this order,
  vertex_normals      rs_hip_vertex_normals with the loader's pass, to host arrays: the whole call on the host clock, and its three
                      stages from the library's event timing (face cross, corner grouping = sort + span starts, chains)
  Cloud.from_mesh     positions and faces up, normals on the device, sampled and indexed there
  Cloud.resampled     the same mesh with host-supplied normals (the loader-pass normals, computed before the clock starts)
so the two cloud calls are interleaved in one run.  Host clock around the synchronous calls; medians and interquartile ranges.
from_mesh minus resampled is what the device normals cost net of the 12 bytes per vertex they no longer upload — not what a caller
without this call pays, who also runs the reference's face loop on the host (tools/normals_fixture/gen.py --time prints its time).
--append FILE: text added to the report as it is (the kernels' registers from tools/kernel_meta.py, the reference's CPU time).

    python tools/normals_timing.py [--repeats 7] [--append notes.txt] [--out profiles/r13/normals_timing.txt]
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

STAGES = (("normals_cross", "k_face_cross (cross products, corner list)"), ("normals_group", "corner grouping (radix sort, span starts)"),
          ("normals_chain", "k_vertex_chain (chains, finish, loader pass)"))


def stats(v, scale=1e3):
    q1, q2, q3 = np.percentile(np.asarray(v) * scale, [25, 50, 75])
    return f"{q2:9.3f}   iqr {q3 - q1:7.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--append", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5
    capi.init(0)
    m = H.big()
    pos, faces = m["pos"], m["faces"]
    nor = capi.vertex_normals(pos, faces, True)
    stage = {k: [] for k, _ in STAGES}
    whole, from_mesh, resampled = [], [], []
    n = None
    for r in range(a.repeats + 1):
        capi.profile_enable(True); capi.profile_reset()
        t0 = time.perf_counter(); got = capi.vertex_normals(pos, faces, True); t_whole = time.perf_counter() - t0
        ms = {k: capi.profile_read(k)[1] for k, _ in STAGES}
        capi.profile_enable(False)
        assert got.tobytes() == nor.tobytes()
        t0 = time.perf_counter(); x = capi.Cloud.from_mesh(pos, faces); t_from = time.perf_counter() - t0
        t0 = time.perf_counter(); y = capi.Cloud.resampled(pos, nor, faces); t_res = time.perf_counter() - t0
        assert x.n == y.n and x._nor.tobytes() == y._nor.tobytes() and x._pos.tobytes() == y._pos.tobytes()
        n = x.n
        x.close(); y.close()
        if r:                                         # the first round warms buffers and code objects up
            whole.append(t_whole); from_mesh.append(t_from); resampled.append(t_res)
            for k in ms: stage[k].append(ms[k] * 1e-3)
    diff = [f - s for f, s in zip(from_mesh, resampled)]
    lines = [f"vertex normals, {len(pos)} vertices, {len(faces)} faces, valence up to {int(np.bincount(faces.ravel()).max())}, {n} samples, "
             f"{capi.load().rs_hip_version().decode()}, {a.repeats} rounds after a warm-up, ms: median, interquartile range"]
    lines += [f"{label:52s}{stats(stage[k])}" for k, label in STAGES]
    lines += [f"{'rs_hip_vertex_normals to host arrays, whole call':52s}{stats(whole)}",
              f"{'Cloud.from_mesh, whole call':52s}{stats(from_mesh)}",
              f"{'Cloud.resampled with host normals, whole call':52s}{stats(resampled)}",
              f"{'from_mesh - resampled, per round':52s}{stats(diff)}"]
    text = "\n".join(lines) + "\n"
    if a.append:
        text += "\n" + open(a.append).read()
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
