"""Times of the greedy step's coverage term and of the scene saliency on the room of tests/golden/scene.npz.

Extensions: C = 256 candidates (the room's objects on a 5 cm pose lattice) on a base of 8 placements, voxel 0.05 —
rs_hip_coverage_extensions against the only earlier way to the same numbers, rs_hip_coverage_scores with 256 arrangements of
9 placements.  Both forms are checked to agree bit for bit before anything is timed.  Per form: a warm-up call, then --repeats
calls of the C ABI (arguments packed once, so that the Python binding's packing is not counted) timed on the host around the synchronous call (perf_counter); median, minimum, maximum and the interquartile range are
reported, the two forms interleaved so that a drift of the machine hits both.  Also: workgroup size, LDS per workgroup, the bytes
of the sub-boxes actually used (tests/ao_restate.py: live_box_bytes), the share of candidates on the slab route, kernel time.
Saliency: rs_hip_scene_saliency at voxel 0.15 for 256 proposals; --reference-ms records the reference's own host time for the same
inputs where somebody measured it (context only: another machine).

    python tools/arrange_timing.py [--repeats 30] [--out profiles/r08/arrange_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rescan_amd import capi, synth  # noqa: E402
import ao_restate as R  # noqa: E402

F = np.float32


def inputs():
    d = np.load(os.path.join(ROOT, "tests", "golden", "scene.npz"))
    pts = np.ascontiguousarray(d["points"], F)
    objs = [np.ascontiguousarray(d[f"obj{i}_pos"], F)[::4] for i in range(int(d["n_obj"]))]       # (level-2-like density: every fourth model point)
    rng = np.random.default_rng(88)
    lo, hi = pts.min(0), pts.max(0)
    pose = lambda: synth.pose_matrix(F(rng.integers(0, 10)) * F(2.0 * np.pi / 10.0),  # noqa: E731
                                     (F(rng.integers(int(lo[0] / 0.05) + 8, int(hi[0] / 0.05) - 8)) * F(0.05), 0.0, F(rng.integers(int(lo[2] / 0.05) + 8, int(hi[2] / 0.05) - 8)) * F(0.05)))
    base = [(k % len(objs), d["obj_pose"][k % len(objs)] if k < len(objs) else pose(), 0) for k in range(8)]
    cand = [(int(rng.integers(0, len(objs))), pose()) for _ in range(256)]
    return pts, lo.astype(F), hi.astype(F), objs, base, cand, d["instance_idx"]


def stats(ts):
    ts = 1e3 * np.sort(np.asarray(ts))
    return f"median {np.median(ts):7.3f}  min {ts[0]:7.3f}  max {ts[-1]:7.3f}  iqr {np.percentile(ts, 75) - np.percentile(ts, 25):6.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--reference-ms", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    capi.init(0)
    pts, lo, hi, objs, base, cand, inst = inputs()
    clouds = [capi.Cloud(o) for o in objs]
    cov = capi.Coverage(lo, hi, pts, None, 0.05)
    b = [(clouds[o], p, s) for o, p, s in base]
    c = [(clouds[o], p) for o, p in cand]
    full = [b + [(cl, p, 0)] for cl, p in c]
    ext = lambda: cov.extensions(b, c)        # noqa: E731
    old = lambda: cov.scores(full)            # noqa: E731
    capi.coverage_extension_routes(reset=True)
    (s1, a1, _), (s0, a0) = ext(), old()      # warm-up of both, and the check
    n_lds, n_slab = capi.coverage_extension_routes()
    assert (a1 == a0).all() and (s1.view(np.uint32) == s0.view(np.uint32)).all(), "the two forms disagree"
    # the timed calls: the C ABI itself, arguments packed once (the Python binding's packing of 264 against 2304 placements is not the library's time)
    lib = capi.load()
    pack = lambda pl: ((C.c_void_p * len(pl))(*[x[0].handle for x in pl]), np.ascontiguousarray([np.asarray(x[1], F).ravel() for x in pl], F))  # noqa: E731
    (bo, bp), (co, cp), (fo, fp) = pack(b), pack(c), pack([x for arr in full for x in arr])
    bs, fs = np.zeros(len(b), np.int32), np.zeros(len(fo), np.int32)
    first = np.arange(0, len(fo) + 1, len(b) + 1, dtype=np.int32)
    sc1, ag1, ba1 = np.zeros(len(c), F), np.zeros(len(c), np.int32), C.c_int32()
    sc0, ag0 = np.zeros(len(c), F), np.zeros(len(c), np.int32)

    def ext():
        rc = lib.rs_hip_coverage_extensions(cov.handle, C.addressof(bo), bp.ctypes.data, bs.ctypes.data, len(b), C.addressof(co), cp.ctypes.data, len(c),
                                            sc1.ctypes.data, ag1.ctypes.data, C.addressof(ba1))
        assert rc == 0

    def old():
        rc = lib.rs_hip_coverage_scores(cov.handle, C.addressof(fo), fp, fs, first, len(c), sc0, ag0.ctypes.data)
        assert rc == 0
    ext(); old()
    assert (ag1 == a0).all() and (ag0 == a0).all() and (sc1.view(np.uint32) == s0.view(np.uint32)).all() and (sc0.view(np.uint32) == s0.view(np.uint32)).all()
    t_ext, t_old = [], []
    for _ in range(a.repeats):
        for fn, ts in ((ext, t_ext), (old, t_old)):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    capi.profile_enable(True)
    capi.profile_reset(); ext(); k_ext = capi.profile_read("coverage")
    capi.profile_reset(); old(); k_old = capi.profile_read("coverage")
    capi.profile_enable(False)
    grid = cov.scene_grid()
    need = np.array([R.live_box_bytes(grid, lo, hi, 0.05, objs, base, cd) for cd in cand])
    m_ext, m_old = float(np.median(t_ext)), float(np.median(t_old))
    spread = 1e-3 * max(np.percentile(1e3 * np.array(t_ext), 75) - np.percentile(1e3 * np.array(t_ext), 25), np.percentile(1e3 * np.array(t_old), 75) - np.percentile(1e3 * np.array(t_old), 25))
    verdict = "faster than" if m_old - m_ext > spread else "slower than" if m_ext - m_old > spread else "within the spread of"
    lines = [f"arrangement timing, {capi.load().rs_hip_version().decode()}",
             f"room: {len(pts)} scan points, grid {cov.res.tolist()} at 0.05 = {cov.n_cells} cells ({(cov.n_cells + 31) // 32 * 4} bytes per plane), {cov.valid_cells} valid",
             f"objects: {[len(o) for o in objs]} points; base 8 placements, 256 candidates; host-timed synchronous calls, {a.repeats} repeats after one warm-up, interleaved (ms)",
             "(the C ABI called with arguments packed once: a call's time is the library's host work, the upload, the clears, the kernels and the read-back; "
             "'kernels' is the device time of the kernels alone)",
             f"  rs_hip_coverage_extensions  (1 base plane + 256 sub-boxes)          {stats(t_ext)}   kernels {k_ext[1]:.3f} ms in {k_ext[0]} spans",
             f"  rs_hip_coverage_scores      (256 arrangements x 9 placements)       {stats(t_old)}   kernels {k_old[1]:.3f} ms in {k_old[0]} spans",
             f"  the new call is {verdict} the batched form: medians {1e3 * m_ext:.3f} vs {1e3 * m_old:.3f} ms (ratio {m_old / m_ext:.2f}), larger interquartile range {1e3 * spread:.3f} ms",
             f"  workgroup 256 threads, one per candidate; LDS per workgroup 16384 B of bits + 28 B; sub-boxes used: median {int(np.median(need))} B, max {int(need.max())} B, "
             f"{int((need == 0).sum())} candidates without a live cell; routes: {n_lds} LDS, {n_slab} slab ({100.0 * n_slab / max(1, n_lds + n_slab):.1f} % slab)"]
    # saliency: the candidates as proposals of dynamic objects, plus 16 static ones (the largest object as a wall stand-in)
    po = np.array([o for o, _ in cand] + [0] * 16, np.int32)
    pp = np.array([p for _, p in cand] + [p for _, p in cand[:16]], F)
    ps = np.array([0] * len(cand) + [1] * 16, np.int32)
    cls = np.where(inst < 3, np.where(inst == 0, 2, 1), 5).astype(np.int32)
    sal = lambda: capi.scene_saliency(lo, hi, clouds, po, pp, ps, pts, cls, 1, 2, 0.15)   # noqa: E731
    q = sal()
    t_sal = []
    for _ in range(a.repeats):
        t0 = time.perf_counter(); sal(); t_sal.append(time.perf_counter() - t0)
    t0 = time.perf_counter(); qr = R.saliency(lo, hi, 0.15, objs, po, pp, ps, pts, cls, 1, 2)[1]; t_np = time.perf_counter() - t0
    assert q.tobytes() == qr.tobytes(), "saliency disagrees with the restatement"
    lines += [f"rs_hip_scene_saliency: {len(po)} proposals, {len(pts)} level-0 points, voxel 0.15 (upload of positions and class ids and download of qualities included)",
              f"  {stats(t_sal)}   ({int(q.sum())} salient points)",
              f"  context only: the NumPy restatement on this host {1e3 * t_np:.1f} ms"
              + (f"; the reference's rsao_compute_scene_saliency on another host {a.reference_ms:.2f} ms" if a.reference_ms is not None else "")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
