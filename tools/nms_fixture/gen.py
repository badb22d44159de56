"""Writes tests/golden/nms_<shape>.npz from the REFERENCE's own isect_get_overlap_factor and mgs_non_maxima_suppresion.

    python tools/nms_fixture/gen.py [--ref /path/to/reference] [--out tests/golden] [--hard]

--hard writes tests/golden/isect_hard.npz instead: the hostile shapes of tests/hard_shapes.py (every family but "random"), their
levels 1 and 3 given to the reference as they are (fx_shape_from_levels).  The clouds are not stored, only their lengths and CRCs.
Cases the reference cannot run (a line of 4097 cells overruns its scanline arrays) are recorded with their expected refusal only.

Run once, by hand, where the reference tree is available; no test runs it.  driver.cpp and the reference's
pose_proposal.cpp are compiled into a temporary directory outside the tree (asserts on, -O2 -std=c++11, no -march, as
oracle/Makefile compiles the reference) and the work is done by a child process whose standard output is read back: a
"WARNING: Grid A count" line of the reference (intersect.h:354: a grid without cells) or a failed assert fails the
generation.  Shapes: synth chair / table / crate; level 1 (boundary) and level 3 (extent) by the reference's own level builder.

Cases per shape (tests/test_isect_cpu.py, tests/test_gpu_isect.py compare every one):
  a identical poses   b disjoint boxes   c boxes touching with equality on x   d ~200 grid-search-like pairs
  e voxel sizes that divide the 0.3 margin and lattice shifts: points on voxel faces, where the fp32 division decides
  f voxelize_inside x normalize_by_smaller   g a voxel so small that the bit planes exceed the LDS route's budget
  h pose-proposal lists for the non-maximum suppression
It also prints the reference's CPU time for the inputs of tools/nms_timing.py (this machine's; context only).
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rescan_amd import synth  # noqa: E402

F = np.float32
SHAPES = (("chair", 101), ("table", 102), ("crate", 103))
LDS_BUDGET = 61440        # ISECT_LDS_BYTES of rescan_amd/csrc/rs_isect.hip


def fp(a):
    return a.ctypes.data_as(C.c_void_p)


class Ref:
    def __init__(self, path):
        L = self.L = C.CDLL(path)
        L.fx_shape_create.restype = C.c_void_p
        L.fx_shape_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.fx_shape_from_levels.restype = C.c_void_p
        L.fx_shape_from_levels.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.fx_level.restype = C.c_int32
        L.fx_level.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.fx_centroid.argtypes = [C.c_void_p, C.c_void_p]
        L.fx_overlap.restype = C.c_float
        L.fx_overlap.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_int32, C.c_void_p]
        L.fx_nms.restype = C.c_int32
        L.fx_nms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]

    def shape(self, pos, nor):
        pos, nor = np.ascontiguousarray(pos, F), np.ascontiguousarray(nor, F)
        h = self.L.fx_shape_create(fp(pos), fp(nor), len(pos))
        lv = {}
        for lvl in (1, 3):
            out = np.zeros((self.L.fx_level(h, lvl, None), 3), F)
            self.L.fx_level(h, lvl, fp(out))
            lv[lvl] = out
        c = np.zeros(3, F)
        self.L.fx_centroid(h, fp(c))
        return h, lv[1], lv[3], c

    def from_levels(self, l1, l3):
        l1, l3 = np.ascontiguousarray(l1, F), np.ascontiguousarray(l3, F)
        return self.L.fx_shape_from_levels(fp(l1), len(l1), fp(l3), len(l3))

    def centroid(self, h):
        c = np.zeros(3, F)
        self.L.fx_centroid(h, fp(c))
        return c

    def overlap(self, h, pa, pb, voxel, inside, by_smaller, hb=None):
        pa, pb = np.ascontiguousarray(pa, F), np.ascontiguousarray(pb, F)
        cnt = np.zeros(3, np.int32)
        ov = self.L.fx_overlap(h, fp(pa), h if hb is None else hb, fp(pb), F(voxel), inside, by_smaller, fp(cnt))
        return F(ov), cnt

    def nms(self, h, poses, scores, thr):
        poses, scores = np.ascontiguousarray(poses, F), np.ascontiguousarray(scores, F)
        n = len(scores)
        kp, ks = np.zeros((n, 16), F), np.zeros(n, F)
        nk = self.L.fx_nms(h, fp(poses), fp(scores), n, F(thr), fp(kp), fp(ks))
        # the kept proposals are a subsequence of the list, in its order (pose_proposal.cpp:441-447)
        marks, j = np.full(n, 2, np.int32), 0
        for i in range(n):
            if j < nk and (poses[i].view(np.uint32) == kp[j].view(np.uint32)).all() and scores[i].view(np.uint32) == ks[j].view(np.uint32):
                marks[i] = 1
                j += 1
        assert j == nk, "kept proposals are not a subsequence of the list"
        return marks


def xform(pose, pts):
    m = np.asarray(pose, F)
    return np.stack([m[r] * pts[:, 0] + m[4 + r] * pts[:, 1] + m[8 + r] * pts[:, 2] + F(1.0) * m[12 + r] for r in range(3)], axis=1)


def lattice_pose(rng, span=8):
    i, j = rng.integers(-span, span + 1, 2)
    k = int(rng.integers(0, 10))
    return synth.pose_matrix(F(k) * F(2.0 * np.pi / 10.0), (F(i) * F(0.1), 0.0, F(j) * F(0.1)))


def shifted(rng, pose, reach=6):
    i, j = rng.integers(-reach, reach + 1, 2)
    k = int(rng.integers(0, 10))
    t = np.asarray(pose, F)[12:15]
    return synth.pose_matrix(F(k) * F(2.0 * np.pi / 10.0), (t[0] + F(i) * F(0.1), 0.0, t[2] + F(j) * F(0.1)))


def touching_pose(extent):
    """Two pure translations along x after which the second box begins EXACTLY where the first one ends."""
    hi_pt, lo_pt = extent[:, 0].max(), extent[:, 0].min()
    tb = F(F(hi_pt - lo_pt) + F(0.001))
    target = F(lo_pt + tb)                       # where the second box begins
    ta = F(target - hi_pt)                       # (a difference of two neighbours' multiples of an ulp: exact)
    pa, pb = synth.pose_matrix(0.0, (ta, 0, 0)), synth.pose_matrix(0.0, (tb, 0, 0))
    if xform(pa, extent)[:, 0].max() != xform(pb, extent)[:, 0].min():
        raise SystemExit("no translation makes the boxes touch with equality")
    return pa, pb


def child(lib, out_dir):
    R = Ref(lib)
    timing_lines = []
    for name, seed in SHAPES:
        rng = np.random.default_rng(seed)
        pos, nor = synth.make_object(name, seed)
        h, l1, l3, cen = R.shape(pos, nor)
        P = []        # (case, pose_a, pose_b, voxel, inside, by_smaller)
        for _ in range(3):
            p = lattice_pose(rng); P.append(("a", p, p, 0.1, 1, 0))
        for _ in range(3):
            p = lattice_pose(rng); q = p.copy(); q[12] += F(5.0); P.append(("b", p, q, 0.1, 1, 0))
        ta, tb = touching_pose(l3)
        P.append(("c", ta, tb, 0.1, 1, 0)); P.append(("c", tb, ta, 0.1, 0, 1))
        for _ in range(200):
            p = lattice_pose(rng); P.append(("d", p, shifted(rng, p), 0.1, 1, 0))
        for voxel in (0.05, 0.06, 0.15, 0.3, 0.1):
            for _ in range(4):
                p = lattice_pose(rng, 3); q = p.copy(); q[12] += F(rng.integers(-3, 4)) * F(voxel); q[14] += F(rng.integers(-3, 4)) * F(voxel)
                P.append(("e", p, q, voxel, 1, 0))
        for inside in (0, 1):
            for by_smaller in (0, 1):
                for _ in range(10):
                    p = lattice_pose(rng); P.append(("f", p, shifted(rng, p, 4), 0.1, inside, by_smaller))
        p = lattice_pose(rng, 2)
        P.append(("g", p, shifted(rng, p, 3), 0.02, 1, 0))
        n = len(P)
        cnt, ov = np.zeros((n, 3), np.int32), np.zeros(n, F)
        on_face = 0
        for k, (case, pa, pb, voxel, inside, by_smaller) in enumerate(P):
            ov[k], cnt[k] = R.overlap(h, pa, pb, voxel, inside, by_smaller)
            if case == "a":
                assert ov[k] == 1.0, (name, k, ov[k])
            if case == "b":
                assert ov[k] == 0.0 and cnt[k].sum() == 0, (name, k)
            if case == "c":
                assert cnt[k, 0] > 0, (name, "touching boxes must make a grid")
            if case in ("e", "d") and cnt[k, 0] > 0:
                # points whose cell the division and the multiply by the inverse put on different sides of a voxel face
                qa, qb = xform(pa, l3), xform(pb, l3)
                origin = np.minimum(qa.min(0), qb.min(0)) - F(0.3)
                for pose in (pa, pb):
                    o = xform(pose, l1) - origin[None, :]
                    on_face += int((np.floor(o / F(voxel)) != np.floor(o * (F(1.0) / F(voxel)))).sum())
            if case == "g":
                lo = np.minimum(xform(pa, l3).min(0), xform(pb, l3).min(0)) - F(0.3)
                hi = np.maximum(xform(pa, l3).max(0), xform(pb, l3).max(0)) + F(0.3)
                res = np.ceil((hi - lo) / F(voxel)).astype(np.int64) + 1
                need = ((res[0] + 31) // 32) * res[1] * res[2] * 4 * 4
                assert need > LDS_BUDGET, (name, "case g fits the LDS route", need)
        assert on_face > 0, (name, "no point of cases d / e separates the division from the multiply")
        # h: the proposal lists
        lists = {}
        alone_total = 0
        for li, n_prop in enumerate((60, 240)):
            poses, scores = synth.nms_proposals(seed * 10 + li, n_prop, span=1.0 if li else 0.6)
            assert (np.unique(scores, return_counts=True)[1] > 1).any() and (scores < 0.01).any() and (scores == 10.0).sum() == 2
            marks = R.nms(h, poses, scores, 0.2)
            # replay of the rounds with the reference's overlap: the same marks, and which discards overlap alone decided
            mk, alone = np.zeros(n_prop, np.int32), 0
            cpts = np.stack([xform(poses[i], cen[None, :])[0] for i in range(n_prop)])
            while (mk == 0).any():
                cand = np.flatnonzero(mk == 0)
                best = cand[np.argmax(scores[cand])]
                mk[best] = 1
                for i in np.flatnonzero(mk == 0):
                    d = cpts[best] - cpts[i]
                    cheap = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2], dtype=F) < F(0.2) or scores[i] < F(0.01)
                    if cheap:
                        mk[i] = 2
                    elif R.overlap(h, poses[best], poses[i], 0.1, 1, 0)[0] > F(0.5):
                        mk[i] = 2; alone += 1
            assert (mk == marks).all(), (name, li, "replay of the rounds disagrees with the reference's marks")
            alone_total += alone
            lists[li] = (poses, scores, marks)
            print(f"{name}: list {li}: {n_prop} proposals, {int((marks == 1).sum())} kept, {alone} discards by overlap alone")
        if name != "chair":
            assert alone_total > 0, (name, "no discard decided by overlap alone")
        out = dict(boundary=l1, extent=l3, centroid=cen,
                   case=np.array([p[0] for p in P], "S1"), pose_a=np.stack([p[1] for p in P]).astype(F), pose_b=np.stack([p[2] for p in P]).astype(F),
                   voxel=np.array([p[3] for p in P], F), inside=np.array([p[4] for p in P], np.int32), by_smaller=np.array([p[5] for p in P], np.int32),
                   counts=cnt, overlap=ov, dist_threshold=F(0.2))
        for li, (poses, scores, marks) in lists.items():
            out[f"list{li}_poses"], out[f"list{li}_scores"], out[f"list{li}_marks"] = poses, scores, marks
        path = os.path.join(out_dir, f"nms_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{name}: level 1 {len(l1)} points, level 3 {len(l3)}, {n} pairs, {on_face} face-deciding points, {os.path.getsize(path)} bytes -> {path}")
        if name == "chair":
            for n_prop in (64, 256, 1024):
                poses, scores = synth.nms_proposals(7, n_prop, span=1.5)
                t0 = time.perf_counter()
                marks = R.nms(h, poses, scores, 0.2)
                timing_lines.append(f"reference CPU (this machine, one thread): chair, {n_prop} proposals: {time.perf_counter() - t0:.3f} s, {int((marks == 1).sum())} kept")
    for ln in timing_lines:
        print(ln)
    sys.stdout.flush()


def hard_child(lib, out_dir):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hard_shapes as H
    R = Ref(lib)
    cases = H.fixture_cases()
    case_first, shape_first, shape_crc = [0], [0], []
    ia, ib, pa, pb, cnt, ov = [], [], [], [], [], []
    warnings = 0
    for c in cases:
        hs = [R.from_levels(b, e) for b, e in c.shapes] if c.reference else []
        for k in range(len(c)):
            o, n = F(0.0), np.zeros(3, np.int32)
            if c.reference:
                o, n = R.overlap(hs[c.ia[k]], c.pose_a[k], c.pose_b[k], c.voxel, c.inside, c.by_smaller, hb=hs[c.ib[k]])
                denom = min(n[0], n[1]) if c.by_smaller else max(n[0], n[1])
                if denom == 0 and o == 1.0:                       # (a pair without a grid has overlap 0)
                    assert c.name == "edges_empty", (c.name, k, "an empty grid outside the empty-boundary case")
                    warnings += 1
            ia.append(c.ia[k]); ib.append(c.ib[k]); pa.append(c.pose_a[k]); pb.append(c.pose_b[k]); cnt.append(n); ov.append(o)
        case_first.append(len(ia)); shape_crc += list(c.crcs()); shape_first.append(len(shape_crc))
        print(f"{c.name}: {len(c)} pairs, {len(c.shapes)} shapes, {'reference' if c.reference else 'expected refusal only: ' + c.expect}")
    # the proposal list: the reference's own centroid, the threshold = one centroid distance's exact fp32 value
    L = H.nms_list()
    h = R.from_levels(*L["shape"])
    cen = R.centroid(h)
    i, j = L["decider"]
    thr = H.centroid_distance(cen, L["poses"][i], L["poses"][j])
    marks = R.nms(h, L["poses"], L["scores"], thr)
    print(f"nms: {len(marks)} proposals, {int((marks == 1).sum())} kept, threshold {thr!r}")
    out = dict(case_name=np.array([c.name for c in cases], "S24"), case_family=np.array([c.family for c in cases], "S8"),
               case_expect=np.array([c.expect for c in cases], "S8"), case_reference=np.array([c.reference for c in cases], np.int32),
               case_voxel=np.array([c.voxel for c in cases], F), case_inside=np.array([c.inside for c in cases], np.int32),
               case_by_smaller=np.array([c.by_smaller for c in cases], np.int32), case_first=np.array(case_first, np.int32),
               shape_first=np.array(shape_first, np.int32), shape_crc=np.array(shape_crc, np.int64).reshape(-1, 4),
               shape_a=np.array(ia, np.int32), shape_b=np.array(ib, np.int32), pose_a=np.stack(pa).astype(F), pose_b=np.stack(pb).astype(F),
               counts=np.stack(cnt).astype(np.int32), overlap=np.array(ov, F),
               nms_shape_crc=np.array([len(L["shape"][0]), H.crc(L["shape"][0]), len(L["shape"][1]), H.crc(L["shape"][1])], np.int64),
               nms_centroid=cen, nms_poses=L["poses"], nms_scores=L["scores"], nms_dist_threshold=F(thr), nms_marks=marks,
               nms_decider=np.array(L["decider"], np.int32))
    path = os.path.join(out_dir, "isect_hard.npz")
    np.savez_compressed(path, **out)
    print(f"{len(ia)} pairs in {len(cases)} cases, {os.path.getsize(path)} bytes -> {path}")
    print(f"EXPECTED_WARNINGS {warnings}")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--hard", action="store_true")
    a = ap.parse_args()
    if a.child:
        return (hard_child if a.hard else child)(a.child, a.out)
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as tmp:
        lib = os.path.join(tmp, "libnmsfx.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++11", "-fPIC", "-w", "-shared",
                               f"-I{a.ref}/lib", f"-I{a.ref}/lib/rs", f"-I{a.ref}/apps/pose_proposal", "-o", lib,
                               os.path.join(here, "driver.cpp"), os.path.join(a.ref, "apps", "pose_proposal", "pose_proposal.cpp"), "-lm"])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, "--out", a.out] + (["--hard"] if a.hard else []), stdout=subprocess.PIPE, text=True)
        print(r.stdout, end="")
        if r.returncode != 0:
            raise SystemExit(f"generation failed (exit {r.returncode}: an assert of the reference or of this script)")
        if a.hard:
            # the empty-grid warning is expected for the rows of the empty-boundary case and for nothing else
            if f"EXPECTED_WARNINGS {r.stdout.count('WARNING: Grid A count')}\n" not in r.stdout:
                raise SystemExit("the reference printed its empty-grid warning outside the empty-boundary case")
        elif "WARNING: Grid A count" in r.stdout:
            raise SystemExit("the reference printed its empty-grid warning: the inputs do not meet the fixtures' condition")


if __name__ == "__main__":
    main()
