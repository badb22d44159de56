"""Writes tests/golden/propose_<case>.npz from the REFERENCE's own mgs__propose_poses_at_level and mgs_propose_poses.

    python tools/propose_fixture/gen.py [--ref /path/to/reference] [--out tests/golden] [--only room,wide,floor,empty]

Run once, by hand, where the reference tree is available; no test runs it.  driver.cpp and the reference's pose_proposal.cpp are
compiled into a temporary directory outside the tree (asserts on, -O2 -std=c++11, no -march, as oracle/Makefile compiles the
reference) and the work is done by a child process.  Every cloud's levels are the reference's own level builder's.

A file holds: the scene's level-1 cloud (the one that is searched) and box; per object its levels 4, 3, 2, whether the reference
calls it static (the caller of rs_hip_propose_poses leaves such an object out; the reference skips it) and, per run (a run = one
(spacing, angle_delta) pair), the proposal storage after each level (stage 0: poses and scores; stages 1, 2: scores — the poses
never change, which is asserted) and mgs_propose_poses' final lists, which the driver has compared with the staged run's.

Cases and the conditions asserted here (tests/test_propose_cpu.py re-checks them from the arrays):
  room   a 2.0 x 1.6 m synth room, two dynamic objects and a static one; a pose survives all levels, one is marked -1 at level 3
         and another at level 2, an object proposes in more than one cell row
  wide   an 8 x 8 m box over a sparse scene, an object of a few dozen points at level 4: 83 * 83 * 10 = 68 890 poses, proposals on
         both sides of pose 65 535
  floor  a dense floor patch larger than the box and a flat plate: two runs with non-default (spacing, angle_delta) whose float
         loops give step counts that differ from the real numbers'; every cell proposes, so the translations show ox and oz
  empty  an object that matches nowhere: counts 0
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rescan_amd import synth  # noqa: E402
import propose_restate as R  # noqa: E402

F = np.float32
LEVELS = (4, 3, 2)
THRESHOLDS = np.array([0.25, 0.35, 0.40], F)          # mgs__score_threshold, pose_proposal.cpp:160-168
DEFAULT = (F(0.10), F(np.float64(6.2831853072) / np.float64(F(10.0))))       # mgs_init_opts, :27-28
MAX_BYTES = 757075
CLASSES = {"unlabelled": 0, "wall": 1, "floor": 2, "chair": 5, "table": 7, "shelf": 15}


def fp(a):
    return a.ctypes.data_as(C.c_void_p)


class Ref:
    def __init__(self, path):
        L = self.L = C.CDLL(path)
        L.fx_cloud.restype = C.c_void_p; L.fx_cloud.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.fx_level.restype = C.c_int32; L.fx_level.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.fx_bbox.argtypes = [C.c_void_p, C.c_void_p]; L.fx_set_bbox.argtypes = [C.c_void_p, C.c_void_p]
        L.fx_db.restype = C.c_void_p
        L.fx_add_class.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
        L.fx_add_object.restype = C.c_int32; L.fx_add_object.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.fx_is_static.restype = C.c_int32; L.fx_is_static.argtypes = [C.c_void_p, C.c_int32]
        L.fx_run.restype = C.c_int32; L.fx_run.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float]
        L.fx_stage_count.restype = C.c_int32; L.fx_stage_count.argtypes = [C.c_int32, C.c_int32]
        L.fx_stage_get.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]

    def cloud(self, pos, nor):
        pos, nor = np.ascontiguousarray(pos, F), np.ascontiguousarray(nor, F)
        return self.L.fx_cloud(fp(pos), fp(nor), len(pos))

    def level(self, h, lvl):
        n = self.L.fx_level(h, lvl, None, None)
        pos, nor = np.zeros((n, 3), F), np.zeros((n, 3), F)
        self.L.fx_level(h, lvl, fp(pos), fp(nor))
        return pos, nor

    def bbox(self, h):
        b = np.zeros(6, F); self.L.fx_bbox(h, fp(b)); return b

    def set_bbox(self, h, b):
        b = np.ascontiguousarray(b, F); self.L.fx_set_bbox(h, fp(b))

    def stage(self, s, o):
        n = self.L.fx_stage_count(s, o)
        p, sc = np.zeros((n, 16), F), np.zeros(n, F)
        if n:
            self.L.fx_stage_get(s, o, fp(p), fp(sc))
        return p, sc


def run_case(ref, name, scene_pts, scene_nor, objects, runs, bbox=None):
    """objects: (pos, nor, class name).  Returns the dict that is saved."""
    scn = ref.cloud(scene_pts, scene_nor)
    if bbox is not None:
        ref.set_bbox(scn, bbox)
    box = ref.bbox(scn)
    db = ref.L.fx_db()
    for k, v in CLASSES.items():
        ref.L.fx_add_class(db, k.encode(), v)
    out = dict(bbox=box, thresholds=THRESHOLDS, radius=F(0.1), max_n_neigh=np.int32(64), height=F(0.0), n_objects=np.int32(len(objects)),
               n_runs=np.int32(len(runs)), levels=np.array(LEVELS, np.int32))
    out["scene_pos"], out["scene_nor"] = ref.level(scn, 1)
    for o, (pos, nor, cls) in enumerate(objects):
        h = ref.cloud(pos, nor)
        assert ref.L.fx_add_object(db, h, CLASSES[cls], 3 + o) == o
        out[f"obj{o}_static"] = np.int32(ref.L.fx_is_static(db, o))
        for l, lvl in enumerate(LEVELS):
            out[f"obj{o}_l{l}_pos"], out[f"obj{o}_l{l}_nor"] = ref.level(h, lvl)
    for r, (spacing, delta) in enumerate(runs):
        assert ref.L.fx_run(db, scn, F(spacing), F(delta)) == 1, (name, "mgs_propose_poses differs from the staged levels")
        out[f"run{r}_spacing"], out[f"run{r}_angle_delta"] = F(spacing), F(delta)
        for o in range(len(objects)):
            p0, s0 = ref.stage(0, o)
            out[f"run{r}_obj{o}_poses"], out[f"run{r}_obj{o}_s0"] = p0, s0
            for s in (1, 2):
                p, sc = ref.stage(s, o)
                assert p.tobytes() == p0.tobytes(), (name, "the storage's poses changed")
                out[f"run{r}_obj{o}_s{s}"] = sc
            out[f"run{r}_obj{o}_final_poses"], out[f"run{r}_obj{o}_final_scores"] = ref.stage(3, o)
            if out[f"obj{o}_static"]:
                assert len(p0) == 0
    return out


def conditions(name, d):
    """The case's condition, from the saved arrays alone (tests/test_propose_cpu.py calls this too)."""
    n_obj, n_runs = int(d["n_objects"]), int(d["n_runs"])
    dyn = [o for o in range(n_obj) if not int(d[f"obj{o}_static"])]
    if name == "room":
        assert len(dyn) == 2 and n_obj == 3
        s2 = np.concatenate([d[f"run0_obj{o}_s2"] for o in dyn]); s1 = np.concatenate([d[f"run0_obj{o}_s1"] for o in dyn])
        assert (s2 > 0).any(), "no pose survives all three levels"
        assert (s1 == -1).any() and ((s1 > 0) & (s2 == -1)).any(), "no -1 mark at level 3 or none at level 2"
        assert any(len(np.unique(d[f"run0_obj{o}_poses"][:, 12])) > 1 for o in dyn), "no object with proposals in more than one cell row"
    if name == "wide":
        ox, oz, yaw = R.grid_plan(d["bbox"][:3], d["bbox"][3:], d["run0_spacing"], d["run0_angle_delta"])
        assert len(ox) * len(oz) * len(yaw) > 65535 and d["bbox"][3] - d["bbox"][0] >= 8.0 and d["bbox"][5] - d["bbox"][2] >= 8.0
        assert any(len(d[f"obj{o}_l0_pos"]) < 100 for o in dyn)
        P = R.grid_poses(d["bbox"][:3], d["height"], ox, oz, yaw)
        idx = {P[i].tobytes(): i for i in range(len(P))}
        where = np.array([idx[p.tobytes()] for o in dyn for p in d[f"run0_obj{o}_poses"]])
        assert (where < 65535).any() and (where >= 65535).any(), "proposals on one side of the chunk boundary only"
    if name == "floor":
        assert n_runs == 2
        for r in range(n_runs):
            sp, de = d[f"run{r}_spacing"], d[f"run{r}_angle_delta"]
            assert (sp, de) != DEFAULT and sp != DEFAULT[0] and de != DEFAULT[1]
            ox, oz, yaw = R.grid_plan(d["bbox"][:3], d["bbox"][3:], sp, de)
            lx = np.float64(F(d["bbox"][3] - d["bbox"][0]))
            real_x = int(np.ceil((lx + 2 * np.float64(sp)) / np.float64(sp)))
            real_yaw = int(np.ceil(np.float64(6.2831853072) / np.float64(de)))
            assert len(ox) != real_x or len(yaw) != real_yaw, (r, "the float loops give the real numbers' step counts")
            for o in dyn:
                assert len(d[f"run{r}_obj{o}_poses"]) == len(ox) * len(oz), (r, "not every cell proposes")
    if name == "empty":
        assert all(len(d[f"run0_obj{o}_final_scores"]) == 0 for o in range(n_obj)) and len(dyn) >= 1


def plate(rng, size, density):
    p, n = synth._sample_rect(rng, np.array([-size / 2, 0.0, -size / 2]), np.array([size, 0, 0.]), np.array([0, 0, size]), (0, 1, 0), density)
    return synth._finish(rng, p, n, synth.JITTER)


def case_room(ref):
    s = synth.make_scene(seed=41, width=2.0, depth=1.6, height=1.2, density=1500.0, objects=("chair", "table"))
    objs = [(o["pos"], o["nor"], o["kind"]) for o in s["objects"]]
    cp, cn = synth.make_object("crate", 5, density=1500.0)
    objs.append((cp, cn, "wall"))                                  # static by its class (rs_database.h:257-288)
    return run_case(ref, "room", s["points"], s["normals"], objs, [DEFAULT])


def case_wide(ref):
    rng = np.random.default_rng(77)
    small, small_n = synth.make_object("chair", 9, density=600.0, scale=0.5)
    P, N = [], []
    for (x, z, a) in ((1.0, 1.2, 0.0), (4.1, 6.3, 2 * np.pi / 10 * 3), (7.9, 2.0, 0.0), (7.9, 7.2, 2 * np.pi / 10 * 7)):
        pose = synth.pose_matrix(a, (x, 0.0, z))
        sp, sn = synth.make_object("chair", 9 + int(x * 10), density=2500.0, scale=0.5)
        P.append(synth.apply_pose(pose, sp)); N.append(synth.apply_pose(pose, sn, False))
        fpts, fn = synth._sample_rect(rng, np.array([x - 0.4, 0.0, z - 0.4]), np.array([0.8, 0, 0.]), np.array([0, 0, 0.8]), (0, 1, 0), 1500.0)
        P.append(fpts.astype(F)); N.append(fn.astype(F))
    return run_case(ref, "wide", np.concatenate(P), np.concatenate(N), [(small, small_n, "chair")], [DEFAULT],
                    bbox=np.array([0, 0, 0, 8.0, 1.0, 8.0], F))


def odd_pairs(length):
    """Two non-default (spacing, angle_delta) whose float loops differ from the real numbers' step counts."""
    found = []
    for sp in (0.07, 0.11, 0.12, 0.13, 0.14, 0.15, 0.16, 0.17, 0.18, 0.19, 0.21, 0.22, 0.23):
        for n in (4, 5, 6, 7, 8, 9, 11, 12):
            de = F(np.float64(6.2831853072) / np.float64(F(n)))
            nx, ny = len(R.offsets(F(length), F(sp))), len(R.yaw_angles(de))
            real_x = int(np.ceil((np.float64(F(length)) + 2 * np.float64(F(sp))) / np.float64(F(sp))))
            real_y = int(np.ceil(np.float64(6.2831853072) / np.float64(de)))
            if nx != real_x and ny != real_y:
                found.append((F(sp), de))
    assert len(found) >= 2, found
    return [found[0], found[-1]]


def case_floor(ref, length=1.2):
    rng = np.random.default_rng(5)
    lo = -0.6
    fpts, fn = synth._sample_rect(rng, np.array([lo, 0.0, lo]), np.array([length - 2 * lo, 0, 0.]), np.array([0, 0, length - 2 * lo]), (0, 1, 0), 2500.0)
    fpts, fn = synth._finish(rng, fpts, fn, synth.JITTER)
    pp, pn = plate(np.random.default_rng(6), 0.3, 2500.0)
    return run_case(ref, "floor", fpts, fn, [(pp, pn, "table")], odd_pairs(length), bbox=np.array([0, 0, 0, length, 0.5, length], F))


def case_empty(ref):
    s = synth.make_scene(seed=43, width=1.0, depth=1.0, height=0.6, density=1500.0, objects=())
    # a tall shelf lying far above anything the room has: nothing of it is near the scan at height 0
    pos, nor = synth.make_object("shelf", 3, density=1500.0)
    pos = pos + np.array([0, 3.0, 0], F)
    return run_case(ref, "empty", s["points"], s["normals"], [(pos, nor, "shelf")], [DEFAULT])


CASES = dict(room=case_room, wide=case_wide, floor=case_floor, empty=case_empty)


def child(lib, out_dir, only):
    ref = Ref(lib)
    for name in only:
        d = CASES[name](ref)
        conditions(name, d)
        path = os.path.join(out_dir, f"propose_{name}.npz")
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        lens = {o: [len(d[f"run{r}_obj{o}_poses"]) for r in range(int(d["n_runs"]))] for o in range(int(d["n_objects"]))}
        print(f"FIXTURE {name}: scene level 1 {len(d['scene_pos'])} points, proposals per object and run {lens}, {size} bytes -> {path}")
        assert size <= MAX_BYTES, (name, size)
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default="room,wide,floor,empty")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.out, a.only.split(","))
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as tmp:
        lib = os.path.join(tmp, "libproposefx.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++11", "-fPIC", "-w", "-shared",
                               f"-I{a.ref}/lib", f"-I{a.ref}/lib/rs", f"-I{a.ref}/apps/pose_proposal", "-o", lib,
                               os.path.join(here, "driver.cpp"), os.path.join(a.ref, "apps", "pose_proposal", "pose_proposal.cpp"), "-lm"])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, "--out", a.out, "--only", a.only], stdout=subprocess.PIPE, text=True)
        print("\n".join(ln[ln.index("FIXTURE"):] for ln in r.stdout.splitlines() if "FIXTURE" in ln))      # (the reference prints its progress too)
        if r.returncode != 0:
            print(r.stdout[-3000:])
            raise SystemExit(f"generation failed (exit {r.returncode}: an assert of the reference or of this script)")


if __name__ == "__main__":
    main()
