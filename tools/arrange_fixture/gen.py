"""Writes tests/golden/arrange_<name>.npz from the REFERENCE's own rsao_compute_scene_saliency, rsao_rasterize_scene_to_grid and
rsao__compute_scene_coverage_score.

    python tools/arrange_fixture/gen.py [--ref /path/to/reference] [--out tests/golden]

Run once, by hand, where the reference tree is available; no test runs it.  driver.cpp and the reference's
arrangement_optimization.cpp are compiled into a temporary directory outside the tree (asserts on, -O2 -std=c++11, no -march, as
oracle/Makefile compiles the reference); every fixture is made by a child process of its own, because the reference caches the
class table's indices in statics (rs_database.h:260-271).

Fixtures (tests/test_arrange_cpu.py, tests/test_gpu_arrange.py compare every array):
  arrange_room    class table with wall / floor / unlabelled / chair / table
  arrange_nowall  the same room without a "wall" class (rsdb_get_class_idx gives -1), some scene points with class id -1
Per fixture: a room scan of a few thousand level-0 points (level 2 = every third point), objects from rescan_amd/synth.py (chair,
table, a static wall, a wall-sized dynamic partition, clouds of 1 / 63 / 64 / 65 / 300 points, a lattice cloud), pose proposals on
the voxel lattice, the saliency at voxel 0.15 and 0.05, and coverage sets (voxel, threshold) = (0.05, 0.5), (0.15, 0.5), (0.05, 2.0:
no valid cell) with three trials each: empty base, base with a static placement, zero candidates.  child() asserts every case the
tests rely on.

    python tools/arrange_fixture/gen.py --hard

writes tests/golden/arrange_hard.npz instead: the hostile candidates and saliency cases of tests/hard_shapes.py (arrangement and
saliency_case, at voxel 0.05 and 0.15, with and without a finite point in cell 0) through the same three reference functions, every
cloud handed over unchanged as an object's level 2 or as the scene.  The file holds each cloud's length and CRC, not the cloud (the
tests regenerate them), the scene grids, the saliency grids and qualities, and per candidate the count and score bits of base +
candidate.  Every case runs: the candidate of no points and the clouds with NaN and infinite coordinates included.  What the
reference does not have is the sub-box of a candidate, so the routes the tests predict are the restatement's alone."""
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
import ao_restate as R  # noqa: E402

F = np.float32
FIXTURES = {"room": {"unlabelled": 0, "wall": 1, "floor": 2, "chair": 5, "table": 7},
            "nowall": {"unlabelled": 0, "floor": 2, "chair": 5, "table": 7}}
LOW_LDS_BUDGET = 64           # bytes: tests lower rs_hip_coverage_lds_budget to this; the partition's sub-box must need more
BLOCK = 256                   # ARR_BLOCK of rescan_amd/csrc/rs_arrange.hip


def fp(a):
    return a.ctypes.data_as(C.c_void_p)


class Ref:
    def __init__(self, path, classes):
        L = self.L = C.CDLL(path)
        L.fx_create.restype = C.c_void_p
        L.fx_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.fx_class_idx.restype = C.c_int32
        L.fx_class_idx.argtypes = [C.c_void_p, C.c_char_p]
        L.fx_add_object.restype = C.c_int32
        L.fx_add_object.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32]
        L.fx_is_static.restype = C.c_int32
        L.fx_is_static.argtypes = [C.c_void_p, C.c_int32]
        L.fx_set_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.fx_add_proposal.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.fx_saliency.restype = C.c_int64
        L.fx_saliency.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fx_scene_grid.restype = C.c_int64
        L.fx_scene_grid.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        L.fx_coverage.restype = C.c_float
        L.fx_coverage.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        names = list(classes)
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        ids = np.array([classes[n] for n in names], np.int32)
        self.h = L.fx_create(C.addressof(arr), fp(ids), len(names))
        self.keep = []

    def class_idx(self, name):
        return self.L.fx_class_idx(self.h, name.encode())

    def add_object(self, pos, class_idx, uidx):
        pos = np.ascontiguousarray(pos, F); self.keep.append(pos)
        return self.L.fx_add_object(self.h, fp(pos), len(pos), class_idx, uidx)

    def saliency(self, voxel):
        res, org = np.zeros(3, np.int32), np.zeros(3, F)
        n = self.L.fx_saliency(self.h, F(voxel), fp(res), fp(org), None)
        grid = np.zeros(n, np.uint8)
        self.L.fx_saliency(self.h, F(voxel), fp(res), fp(org), fp(grid))
        return res, org, grid

    def scene_grid(self, voxel, thr):
        res = np.zeros(3, np.int32)
        n = self.L.fx_scene_grid(self.h, F(voxel), F(thr), fp(res), None)
        grid = np.zeros(n, np.uint8)
        self.L.fx_scene_grid(self.h, F(voxel), F(thr), fp(res), fp(grid))
        return res, grid

    def coverage(self, objs, poses):
        objs = np.ascontiguousarray(objs, np.int32); poses = np.ascontiguousarray(poses, F).reshape(-1, 16)
        a = C.c_int32()
        s = self.L.fx_coverage(self.h, fp(objs), fp(poses), len(objs), C.addressof(a))
        return F(s), a.value


def lattice_pose(k, i, j, y=0.0, voxel=0.05):
    """Rotation about +y by k tenths of a turn, translation on the voxel lattice."""
    return synth.pose_matrix(F(k) * F(2.0 * np.pi / 10.0), (F(i) * F(voxel), F(y), F(j) * F(voxel)))


def rect(rng, w, h, density):
    n = int(round(w * h * density))
    ab = rng.random((n, 2))
    return np.stack([ab[:, 0] * w, ab[:, 1] * h, np.zeros(n)], axis=1).astype(F)


def child(lib, out_dir, name):
    classes = FIXTURES[name]
    ref = Ref(lib, classes)
    rng = np.random.default_rng({"room": 811, "nowall": 812}[name])
    wall_idx, floor_idx = ref.class_idx("wall"), ref.class_idx("floor")
    assert floor_idx == 2 and wall_idx == (1 if name == "room" else -1)
    bmin, bmax = np.array([0, 0, 0], F), np.array([3.0, 1.5, 3.0], F)
    dens = 260.0
    # ---- objects (level-2 clouds) ----
    chair = synth.make_object("chair", 31, dens)[0]
    table = synth.make_object("table", 32, dens)[0]
    wall = rect(rng, 3.0, 1.2, 110.0)
    lattice = np.stack(np.meshgrid(np.arange(-3, 4), np.arange(0, 5), np.arange(-3, 4), indexing="ij"), -1).reshape(-1, 3).astype(F) * F(0.05)
    static_class = classes["wall"] if "wall" in classes else classes["unlabelled"]
    objects, obj_class = [], []
    for pos, cls in ((chair, 5), (table, 7), (wall, static_class), (wall, 5), (chair[:1], 5), (chair[:63], 5), (chair[:64], 5),
                     (chair[:65], 5), (np.concatenate([table, chair])[:300], 7), (lattice, 5)):
        assert ref.add_object(pos, cls, len(objects)) == len(objects)
        objects.append(np.ascontiguousarray(pos, F)); obj_class.append(cls)
    CHAIR, TABLE, WALL, PART, ONE, N63, N64, N65, N300, LAT = range(10)
    sizes = [len(o) for o in objects]
    assert sizes[ONE] == 1 and sizes[N63] == 63 and sizes[N64] == 64 and sizes[N65] == 65 and sizes[N300] == 300 > BLOCK
    assert 30 <= sizes[CHAIR] <= 600 and 30 <= sizes[TABLE] <= 900 and len(lattice) == 245
    obj_static = np.array([ref.L.fx_is_static(ref.h, o) for o in range(len(objects))], np.int32)
    assert obj_static.tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    # ---- the scan: room shell, the furniture where it stands, clutter, points outside the grid on either side of each axis ----
    stand = [(CHAIR, lattice_pose(2, 20, 18)), (TABLE, lattice_pose(0, 38, 40)), (CHAIR, lattice_pose(7, 44, 14))]
    parts, cls = [], []
    for pts, c in ((rect(rng, 3.0, 3.0, dens)[:, [0, 2, 1]], floor_idx), (rect(rng, 3.0, 1.2, dens)[:, [2, 1, 0]], static_class),
                   (rect(rng, 3.0, 1.2, dens), static_class)):
        parts.append(pts); cls.append(np.full(len(pts), c))
    for seed, (o, pose) in enumerate(stand):
        scan = synth.make_object("chair" if o == CHAIR else "table", 900 + seed, dens)[0]
        parts.append(R.xform(pose, scan)); cls.append(np.full(len(scan), obj_class[o]))
    clutter = rng.uniform([0.2, 0.0, 0.2], [2.8, 1.2, 2.8], (300, 3)).astype(F)
    parts.append(clutter); cls.append(np.full(len(clutter), 0 if name == "room" else -1))
    far = np.array([[-0.5, 0.5, 1.0], [3.5, 0.5, 1.0], [1.0, -0.4, 1.0], [1.0, 1.95, 1.0], [1.0, 0.5, -0.45], [1.0, 0.5, 3.6],
                    [-0.3000001, 0.5, 1.0], [-0.3, 0.5, 1.0]], F)
    parts.append(far); cls.append(np.full(len(far), 5))
    pos0 = np.concatenate(parts).astype(F); pos0 = pos0 + np.where(np.arange(len(pos0))[:, None] < len(pos0) - len(far), rng.normal(0, 0.0007, pos0.shape), 0).astype(F)
    class0 = np.concatenate(cls).astype(np.int32)
    perm = rng.permutation(len(pos0)); pos0, class0 = np.ascontiguousarray(pos0[perm]), np.ascontiguousarray(class0[perm])
    assert 2000 <= len(pos0) <= 9000
    quality0 = np.full(len(pos0), 0.25, F)
    sub = np.arange(0, len(pos0), 3)
    pos2, quality2 = np.ascontiguousarray(pos0[sub]), np.zeros(len(sub), F)
    ref.L.fx_set_scene(ref.h, fp(pos0), fp(class0), fp(quality0), len(pos0), fp(pos2), fp(quality2), len(pos2), fp(bmin), fp(bmax))
    # ---- proposals ----
    props = [(o, p) for o, p in stand]
    for o in (CHAIR, TABLE, N65, LAT):
        for _ in range(7):
            props.append((o, lattice_pose(int(rng.integers(0, 10)), int(rng.integers(6, 54)), int(rng.integers(6, 54)))))
    props += [(LAT, lattice_pose(0, 10, 12, 0.0, 0.15)), (LAT, lattice_pose(0, 3, 9, 0.15, 0.15)), (LAT, lattice_pose(5, 30, 30))]
    # partly or wholly outside the grid, on the negative and on the positive side of each axis
    for t in ((-0.45, 0, 1.0), (3.4, 0, 1.0), (1.0, -0.6, 1.0), (1.0, 1.2, 1.0), (1.0, 0, -0.45), (1.0, 0, 3.45), (-2.0, 0, -2.0), (6.0, 3.0, 6.0)):
        props.append((CHAIR, synth.pose_matrix(0.3, t)))
    props.append((PART, synth.pose_matrix(F(-0.872), (0.3, 0.0, 0.1))))                        # the partition across the room, through a chair and the table
    props.append((WALL, synth.pose_matrix(0.0, (0.0, 0.0, 0.0))))                              # static: along z = 0
    props.append((WALL, synth.pose_matrix(F(-np.pi / 2), (1.0, 0.0, 0.0))))                    # static: through the chair at (1.0, 0.9)
    prop_obj = np.array([o for o, _ in props], np.int32)
    prop_pose = np.stack([p for _, p in props]).astype(F)
    prop_static = obj_static[prop_obj]
    for o, p in props:
        ref.L.fx_add_proposal(ref.h, int(o), fp(np.ascontiguousarray(p, F)))
    out = dict(class_names=np.array(list(classes), "S16"), class_ids=np.array(list(classes.values()), np.int32), wall_idx=np.int32(wall_idx),
               floor_idx=np.int32(floor_idx), bbox_min=bmin, bbox_max=bmax, pos0=pos0, class0=class0, sub=sub.astype(np.int32),
               n_obj=np.int32(len(objects)), obj_class=np.array(obj_class, np.int32), obj_static=obj_static,
               prop_obj=prop_obj, prop_pose=prop_pose, prop_static=prop_static, low_lds_budget=np.int32(LOW_LDS_BUDGET))
    for i, o in enumerate(objects):
        out[f"obj{i}_pos"] = o
    # ---- saliency ----
    sal_quality = None
    for j, voxel in enumerate((0.15, 0.05)):
        quality0[:] = 0.25
        res, org, grid = ref.saliency(voxel)
        out[f"sal{j}_voxel"], out[f"sal{j}_res"], out[f"sal{j}_origin"], out[f"sal{j}_grid"], out[f"sal{j}_quality"] = F(voxel), res, org, grid, quality0.copy()
        assert set(np.unique(quality0)) == {F(0.0), F(1.0)}
        origin, rres = R.grid_shape(bmin, bmax, voxel)
        assert (origin == org).all() and (rres == res).all()
        # the cases: cells that dynamic proposals lit and static ones cleared; wall / floor points inside lit cells; points outside
        dyn = np.zeros(len(grid), bool); sta = np.zeros(len(grid), bool); on_face = 0; neg = np.zeros(3, int); posi = np.zeros(3, int)
        for k in range(len(props)):
            q = R.xform(prop_pose[k], objects[prop_obj[k]])
            c = R.cells(origin, rres, voxel, q)
            (sta if prop_static[k] else dyn)[c[c >= 0]] = True
            cc = R.cell_coords(origin, voxel, q)
            neg += (cc < 0).any(0); posi += (cc >= rres[None, :]).any(0)
            t = (q - origin[None, :]) * (F(1.0) / F(voxel))
            on_face += int((t == np.floor(t)).sum())
        assert (dyn & sta).any() and (grid[dyn & sta] == 0).all() and grid[dyn & ~sta].all(), "a static proposal must clear cells a dynamic one lit"
        assert (neg > 0).all() and (posi > 0).all(), ("proposal points outside the grid on both sides of each axis", neg, posi)
        assert on_face > 0, "no transformed point on a voxel face"
        c0 = R.cells(origin, rres, voxel, pos0)
        inside = c0 >= 0
        shell = (class0 == wall_idx) | (class0 == floor_idx)
        assert (shell & inside & (grid[np.maximum(c0, 0)] == 1)).any(), "no wall / floor point inside a lit cell"
        assert (quality0[shell] == 0).all() and (~inside).sum() >= 6 and (quality0[~inside] == 0).all()
        if name == "nowall":
            assert (class0 == -1).any() and (quality0[class0 == -1] == 0).all(), "class id -1 equals the absent wall's -1"
        if j == 0:
            sal_quality = quality0.copy()
    assert 50 < int(sal_quality.sum()) < len(pos0)
    quality2[:] = sal_quality[sub]
    # ---- coverage ----
    dyn_props = [(int(o), p) for (o, p), s in zip(props, prop_static) if not s]
    extra = [(ONE, lattice_pose(2, 20, 18)), (N63, lattice_pose(2, 20, 18)), (N64, lattice_pose(7, 44, 14)), (N300, lattice_pose(0, 38, 40))]
    cands = dyn_props + extra
    bases = [[], [(TABLE, stand[1][1]), (CHAIR, stand[0][1]), (WALL, props[-2][1]), (N300, lattice_pose(3, 30, 22))], [(CHAIR, stand[2][1]), (WALL, props[-1][1])]]
    trial_cands = [cands, cands, []]
    assert any(o == CHAIR and (p == stand[0][1]).all() for o, p in cands)
    for j, (voxel, thr) in enumerate(((0.05, 0.5), (0.15, 0.5), (0.05, 2.0))):
        res, grid = ref.scene_grid(voxel, thr)
        valid = int((grid > 0).sum())
        out[f"cov{j}_voxel"], out[f"cov{j}_threshold"], out[f"cov{j}_res"], out[f"cov{j}_grid"], out[f"cov{j}_valid"] = F(voxel), F(thr), res, grid, np.int32(valid)
        assert (valid == 0) == (thr > 1.0)
        zero_fresh = several = straddle = slab = 0
        for t, (base, cl) in enumerate(zip(bases, trial_cands)):
            bo = np.array([o for o, _ in base], np.int32); bp = np.array([p for _, p in base], F).reshape(-1, 16)
            bscore, bagree = ref.coverage(bo, bp)
            agree, score = np.zeros(len(cl), np.int32), np.zeros(len(cl), F)
            for k, (o, p) in enumerate(cl):
                score[k], agree[k] = ref.coverage(np.append(bo, o), np.concatenate([bp, np.asarray(p, F).reshape(1, 16)]))
            pre = f"cov{j}_t{t}_"
            out[pre + "base_obj"], out[pre + "base_pose"], out[pre + "base_static"] = bo, bp, obj_static[bo] if len(bo) else np.zeros(0, np.int32)
            out[pre + "cand_obj"], out[pre + "cand_pose"] = np.array([o for o, _ in cl], np.int32), np.array([p for _, p in cl], F).reshape(-1, 16)
            out[pre + "base_agree"], out[pre + "base_score"], out[pre + "agree"], out[pre + "score"] = np.int32(bagree), bscore, agree, score
            if valid == 0:
                assert bscore == 0 and (score == 0).all() and (agree == 0).all()
                continue
            origin, rres = R.grid_shape(bmin, bmax, voxel)
            for k, (o, p) in enumerate(cl):
                c = R.cells(origin, rres, voxel, R.xform(p, objects[o])); c = c[c >= 0]; c = c[grid[c] > 0]
                several += int(len(c) > len(np.unique(c)))
                straddle += int(len(np.unique(c >> 5)) > 1)
                zero_fresh += int(agree[k] == bagree and len(c) > 0)
                if o == PART and voxel == 0.05:
                    need = R.live_box_bytes(grid, bmin, bmax, voxel, objects, [(a, b, obj_static[a]) for a, b in base], (o, p))
                    assert t != 0 or need > LOW_LDS_BUDGET, ("the partition's sub-box fits the lowered LDS budget", need)
                    slab += int(need > LOW_LDS_BUDGET)
            small = [R.live_box_bytes(grid, bmin, bmax, voxel, objects, [(a, b, obj_static[a]) for a, b in base], c) for c in cl]
            assert not cl or any(0 < b <= LOW_LDS_BUDGET for b in small), ("no candidate keeps the LDS route under the lowered budget", small)
            print(f"{name}: cov{j} trial {t}: base {len(base)} placements agree {bagree}, {len(cl)} candidates, agree {agree.min() if len(cl) else 0}..{agree.max() if len(cl) else 0} of {valid}")
        if valid:
            assert zero_fresh > 0, "no candidate whose scene-active cells the base already covers"
            assert several > 0 and straddle > 0 and (slab > 0 or voxel != 0.05)
    path = os.path.join(out_dir, f"arrange_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(pos0)} level-0 points, {len(props)} proposals ({int(prop_static.sum())} static), object sizes {sizes}, {os.path.getsize(path)} bytes -> {path}")
    sys.stdout.flush()


def hard_child(lib, out_dir):
    """arrange_hard.npz.  One class table ("nowall": no wall class, "unlabelled" is static) and one database per case."""
    import hard_shapes as H
    out = {}
    for voxel, cell0 in H.ARR_CASES:
        # ---- coverage: base + every candidate ----
        a = H.arrangement(voxel, cell0)
        ref = Ref(lib, FIXTURES["nowall"])
        for k, pos in enumerate(a["objects"]):
            assert ref.add_object(pos, 5, k) == k and not ref.L.fx_is_static(ref.h, k)
        scene = np.ascontiguousarray(a["scene"], F)
        cls, q = np.zeros(len(scene), np.int32), np.ones(len(scene), F)
        ref.L.fx_set_scene(ref.h, fp(scene), fp(cls), fp(q), len(scene), fp(scene), fp(q), len(scene), fp(H.ARR_BMIN), fp(H.ARR_BMAX))
        res, grid = ref.scene_grid(voxel, 0.0)
        assert (res == a["res"]).all() and grid[0] == int(cell0)
        bo = np.array([o for o, _, _ in a["base"]], np.int32); bp = np.array([p for _, p, _ in a["base"]], F).reshape(-1, 16)
        assert not any(s for _, _, s in a["base"])
        bscore, bagree = ref.coverage(bo, bp)
        agree, score = np.zeros(len(a["cands"]), np.int32), np.zeros(len(a["cands"]), F)
        for k, (o, p) in enumerate(a["cands"]):
            score[k], agree[k] = ref.coverage(np.append(bo, o), np.concatenate([bp, np.asarray(p, F).reshape(1, 16)]))
        pre = H.arr_key("cov", voxel, cell0)
        out[pre + "crc"], out[pre + "names"], out[pre + "res"] = H.cloud_crcs(scene, a["objects"]), np.array(a["names"], "S24"), res
        out[pre + "grid"], out[pre + "valid"] = np.packbits(grid), np.int32((grid > 0).sum())
        out[pre + "base_agree"], out[pre + "base_score"], out[pre + "agree"], out[pre + "score"] = np.int32(bagree), bscore, agree, score
        f = dict(zip(a["names"], agree - bagree))
        assert set(np.unique(grid)) == {0, 1} and f["non_finite"] == f["off_grid"] == f["empty"] == 0 and f["three_cells_5000"] == 3, f
        print(f"hard: coverage voxel {voxel} cell0 {int(cell0)}: {int((grid > 0).sum())} valid cells, base agree {bagree}, fresh {dict((k, int(v)) for k, v in f.items())}")
        # ---- saliency ----
        s = H.saliency_case(voxel, cell0)
        ref = Ref(lib, FIXTURES["nowall"])
        assert ref.class_idx("wall") == -1 and ref.class_idx("floor") == 2
        static = {int(o): int(st) for o, st in zip(s["prop_obj"], s["prop_static"])}
        for k, pos in enumerate(s["objects"]):
            assert ref.add_object(pos, 0 if static.get(k, 1) else 5, k) == k and ref.L.fx_is_static(ref.h, k) == static.get(k, 1)
        scene, cls = np.ascontiguousarray(s["scene"], F), np.ascontiguousarray(s["cls"], np.int32)
        q = np.full(len(scene), 0.25, F)
        ref.L.fx_set_scene(ref.h, fp(scene), fp(cls), fp(q), len(scene), fp(scene), fp(q), len(scene), fp(H.ARR_BMIN), fp(H.ARR_BMAX))
        for o, p in zip(s["prop_obj"], s["prop_pose"]):
            ref.L.fx_add_proposal(ref.h, int(o), fp(np.ascontiguousarray(p, F)))
        res, org, grid = ref.saliency(voxel)
        pre = H.arr_key("sal", voxel, cell0)
        out[pre + "crc"], out[pre + "res"], out[pre + "grid"], out[pre + "quality"] = H.cloud_crcs(scene, s["objects"]), res, np.packbits(grid), q.copy()
        assert set(np.unique(q)) == {F(0.0), F(1.0)} and grid[0] == int(cell0) and q[-1] == F(cell0), (grid[0], q[-4:])
        print(f"hard: saliency voxel {voxel} cell0 {int(cell0)}: {int(grid.sum())} lit cells, {int(q.sum())} of {len(q)} salient points, cell 0 = {grid[0]}")
    path = os.path.join(out_dir, "arrange_hard.npz")
    np.savez_compressed(path, **out)
    print(f"hard: {os.path.getsize(path)} bytes -> {path}")
    sys.stdout.flush()


def time_child(lib):
    """The reference's own time for the inputs of tools/arrange_timing.py (this machine, one thread; context only)."""
    import importlib.util
    import time
    spec = importlib.util.spec_from_file_location("arrange_timing", os.path.join(ROOT, "tools", "arrange_timing.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    pts, lo, hi, objs, base, cand, inst = T.inputs()
    ref = Ref(lib, FIXTURES["room"])
    for k, o in enumerate(objs):
        ref.add_object(o, 5, k)
    wall = ref.add_object(objs[0], 1, len(objs))               # the stand-in for static proposals
    pos0 = np.ascontiguousarray(pts, F); cls = np.ascontiguousarray(np.where(inst < 3, np.where(inst == 0, 2, 1), 5), np.int32)
    q0 = np.zeros(len(pos0), F)
    ref.L.fx_set_scene(ref.h, fp(pos0), fp(cls), fp(q0), len(pos0), fp(pos0), fp(q0), len(pos0), fp(lo), fp(hi))
    for o, p in cand:
        ref.L.fx_add_proposal(ref.h, int(o), fp(np.ascontiguousarray(p, F)))
    for o, p in cand[:16]:
        ref.L.fx_add_proposal(ref.h, wall, fp(np.ascontiguousarray(p, F)))
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); ref.saliency(0.15); ts.append(time.perf_counter() - t0)
    print(f"reference CPU (this machine, one thread): rsao_compute_scene_saliency, {len(cand) + 16} proposals, {len(pos0)} level-0 points: median {1e3 * np.median(ts):.2f} ms, {int(q0.sum())} salient points")
    q0[:] = 1.0
    ref.scene_grid(0.05, 0.5)
    bo = np.array([o for o, _, _ in base], np.int32); bp = np.array([p for _, p, _ in base], F)
    t0 = time.perf_counter()
    for o, p in cand:
        ref.coverage(np.append(bo, o), np.concatenate([bp, np.asarray(p, F).reshape(1, 16)]))
    print(f"reference CPU (this machine, one thread): rsao__compute_scene_coverage_score, 256 arrangements of 9 placements: {1e3 * (time.perf_counter() - t0):.1f} ms (fx_coverage's own recount of the grids included)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="only print the reference's CPU time for the inputs of tools/arrange_timing.py")
    ap.add_argument("--hard", action="store_true", help="write arrange_hard.npz (the hostile cases of tests/hard_shapes.py) instead of the room fixtures")
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--child", nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        return time_child(a.child[0]) if a.child[1] == "TIME" else hard_child(a.child[0], a.out) if a.child[1] == "HARD" else child(a.child[0], a.out, a.child[1])
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as tmp:
        lib = os.path.join(tmp, "libarrfx.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++11", "-fPIC", "-w", "-shared",
                               f"-I{a.ref}/lib", f"-I{a.ref}/lib/rs", f"-I{a.ref}/apps/pose_proposal", f"-I{a.ref}/apps/segment_transfer", "-o", lib,
                               os.path.join(here, "driver.cpp"), os.path.join(a.ref, "apps", "segment_transfer", "arrangement_optimization.cpp"), "-lm"])
        for name in (["TIME"] if a.time else ["HARD"] if a.hard else FIXTURES):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, name, "--out", a.out], stdout=subprocess.PIPE, text=True)
            print("\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("RSAO_SALIENCY")))
            if r.returncode != 0:
                raise SystemExit(f"generation of {name} failed (exit {r.returncode}: an assert of the reference or of this script)")


if __name__ == "__main__":
    main()
