"""Writes tests/golden/fuse_<name>.npz from the REFERENCE's own rs_pointcloud_copy_by_ids, msh_mat4_inverse, icp_align,
rs_pointcloud_transform and rs_pointcloud_merge, called in the order rsdu_augment_database calls them
(apps/segment_transfer/database_update.cpp:35-85).

    python tools/fuse_fixture/gen.py [--ref /path/to/reference] [--out tests/golden]

Run once, by hand, where the reference tree is available; no test runs it.  driver.cpp is compiled into a temporary directory
outside the tree (-O2 -std=c++11, no -march, as oracle/Makefile compiles the reference: no FMA contraction).

Fixtures (tests/test_fuse_cpu.py, tests/test_gpu_fuse.py compare every array bit for bit):
  fuse_perm   the permutation of rs_pointcloud_merge's shuffle for n in PERM_SIZES, read back from a merge of two planar patches
              whose instance ids carry the element's index.  perm_<n> in full up to 4 097; beyond that the SHA-256 of the array's
              bytes and its first and last 256 entries.
  fuse_chair  a dynamic placement: a scan level 1 of a few thousand points with four instance ids (floor, two walls, a chair), a
              chair model level 0, the chair's pose perturbed.  The scan's and the model's seven arrays, the extracted arrays, xform
              after the ICP, the ICP's error, the seven merged arrays, the sizes of the merged cloud's five levels.
  fuse_wall   a static placement (no ICP) of one wall of a sparser scan, and an id that no scan point carries: nothing extracted.
  fuse_hostile  rs_pointcloud_transform of the points of tests/hard_fuse.py (+-0, subnormal, Inf, NaN, FLT_MAX coordinates; and a
              finite set) under each of its transforms: identity, a translation of 1e4, a rotation, scales of 1e-20 and 1e20, a
              matrix of -0.0, a translation of Inf and NaN.
  fuse_arrangement  the whole loop over an arrangement of five placements in a small room (floor, two walls, a chair, a table), in
              loop order: the chair (dynamic, its pose perturbed), a wall (static), a uidx no scan point carries, the table (dynamic),
              and a novel copy of the chair whose model is what the chair's placement left (model_from = 0: the reference's :51
              after :89) — its model arrays are the first placement's merged arrays, fed back through the same functions.  Per
              placement p: p<k>_model_* (where model_from is -1), p<k>_extracted_*, p<k>_merged_*, p<k>_xform, p<k>_icp_err; and
              uidx, is_static, model_from, poses, n_extracted for all.

    python tools/fuse_fixture/gen.py --time

prints the reference's own times for the two placements of tools/fuse_timing.py (this machine, one thread; context only)."""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from rescan_amd import synth  # noqa: E402

F = np.float32
KEYS = ("pos", "nor", "col", "radii", "qual", "cls", "inst")
PERM_SIZES = (2, 3, 64, 65, 4097, 65537, 200001)
ENDS = 256
LARGEST = 757075          # the largest fixture there is (scene.npz)


class Arrays(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in KEYS]


def empty(n):
    return dict(pos=np.zeros((n, 3), F), nor=np.zeros((n, 3), F), col=np.zeros((n, 3), F), radii=np.zeros(n, F), qual=np.zeros(n, F),
                cls=np.zeros(n, np.int32), inst=np.zeros(n, np.int32))


def handle(a):
    for k in KEYS:
        assert a[k].flags["C_CONTIGUOUS"] and a[k].dtype in (F, np.int32), k
    return Arrays(*[a[k].ctypes.data for k in KEYS])


def attributes(rng, pos, nor, cls, inst):
    n = len(pos)
    return dict(pos=np.ascontiguousarray(pos, F), nor=np.ascontiguousarray(nor, F), col=rng.uniform(0, 1, (n, 3)).astype(F),
                radii=rng.uniform(0.004, 0.012, n).astype(F), qual=rng.uniform(0, 1, n).astype(F),
                cls=np.ascontiguousarray(cls, np.int32), inst=np.ascontiguousarray(inst, np.int32))


def load(lib):
    L = C.CDLL(lib)
    L.fx_augment.restype = C.c_void_p
    L.fx_augment.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p] + [C.c_void_p] * 6
    L.fx_get.argtypes = [C.c_void_p, C.c_void_p]
    L.fx_free.argtypes = [C.c_void_p]
    L.fx_merge_ids.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    L.fx_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return L


def augment(L, scan, model, pose, uidx, is_static):
    """The reference's placement: dict(extracted, xform, err, merged, levels, seconds), merged None when nothing was extracted."""
    ns, nm = len(scan["pos"]), len(model["pos"])
    ext = empty(ns)
    n_ext, n_merged, err = C.c_int64(), C.c_int64(), C.c_float()
    xform = np.zeros(16, F); levels = np.zeros(5, np.int64); seconds = np.zeros(3, np.float64)
    hs, hm, he = handle(scan), handle(model), handle(ext)
    pose = np.ascontiguousarray(pose, F)
    h = L.fx_augment(C.addressof(hs), ns, C.addressof(hm), nm, pose.ctypes.data, int(uidx), int(is_static), C.addressof(he), C.addressof(n_ext),
                     xform.ctypes.data, C.addressof(err), C.addressof(n_merged), levels.ctypes.data, seconds.ctypes.data)
    out = dict(extracted={k: ext[k][:n_ext.value].copy() for k in KEYS}, xform=xform, err=F(err.value), merged=None, levels=levels, seconds=seconds)
    if h:
        m = empty(n_merged.value); hm2 = handle(m)
        L.fx_get(h, C.addressof(hm2)); L.fx_free(h)
        out["merged"] = m
    return out


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def save(out_dir, name, out):
    path = os.path.join(out_dir, f"fuse_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < LARGEST, f"{path}: {size} bytes, not below the largest fixture there is"
    return path, size


def patch(rng, n):
    """n points of a planar patch at the level-0 spacing (0.005: the level build at the end of rs_pointcloud_merge stays cheap)."""
    side = int(np.ceil(np.sqrt(max(n, 1))))
    k = np.arange(n)
    pos = np.stack([(k % side) * 0.005, np.zeros(n), (k // side) * 0.005], axis=1) + rng.normal(0, 0.0005, (n, 3))
    nor = np.tile([0.0, 1.0, 0.0], (n, 1))
    return attributes(rng, pos, nor, np.zeros(n), np.zeros(n))


def write_perm(L, out_dir):
    rng = np.random.default_rng(401)
    out = dict(sizes=np.array(PERM_SIZES, np.int64))
    for n in PERM_SIZES:
        n_a = n // 3
        a, b = patch(rng, n_a), patch(rng, n - n_a)
        ha, hb = handle(a), handle(b)
        perm = np.zeros(n, np.int32)
        L.fx_merge_ids(C.addressof(ha), n_a, C.addressof(hb), n - n_a, perm.ctypes.data)
        assert (np.sort(perm) == np.arange(n)).all(), n
        if n <= 4097:
            out[f"perm_{n}"] = perm
        else:
            out[f"sha256_{n}"], out[f"head_{n}"], out[f"tail_{n}"] = digest(perm), perm[:ENDS], perm[n - ENDS:]
    path, size = save(out_dir, "perm", out)
    print(f"perm: sizes {PERM_SIZES}, {size} bytes -> {path}")


def small_scene(density, seed):
    """A 2 m x 2 m room 0.6 m high with one chair: instance ids 0 (floor), 1 and 2 (walls), 3 (the chair)."""
    return synth.make_scene(seed=seed, width=2.0, depth=2.0, height=0.6, density=density, objects=("chair",))


def write_chair(L, out_dir):
    rng = np.random.default_rng(402)
    s = small_scene(800.0, 21)
    o = s["objects"][0]
    scan = attributes(rng, s["points"], s["normals"], s["class_idx"], s["instance_idx"])
    model = attributes(rng, o["pos"], o["nor"], np.full(len(o["pos"]), o["class_idx"]), np.full(len(o["pos"]), o["uidx"]))
    pose = synth.perturbed_pose(o["pose"], rng)
    r = augment(L, scan, model, pose, o["uidx"], 0)
    n_ext = len(r["extracted"]["pos"])
    assert len(np.unique(scan["inst"])) == 4 and 2000 <= len(scan["pos"]) <= 9000, (np.unique(scan["inst"]), len(scan["pos"]))
    assert n_ext == int((scan["inst"] == o["uidx"]).sum()) and 0 < n_ext <= 16384, n_ext
    # the ICP moved the pose: what it started from is the inverse of the perturbed pose
    start = np.linalg.inv(pose.astype(np.float64).reshape(4, 4).T).T.ravel()
    moved = float(np.linalg.norm(r["xform"].astype(np.float64) - start))
    assert moved > 1e-3, moved
    assert r["merged"] is not None and len(r["merged"]["pos"]) == n_ext + len(model["pos"]) and (r["merged"]["inst"] == o["uidx"]).all()
    out = {"scan_" + k: scan[k] for k in KEYS}
    out.update({"model_" + k: model[k] for k in KEYS})
    out.update({"extracted_" + k: r["extracted"][k] for k in KEYS})
    out.update({"merged_" + k: r["merged"][k] for k in KEYS})
    out.update(pose=pose, uidx=np.int32(o["uidx"]), is_static=np.int32(0), xform=r["xform"], icp_err=r["err"], level_counts=r["levels"],
               max_dist=F(0.05), max_angle=F(10.0 * 0.005555555556 * np.pi))          # msh_deg2rad( 10.0f )
    path, size = save(out_dir, "chair", out)
    print(f"chair: {len(scan['pos'])} scan points, {n_ext} extracted, {len(model['pos'])} model points, ICP error {float(r['err'])!r}, pose moved by "
          f"{moved:.4f} (Frobenius), levels {r['levels'].tolist()}, {size} bytes -> {path}")


def write_wall(L, out_dir):
    rng = np.random.default_rng(403)
    s = small_scene(200.0, 22)
    scan = attributes(rng, s["points"], s["normals"], s["class_idx"], s["instance_idx"])
    pose = synth.pose_matrix(0.3, (0.5, 0.0, 0.2))
    # the wall's model: another sampling of the same plane, in the frame the pose places it from
    wall = synth.make_room_shell(np.random.default_rng(404), 2.0, 2.0, 0.6, 150.0)[1]
    inv = np.linalg.inv(pose.astype(np.float64).reshape(4, 4).T).T.ravel().astype(F)
    model = attributes(rng, synth.apply_pose(inv, wall[0]), synth.apply_pose(inv, wall[1], False), np.full(len(wall[0]), 1), np.full(len(wall[0]), 1))
    r = augment(L, scan, model, pose, 1, 1)
    n_ext = len(r["extracted"]["pos"])
    assert n_ext == int((scan["inst"] == 1).sum()) > 0 and r["merged"] is not None and float(r["err"]) == 0.0
    absent = augment(L, scan, model, pose, 99, 1)
    assert not (scan["inst"] == 99).any() and absent["merged"] is None and len(absent["extracted"]["pos"]) == 0
    out = {"scan_" + k: scan[k] for k in KEYS}
    out.update({"model_" + k: model[k] for k in KEYS})
    out.update({"extracted_" + k: r["extracted"][k] for k in KEYS})
    out.update({"merged_" + k: r["merged"][k] for k in KEYS})
    out.update(pose=pose, uidx=np.int32(1), is_static=np.int32(1), xform=r["xform"], level_counts=r["levels"], absent_uidx=np.int32(99),
               absent_n_extracted=np.int64(0))
    path, size = save(out_dir, "wall", out)
    print(f"wall: {len(scan['pos'])} scan points, {n_ext} extracted, {len(model['pos'])} model points, levels {r['levels'].tolist()}, {size} bytes -> {path}")


def write_hostile(L, out_dir):
    """fuse_hostile: rs_pointcloud_transform of the points of tests/hard_fuse.py under each of its transforms (inputs included)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hard_fuse as H
    out = {}
    for tag, pts in (("", H.points()), ("finite_", H.points(finite=True))):
        out[tag + "a_pos"], out[tag + "a_nor"] = pts["a_pos"], pts["a_nor"]
        for name, x in H.transforms().items():
            pos, nor = pts["a_pos"].copy(), pts["a_nor"].copy()
            L.fx_transform(pos.ctypes.data, nor.ctypes.data, len(pos), x.ctypes.data)
            out[f"{tag}{name}_xform"], out[f"{tag}{name}_pos"], out[f"{tag}{name}_nor"] = x, pos, nor
    out["names"] = np.array(list(H.transforms()))
    z = out["negzero_nor"][(out["a_nor"] == 0).all(axis=1)]
    assert len(z) and not np.signbit(z).any(), "the zero normals under the -0 matrix are not +0"
    assert np.isnan(out["inf_nan_nor"]).all() and np.isinf(out["huge_pos"]).any() and np.isnan(out["huge_pos"]).any()
    path, size = save(out_dir, "hostile", out)
    print(f"hostile: {len(out['a_pos'])} points x {len(out['names'])} transforms, twice, {size} bytes -> {path}")


def write_arrangement(L, out_dir):
    """fuse_arrangement: rsdu_augment_database's loop, placement by placement through fx_augment, a merged result chained in as a
    later placement's model."""
    rng = np.random.default_rng(406)
    s = synth.make_scene(seed=23, width=2.0, depth=2.0, height=0.6, density=330.0, objects=("chair", "table"))
    scan = attributes(rng, s["points"], s["normals"], s["class_idx"], s["instance_idx"])
    chair, table = s["objects"]
    assert chair["kind"] == "chair" and len(np.unique(scan["inst"])) == 5 and 2000 <= len(scan["pos"]) <= 9000, len(scan["pos"])

    def model_of(o):
        return attributes(rng, o["pos"], o["nor"], np.full(len(o["pos"]), o["class_idx"]), np.full(len(o["pos"]), o["uidx"]))
    wall_pose = synth.pose_matrix(0.3, (0.5, 0.0, 0.2))
    wall = synth.make_room_shell(np.random.default_rng(407), 2.0, 2.0, 0.6, 120.0)[1]
    inv = np.linalg.inv(wall_pose.astype(np.float64).reshape(4, 4).T).T.ravel().astype(F)
    wall_model = attributes(rng, synth.apply_pose(inv, wall[0]), synth.apply_pose(inv, wall[1], False), np.full(len(wall[0]), 1), np.full(len(wall[0]), 1))
    # (uidx, is_static, model_from, model, pose)
    plan = [(chair["uidx"], 0, -1, model_of(chair), synth.perturbed_pose(chair["pose"], rng)),
            (1, 1, -1, wall_model, wall_pose),
            (99, 0, -1, model_of(table), table["pose"]),
            (table["uidx"], 0, -1, model_of(table), synth.perturbed_pose(table["pose"], rng)),
            (chair["uidx"], 0, 0, None, synth.perturbed_pose(chair["pose"], rng))]
    out = {"scan_" + k: scan[k] for k in KEYS}
    shapes, n_ext_all = [], []
    for p, (uidx, is_static, model_from, model, pose) in enumerate(plan):
        if model_from >= 0:
            model = shapes[model_from]                                                  # the shape that placement left
            assert len(model["pos"]) == len(out[f"p{model_from}_merged_pos"]), "the dependent placement's model is not the merged cloud"
        else:
            out.update({f"p{p}_model_" + k: model[k] for k in KEYS})
        r = augment(L, scan, model, pose, uidx, is_static)
        n_ext = len(r["extracted"]["pos"])
        assert n_ext == int((scan["inst"] == uidx).sum())
        n_ext_all.append(n_ext)
        out.update({f"p{p}_extracted_" + k: r["extracted"][k] for k in KEYS})
        out[f"p{p}_xform"], out[f"p{p}_icp_err"] = r["xform"], r["err"]
        if r["merged"] is None:
            assert n_ext == 0
            shapes.append(model)                                                        # database_update.cpp:58: the object stays
            continue
        assert len(r["merged"]["pos"]) == n_ext + len(model["pos"]) and (r["merged"]["inst"] == uidx).all()
        if not is_static:
            assert 0 < n_ext <= 16384, n_ext
        out.update({f"p{p}_merged_" + k: r["merged"][k] for k in KEYS})
        shapes.append(r["merged"])
    assert n_ext_all[2] == 0 and "p2_merged_pos" not in out and n_ext_all[1] > 0 and float(out["p1_icp_err"]) == 0.0
    start = np.linalg.inv(plan[0][4].astype(np.float64).reshape(4, 4).T).T.ravel()
    moved = float(np.linalg.norm(out["p0_xform"].astype(np.float64) - start))
    assert moved > 1e-3, moved
    assert len(out["p4_merged_pos"]) == n_ext_all[4] + len(out["p0_merged_pos"])
    out.update(uidx=np.array([q[0] for q in plan], np.int32), is_static=np.array([q[1] for q in plan], np.int32),
               model_from=np.array([q[2] for q in plan], np.int32), poses=np.stack([q[4] for q in plan]).astype(F),
               n_extracted=np.array(n_ext_all, np.int64), max_dist=F(0.05), max_angle=F(10.0 * 0.005555555556 * np.pi))
    path, size = save(out_dir, "arrangement", out)
    print(f"arrangement: {len(scan['pos'])} scan points, extracted {n_ext_all}, merged {[len(x['pos']) for x in shapes]}, the chair's pose moved by "
          f"{moved:.4f} (Frobenius), {size} bytes -> {path}")


def time_reference(L):
    import fuse_timing as T
    rng = np.random.default_rng(405)
    for name, case in (("dynamic", T.dynamic_case()), ("static", T.static_case())):
        ns, nm = len(case["scan_pos"]), len(case["model_pos"])
        scan = attributes(rng, case["scan_pos"], case["scan_nor"], np.zeros(ns), case["scan_ids"])
        model = attributes(rng, case["model_pos"], case["model_nor"], np.zeros(nm), np.full(nm, case["uidx"]))
        r = augment(L, scan, model, case["pose"], case["uidx"], 0 if case["refine"] else 1)
        s = 1e3 * r["seconds"]
        print(f"reference CPU (this machine, one thread), {name}: {len(r['extracted']['pos'])} extracted of {ns} scan points + {nm} model points: "
              f"copy_by_ids + inverse + transform {s[0]:.1f} ms | icp_align {s[1]:.1f} ms | rs_pointcloud_merge with its level build {s[2]:.1f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="only print the reference's CPU times for the placements of tools/fuse_timing.py")
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default="", help="write this fixture alone (perm, chair, wall, hostile, arrangement)")
    a = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as tmp:
        lib = os.path.join(tmp, "librsfx.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++11", "-fPIC", "-w", "-shared", f"-I{a.ref}/lib", f"-I{a.ref}/lib/rs",
                               "-o", lib, os.path.join(here, "driver.cpp"), "-lm"])
        L = load(lib)
        if a.time:
            return time_reference(L)
        for name, write in (("perm", write_perm), ("chair", write_chair), ("wall", write_wall), ("hostile", write_hostile),
                            ("arrangement", write_arrangement)):
            if a.only in ("", name):
                write(L, a.out)


if __name__ == "__main__":
    main()
