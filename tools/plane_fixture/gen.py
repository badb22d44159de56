"""Writes tests/golden/planes_<name>.npz from the REFERENCE's own rspf__detect_floor, rspf__detect_walls, evaluate_plane_model,
remove_inliers, rspf__gather_model_inliers, rspf_relabel_walls_and_floors and msh_discrete_distribution_*
(lib/rs/rs_pointcloud_filters.cpp:96-323, 617-671; lib/msh/msh_std.h:1863-1941).

    python tools/plane_fixture/gen.py [--ref /path/to/reference] [--out tests/golden]

Run once, by hand, where the reference tree is available; no test runs it.  rspf_detector_params_t is defined inside the
reference's .cpp, so the compiled translation unit is a scratch file in a temporary directory outside the tree: that file's lines
1-14 and 16-879 followed by driver.cpp (the recipe the test infrastructure's Makefile uses for the filters library, with its two checks), compiled with
-O2 -std=c++11 and no -march: no FMA contraction.  The scratch file goes with the directory.

Fixtures (tests/test_planes_cpu.py, tests/test_gpu_planes.py compare every array bit for bit):
  planes_room    a 2 m x 2 m x 0.6 m room with one chair as a level-2 cloud; both candidate masks; per round (0: the floor, 1..: the
                 walls) the sampled triples, normals (the centre is the triple's first point), up-test flags, ALL hypothesis counts from evaluate_plane_model, the
                 best index and the mask after remove_inliers; the models and counts the two detect functions return.
  planes_quirks  cases a-e of small clouds: (a) no wall hypothesis passes the up test, the pop removes the floor; (b) the same
                 without a floor: inputs only, the reference would pop an empty array; (c) duplicated lattice points: ties;
                 (d) a floor set of one candidate; (e) a count threshold that ends the loop after one round.  The hypotheses' normals
                 are kept for a and d only (size).
  planes_gather  a level-0-like and a level-1-like cloud, four hand-made models (one invalid, two overlapping), the index lists of
                 both parameter sets, class / instance ids before and after the relabel.
  planes_hostile trimmed subsets of the families of tests/hard_planes.py, inputs included: per vote case 512 points x 64 hypotheses,
                 evaluate_plane_model's counts under three masks and remove_inliers' masks for eight planes; per gather family (257
                 points) the index lists of both parameter sets and the ids before and after the relabel; the probe room and one tie
                 cloud with every round of the detection.
The per-round recordings are replayed from the reference's pieces; every replay is checked here against what the reference's two
detect functions return for the same input.

    python tools/plane_fixture/gen.py --time

prints the reference's own time for the detect call of tools/plane_timing.py (this machine, one thread; context only)."""
import argparse
import ctypes as C
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
LARGEST = 757075          # the largest fixture there is (scene.npz)
FLOOR_ITERS, WALL_ITERS = 2500, 5000          # rs_pointcloud_filters.cpp:149,219
REF_CALL = dict(dot=F(0.8), dist=F(0.033), count=250)          # :503-505
PRE = ["cassert", "cmath", "cstring", "cstdint", "cstdarg", "cstddef", "cstdbool", "cstdio", "cstdlib", "cfloat", "cctype", "algorithm"]


class Models(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("center", "normal", "axes", "extends", "valid", "up_dot", "n_inliers")]


def build(ref, tmp):
    src = os.path.join(ref, "lib", "rs", "rs_pointcloud_filters.cpp")
    lines = open(src).read().split("\n")
    assert lines[14].replace(" ", "").strip() == '#include"GCoptimization.h"', "line 15 is not the gco include"
    assert lines[878].startswith("}"), "line 879 does not close rspf_arrangement_to_labels"
    here = os.path.dirname(os.path.abspath(__file__))
    gen = os.path.join(tmp, "planes_gen.cpp")
    with open(gen, "w") as f:
        f.write("\n".join(lines[:14] + lines[15:879]) + "\n" + open(os.path.join(here, "driver.cpp")).read())
    lib = os.path.join(tmp, "librsfx_planes.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++11", "-fPIC", "-w", "-shared", f"-I{ref}/lib", f"-I{ref}/lib/rs", f"-I{ref}/apps/segment_transfer"]
    for h in PRE:
        cmd += ["-include", h]
    subprocess.check_call(cmd + ["-o", lib, gen, "-lm"])
    L = C.CDLL(lib)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    L.fx_detect.argtypes = [vp, vp, i64, f32, f32, i64, vp, vp, vp, vp, vp]
    L.fx_sample.argtypes = [vp, i64, i32, i32, vp]
    L.fx_score.argtypes = [vp, i64, vp, vp, i32, f32, f32, vp, vp, vp, vp]
    L.fx_remove.argtypes = [vp, i64, vp, vp, vp, f32]
    L.fx_votes.argtypes = [vp, i64, vp, vp, vp, i32, f32, vp]
    L.fx_gather.argtypes = [vp, vp, i64, vp, i32, f32, f32, i32, i32, vp, vp]
    L.fx_relabel.argtypes = [vp, vp, i64, vp, i32, i32, i32, i32, vp, vp]
    return L


def detect(L, pos, nor, dot, dist, count):
    c = np.zeros((64, 3), F); nn = np.zeros((64, 3), F); k = np.zeros(64, np.int64)
    m = Models(c.ctypes.data, nn.ctypes.data, None, None, None, None, k.ctypes.data)
    nf, nw, nm = C.c_int32(), C.c_int32(), C.c_int32(); s = C.c_double()
    L.fx_detect(pos.ctypes.data, nor.ctypes.data, len(pos), float(dot), float(dist), int(count), C.addressof(m), C.addressof(nf), C.addressof(nw),
                C.addressof(nm), C.addressof(s))
    assert nm.value <= 64
    return dict(centers=c[:nm.value].copy(), normals=nn[:nm.value].copy(), n_inliers=k[:nm.value].copy(), n_floors=nf.value, n_walls=nw.value,
                seconds=s.value)


def masks(nor, dot):
    """:141-146, :209-214 in fp32"""
    d = nor[:, 0] * F(0) + nor[:, 1] * F(1) + nor[:, 2] * F(0)
    a = np.where(d < 0, -d, d)
    return (d > F(dot)).astype(np.uint8), (a < (F(1) - F(dot))).astype(np.uint8)


def one_round(L, pos, w, n_iter, distinct, dot, dist):
    idx = np.zeros((n_iter, 3), np.int32)
    L.fx_sample(w.ctypes.data, len(pos), n_iter, distinct, idx.ctypes.data)
    c = np.zeros((n_iter, 3), F); nn = np.zeros((n_iter, 3), F); valid = np.zeros(n_iter, np.uint8); counts = np.zeros(n_iter, np.int32)
    L.fx_score(pos.ctypes.data, len(pos), w.ctypes.data, idx.ctypes.data, n_iter, float(dot), float(dist), c.ctypes.data, nn.ctypes.data,
               valid.ctypes.data, counts.ctypes.data)
    if not distinct:
        valid[:] = 1
    scored = np.where(valid != 0, counts, 0)
    best = int(np.argmax(scored)) if scored.max() > 0 else -1          # the first of the maximal counts: strict > (:181, :241)
    return dict(idx=idx, center=c, normal=nn, valid=valid, counts=counts, best=np.int32(best), mask_before=(w > 0.01).astype(np.uint8))


def replay(L, pos, nor, dot, dist, count):
    """The rounds of the two detect functions, from the reference's pieces; checked against the functions themselves."""
    floor_mask, wall_mask = masks(nor, dot)
    rounds, models = [], []
    w = floor_mask.astype(np.float64)
    r = one_round(L, pos, w, FLOOR_ITERS, 0, dot, dist)
    r["mask_after"] = r["mask_before"].copy()
    rounds.append(r)
    n_floors = 0
    if r["best"] >= 0:
        models.append((r["center"][r["best"]], r["normal"][r["best"]], int(r["counts"][r["best"]]))); n_floors = 1
    w = wall_mask.astype(np.float64)
    best = (np.zeros(3, F), np.zeros(3, F), 0)
    n_walls = 0
    while True:
        r = one_round(L, pos, w, WALL_ITERS, 1, dot, dist)
        best = (best[0], best[1], 0)
        if r["best"] >= 0:
            best = (r["center"][r["best"]].copy(), r["normal"][r["best"]].copy(), int(r["counts"][r["best"]]))
            models.append(best)
        L.fx_remove(pos.ctypes.data, len(pos), w.ctypes.data, best[0].ctypes.data, best[1].ctypes.data, float(dist))
        r["mask_after"] = (w > 0.01).astype(np.uint8)
        rounds.append(r)
        n_walls += 1
        if not best[2] > count:
            break
    assert models, "the reference would pop an empty array"
    models.pop(); n_walls -= 1
    want = detect(L, pos, nor, dot, dist, count)
    assert want["n_floors"] == n_floors and want["n_walls"] == n_walls and len(want["centers"]) == len(models)
    for k, m in enumerate(models):
        assert want["centers"][k].tobytes() == m[0].tobytes() and want["normals"][k].tobytes() == m[1].tobytes() and want["n_inliers"][k] == m[2], k
    return floor_mask, wall_mask, rounds, want


def pack(prefix, pos, nor, dot, dist, count, floor_mask, wall_mask, rounds, want, normals=True):
    out = {prefix + "pos": pos, prefix + "nor": nor, prefix + "dot_threshold": F(dot), prefix + "dist_threshold": F(dist),
           prefix + "count_threshold": np.int64(count), prefix + "floor_mask": floor_mask, prefix + "wall_mask": wall_mask,
           prefix + "n_rounds": np.int32(len(rounds)), prefix + "centers": want["centers"], prefix + "normals": want["normals"],
           prefix + "n_inliers": want["n_inliers"], prefix + "n_floors": np.int32(want["n_floors"]), prefix + "n_walls": np.int32(want["n_walls"])}
    for k, r in enumerate(rounds):
        for key, a in r.items():
            if key != "center" and (normals or key != "normal"):          # the centre is pos[idx[:, 0]], bit for bit: not stored
                out[f"{prefix}r{k}_{key}"] = a
        assert r["center"].tobytes() == pos[r["idx"][:, 0]].tobytes()
    return out


def save(out_dir, name, out):
    path = os.path.join(out_dir, f"planes_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < LARGEST, f"{path}: {size} bytes, not below the largest fixture there is"
    return path, size


def ties(rounds):
    return [k for k, r in enumerate(rounds) if r["best"] >= 0 and (np.where(r["valid"] != 0, r["counts"], 0) == r["counts"][r["best"]]).sum() > 1]


def write_room(L, out_dir):
    s = synth.make_scene(seed=31, width=2.0, depth=2.0, height=0.6, density=1400.0, objects=("chair",))
    pos, nor = np.ascontiguousarray(s["points"], F), np.ascontiguousarray(s["normals"], F)
    assert 8000 <= len(pos) <= 20000, len(pos)
    fm, wm, rounds, want = replay(L, pos, nor, **REF_CALL)
    assert len(rounds) - 1 >= 3 and want["n_floors"] == 1, (len(rounds), want["n_floors"])
    out = pack("", pos, nor, REF_CALL["dot"], REF_CALL["dist"], REF_CALL["count"], fm, wm, rounds, want)
    out["tied_rounds"] = np.array(ties(rounds), np.int32)          # may be empty: planes_quirks case c records ties
    path, size = save(out_dir, "room", out)
    print(f"room: {len(pos)} points, {int(fm.sum())} floor / {int(wm.sum())} wall candidates, {len(rounds) - 1} wall rounds, models "
          f"{want['n_inliers'].tolist()}, tied rounds {out['tied_rounds'].tolist()}, {size} bytes -> {path}")


def lattice(origin, eu, ev, nu, nv, normal):
    a, b = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    P = np.asarray(origin, np.float64) + a.reshape(-1, 1) * np.asarray(eu, np.float64) + b.reshape(-1, 1) * np.asarray(ev, np.float64)
    return P, np.tile(np.asarray(normal, np.float64), (len(P), 1))


def patch(rng, origin, eu, ev, normal, n, jitter=0.002):
    P = np.asarray(origin, np.float64) + rng.uniform(0, 1, (n, 1)) * np.asarray(eu, np.float64) + rng.uniform(0, 1, (n, 1)) * np.asarray(ev, np.float64)
    P = P + rng.normal(0, jitter, P.shape)
    N = np.tile(np.asarray(normal, np.float64), (n, 1)) + rng.normal(0, 0.02, (n, 3))
    return P, N / np.linalg.norm(N, axis=1, keepdims=True)


def cloud(rng, parts):
    P = np.concatenate([p[0] for p in parts]); N = np.concatenate([p[1] for p in parts])
    o = rng.permutation(len(P))
    return np.ascontiguousarray(P[o], F), np.ascontiguousarray(N[o], F)


def write_quirks(L, out_dir):
    rng = np.random.default_rng(501)
    out = {}
    floor = lambda n: patch(rng, (0, 0, 0), (1.5, 0, 0), (0, 0, 1.5), (0, 1, 0), n)
    wall_x = lambda n: patch(rng, (0, 0, 0), (0, 0.6, 0), (0, 0, 1.5), (1, 0, 0), n)
    wall_z = lambda n: patch(rng, (0, 0, 0), (1.5, 0, 0), (0, 0.6, 0), (0, 0, 1), n)

    def clutter(n):
        P = rng.uniform(0.2, 1.3, (n, 3)); N = rng.normal(0, 1, (n, 3)); N[:, 1] = 0
        return P, N / np.linalg.norm(N, axis=1, keepdims=True)

    def flat_walls(n):          # horizontal normals, positions all at y = 0.25 exactly
        P = rng.uniform(0, 1.5, (n, 3)); P[:, 1] = 0.25
        return P, np.tile([1.0, 0.0, 0.0], (n, 1))

    # (a) no wall hypothesis passes the up test: round 1 detects nothing, the zero plane removes every candidate, the pop takes the floor
    pos, nor = cloud(rng, [floor(600), flat_walls(300)])
    fm, wm, rounds, want = replay(L, pos, nor, F(0.8), F(0.033), 250)
    assert want["n_floors"] == 1 and want["n_walls"] == 0 and len(want["centers"]) == 0 and len(rounds) == 2 and rounds[1]["best"] == -1
    assert not rounds[1]["valid"].any() and not rounds[1]["mask_after"].any()
    out.update(pack("a_", pos, nor, 0.8, 0.033, 250, fm, wm, rounds, want))
    # (b) the same with a floor set of one candidate: no floor, nothing to pop.  Inputs only: the reference is not run on it.
    one = (np.array([[0.7, 0.0, 0.7]]), np.array([[0.0, 1.0, 0.0]]))
    pos, nor = cloud(rng, [one, flat_walls(300)])
    fm, wm = masks(nor, F(0.8))
    assert fm.sum() == 1 and wm.sum() == 300
    out.update({"b_pos": pos, "b_nor": nor, "b_dot_threshold": F(0.8), "b_dist_threshold": F(0.033), "b_count_threshold": np.int64(250)})
    # (c) exact lattices, every point four times: distinct triples give identical planes and counts
    parts = [lattice((0, 0, 0), (0.125, 0, 0), (0, 0, 0.125), 12, 12, (0, 1, 0)), lattice((0, 0.0625, 0), (0, 0.0625, 0), (0, 0, 0.125), 8, 12, (1, 0, 0)),
             lattice((0.125, 0.0625, 0), (0.125, 0, 0), (0, 0.0625, 0), 11, 8, (0, 0, 1)), clutter(40)]
    parts = [(np.repeat(p[0], 4, axis=0), np.repeat(p[1], 4, axis=0)) for p in parts[:3]] + parts[3:]
    pos, nor = cloud(rng, parts)
    fm, wm, rounds, want = replay(L, pos, nor, F(0.8), F(0.033), 100)
    t = ties(rounds)
    assert 0 in t and len(t) >= 2 and want["n_floors"] == 1 and want["n_walls"] >= 1, (t, want["n_walls"])
    out.update(pack("c_", pos, nor, 0.8, 0.033, 100, fm, wm, rounds, want, normals=False)); out["c_tied_rounds"] = np.array(t, np.int32)
    # (d) a floor set of one candidate: every floor hypothesis is NaN, no floor, no refusal
    pos, nor = cloud(rng, [one, wall_x(500), wall_z(400), clutter(40)])
    fm, wm, rounds, want = replay(L, pos, nor, F(0.8), F(0.033), 100)
    assert fm.sum() == 1 and want["n_floors"] == 0 and np.isnan(rounds[0]["normal"]).all() and not rounds[0]["counts"].any() and want["n_walls"] == 2
    out.update(pack("d_", pos, nor, 0.8, 0.033, 100, fm, wm, rounds, want))
    # (e) a count threshold no wall reaches: one round, and the pop takes the wall it found
    pos, nor = cloud(rng, [floor(600), wall_x(500), wall_z(400), clutter(40)])
    fm, wm, rounds, want = replay(L, pos, nor, F(0.8), F(0.033), 100000)
    assert len(rounds) == 2 and rounds[1]["best"] >= 0 and want["n_walls"] == 0 and want["n_floors"] == 1 and len(want["centers"]) == 1
    out.update(pack("e_", pos, nor, 0.8, 0.033, 100000, fm, wm, rounds, want, normals=False))
    path, size = save(out_dir, "quirks", out)
    print(f"quirks: a-e, {size} bytes -> {path}")


def gather(L, pos, nor, M, dot, dist, check_validity, check_extends):
    m = len(M["center"])
    h = Models(M["center"].ctypes.data, M["normal"].ctypes.data, M["axes"].ctypes.data, M["extends"].ctypes.data, M["valid"].ctypes.data,
               M["up_dot"].ctypes.data, None)
    index = np.zeros(m * len(pos) + 1, np.int32); offsets = np.zeros(m + 1, np.int64)
    L.fx_gather(pos.ctypes.data, nor.ctypes.data, len(pos), C.addressof(h), m, float(dot), float(dist), int(check_validity), int(check_extends),
                index.ctypes.data, offsets.ctypes.data)
    return index[:offsets[m]].copy(), offsets


def write_gather(L, out_dir):
    rng = np.random.default_rng(502)
    # models: 0 the floor, 1 the wall x = 0, 2 invalid (the wall z = 0), 3 a second, smaller quad in the floor's plane whose
    # features call it a wall (normal_up_dot <= 0.8): a point inside 0 and 3 has each field decided by model 0
    M = dict(center=np.array([[1.0, 0, 1.0], [0, 0.3, 1.0], [1.0, 0.3, 0], [0.5, 0.004, 0.5]], F),
             normal=np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 1, 0]], F),
             axes=np.array([[1, 0, 0, 0, 0, 1, 0, 1, 0], [0, 0, 1, 0, 1, 0, 1, 0, 0], [1, 0, 0, 0, 1, 0, 0, 0, 1], [1, 0, 0, 0, 0, 1, 0, 1, 0]], F),
             extends=np.array([[0.75, 0.5, -0.875, -0.625], [0.8, 0.25, -0.9, -0.2], [0.9, 0.3, -0.9, -0.3], [0.7, 0.7, -0.3, -0.3]], F),
             valid=np.array([1, 1, 0, 1], np.int8), up_dot=np.array([1.0, 0.0, 0.0, 0.5], F))
    out = {"model_" + k: v for k, v in M.items()}
    # hand-placed floor points of model 0 (centre (1, 0, 1), x in [0.125, 1.75], z in [0.375, 1.5]): exactly on the edges, just
    # outside the three tested ones, and beyond the fourth, untested one (z > 1.5 within the x range), which the reference accepts
    special = np.array([[1.75, 0, 1.0], [1.7500001, 0, 1.0], [0.125, 0, 1.0], [0.12499999, 0, 1.0], [1.0, 0, 0.375], [1.0, 0, 0.37499997],
                        [1.0, 0, 1.5], [1.0, 0, 1.9], [0.5, 0, 1.95], [1.75, 0, 0.375], [0.125, 0, 0.375], [1.9, 0, 1.9], [0.0, 0, 1.9],
                        [0.6, 0.01, 0.6], [0.3, 0.0, 0.7], [0.75, 0.02, 0.75]], np.float64)
    special = (special, np.tile([0.0, 1.0, 0.0], (len(special), 1)))
    for name, density, seed in (("l0", 650.0, 41), ("l1", 300.0, 42)):
        s = synth.make_scene(seed=seed, width=2.0, depth=2.0, height=0.6, density=density, objects=("chair",))
        P, N = s["points"].astype(np.float64), s["normals"].astype(np.float64)
        pos, nor = cloud(rng, [(P, N), special])
        assert 1500 <= len(pos) <= 6000, len(pos)
        out[name + "_pos"], out[name + "_nor"] = pos, nor
    for name, cl, dot, dist, cv, ce in (("plain", "l0", 0.8, 0.05, 0, 0), ("checked", "l1", 0.0, 0.05, 1, 1)):
        index, offsets = gather(L, out[cl + "_pos"], out[cl + "_nor"], M, F(dot), F(dist), cv, ce)
        out[name + "_index"], out[name + "_offsets"] = index, offsets
        out[name + "_dot_threshold"], out[name + "_dist_threshold"] = F(dot), F(dist)
        assert (np.diff(offsets) > 0).sum() >= (3 if cv else 4), offsets
    o = out["checked_offsets"]
    assert o[2] == o[3], "the invalid model gathered something"
    in0, in3 = set(out["checked_index"][o[0]:o[1]].tolist()), set(out["checked_index"][o[3]:o[4]].tolist())
    assert in0 & in3 and in3 - in0, "no point inside two valid models, or none in the second alone"
    # the relabel: ids before and after.  classes: 0 unlabelled, 1 wall, 2 floor, 5 something else
    pos, nor = out["l1_pos"], out["l1_nor"]
    n = len(pos)
    cls = rng.choice(np.array([0, 0, 0, 1, 2, 5], np.int32), n).astype(np.int32)
    inst = rng.choice(np.array([3, 7, 1023, 1024, 1024, 2000], np.int32), n).astype(np.int32)
    out["class_before"], out["instance_before"] = cls.copy(), inst.copy()
    h = Models(M["center"].ctypes.data, M["normal"].ctypes.data, M["axes"].ctypes.data, M["extends"].ctypes.data, M["valid"].ctypes.data,
               M["up_dot"].ctypes.data, None)
    L.fx_relabel(pos.ctypes.data, nor.ctypes.data, n, C.addressof(h), 4, 2, 1, 0, cls.ctypes.data, inst.ctypes.data)
    out["class_after"], out["instance_after"] = cls, inst
    out["floor_idx"], out["wall_idx"], out["unlabelled_idx"] = np.int32(2), np.int32(1), np.int32(0)
    changed = (out["class_before"] != cls) | (out["instance_before"] != inst)
    both = np.array(sorted(in0 & in3))
    assert changed.any() and (cls[both][out["class_before"][both] == 0] == 2).all() and (inst == 1).any() and (inst == 0).any() and (cls == 1).any()
    path, size = save(out_dir, "gather", out)
    print(f"gather: level 0 {len(out['l0_pos'])} points, offsets {out['plain_offsets'].tolist()}; level 1 {n} points, offsets {o.tolist()}, "
          f"{int(changed.sum())} points relabelled, {size} bytes -> {path}")


def write_hostile(L, out_dir):
    """planes_hostile: the reference on trimmed subsets of the families of tests/hard_planes.py (inputs included)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hard_planes as H
    out = {}
    names = []
    for case in H.vote_cases():
        c = H.trimmed(case)
        p = f"votes_{c['name']}_"
        names.append(c["name"])
        n, h, thr = len(c["pos"]), len(c["center"]), float(c["dist_threshold"])
        out.update({p + k: c[k] for k in ("pos", "center", "normal", "dist_threshold")})
        for mname, m in H.vote_masks(c).items():
            w = m.astype(np.float64); counts = np.zeros(h, np.int32)
            L.fx_votes(c["pos"].ctypes.data, n, w.ctypes.data, c["center"].ctypes.data, c["normal"].ctypes.data, h, thr, counts.ctypes.data)
            out[p + "counts_" + mname] = counts
        removed = np.zeros((8, n), np.uint8)
        for j in range(8):                                 # remove_inliers from a full mask, one hypothesis at a time
            w = np.ones(n, np.float64)
            L.fx_remove(c["pos"].ctypes.data, n, w.ctypes.data, c["center"][j].ctypes.data, c["normal"][j].ctypes.data, thr)
            removed[j] = w > 0.01
        out[p + "removed"] = removed
    out["vote_cases"] = np.array(names)
    for name, family in H.GATHER_FAMILIES.items():
        c = family(257)
        M, p = c["models"], f"gather_{name}_"
        m = len(M["center"])
        out.update({p + "pos": c["pos"], p + "nor": c["nor"], p + "class_before": c["cls"], p + "instance_before": c["inst"]})
        out.update({p + "model_" + k: v for k, v in M.items()})
        for pname, dot, dist, cv, ce in (("plain", 0.8, 0.05, 0, 0), ("checked", 0.0, 0.05, 1, 1)):
            out[p + pname + "_index"], out[p + pname + "_offsets"] = gather(L, c["pos"], c["nor"], M, F(dot), F(dist), cv, ce)
        cls, inst = c["cls"].copy(), c["inst"].copy()
        h = Models(M["center"].ctypes.data, M["normal"].ctypes.data, M["axes"].ctypes.data, M["extends"].ctypes.data, M["valid"].ctypes.data,
                   M["up_dot"].ctypes.data, None)
        L.fx_relabel(c["pos"].ctypes.data, c["nor"].ctypes.data, len(c["pos"]), C.addressof(h), m, *c["ids"], cls.ctypes.data, inst.ctypes.data)
        out[p + "class_after"], out[p + "instance_after"] = cls, inst
        assert ((cls != c["cls"]) | (inst != c["inst"])).any(), name
    # the probe room: the masks are those of masks() above; the replay they lead to is checked against the reference's two functions
    r = H.room_with_probes()
    fm, wm, rounds, want = replay(L, r["pos"], r["nor"], **REF_CALL)
    assert want["n_floors"] == 1 and want["n_walls"] >= 2 and int(rounds[1]["best"]) == r["best"]
    out.update(pack("room_", r["pos"], r["nor"], REF_CALL["dot"], REF_CALL["dist"], REF_CALL["count"], fm, wm, rounds, want, normals=False))
    out.update(room_band=r["band"].astype(np.int32), room_probes=r["probes"].astype(np.int32))
    # one tie cloud: the detection, rounds included
    t = H.tie_clouds(("t3",))[0]
    fm, wm, rounds, want = replay(L, t["pos"], t["nor"], F(0.8), F(0.033), t["count_threshold"])
    assert len(ties(rounds)) >= 3, ties(rounds)
    out.update(pack("tie_", t["pos"], t["nor"], 0.8, 0.033, t["count_threshold"], fm, wm, rounds, want, normals=False))
    path, size = save(out_dir, "hostile", out)
    print(f"hostile: vote cases {names}, gather families {list(H.GATHER_FAMILIES)}, probe room {len(r['pos'])} points / {len(rounds)} rounds, "
          f"tie cloud {len(t['pos'])} points, {size} bytes -> {path}")


def time_reference(L):
    import plane_timing as T
    pos, nor = T.detect_case()
    r = detect(L, pos, nor, **REF_CALL)
    print(f"reference CPU (this machine, one thread): rspf__detect_floor + rspf__detect_walls on {len(pos)} points: {r['seconds']:.2f} s, "
          f"{r['n_floors']} floor + {r['n_walls']} walls, inliers {r['n_inliers'].tolist()}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="only print the reference's CPU time for the detect call of tools/plane_timing.py")
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default="", help="write this fixture alone (room, quirks, gather, hostile)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        L = build(a.ref, tmp)
        if a.time:
            return time_reference(L)
        for name, write in (("room", write_room), ("quirks", write_quirks), ("gather", write_gather), ("hostile", write_hostile)):
            if a.only in ("", name):
                write(L, a.out)


if __name__ == "__main__":
    main()
