"""CPU: coverage by footprints.  The restated footprints (tests/footprint_restate.py) of base and candidates, fed to the library's
host-only rs_hip_footprints_from_arrays / rs_hip_footprints_scores, reproduce every agree, base_agree, score and base_score the
REFERENCE recorded (tests/golden/arrange_room.npz, arrange_nowall.npz, the four sets of arrange_hard.npz), as counts and float bits;
the edge arrangements (empty, repeated and static members, a grid with no valid cell, 1 000 seeded member lists against
ao_restate.coverage); the fixtures hold the routes the GPU tests rely on; the new symbols exist, refuse bad arguments before a
device is touched and rs_hip_coverage_footprints fails loudly without one.  No tolerances anywhere."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import ao_restate as R
import footprint_restate as FR
from test_arrange_cpu import NAMES, fixture, hard_fixture, trials

LIB = os.path.join(ROOT, "rescan_amd", "librescan_hip.so")
DROPIN = os.path.join(ROOT, "rescan_amd", "librescan_dropin.so")
F = np.float32
HARD = [(0.05, True), (0.05, False), (0.15, True), (0.15, False)]


@pytest.fixture(scope="module")
def capi():
    from rescan_amd import build, capi as m
    build.build()
    return m


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def trial_footprints(g, j, base, cand):
    """(placements base + candidates, their restated footprints, their sub-box bytes) on coverage set j of a room fixture."""
    grid = g[f"cov{j}_grid"]
    plc = list(base) + [(o, p, 0) for o, p in cand]
    args = (grid, g["bbox_min"], g["bbox_max"], g[f"cov{j}_voxel"], g["objects"])
    return plc, [FR.footprint(*args, p) for p in plc], [FR.footprint_box_bytes(*args, p) for p in plc]


def hard_footprints(voxel, cell0):
    """(case, scene grid, placements base + candidates, footprints, sub-box bytes) of one hostile set."""
    import hard_shapes as H
    a, grid = H.arrangement_expectations(voxel, cell0)[:2]
    plc = list(a["base"]) + [(o, p, 0) for o, p in a["cands"]]
    args = (grid, H.ARR_BMIN, H.ARR_BMAX, voxel, a["objects"])
    return a, grid, plc, [FR.footprint(*args, p) for p in plc], [FR.footprint_box_bytes(*args, p) for p in plc]


@pytest.mark.parametrize("name", NAMES)
def test_unions_of_footprints_are_the_references_numbers(capi, name):
    g = fixture(name)
    n_arr = 0
    for j, t, pre, base, cand in trials(g):
        plc, fps, _ = trial_footprints(g, j, base, cand)
        for f in fps:
            assert f.dtype == np.int32 and (np.diff(f) > 0).all()
        valid = int(g[f"cov{j}_valid"])
        fp = capi.Footprints.from_arrays(len(g[f"cov{j}_grid"]), valid, *FR.csr(fps))
        assert (fp.n_placements, fp.n_cells, fp.valid_cells, fp.total_cells) == (len(plc), len(g[f"cov{j}_grid"]), valid, sum(map(len, fps)))
        for k, f in enumerate(fps):
            assert fp.cells(k).dtype == np.int32 and (fp.cells(k) == f).all()
        nb = len(base)
        sc, ag = fp.scores([list(range(nb))] + [list(range(nb)) + [nb + k] for k in range(len(cand))])
        assert ag[0] == int(g[pre + "base_agree"]) and bits(sc)[0] == bits(g[pre + "base_score"])[0], (j, t)
        assert (ag[1:] == g[pre + "agree"]).all() and (bits(sc[1:]) == bits(g[pre + "score"])).all(), (j, t)
        # the restatement of the union itself, on the same numbers
        for k in range(len(cand)):
            a, s = FR.union_score(fps, list(range(nb)) + [nb + k], valid)
            assert a == int(g[pre + "agree"][k]) and bits(s)[0] == bits(g[pre + "score"][k])[0]
        n_arr += 1 + len(cand)
    assert n_arr > 150


@pytest.mark.parametrize("voxel,cell0", HARD)
def test_unions_of_hostile_footprints_are_the_references_numbers(capi, voxel, cell0):
    import hard_shapes as H
    g = hard_fixture()
    a, grid, plc, fps, _ = hard_footprints(voxel, cell0)
    pre = H.arr_key("cov", voxel, cell0)
    fp = capi.Footprints.from_arrays(len(grid), int(g[pre + "valid"]), *FR.csr(fps))
    nb = len(a["base"])
    sc, ag = fp.scores([list(range(nb))] + [list(range(nb)) + [nb + k] for k in range(len(a["cands"]))])
    assert ag[0] == int(g[pre + "base_agree"]) and bits(sc)[0] == bits(g[pre + "base_score"])[0]
    assert (ag[1:] == g[pre + "agree"]).all() and (bits(sc[1:]) == bits(g[pre + "score"])).all()


@pytest.mark.parametrize("name", NAMES)
def test_room_fixtures_hold_the_routes(name):
    """What tests/test_gpu_footprints.py relies on, so that a regenerated fixture cannot hollow it out: every trial on a grid with
    valid cells has a non-empty footprint; at the fixture's low LDS budget (64 bytes) the first trial has placements on both routes."""
    g = fixture(name)
    low = int(g["low_lds_budget"])
    assert low == 64
    for j, t, pre, base, cand in trials(g):
        plc, fps, need = trial_footprints(g, j, base, cand)
        if int(g[f"cov{j}_valid"]) > 0 and plc:
            assert any(len(f) for f in fps), (j, t)
        assert all((b == 0) == (len(f) == 0) for b, f in zip(need, fps)) and max(need, default=0) <= 16384
        if int(g[f"cov{j}_valid"]) == 0:
            assert not any(len(f) for f in fps)
        if j == 0 and cand:
            # (as the fixtures stand: 7 to 10 placements of such a trial above 64 bytes, 39 to 42 at or below, 24 to 28 of those without a cell)
            above, below = sum(b > low for b in need), sum(0 < b <= low for b in need)
            assert above >= 5 and below >= 5, (t, above, below)


@pytest.mark.parametrize("voxel,cell0", HARD)
def test_hostile_sets_hold_the_routes(voxel, cell0):
    """Cases on both sides of each lowered budget (the rod's own sub-box, and 4 bytes less), and the shapes the compaction meets."""
    a, grid, plc, fps, need = hard_footprints(voxel, cell0)
    nb = len(a["base"])
    by = dict(zip(a["names"], zip(fps[nb:], need[nb:])))
    rod = by["rod"][1]
    assert 0 < rod <= 16384 and rod % 4 == 0
    for budget in (rod, rod - 4):
        assert any(b > budget for b in need) and any(0 < b <= budget for b in need), budget
    assert sum(b > rod - 4 for b in need) == sum(b > rod for b in need) + 1                  # exactly the budget: LDS; 4 bytes less: the slab
    for k in (255, 256, 257, 5000):
        assert len(by[f"three_cells_{k}"][0]) == 3 and len(by[f"spread_cells_{k}"][0]) == 3    # cells, not points
    for name in ("off_grid", "scene_inactive", "empty", "non_finite"):
        assert len(by[name][0]) == 0 and by[name][1] == 0
    assert len(by["inside_base"][0]) > 0                      # (no base is excluded from a footprint)
    assert len(by["rod"][0]) >= 10 and len(by["faces_x"][0]) > 0 and len(by["faces_y"][0]) > 0 and len(by["faces_z"][0]) > 0


def test_edge_arrangements(capi):
    g = fixture("room")
    j, t, pre, base, cand = next(x for x in trials(g) if x[0] == 0 and x[3] and x[4] and any(s for _, _, s in x[3]))
    plc, fps, _ = trial_footprints(g, j, base, cand)
    valid = int(g[f"cov{j}_valid"])
    grid = g[f"cov{j}_grid"]
    fp = capi.Footprints.from_arrays(len(grid), valid, *FR.csr(fps))
    static = [k for k, p in enumerate(plc) if p[2]]
    busy = int(np.argmax([len(f) for f in fps]))
    assert static and len(fps[busy]) > 0 and all(len(fps[k]) == 0 for k in static)
    sc, ag = fp.scores([[], [busy], [busy, busy, busy], static, static + [busy] + static])
    assert ag.tolist() == [0, len(fps[busy]), len(fps[busy]), 0, len(fps[busy])]
    assert bits(sc).tolist() == bits([F(0) / F(valid), F(len(fps[busy])) / F(valid), F(len(fps[busy])) / F(valid), F(0) / F(valid), F(len(fps[busy])) / F(valid)]).tolist()
    sc0, ag0 = fp.scores([])
    assert len(sc0) == 0 and len(ag0) == 0
    # a scene grid with no valid cell: every score is 0 (:367-368), every footprint empty
    j2, t2, pre2, base2, cand2 = next(x for x in trials(g) if x[0] == 2 and x[4])
    plc2, fps2, _ = trial_footprints(g, 2, base2, cand2)
    assert int(g["cov2_valid"]) == 0
    fp2 = capi.Footprints.from_arrays(len(g["cov2_grid"]), 0, *FR.csr(fps2))
    sc2, ag2 = fp2.scores([[], list(range(len(plc2)))])
    assert bits(sc2).tolist() == [0, 0] and ag2.tolist() == [0, 0]
    # valid == 0 with cells all the same (arrays from a caller): still 0, not a division by zero's result
    fp3 = capi.Footprints.from_arrays(100, 0, [0, 2], [5, 7])
    assert bits(fp3.scores([[0]])[0]).tolist() == [0] and fp3.scores([[0]])[1].tolist() == [2]
    # 1 000 seeded member lists against the whole-arrangement restatement
    rng = np.random.default_rng(1806)
    lists = [rng.integers(0, len(plc), int(rng.integers(0, 9))).tolist() for _ in range(1000)]
    sc, ag = fp.scores(lists)
    one, agree_one = fp.scores([lists[17]])                                          # (and one arrangement per call, as the loop makes them)
    assert bits(one)[0] == bits(sc)[17] and agree_one[0] == ag[17]
    for m, s, a in zip(lists, sc, ag):
        want_a, want_valid, want_s = R.coverage(grid, g["bbox_min"], g["bbox_max"], g[f"cov{j}_voxel"], g["objects"], [plc[k] for k in m])
        assert a == want_a and want_valid == valid and bits(s)[0] == bits(want_s)[0], m
    assert len({int(a) for a in ag}) > 50


def test_new_symbols_exist(capi):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    names = ("rs_hip_coverage_footprints", "rs_hip_footprints_from_arrays", "rs_hip_footprints_destroy", "rs_hip_footprints_info", "rs_hip_footprints_arrays",
             "rs_hip_footprints_scores", "rs_hip_coverage_footprint_routes")
    for s in names:
        assert re.search(r" T %s\b" % s, out), s
        assert s in capi.SIGNATURES
    out = subprocess.check_output(["nm", "-D", "--defined-only", DROPIN], text=True)
    for s in ("rsd_coverage_footprints", "rsd_footprints_score", "rsd_footprints_destroy"):
        assert re.search(r" T %s\b" % s, out), s
    assert callable(capi.Coverage.footprints) and callable(capi.Footprints.from_arrays) and callable(capi.Footprints.scores) and callable(capi.Footprints.cells)
    assert callable(capi.coverage_footprint_routes)
    header = open(os.path.join(ROOT, "include", "rescan_hip.h")).read()
    for s in names:
        assert s + "(" in header
    assert capi.coverage_footprint_routes() == (0, 0)                               # (reads two counters: no device)


def test_arguments_are_checked_before_a_device_is_touched(capi):
    """In a child process (a regression would read through a null pointer).  The calls that return an int give RS_HIP_E_ARG (-2);
    the two that return a handle give NULL and leave RS_HIP_E_ARG's or RS_HIP_E_CAPACITY's text in rs_hip_last_error.  The host-only
    calls then WORK in that process, device or not; rs_hip_coverage_footprints with valid arguments and no device gives NULL and says why."""
    code = r"""
import ctypes as C, sys
lib = C.CDLL(sys.argv[1]); no_gpu = sys.argv[2] == "1"
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
lib.rs_hip_last_error.restype = C.c_char_p
mk = lib.rs_hip_footprints_from_arrays; mk.restype = vp; mk.argtypes = [i64, i64, vp, vp, i32]
sc = lib.rs_hip_footprints_scores; sc.restype = C.c_int; sc.argtypes = [vp, vp, vp, i32, vp, vp]
info = lib.rs_hip_footprints_info; info.restype = C.c_int; info.argtypes = [vp, vp, vp, vp, vp]
arr = lib.rs_hip_footprints_arrays; arr.restype = C.c_int; arr.argtypes = [vp, vp, vp]
lib.rs_hip_footprints_destroy.argtypes = [vp]
fpc = lib.rs_hip_coverage_footprints; fpc.restype = vp; fpc.argtypes = [vp, vp, vp, vp, i32]
off = (i64 * 3)(0, 2, 3); cells = (i32 * 3)(4, 9, 4)
err = lambda: lib.rs_hip_last_error()
refused = lambda h, word: h is None and word in err()
assert refused(mk(10, 5, None, cells, 2), b"bad arguments")
assert refused(mk(10, 5, off, None, 2), b"bad arguments")
assert refused(mk(-1, 0, off, cells, 2), b"bad arguments") and refused(mk(10, -1, off, cells, 2), b"bad arguments") and refused(mk(10, 11, off, cells, 2), b"bad arguments")
assert refused(mk(10, 5, off, cells, -1), b"bad arguments")
assert refused(mk(10, 5, (i64 * 3)(1, 2, 3), cells, 2), b"bad arguments")                      # offsets start at 0
assert refused(mk(10, 5, (i64 * 3)(0, 2, 1), cells, 2), b"offsets decrease at placement 1")
assert refused(mk(10, 5, off, (i32 * 3)(9, 4, 4), 2), b"placement 0")                          # unsorted
assert refused(mk(10, 5, off, (i32 * 3)(4, 4, 4), 2), b"placement 0")                          # duplicate
assert refused(mk(10, 5, off, (i32 * 3)(4, 10, 4), 2), b"placement 0")                         # a cell outside [0, n_cells)
assert refused(mk(10, 5, off, (i32 * 3)(4, 9, -1), 2), b"placement 1")
assert refused(mk(3000000000, 5, off, cells, 2), b"int32 cell index")                          # RS_HIP_E_CAPACITY's case
h = mk(10, 5, off, cells, 2)
assert h
n = i32(); nc = i64(); v = i64(); tot = i64()
assert info(None, C.addressof(n), None, None, None) == -2 and info(h, C.addressof(n), C.addressof(nc), C.addressof(v), C.addressof(tot)) == 0
assert (n.value, nc.value, v.value, tot.value) == (2, 10, 5, 3) and info(h, None, None, None, None) == 0
o2 = (i64 * 3)(); c2 = (i32 * 3)()
assert arr(None, o2, c2) == -2 and arr(h, None, c2) == -2 and arr(h, o2, None) == -2 and arr(h, o2, c2) == 0
assert list(o2) == [0, 2, 3] and list(c2) == [4, 9, 4]
mem = (i32 * 3)(0, 1, 1); first = (i32 * 3)(0, 1, 3); s = (C.c_float * 2)(7, 7); ag = (i32 * 2)(7, 7)
assert sc(None, mem, first, 2, s, ag) == -2 and sc(h, None, first, 2, s, ag) == -2 and sc(h, mem, None, 2, s, ag) == -2
assert sc(h, mem, first, -1, s, ag) == -2 and sc(h, mem, first, 2, None, ag) == -2
assert sc(h, (i32 * 3)(0, 1, 2), first, 2, s, ag) == -2 and b"arrangement 1 names member 2" in err()
assert sc(h, (i32 * 3)(-1, 1, 1), first, 2, s, ag) == -2 and b"arrangement 0" in err()
assert sc(h, mem, (i32 * 3)(0, 2, 1), 2, s, ag) == -2
assert list(s) == [7, 7] and list(ag) == [7, 7]                                                # nothing written by a refused call
assert sc(h, mem, first, 2, s, None) == 0 and sc(h, mem, first, 2, s, ag) == 0 and list(ag) == [2, 1] and list(s) == [0.4000000059604645, 0.20000000298023224]
assert sc(h, None, (i32 * 2)(0, 0), 1, s, ag) == 0 and ag[0] == 0 and s[0] == 0.0              # the empty arrangement needs no members
empty = mk(10, 5, (i64 * 1)(0), None, 0)
assert empty and info(empty, C.addressof(n), None, None, C.addressof(tot)) == 0 and (n.value, tot.value) == (0, 0)
lib.rs_hip_footprints_destroy(empty); lib.rs_hip_footprints_destroy(h); lib.rs_hip_footprints_destroy(None)
objs = (vp * 2)(1, 1); poses = (C.c_float * 32)(); st = (i32 * 2)(0, 1)
assert refused(fpc(None, objs, poses, st, 2), b"bad arguments") and refused(fpc(1, None, poses, st, 2), b"bad arguments")
assert refused(fpc(1, objs, None, st, 2), b"bad arguments") and refused(fpc(1, objs, poses, None, 2), b"bad arguments") and refused(fpc(1, objs, poses, st, -1), b"bad arguments")
assert refused(fpc(1, (vp * 2)(None, None), poses, st, 2), b"placement 0 has no object cloud")
lib.rs_hip_arrange_release.restype = C.c_int
assert lib.rs_hip_arrange_release() == 0
if no_gpu:
    assert fpc(1, (vp * 2)(1, None), poses, st, 2) is None and len(err()) > 0 and b"bad arguments" not in err()      # (a static placement needs no cloud)
print("ok")
"""
    import torch
    no_gpu = "0" if torch.cuda.is_available() else "1"
    out = subprocess.run([sys.executable, "-c", code, LIB, no_gpu], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


def test_python_layer_and_shim_check_their_arguments(capi):
    I = np.eye(4, dtype=F).ravel()
    cov = capi.Coverage.__new__(capi.Coverage)
    cov.handle = None
    with pytest.raises(ValueError):
        cov.footprints([(None, I, 0)])
    with pytest.raises(ValueError):
        cov.footprints([(None, I[:3], 1)])
    with pytest.raises(ValueError):
        capi.Footprints.from_arrays(10, 5, [0, 4], [1, 2])
    with pytest.raises(capi.RescanHipError):
        capi.Footprints.from_arrays(10, 5, [0, 2], [2, 1])
    fp = capi.Footprints.from_arrays(10, 5, [0, 2], [1, 2])
    with pytest.raises(capi.RescanHipError):
        fp.scores([[1]])
    with pytest.raises(IndexError):
        fp.cells(1)
    code = r"""
import ctypes as C, sys
lib = C.CDLL(sys.argv[1]); hip = C.CDLL(sys.argv[2]); no_gpu = sys.argv[3] == "1"
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
mk = hip.rs_hip_footprints_from_arrays; mk.restype = vp; mk.argtypes = [i64, i64, vp, vp, i32]
fpc = lib.rsd_coverage_footprints; fpc.restype = vp; fpc.argtypes = [vp, vp, vp, vp, vp, i32]
score = lib.rsd_footprints_score; score.restype = C.c_float; score.argtypes = [vp, vp, i32]
lib.rsd_footprints_destroy.argtypes = [vp]
pts = (C.c_float * 30)(); poses = (C.c_float * 32)(); ptrs = (vp * 2)(C.addressof(pts), C.addressof(pts)); ns = (i32 * 2)(10, 10); st = (i32 * 2)(0, 1)
assert fpc(None, ptrs, ns, poses, st, 2) is None and fpc(1, None, ns, poses, st, 2) is None and fpc(1, ptrs, ns, poses, st, -1) is None
assert fpc(1, (vp * 2)(None, None), ns, poses, st, 2) is None and fpc(1, ptrs, (i32 * 2)(-1, 0), poses, st, 2) is None
if no_gpu:
    assert fpc(1, ptrs, ns, poses, st, 2) is None
h = mk(10, 4, (i64 * 3)(0, 2, 3), (i32 * 3)(4, 9, 4), 2)
assert score(h, (i32 * 3)(0, 1, 1), 3) == 0.5 and score(h, None, 0) == 0.0 and score(h, (i32 * 1)(2), 1) < 0 and score(None, None, 0) < 0
lib.rsd_footprints_destroy(h)
print("ok")
"""
    import torch
    no_gpu = "0" if torch.cuda.is_available() else "1"
    out = subprocess.run([sys.executable, "-c", code, DROPIN, LIB, no_gpu], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
