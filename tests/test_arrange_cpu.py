"""CPU: the arrangement fixtures (tests/golden/arrange_*.npz, written by the reference's own rsao_compute_scene_saliency,
rsao_rasterize_scene_to_grid and rsao__compute_scene_coverage_score: tools/arrange_fixture) are reproduced IDENTICALLY by the NumPy
restatement of what include/rescan_hip.h documents (tests/ao_restate.py) — saliency grid, qualities, scene grids, counts, score
bits — and the reference's own numbers obey agree( base + k ) = agree( base ) + fresh[k]; the fixtures hold the cases they were
made for; the new entry points exist, check their arguments before they touch a device and fail loudly without one."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
import ao_restate as R

NAMES = ("room", "nowall")
LIB = os.path.join(ROOT, "rescan_amd", "librescan_hip.so")
DROPIN = os.path.join(ROOT, "rescan_amd", "librescan_dropin.so")
F = np.float32


def fixture(name):
    g = load_golden(f"arrange_{name}.npz")
    g["objects"] = [g[f"obj{i}_pos"] for i in range(int(g["n_obj"]))]
    return g


def trials(g):
    """(coverage set j, trial t, base [(obj, pose, static)], candidates [(obj, pose)]) of a fixture."""
    for j in range(3):
        for t in range(3):
            pre = f"cov{j}_t{t}_"
            base = [(int(o), p, int(s)) for o, p, s in zip(g[pre + "base_obj"], g[pre + "base_pose"], g[pre + "base_static"])]
            cand = [(int(o), p) for o, p in zip(g[pre + "cand_obj"], g[pre + "cand_pose"])]
            yield j, t, pre, base, cand


@pytest.fixture(scope="module")
def built():
    from rescan_amd import build
    build.build()


@pytest.mark.parametrize("name", NAMES)
def test_fixtures_hold_every_case(name):
    g = fixture(name)
    biggest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                  if f.endswith(".npz") and not f.startswith("arrange_"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"arrange_{name}.npz")) <= biggest
    sizes = [len(o) for o in g["objects"]]
    assert {1, 63, 64, 65}.issubset(sizes) and any(256 < s <= 400 for s in sizes) and 2000 <= len(g["pos0"]) <= 9000
    assert int(g["wall_idx"]) == (1 if name == "room" else -1) and int(g["floor_idx"]) == 2
    assert (name == "room") or (g["class0"] == -1).any()
    assert g["prop_static"].any() and not g["prop_static"].all()
    assert [float(g[f"sal{j}_voxel"]) for j in range(2)] == [float(F(0.15)), float(F(0.05))]
    bmin, bmax, objs = g["bbox_min"], g["bbox_max"], g["objects"]
    for j in range(2):
        voxel, grid = g[f"sal{j}_voxel"], g[f"sal{j}_grid"]
        origin, res = R.grid_shape(bmin, bmax, voxel)
        dyn, sta = np.zeros(len(grid), bool), np.zeros(len(grid), bool)
        neg, pos, on_face = np.zeros(3, int), np.zeros(3, int), 0
        for o, pose, s in zip(g["prop_obj"], g["prop_pose"], g["prop_static"]):
            q = R.xform(pose, objs[o])
            c = R.cells(origin, res, voxel, q)
            (sta if s else dyn)[c[c >= 0]] = True
            cc = R.cell_coords(origin, voxel, q)
            neg += (cc < 0).any(0); pos += (cc >= res[None, :]).any(0)
            t = (q - origin[None, :]) * (F(1.0) / F(voxel))
            on_face += int((t == np.floor(t)).sum())
        assert (dyn & sta).any() and (grid[dyn & sta] == 0).all()              # a static proposal clears what a dynamic one lit; shared cells
        assert (neg > 0).all() and (pos > 0).all() and on_face > 0             # outside on either side of each axis; points on voxel faces
        c0 = R.cells(origin, res, voxel, g["pos0"])
        shell = (g["class0"] == g["wall_idx"]) | (g["class0"] == g["floor_idx"])
        assert (shell & (c0 >= 0) & (grid[np.maximum(c0, 0)] == 1)).any()      # wall / floor points inside lit cells
        assert (c0 < 0).sum() >= 6
    assert int(g["cov2_valid"]) == 0 and int(g["cov0_valid"]) > 0 and int(g["cov1_valid"]) > 0      # a scene grid with no valid cell
    assert [float(g[f"cov{j}_voxel"]) for j in range(3)] == [float(F(0.05)), float(F(0.15)), float(F(0.05))]
    seen = dict(empty_base=0, static_base=0, no_cand=0, zero_fresh=0, several=0, straddle=0, slab=0, lds=0)
    for j, t, pre, base, cand in trials(g):
        seen["empty_base"] += not base
        seen["static_base"] += any(s for _, _, s in base)
        seen["no_cand"] += not cand
        if not int(g[f"cov{j}_valid"]):
            continue
        voxel, grid = g[f"cov{j}_voxel"], g[f"cov{j}_grid"]
        origin, res = R.grid_shape(bmin, bmax, voxel)
        for k, (o, p) in enumerate(cand):
            c = R.cells(origin, res, voxel, R.xform(p, objs[o])); c = c[c >= 0]; c = c[grid[c] > 0]
            seen["several"] += len(c) > len(np.unique(c))
            seen["straddle"] += len(np.unique(c >> 5)) > 1
            seen["zero_fresh"] += len(c) > 0 and g[pre + "agree"][k] == g[pre + "base_agree"]
            if j == 0 and t == 0:
                need = R.live_box_bytes(grid, bmin, bmax, voxel, objs, base, (o, p))
                seen["slab"] += need > int(g["low_lds_budget"])
                seen["lds"] += 0 < need <= int(g["low_lds_budget"])
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_saliency(name):
    g = fixture(name)
    for j in range(2):
        origin, res = R.grid_shape(g["bbox_min"], g["bbox_max"], g[f"sal{j}_voxel"])
        assert (origin.view(np.uint32) == g[f"sal{j}_origin"].view(np.uint32)).all() and (res == g[f"sal{j}_res"]).all()
        grid, quality = R.saliency(g["bbox_min"], g["bbox_max"], g[f"sal{j}_voxel"], g["objects"], g["prop_obj"], g["prop_pose"], g["prop_static"],
                                   g["pos0"], g["class0"], int(g["wall_idx"]), int(g["floor_idx"]))
        assert grid.tobytes() == g[f"sal{j}_grid"].tobytes()
        assert quality.tobytes() == g[f"sal{j}_quality"].tobytes()
        assert set(np.unique(quality)) == {F(0.0), F(1.0)}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_every_count_and_score_bit(name):
    g = fixture(name)
    pos2, q2 = g["pos0"][g["sub"]], g["sal0_quality"][g["sub"]]
    n_cand = 0
    for j, t, pre, base, cand in trials(g):
        voxel = g[f"cov{j}_voxel"]
        grid = R.scene_grid(g["bbox_min"], g["bbox_max"], voxel, pos2, q2, g[f"cov{j}_threshold"])
        assert grid.tobytes() == g[f"cov{j}_grid"].tobytes() and int((grid > 0).sum()) == int(g[f"cov{j}_valid"])
        agree, valid, score = R.coverage(grid, g["bbox_min"], g["bbox_max"], voxel, g["objects"], base)
        assert agree == int(g[pre + "base_agree"]) and F(score).view(np.uint32) == g[pre + "base_score"].view(np.uint32)
        # the whole arrangement base + candidate k, as the reference scored it ...
        for k, (o, p) in enumerate(cand):
            a, _, s = R.coverage(grid, g["bbox_min"], g["bbox_max"], voxel, g["objects"], base + [(o, p, 0)])
            assert a == int(g[pre + "agree"][k]) and F(s).view(np.uint32) == g[pre + "score"][k].view(np.uint32), (j, t, k)
        # ... and the incremental form: agree( base + k ) = agree( base ) + fresh[k], on the reference's numbers
        base_agree, fresh, agree_k, scores = R.extensions(grid, g["bbox_min"], g["bbox_max"], voxel, g["objects"], base, cand)
        assert base_agree == int(g[pre + "base_agree"])
        assert (int(g[pre + "base_agree"]) + fresh == g[pre + "agree"]).all() and (fresh >= 0).all()
        assert (agree_k == g[pre + "agree"]).all() and scores.tobytes() == g[pre + "score"].astype(F).tobytes()
        n_cand += len(cand)
    assert n_cand > 150


def hard_fixture():
    return load_golden("arrange_hard.npz")


def test_hard_fixture_is_small_and_holds_every_case():
    """tests/golden/arrange_hard.npz (tools/arrange_fixture/gen.py --hard): EVERY hostile case of tests/hard_shapes.py went through
    the reference unchanged, each cloud as an object's level 2 or as the scene — the candidate of no points and the clouds with NaN
    and infinite coordinates included — so none is pinned by the restatement alone.  Only the predicted ROUTE of a candidate (its
    live sub-box's bytes) has no counterpart in the reference.  The file holds lengths and CRCs instead of clouds."""
    import hard_shapes as H
    g = hard_fixture()
    biggest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                  if f.endswith(".npz") and not f.startswith("arrange_"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "arrange_hard.npz")) <= biggest
    for voxel, cell0 in H.ARR_CASES:
        a, s = H.arrangement(voxel, cell0), H.saliency_case(voxel, cell0)
        pre = H.arr_key("cov", voxel, cell0)
        assert (g[pre + "crc"] == H.cloud_crcs(a["scene"], a["objects"])).all()          # the regenerated clouds are the ones the reference saw
        assert [n.decode() for n in g[pre + "names"]] == a["names"] and len(g[pre + "agree"]) == len(a["cands"]) == len(g[pre + "score"])
        assert (g[H.arr_key("sal", voxel, cell0) + "crc"] == H.cloud_crcs(s["scene"], s["objects"])).all()


@pytest.mark.parametrize("voxel,cell0", [(0.05, True), (0.05, False), (0.15, True), (0.15, False)])
def test_restatement_reproduces_the_hard_fixture(voxel, cell0):
    """The reference's own scene grid, counts, score bits, saliency grid and qualities of the hostile cases, IDENTICALLY — among them
    what the reference makes of a NaN or infinite coordinate: outside the grid, so cell 0 is active / lit only where a finite point is."""
    import hard_shapes as H
    g = hard_fixture()
    a, grid, base_agree, fresh, agree, scores, _ = H.arrangement_expectations(voxel, cell0)
    pre = H.arr_key("cov", voxel, cell0)
    want = np.unpackbits(g[pre + "grid"])[:len(grid)]
    assert (g[pre + "res"] == a["res"]).all() and want[0] == int(cell0) and int(want.sum()) == int(g[pre + "valid"])
    assert grid.tobytes() == want.tobytes()
    assert base_agree == int(g[pre + "base_agree"]) and (agree == g[pre + "agree"]).all() and scores.tobytes() == g[pre + "score"].tobytes()
    assert R.coverage(grid, H.ARR_BMIN, H.ARR_BMAX, voxel, a["objects"], a["base"])[2].view(np.uint32) == g[pre + "base_score"].view(np.uint32)
    s = H.saliency_case(voxel, cell0)
    sal, quality = R.saliency(H.ARR_BMIN, H.ARR_BMAX, voxel, s["objects"], s["prop_obj"], s["prop_pose"], s["prop_static"], s["scene"], s["cls"], -1, 2)
    pre = H.arr_key("sal", voxel, cell0)
    want = np.unpackbits(g[pre + "grid"])[:len(sal)]
    assert want[0] == int(cell0) and sal.tobytes() == want.tobytes() and quality.tobytes() == g[pre + "quality"].tobytes()


@pytest.mark.parametrize("voxel,cell0", [(0.05, True), (0.05, False), (0.15, True), (0.15, False)])
def test_hard_candidates_hold_every_case(voxel, cell0):
    import hard_shapes as H
    a, grid, base_agree, fresh, agree, scores, need = H.arrangement_expectations(voxel, cell0)
    origin, res = R.grid_shape(H.ARR_BMIN, H.ARR_BMAX, voxel)
    assert (res == a["res"]).all() and base_agree > 0
    # the scene holds NaN and infinite points; cell 0 is active only by the finite point of the cell0 run.  Per the restatement a
    # non-finite scene point is outside: one taken for cell 0 would light it in the run without that point
    assert not np.isfinite(a["scene"]).all() and np.isnan(a["scene"]).all(1).any() and grid[0] == int(cell0)
    assert int(grid.sum()) == int(H.arrangement_expectations(voxel, True)[1].sum()) - int(not cell0)
    f = dict(zip(a["names"], fresh))
    b = dict(zip(a["names"], need))
    n_pts = {name: len(a["objects"][o]) for name, (o, _) in zip(a["names"], a["cands"])}
    for k in (1, 255, 256, 257, 5000):
        assert n_pts[f"three_cells_{k}"] == k and f[f"three_cells_{k}"] == min(k, 3) and f[f"spread_cells_{k}"] == min(k, 3)      # cells, not points
        assert b[f"three_cells_{k}"] == 4 and (k < 3 or b[f"spread_cells_{k}"] > 64 * 4)                  # ... in one word, and over several waves' words
    assert f["off_grid"] == f["inside_base"] == f["scene_inactive"] == f["empty"] == f["non_finite"] == 0
    assert b["off_grid"] == b["inside_base"] == b["scene_inactive"] == b["empty"] == b["non_finite"] == 0        # no sub-box is made
    assert n_pts["inside_base"] > 0 and n_pts["scene_inactive"] > 0 and n_pts["empty"] == 0
    rod = a["objects"][a["cands"][a["names"].index("rod")][0]]
    cc = R.cell_coords(origin, voxel, rod)
    ext = cc.max(0) - cc.min(0) + 1
    assert f["rod"] == len(rod) and (ext == len(rod)).all() and len(rod) >= 10 and b["rod"] == (len(rod) ** 3 + 31) // 32 * 4 and b["rod"] <= 16384
    assert len({int(v) >> 5 for v in (cc - cc.min(0)) @ np.array([1, len(rod) ** 2, len(rod)])}) >= 10       # the bit index crosses many words
    assert f["plate_yz"] == n_pts["plate_yz"] == 5 * (int(res[2]) - 6) and int(res[2]) - 6 > 5         # 5 cells along y, more along z
    for axis, name in enumerate(("faces_x", "faces_y", "faces_z")):
        pts = a["objects"][a["cands"][a["names"].index(name)][0]]
        c = R.cell_coords(origin, voxel, pts)[:, axis]
        t = (pts[:, axis] - origin[axis]) * (F(1.0) / F(voxel))
        assert (c == -1).any() and (c == 0).any() and (c == res[axis] - 1).any() and (c == res[axis]).any()      # one step outside on either side
        assert (t == 0).any() and (t == F(res[axis])).any() and (t == np.floor(t)).sum() >= 3 and f[name] > 0    # floorf of exactly 0 and of exactly res


@pytest.mark.parametrize("voxel", (0.05, 0.15))
def test_hard_saliency_holds_every_case(voxel):
    import hard_shapes as H
    for cell0 in (False, True):
        s = H.saliency_case(voxel, cell0)
        grid, quality = R.saliency(H.ARR_BMIN, H.ARR_BMAX, voxel, s["objects"], s["prop_obj"], s["prop_pose"], s["prop_static"], s["scene"], s["cls"], -1, 2)
        origin, res = R.grid_shape(H.ARR_BMIN, H.ARR_BMAX, voxel)
        dyn = R.cells(origin, res, voxel, s["objects"][0]); sta = R.cells(origin, res, voxel, s["objects"][1])
        assert s["prop_static"][0] == 1 and s["prop_static"][1] == 0                   # the static proposal is listed first ...
        both = np.intersect1d(dyn, sta)
        assert len(both) > 0 and (grid[both] == 0).all() and grid[np.setdiff1d(dyn, sta)].all()       # ... and still clears what the dynamic one lit
        c0 = R.cells(origin, res, voxel, s["scene"])
        lit = (c0 >= 0) & (grid[np.maximum(c0, 0)] == 1)
        assert (lit & (s["cls"] == 2)).any() and (quality[lit & (s["cls"] == 2)] == 0).all()      # floor points in lit cells
        assert (lit & (s["cls"] == -1)).any() and (quality[lit & (s["cls"] == -1)] == 0).all()    # class -1 with wall_idx -1: "wall", quality 0
        assert (quality[lit & (s["cls"] == 1)] == 1).all() and (lit & (s["cls"] == 1)).any()
        # non-finite coordinates light and read nothing: cell 0 is lit only by the finite point of the second run
        wild = R.cells(origin, res, voxel, s["objects"][2])
        assert (wild[:6] == -1).all() and grid[0] == int(cell0) and (wild == 0).sum() == int(cell0)
        assert (c0[-4:-1] == -1).all() and (quality[-4:-1] == 0).all() and c0[-1] == 0 and quality[-1] == F(cell0)


def test_new_symbols_exist(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    for s in ("rs_hip_scene_saliency", "rs_hip_coverage_extensions", "rs_hip_coverage_lds_budget", "rs_hip_coverage_extension_routes", "rs_hip_voxel_grid_shape",
              "rs_hip_arrange_release"):
        assert re.search(r" T %s\b" % s, out), s
    out = subprocess.check_output(["nm", "-D", "--defined-only", DROPIN], text=True)
    for s in ("rsd_scene_saliency", "rsd_coverage_extensions"):
        assert re.search(r" T %s\b" % s, out), s
    from rescan_amd import capi
    assert callable(capi.scene_saliency) and callable(capi.Coverage.extensions) and callable(capi.coverage_lds_budget)
    for s in ("rs_hip_scene_saliency", "rs_hip_coverage_extensions"):
        assert s in capi.SIGNATURES


def test_grid_shape_is_the_references(built):
    """rs_hip_voxel_grid_shape runs on the host: the fixtures' grids, without a device."""
    from rescan_amd import capi
    for name in NAMES:
        g = fixture(name)
        for key in ("sal0", "sal1", "cov0", "cov1"):
            res, org, n = capi.voxel_grid_shape(g["bbox_min"], g["bbox_max"], g[key + "_voxel"])
            assert (res == g[key + "_res"]).all() and n == len(g[key + "_grid"])
            if key.startswith("sal"):
                assert org.tobytes() == g[key + "_origin"].tobytes()


def test_arguments_are_checked_before_a_device_is_touched(built):
    """In a child process (a regression would read through a null pointer): RS_HIP_E_ARG (-2) for NULL arrays, negative counts, an
    object index out of range, voxel <= 0 — with or without a device; with valid arguments and no device RS_HIP_E_NODEVICE (-1)."""
    code = r"""
import ctypes as C, sys
lib = C.CDLL(sys.argv[1]); no_gpu = sys.argv[2] == "1"
vp, i32, i64, f = C.c_void_p, C.c_int32, C.c_int64, C.c_float
lib.rs_hip_last_error.restype = C.c_char_p
sal = lib.rs_hip_scene_saliency; sal.restype = C.c_int
sal.argtypes = [vp, vp, f, vp, i32, vp, vp, vp, i32, vp, vp, i64, i32, i32, vp, vp, i64]
bmin = (C.c_float * 3)(0, 0, 0); bmax = (C.c_float * 3)(1, 1, 1)
objs = (vp * 2)(1, 1)                                  # never dereferenced by the checks
po = (i32 * 3)(0, 1, 0); pp = (C.c_float * 48)(); ps = (i32 * 3)(0, 0, 1)
pos = (C.c_float * 12)(); cls = (i32 * 4)(); q = (C.c_float * 4)(7, 7, 7, 7); grid = (C.c_uint8 * 8)()
ok = lambda *a: sal(*a)
A = lambda **kw: [kw.get("bmin", bmin), kw.get("bmax", bmax), kw.get("voxel", 0.15), kw.get("objs", objs), kw.get("n_obj", 2), kw.get("po", po), kw.get("pp", pp),
                  kw.get("ps", ps), kw.get("n_props", 3), kw.get("pos", pos), kw.get("cls", cls), kw.get("n", 4), 1, 2, kw.get("q", q), kw.get("grid", None), kw.get("cap", 0)]
for bad in (dict(bmin=None), dict(bmax=None), dict(voxel=0.0), dict(voxel=-0.15), dict(voxel=float("nan")), dict(objs=None), dict(n_obj=-1), dict(po=None), dict(pp=None),
            dict(ps=None), dict(n_props=-1), dict(pos=None), dict(cls=None), dict(n=-1), dict(q=None)):
    assert sal(*A(**bad)) == -2, bad
assert sal(*A(po=(i32 * 3)(0, 2, 0))) == -2 and b"proposal 1" in lib.rs_hip_last_error()
assert sal(*A(po=(i32 * 3)(0, 1, -1))) == -2 and b"proposal 2" in lib.rs_hip_last_error()
assert sal(*A(objs=(vp * 2)(1, None))) == -2
assert sal(*A(grid=grid, cap=8)) == -4                # RS_HIP_E_CAPACITY: the grid array is smaller than the grid
assert sal(*A(bmax=(C.c_float * 3)(1e6, 1e6, 1e6), voxel=0.01)) == -4
ext = lib.rs_hip_coverage_extensions; ext.restype = C.c_int
ext.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp]
bs = (i32 * 2)(0, 1); sc = (C.c_float * 2)(7, 7); ag = (i32 * 2)(7, 7); ba = i32(-5)
assert ext(None, objs, pp, bs, 2, objs, pp, 2, sc, ag, C.addressof(ba)) == -2
assert ext(1, None, pp, bs, 2, objs, pp, 2, sc, ag, C.addressof(ba)) == -2
assert ext(1, objs, None, bs, 2, objs, pp, 2, sc, ag, C.addressof(ba)) == -2
assert ext(1, objs, pp, None, 2, objs, pp, 2, sc, ag, C.addressof(ba)) == -2
assert ext(1, objs, pp, bs, -1, objs, pp, 2, sc, ag, C.addressof(ba)) == -2
assert ext(1, objs, pp, bs, 2, None, pp, 2, sc, ag, C.addressof(ba)) == -2
assert ext(1, objs, pp, bs, 2, objs, None, 2, sc, ag, C.addressof(ba)) == -2
assert ext(1, objs, pp, bs, 2, objs, pp, -2, sc, ag, C.addressof(ba)) == -2
assert ext(1, objs, pp, bs, 2, objs, pp, 2, None, ag, C.addressof(ba)) == -2
assert ext(1, (vp * 2)(None, None), pp, bs, 2, objs, pp, 2, sc, ag, C.addressof(ba)) == -2 and b"base placement 0" in lib.rs_hip_last_error()
assert ext(1, objs, pp, bs, 2, (vp * 2)(1, None), pp, 2, sc, ag, C.addressof(ba)) == -2 and b"candidate 1" in lib.rs_hip_last_error()
shape = lib.rs_hip_voxel_grid_shape; shape.restype = C.c_int; shape.argtypes = [vp, vp, f, vp, vp, vp]
assert shape(None, bmax, 0.1, None, None, None) == -2 and shape(bmin, bmax, 0.0, None, None, None) == -2
assert list(q) == [7, 7, 7, 7] and list(sc) == [7, 7] and list(ag) == [7, 7] and ba.value == -5
lib.rs_hip_arrange_release.restype = C.c_int
assert lib.rs_hip_arrange_release() == 0              # nothing held by this thread: nothing to free, no device needed
if no_gpu:
    assert sal(*A()) == -1
    assert ext(1, (vp * 2)(1, None), pp, bs, 2, objs, pp, 2, sc, ag, C.addressof(ba)) == -1      # (a static placement needs no cloud)
    assert list(q) == [7, 7, 7, 7] and list(sc) == [7, 7] and ba.value == -5
print("ok")
"""
    import torch
    no_gpu = "0" if torch.cuda.is_available() else "1"
    out = subprocess.run([sys.executable, "-c", code, LIB, no_gpu], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


def test_python_layer_checks_before_the_library(built):
    from rescan_amd import capi
    I = np.eye(4, dtype=F).ravel()
    with pytest.raises(ValueError):
        capi.scene_saliency([0, 0, 0], [1, 1, 1], [None], [0], [I], [0], np.zeros((2, 3), F), [0, 0], 1, 2)
    with pytest.raises(ValueError):
        capi.scene_saliency([0, 0, 0], [1, 1, 1], [], [0], [I], [0], np.zeros((2, 3), F), [0, 0], 1, 2)
    with pytest.raises(ValueError):
        capi.scene_saliency([0, 0, 0], [1, 1, 1], [], [], np.zeros((0, 16), F), [], np.zeros((2, 3), F), [0], 1, 2)
    with pytest.raises(ValueError):
        capi.scene_saliency([0, 0, 0], [1, 1, 1], [], [], np.zeros((0, 16), F), [], np.zeros((2, 3), F), [0, 0], 1, 2, voxel_size=0.0)
    cov = capi.Coverage.__new__(capi.Coverage)
    cov.handle = None
    with pytest.raises(ValueError):
        cov.extensions([(None, I, 0)], [])
    with pytest.raises(ValueError):
        cov.extensions([], [(None, I)])


def test_shim_fails_loudly_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    code = r"""
import ctypes as C, sys
lib = C.CDLL(sys.argv[1])
vp, i32, f = C.c_void_p, C.c_int32, C.c_float
pts = (C.c_float * 30)(); poses = (C.c_float * 32)(); bmin = (C.c_float * 3)(0, 0, 0); bmax = (C.c_float * 3)(1, 1, 1)
ptrs = (vp * 2)(C.addressof(pts), C.addressof(pts)); ns = (i32 * 2)(10, 10); po = (i32 * 2)(0, 1); ps = (i32 * 2)(0, 1)
cls = (i32 * 10)(); q = (C.c_float * 10)(*([7.0] * 10))
sal = lib.rsd_scene_saliency; sal.restype = C.c_int
sal.argtypes = [vp, vp, f, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, i32, vp]
assert sal(bmin, bmax, 0.15, ptrs, ns, 2, po, poses, ps, 2, pts, cls, 10, 1, 2, q) < 0 and list(q) == [7.0] * 10
assert sal(bmin, bmax, 0.15, ptrs, ns, 2, (i32 * 2)(0, 5), poses, ps, 2, pts, cls, 10, 1, 2, q) == -2
ext = lib.rsd_coverage_extensions; ext.restype = C.c_int
ext.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp]
sc = (C.c_float * 2)(7.0, 7.0)
assert ext(None, ptrs, ns, poses, ps, 2, ptrs, ns, poses, 2, sc) == -2
assert ext(1, ptrs, ns, poses, ps, 2, ptrs, ns, poses, 2, sc) < 0 and list(sc) == [7.0, 7.0]
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code, DROPIN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
