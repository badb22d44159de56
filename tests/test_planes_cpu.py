"""CPU: the plane fixtures (tests/golden/planes_*.npz, written by the reference's own rspf__detect_floor, rspf__detect_walls,
evaluate_plane_model, remove_inliers, rspf__gather_model_inliers and rspf_relabel_walls_and_floors: tools/plane_fixture) are
reproduced bit for bit by the NumPy restatement (tests/planes_restate.py); the host planner behind rs_hip_plane_hypotheses gives the
reference's triples, centres and normals without a device; every refusal that needs no device is decided without one; the new entry
points exist; the resampler's alias table is what it was before the table builder was shared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
import planes_restate as R
import resample_restate as RR

LIB = os.path.join(ROOT, "rescan_amd", "librescan_hip.so")
DROPIN = os.path.join(ROOT, "rescan_amd", "librescan_dropin.so")
E_ARG, E_CAPACITY = -2, -4
F = np.float32
SYMBOLS = ("rs_hip_plane_hypotheses", "rs_hip_plane_votes", "rs_hip_detect_planes", "rs_hip_gather_plane_inliers",
           "rs_hip_relabel_walls_and_floors", "rs_hip_plane_votes_form")
SHIM_SYMBOLS = ("rsd_detect_floor_and_walls", "rsd_gather_model_inliers", "rsd_relabel_walls_and_floors")
CASES = (("planes_room.npz", ""), ("planes_quirks.npz", "a_"), ("planes_quirks.npz", "c_"), ("planes_quirks.npz", "d_"), ("planes_quirks.npz", "e_"))


@pytest.fixture(scope="module")
def lib():
    from rescan_amd import build
    build.build()
    lib = C.CDLL(LIB)
    lib.rs_hip_plane_hypotheses.restype = C.c_int
    lib.rs_hip_plane_hypotheses.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rs_hip_plane_votes.restype = C.c_int
    lib.rs_hip_plane_votes.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p]
    lib.rs_hip_last_error.restype = C.c_char_p
    return lib


def planner(lib, pos, active, n_iter, distinct, seed=12346):
    idx = np.full((n_iter, 3), -7, np.int32); c = np.zeros((n_iter, 3), F); nn = np.zeros((n_iter, 3), F)
    active = np.ascontiguousarray(active, np.uint8)
    rc = lib.rs_hip_plane_hypotheses(pos.ctypes.data, len(pos), active.ctypes.data, n_iter, distinct, seed, idx.ctypes.data, c.ctypes.data, nn.ctypes.data)
    return rc, idx, c, nn


def rounds_of(g, prefix):
    return [{k: g[f"{prefix}r{r}_{k}"] for k in ("idx", "normal", "valid", "counts", "best", "mask_before", "mask_after") if f"{prefix}r{r}_{k}" in g}
            for r in range(int(g[prefix + "n_rounds"]))]


def test_fixtures_are_small_and_hold_the_cases():
    for name in ("room", "quirks", "gather", "hostile"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"planes_{name}.npz")) < 757075
    g = load_golden("planes_room.npz")
    assert 8000 <= len(g["pos"]) <= 20000 and int(g["n_rounds"]) - 1 >= 3 and int(g["n_floors"]) == 1
    q = load_golden("planes_quirks.npz")
    assert len(g["tied_rounds"]) or len(q["c_tied_rounds"])
    assert int(q["a_r1_best"]) == -1 and len(q["a_centers"]) == 0 and int(q["a_n_floors"]) == 1 and int(q["a_n_walls"]) == 0
    assert int(q["d_n_floors"]) == 0 and int(q["d_floor_mask"].sum()) == 1 and np.isnan(q["d_r0_normal"]).all()
    assert int(q["e_n_rounds"]) == 2 and int(q["e_n_walls"]) == 0 and len(q["e_centers"]) == 1
    t = load_golden("planes_gather.npz")
    o = t["checked_offsets"]
    assert o[2] == o[3] and t["model_valid"].tolist() == [1, 1, 0, 1]
    assert (t["instance_before"] >= 1024).any() and (t["class_before"] != 0).any() and ((t["class_before"] != t["class_after"]) | (t["instance_before"] != t["instance_after"])).any()
    h = load_golden("planes_hostile.npz")                # tests/test_hard_planes_cpu.py compares every array of it
    assert len(h["vote_cases"]) == 8 and all(h[f"votes_{k}_counts_all"].shape == (64,) and h[f"votes_{k}_removed"].shape[0] == 8 for k in h["vote_cases"])
    assert not np.isfinite(h["votes_special_pos"]).all() and not np.isfinite(h["room_nor"]).all() and int(h["room_n_rounds"]) >= 3 and int(h["tie_n_rounds"]) >= 3
    assert all(f"gather_{k}_{a}" in h for k in ("dot_band", "quad_edges", "labels") for a in ("plain_index", "checked_index", "class_after", "instance_after"))


@pytest.mark.parametrize("name,prefix", CASES)
def test_restatement_reproduces_the_detection(name, prefix):
    g = load_golden(name)
    fm, wm = R.candidate_masks(g[prefix + "nor"], g[prefix + "dot_threshold"])
    assert (fm == g[prefix + "floor_mask"]).all() and (wm == g[prefix + "wall_mask"]).all()
    got = R.detect(g[prefix + "pos"], g[prefix + "nor"], g[prefix + "dot_threshold"], g[prefix + "dist_threshold"], int(g[prefix + "count_threshold"]))
    want = rounds_of(g, prefix)
    assert len(got["rounds"]) == len(want)
    for k, (a, b) in enumerate(zip(got["rounds"], want)):
        assert (a["idx"] == b["idx"]).all() and (a["valid"] == b["valid"]).all() and a["best"] == int(b["best"]), (prefix, k)
        assert (a["counts"] == np.where(b["valid"] != 0, b["counts"], 0)).all(), (prefix, k)
        assert (a["mask_before"] == b["mask_before"]).all() and (a["mask_after"] == b["mask_after"]).all(), (prefix, k)
        if "normal" in b:
            assert R.same_bits(a["normal"], b["normal"]), (prefix, k)
            # evaluate_plane_model's count of a hypothesis that failed the up test, too
            assert (R.votes(g[prefix + "pos"], b["mask_before"], a["center"], a["normal"], g[prefix + "dist_threshold"]) == b["counts"]).all(), (prefix, k)
    assert R.same_bits(got["centers"], g[prefix + "centers"]) and R.same_bits(got["normals"], g[prefix + "normals"])
    assert (got["n_inliers"] == g[prefix + "n_inliers"]).all() and got["n_floors"] == int(g[prefix + "n_floors"]) and got["n_walls"] == int(g[prefix + "n_walls"])


def test_restatement_refuses_the_empty_pop():
    g = load_golden("planes_quirks.npz")
    with pytest.raises(R.Refused) as e:
        R.detect(g["b_pos"], g["b_nor"], g["b_dot_threshold"], g["b_dist_threshold"], int(g["b_count_threshold"]))
    assert e.value.code == E_ARG


def test_restatement_reproduces_gather_and_relabel():
    g = load_golden("planes_gather.npz")
    M = {k: g["model_" + k] for k in ("center", "normal", "axes", "extends", "valid", "up_dot")}
    for name, cl, cv, ce in (("plain", "l0", False, False), ("checked", "l1", True, True)):
        got = R.gather(g[cl + "_pos"], g[cl + "_nor"], M["center"], M["normal"], M["axes"], M["extends"], M["valid"], g[name + "_dot_threshold"],
                       g[name + "_dist_threshold"], cv, ce)
        o = g[name + "_offsets"]
        for m in range(4):
            assert (got[m] == g[name + "_index"][o[m]:o[m + 1]]).all(), (name, m)
    assert float(g["checked_dot_threshold"]) == 0.0
    cls, inst = R.relabel(g["l1_pos"], g["l1_nor"], M["center"], M["normal"], M["axes"], M["extends"], M["valid"], M["up_dot"], int(g["floor_idx"]),
                          int(g["wall_idx"]), int(g["unlabelled_idx"]), g["class_before"], g["instance_before"])
    assert (cls == g["class_after"]).all() and (inst == g["instance_after"]).all()


@pytest.mark.parametrize("name,prefix", CASES)
def test_host_planner_reproduces_the_recorded_rounds(lib, name, prefix):
    g = load_golden(name)
    pos = g[prefix + "pos"]
    for k, b in enumerate(rounds_of(g, prefix)):
        n_iter = len(b["idx"])
        rc, idx, c, nn = planner(lib, pos, b["mask_before"], n_iter, 0 if k == 0 else 1)
        assert rc == 0, lib.rs_hip_last_error()
        assert (idx == b["idx"]).all(), (prefix, k)
        assert c.view(np.uint32).tobytes() == pos[b["idx"][:, 0]].view(np.uint32).tobytes(), (prefix, k)
        want = b["normal"] if "normal" in b else R.hypotheses(pos, b["idx"])[1]
        assert R.same_bits(nn, want) and (np.isnan(nn) == np.isnan(want)).all(), (prefix, k)


def test_host_planner_equals_the_restatement_on_other_seeds_and_masks(lib):
    rng = np.random.default_rng(5)
    pos = rng.uniform(-1, 1, (777, 3)).astype(F)
    for seed, mask in ((1, np.ones(777, np.uint8)), (64321, (np.arange(777) % 3 == 0).astype(np.uint8)), (0xFFFFFFFF, (np.arange(777) >= 775).astype(np.uint8))):
        for distinct in (0, 1):
            rc, idx, c, nn = planner(lib, pos, mask, 300, distinct, seed)
            assert rc == 0 and (idx == R.triples(mask, 300, distinct, seed)).all(), (seed, distinct)
            assert mask[idx].all()
            if distinct:
                assert (idx[:, 0] != idx[:, 1]).all() and (idx[:, 1] != idx[:, 2]).all()
            assert R.same_bits(nn, R.hypotheses(pos, idx)[1])


def test_refusals_need_no_device(lib):
    pos = np.zeros((4, 3), F); idx = np.zeros((8, 3), np.int32)
    def call(pos_p, n, act, n_iter, distinct):
        return lib.rs_hip_plane_hypotheses(pos_p, n, None if act is None else act.ctypes.data, n_iter, distinct, 12346, idx.ctypes.data, None, None)
    none, one, two = np.zeros(4, np.uint8), np.array([0, 1, 0, 0], np.uint8), np.array([0, 1, 0, 1], np.uint8)
    assert call(None, 4, two, 8, 0) == E_ARG and call(pos.ctypes.data, 4, None, 8, 0) == E_ARG and call(pos.ctypes.data, -1, two, 8, 0) == E_ARG
    assert call(pos.ctypes.data, 4, two, -1, 0) == E_ARG
    assert call(pos.ctypes.data, 4, none, 8, 0) == E_ARG and b"uninitialised" in lib.rs_hip_last_error()
    assert call(pos.ctypes.data, 4, one, 8, 1) == E_ARG and b"never end" in lib.rs_hip_last_error()
    assert call(pos.ctypes.data, 4, one, 8, 0) == 0 and (idx[:8] == 1).all()          # the floor has no distinctness test
    assert call(pos.ctypes.data, 4, two, 8, 1) == 0
    big = np.zeros(1, np.uint8)
    assert call(pos.ctypes.data, (1 << 24) + 1, big, 8, 0) == E_CAPACITY and b"2^24" in lib.rs_hip_last_error()
    counts = np.zeros(8, np.int32)
    assert lib.rs_hip_plane_votes(None, 4, two.ctypes.data, pos.ctypes.data, pos.ctypes.data, None, 1, 0.033, counts.ctypes.data) == E_ARG
    assert lib.rs_hip_plane_votes(pos.ctypes.data, -1, two.ctypes.data, pos.ctypes.data, pos.ctypes.data, None, 1, 0.033, counts.ctypes.data) == E_ARG
    assert lib.rs_hip_plane_votes(pos.ctypes.data, (1 << 24) + 1, two.ctypes.data, pos.ctypes.data, pos.ctypes.data, None, 1, 0.033, counts.ctypes.data) == E_CAPACITY


def test_new_symbols_exist_in_both_libraries(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert f" T {s}\n" in out, s
    out = subprocess.run(["nm", "-D", "--defined-only", DROPIN], capture_output=True, text=True, check=True).stdout
    for s in SHIM_SYMBOLS:
        assert f" T {s}\n" in out, s


def test_resampler_alias_table_is_unchanged():
    """The table builder is now shared with the plane sampler: rs_hip_resample_plan still gives the restatement's table, bit for bit,
    on a skewed mesh (tests/test_resample_cpu.py holds it against the reference's recordings)."""
    from rescan_amd import capi
    rng = np.random.default_rng(9)
    pos = rng.uniform(-1, 1, (400, 3)).astype(F); pos[:40] *= F(30.0)
    faces = rng.integers(0, 400, (1500, 3)).astype(np.int32)
    g_n, g_total, g_prob, g_alias = capi.resample_plan(pos, faces)
    n_samples, total, prob, alias = RR.plan(pos, faces)
    assert g_n == n_samples and g_total == total
    assert g_prob.tobytes() == prob.tobytes() and (g_alias == alias).all()
