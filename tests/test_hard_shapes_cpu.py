"""CPU: the hostile shapes of tests/hard_shapes.py.  tests/golden/isect_hard.npz holds what the reference's own
isect_get_overlap_factor and mgs_non_maxima_suppresion made of them (tools/nms_fixture/gen.py --hard; the clouds are regenerated
here and checked against their stored CRCs); tests/isect_restate.py reproduces every row IDENTICALLY, which anchors it at the edges
before tests/test_gpu_hard_shapes.py trusts it for the "random" family.  A census computed from the restatement's boundary grids
states what the fixture contains: conditions, not measurements — if a generator is edited and loses a case, the census fails.
Pinned by the restatement alone (the reference cannot run them): the two 4097-cell cases, whose lines overrun its scanline arrays,
and the NaN case.  The empty-boundary case IS in the fixture: the reference runs it, printing its empty-grid warning."""
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden
import hard_shapes as H
import isect_restate as R

F = np.float32
LDS_BUDGET = 61440          # ISECT_LDS_BYTES of rescan_amd/csrc/rs_isect.hip


@pytest.fixture(scope="module")
def fx():
    g = load_golden("isect_hard.npz")
    cases = H.fixture_cases()
    assert [c.name for c in cases] == [n.decode() for n in g["case_name"]]
    for j, c in enumerate(cases):                      # the regenerated clouds are the ones the reference saw
        assert (c.crcs() == g["shape_crc"][g["shape_first"][j]:g["shape_first"][j + 1]]).all(), c.name
        rows = slice(g["case_first"][j], g["case_first"][j + 1])
        assert (c.ia == g["shape_a"][rows]).all() and (c.ib == g["shape_b"][rows]).all()
        assert c.pose_a.tobytes() == g["pose_a"][rows].tobytes() and c.pose_b.tobytes() == g["pose_b"][rows].tobytes(), c.name
        assert (c.voxel, c.inside, c.by_smaller, c.expect, int(c.reference)) == \
            (g["case_voxel"][j], g["case_inside"][j], g["case_by_smaller"][j], g["case_expect"][j].decode(), g["case_reference"][j])
    return g, cases


@pytest.fixture(scope="module")
def census(fx):
    """One pass over every fixture row: the restatement's answer next to the reference's, and what the boundary grids contain."""
    g, cases = fx
    seen = dict(x_res={}, z_res={}, fwd_seam=0, bwd_seam=0, both_seam=0, odd_word1=0, odd_word2=0, x0=0, x_last=0, z0=0, z_last=0, y0=0, y_last=0,
                disagree_x=0, disagree_z=0, no_grid=0, lds=0, glob=0, z_fwd_seam=0, z_bwd_seam=0)
    bad = []
    for j, c in enumerate(cases):
        for k in range(len(c)):
            row = int(g["case_first"][j]) + k
            sa, sb = c.shapes[c.ia[k]], c.shapes[c.ib[k]]
            if not c.reference:
                with pytest.raises(R.LineTooLong if c.expect == "capacity" else R.OutsideGrid):
                    R.overlap(sa, c.pose_a[k], sb, c.pose_b[k], c.voxel, c.inside, c.by_smaller)
                continue
            ov, cnt = R.overlap(sa, c.pose_a[k], sb, c.pose_b[k], c.voxel, c.inside, c.by_smaller)
            if tuple(cnt) != tuple(int(v) for v in g["counts"][row]) or F(ov).view(np.uint32) != g["overlap"][row].view(np.uint32):
                bad.append((c.name, k, cnt, g["counts"][row], ov, g["overlap"][row]))
            ba, bb = R.box(c.pose_a[k], sa[1]), R.box(c.pose_b[k], sb[1])
            if not R.boxes_intersect(ba, bb):
                seen["no_grid"] += 1
                continue
            origin, res = R.grid_of(ba, bb, c.voxel)
            seen["lds" if H.plane_bytes(res, c.inside) <= LDS_BUDGET else "glob"] += 1
            if c.inside:
                seen["x_res"][int(res[0])] = seen["x_res"].get(int(res[0]), 0) + 1
                seen["z_res"][int(res[2])] = seen["z_res"].get(int(res[2]), 0) + 1
            for shape, pose in ((sa, c.pose_a[k]), (sb, c.pose_b[k])):
                b = R.boundary_grid(pose, shape[0], origin, res, c.voxel)             # [y, z, x]
                seen["x0"] += int(b[:, :, 0].sum()); seen["x_last"] += int(b[:, :, -1].sum())
                seen["z0"] += int(b[:, 0, :].sum()); seen["z_last"] += int(b[:, -1, :].sum())
                seen["y0"] += int(b[0].sum()); seen["y_last"] += int(b[-1].sum())
                if not c.inside:
                    continue
                fx_, bx_ = R.parities(b, 2)
                fz_, bz_ = R.parities(b, 1)
                seen["disagree_x"] += int((~b & (fx_ != bx_)).any()); seen["disagree_z"] += int((~b & (fz_ != bz_)).any())
                if res[0] > 33:
                    f, w = b[:, :, 31] & ~b[:, :, 32], ~b[:, :, 31] & b[:, :, 32]
                    seen["fwd_seam"] += int(f.sum()); seen["bwd_seam"] += int(w.sum()); seen["both_seam"] += int((b[:, :, 31] & b[:, :, 32]).sum())
                    seen["odd_word1"] += int(fx_[:, :, 31].sum())
                if res[0] > 65:
                    seen["odd_word2"] += int(fx_[:, :, 63].sum())
                if res[2] > 33:
                    seen["z_fwd_seam"] += int((b[:, 31, :] & ~b[:, 32, :]).sum()); seen["z_bwd_seam"] += int((~b[:, 31, :] & b[:, 32, :]).sum())
    return bad, seen


def test_fixture_is_small_and_complete(fx):
    g, cases = fx
    biggest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                  if f.endswith(".npz") and not f.startswith("nms_"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "isect_hard.npz")) <= biggest
    assert {c.family for c in cases} == {"widths", "seams", "edges", "routes"}
    assert int(g["case_first"][-1]) == len(g["overlap"]) == sum(len(c) for c in cases)
    assert {c.name for c in cases if not c.reference} == {"widths_x4097", "widths_z4097"}


def test_restatement_reproduces_every_row(census):
    bad, _ = census
    assert not bad, bad[:5]


def test_census_of_the_fixture(census):
    _, seen = census
    for t in H.WIDTHS + (4096,):
        assert seen["x_res"].get(t, 0) >= 1 and seen["z_res"].get(t, 0) >= 1, (t, seen["x_res"], seen["z_res"])
    for key in ("fwd_seam", "bwd_seam", "both_seam", "z_fwd_seam", "z_bwd_seam", "odd_word1", "odd_word2", "x0", "x_last", "z0", "z_last", "y0", "y_last",
                "disagree_x", "disagree_z", "no_grid", "lds", "glob"):
        assert seen[key] >= 1, (key, seen)


def test_routes_call_mixes_its_routes(fx):
    """The "routes" call: disjoint, LDS, global, LDS, disjoint, ... at the default budget; the named pair's planes fit an LDS budget of
    their own size exactly, and other pairs lie on either side of it."""
    _, cases = fx
    c = next(c for c in cases if c.name == "routes")
    kinds = []
    for k in range(len(c)):
        ba, bb = R.box(c.pose_a[k], c.shapes[c.ia[k]][1]), R.box(c.pose_b[k], c.shapes[c.ib[k]][1])
        kinds.append("none" if not R.boxes_intersect(ba, bb) else H.plane_bytes(R.grid_of(ba, bb, c.voxel)[1]))
    assert len(c) == 40 and len({int(i) for i in c.ia} | {int(i) for i in c.ib}) == 2
    assert all((kinds[k] == "none") == (k % 4 == 0) for k in range(40))
    assert all(kinds[k] <= LDS_BUDGET for k in range(40) if k % 2) and all(kinds[k] > LDS_BUDGET for k in range(40) if k % 4 == 2)
    named = kinds[H.ROUTES_NAMED]
    grids = [v for v in kinds if v != "none"]
    assert any(v < named for v in grids) and any(v > named for v in grids) and named % 4 == 0


def test_restatement_reproduces_the_list(fx):
    g, _ = fx
    L = H.nms_list()
    assert (g["nms_shape_crc"] == [len(L["shape"][0]), H.crc(L["shape"][0]), len(L["shape"][1]), H.crc(L["shape"][1])]).all()
    assert L["poses"].tobytes() == g["nms_poses"].tobytes() and L["scores"].tobytes() == g["nms_scores"].tobytes()
    cen, poses, scores, thr = g["nms_centroid"], g["nms_poses"], g["nms_scores"], g["nms_dist_threshold"]
    i, j = (int(v) for v in g["nms_decider"])
    assert H.centroid_distance(cen, poses[i], poses[j]).view(np.uint32) == thr.view(np.uint32)          # one distance's exact fp32 value
    trace = []
    marks, keep, rounds, by_overlap = R.nms(L["shape"], cen, poses, scores, thr, trace)
    assert (marks == g["nms_marks"]).all() and (keep == np.flatnonzero(g["nms_marks"] == 1)).all() and rounds == len(keep)
    assert len(by_overlap) >= 5                                          # discards that the overlap alone decides
    # `<` rather than `<=` decides: one ulp more and the decider, second in score, is discarded by distance in the first round
    assert marks[i] == 1 and marks[j] == 1
    m2 = R.nms(L["shape"], cen, poses, scores, np.nextafter(thr, F(1)))[0]
    assert m2[j] == 2
    # equal scores: the first index of a group is picked first, and then discards or outlives the later ones; 0.01f and its neighbours
    assert (np.unique(scores, return_counts=True)[1] > 1).any()
    assert scores[21] == F(0.01) and scores[20] < F(0.01) < scores[22] and marks[20] == 2 and marks[21] == 1 and marks[22] == 1
    # a round whose launch holds both routes at the default budget.  The list was meant to mix routes in every round; it does so
    # in the early rounds only (10 of the 27, 24 of which have a grid at all): as the list thins out, the later rounds' few remaining pairs
    # are global-only or have no grid.  The census asks for one such round.
    per_round = {}
    for r, _, res in trace:
        if res is not None:
            per_round.setdefault(r, set()).add(H.plane_bytes(res) <= LDS_BUDGET)
    assert sum(v == {True, False} for v in per_round.values()) >= 1


def test_random_family_is_stable():
    """The clouds of the "random" family are the same bytes on every machine (they are compared with the restatement at test time)."""
    a, b = H.random_pairs(), H.random_pairs()
    assert [(x.crcs() == y.crcs()).all() and x.pose_b.tobytes() == y.pose_b.tobytes() for x, y in zip(a, b)] == [True, True]
    assert sum(len(c) for c in a) == 200 and {float(c.voxel) for c in a} == {float(F(0.05)), float(F(0.1))}
    grids = 0
    for c in a:
        for k in range(0, len(c), 10):
            ov, cnt = R.overlap(c.shapes[c.ia[k]], c.pose_a[k], c.shapes[c.ib[k]], c.pose_b[k], c.voxel, c.inside, c.by_smaller)
            grids += cnt[0] > 0
    assert grids >= 5
