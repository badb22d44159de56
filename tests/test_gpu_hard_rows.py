"""GPU: the three consumers on top of the rows primitives of rescan_amd/csrc/rs_rows.hip -- the level builder (k_level_*), the
neighbourhood graph (k_rows + k_edge_*) and label transfer (k_label, k_label_fold*) -- on the hostile geometry of
tests/hard_clouds.py and the inputs tests/rows_restate.py adds to it, against the numpy restatements of rows_restate, which
tests/test_hard_rows_cpu.py holds to the CPU oracle.  Comparisons are exact (indices, labels, uint32 bits of min_dists) except
  - edge weights: the reference's float weight is defined up to its last bit (_weights_match, as tests/test_gpu_parity.py);
  - the two edge inputs with an exact tie across the 8th slot of a row, and the repeated-point cloud: the must / may bounds of
    rows_restate.edge_bounds, which every correct answer meets whichever tied point a row keeps.

The GPU work runs in child processes (this file, run as a script with a case name), each under its own time limit; nothing here
provokes a fault: every refusal is decided on the host -- the 127-placement cap before any launch, the level builder's
max_n_neigh after its counting pass (which writes two counts per point and a flag) and before anything is written through them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hard_clouds as hc_
import rows_restate as R_

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

pytestmark = pytest.mark.gpu

E_CAPACITY = "error -4"                                       # RS_HIP_E_CAPACITY, as capi reports it
LEVEL_EXTRA = ("collinear_sorted", "planar_raster", "repeated", "lattice0625", "lattice0625_shuffled")
EXPONENTS = ((15.0, 16.0), (2.0, 3.0), (1.0, 1.0), (0.0, 0.0), (64.0, 64.0), (65.0, 65.0), (1.5, 0.5))


def run_child(case, *args, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), case, *[str(a) for a in args]],
                         capture_output=True, text=True)
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139) or "illegal memory access" in out.stderr:
        # a time limit, an abort or a fault (timeout hands on its child's fatal signal: -6, -11, -9): nothing more is started on
        # this GPU, the evidence is what the child printed
        pytest.exit(f"{case} {args}: the child ended with {out.returncode}; the session stops here\n{out.stdout[-3000:]}\n{out.stderr[-3000:]}", 3)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


# ================================================================================================================================
# child side
# ================================================================================================================================

def _child_setup(with_torch):
    """(capi, oracle, rows_restate, hard_clouds) in a fresh process.  torch, where a case needs device memory of its own, has to
    initialise HIP before librescan_hip.so does (tests/conftest.py)."""
    for p in (HERE, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    if with_torch:
        import torch
        torch.cuda.init()
    from rescan_amd import capi
    from oracle.pyoracle import Oracle
    import hard_clouds as hc
    import rows_restate as R
    capi.init(0)
    return capi, Oracle(), R, hc


def _refused(capi, call):
    """The call raises capi's error with RS_HIP_E_CAPACITY."""
    try:
        call()
    except capi.RescanHipError as e:
        assert E_CAPACITY in str(e), str(e)
        return True
    return False


# ---- level builder ---------------------------------------------------------------------------------------------------------

def _level_input(R, name):
    """(points, [(radius, max_n_neigh), ...] in call order)."""
    from oracle.pyoracle import LEVEL_VOXEL, level_max_n_neigh
    if name.startswith("lattice0625"):                        # (the hard family "lattice" has spacing 0.125 and goes below)
        return R.lattice(shuffled=name.endswith("shuffled")), [(0.125, 512)]
    extra = R.level_extra_inputs()
    # 4, 1, 3, 2: the lanes per frontier item change between calls, and a small adjacency follows a large one in the workspace
    p, levels = (extra[name][0], (4, 1, 2)) if name in extra else (R.family(name)["points"], (4, 1, 3, 2))
    return p, [(LEVEL_VOXEL[lv], level_max_n_neigh(lv)) for lv in levels]


def _assert_samples(got, want, what):
    assert got.dtype == np.int32 and len(got) == len(want), (what, len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (what, len(bad), int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    assert (np.diff(got) > 0).all(), what


def case_levels(name):
    capi, O, R, hc = _child_setup(False)
    from oracle.pyoracle import LEVEL_VOXEL
    p, calls = _level_input(R, name)
    cloud = capi.Cloud(p, None)
    for r, cap in calls:
        stats = {}
        want, within = R.level_samples(p, r, stats)
        assert within <= cap
        got, rounds = capi.level_samples(cloud, r, cap)
        _assert_samples(got, want, (name, r))
        assert rounds >= 1
        print(name, r, "samples", len(got), "rounds", rounds, "depth", stats["depth"], "avg later", round(stats["avg_later"], 2))
        if name == "collinear_sorted" and r in (LEVEL_VOXEL[1], LEVEL_VOXEL[2]):     # levels 1 and 2: chains of 396 and 572 rounds
            assert stats["depth"] > 100 and rounds >= 100, rounds    # several 16-launch batches, the count carried between them
    cloud.close()


def case_level_cap():
    capi, O, R, hc = _child_setup(False)
    from oracle.pyoracle import LEVEL_VOXEL, level_max_n_neigh
    room = R.family("offset_1e3")["points"]
    rc = capi.Cloud(room, None)
    want = {lv: R.level_samples(room, LEVEL_VOXEL[lv])[0] for lv in (1, 2, 3, 4)}

    def room_still_right(lv):
        got, _ = capi.level_samples(rc, LEVEL_VOXEL[lv], level_max_n_neigh(lv))
        _assert_samples(got, want[lv], ("room after a refusal", lv))

    c256, c257 = R.cluster(256, 0.01), R.cluster(257, 0.01)
    got, _ = capi.level_samples(capi.Cloud(c256, None), 0.01, 256)
    assert list(got) == [0]                                   # exactly max_n_neigh within the radius: accepted, one sample
    assert _refused(capi, lambda: capi.level_samples(capi.Cloud(c257, None), 0.01, 256))
    room_still_right(2)
    got, _ = capi.level_samples(capi.Cloud(c257, None), 0.01, 257)
    assert list(got) == [0]
    dense = capi.Cloud(R.family("contrast")["points"], None)
    for lv in (1, 2, 3, 4):
        assert _refused(capi, lambda: capi.level_samples(dense, LEVEL_VOXEL[lv], level_max_n_neigh(lv))), lv
        room_still_right(lv)
    try:                                                      # the level cloud of a refused level: no cloud, the same reason
        capi.Cloud.level_of(dense, LEVEL_VOXEL[2], level_max_n_neigh(2))
        raise AssertionError("level_of built a level the level builder refuses")
    except capi.RescanHipError as e:
        assert "max_n_neigh" in str(e), str(e)
    room_still_right(2)


def case_level_of(name):
    capi, O, R, hc = _child_setup(False)
    from oracle.pyoracle import LEVEL_VOXEL, level_max_n_neigh
    f = R.family(name)
    p, nor = f["points"], f["normals"]
    r, cap = LEVEL_VOXEL[2], level_max_n_neigh(2)
    base = capi.Cloud(p, nor)
    want, within = R.level_samples(p, r)
    assert within <= cap
    lvl, idx = capi.Cloud.level_of(base, r, cap)
    _assert_samples(idx, want, name)
    got, _ = capi.level_samples(base, r, cap)
    _assert_samples(got, want, name)
    assert lvl.n == len(want)
    host = capi.Cloud(p[idx], nor[idx])
    q = np.ascontiguousarray(f["queries"][:1024])
    for k in (8, 16):
        a = capi.radius_search(lvl, q, 0.05, k); b = capi.radius_search(host, q, 0.05, k)
        assert (a[2] == b[2]).all() and a[3] == b[3] and a[3] > 0
        valid = np.arange(k)[None, :] < a[2][:, None]
        assert (a[0].view(np.uint32)[valid] == b[0].view(np.uint32)[valid]).all()
        hc.assert_rows(hc.brute_rows(p[idx], q, 0.05, k)[:4], a, p[idx], q)


# ---- neighbourhood graph ---------------------------------------------------------------------------------------------------

def _weights_match(got, want):
    """tests/test_gpu_parity.py: _weights_match, unchanged -- never more than 1 float ulp apart, identical on more than 99.8 %."""
    du = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert du.max() <= 1
    assert (du == 0).mean() > 0.998
    return int((du != 0).sum())


def _assert_weights(O, R, p, nor, a, b, w, r2, de=15.0, ae=16.0):
    d2, dot = R.edge_inputs(p, nor, a, b)
    want = R.edge_costs(O, d2, dot, r2, de, ae)
    assert np.isfinite(w).all()
    if de == np.floor(de) and ae == np.floor(ae):
        return _weights_match(w, want)
    assert np.abs(w - want).max() < 1e-6                      # fractional exponents: the bar of tests/test_gpu_parity.py
    return 0


def _assert_edge_rules(R, p, a, b, K, radius, cache, what):
    """What every correct answer meets, whichever of several exactly tied points fills the last slot of a full row."""
    n = len(p)
    must, may, tied = R.edge_bounds(p, radius, K, cache)
    assert ((a >= 0) & (a < n) & (b >= 0) & (b < n)).all(), what
    key = R.edge_key(a, b, n)
    assert len(np.unique(key)) == len(key), (what, "an undirected pair appears twice")
    assert (np.bincount(a, minlength=n) <= K).all(), (what, "more than K edges out of one row")
    a64, b64 = a.astype(np.int64), b.astype(np.int64)
    assert np.isin(a64 * n + b64, may).all(), (what, "an edge that no correct row holds")
    mi, mj = must // n, must % n
    assert np.isin(R.edge_key(mi, mj, n), key).all(), (what, "a pair that every correct row holds is missing")
    back = a64 > b64
    assert not np.isin(b64[back] * n + a64[back], must).any(), (what, "(i, j), i > j, although i is forced into row j")
    return tied


def _assert_edges_exact(R, rows, a, b, n, what):
    wa, wb = R.edges(rows[0], rows[1], rows[2], n)
    o = np.argsort(R.edge_key(a, b, n), kind="stable")
    assert len(a) == len(wa), (what, len(a), len(wa))
    assert (a[o] == wa).all() and (b[o] == wb).all(), (what, "pairs or orientation differ")


def case_edges(name):
    capi, O, R, hc = _child_setup(False)
    p, nor = R.edge_input(name)
    n, r = len(p), R.graph_radius(R.EDGE_R2)
    cloud = capi.Cloud(p, nor)
    a, b, w = capi.compute_neighborhood(cloud, R.EDGE_K, R.EDGE_R2)
    tied = _assert_edge_rules(R, p, a, b, R.EDGE_K, r, {}, name)
    if name in R.EDGE_TIE_FREE:
        assert len(tied) == 0
        _assert_edges_exact(R, hc.brute_rows(p, p, r, R.EDGE_K), a, b, n, name)
        assert (a == b).sum() == n
    else:
        assert len(tied) > 0
    print(name, "edges", len(a), "tied rows", len(tied), "weights off by an ulp", _assert_weights(O, R, p, nor, a, b, w, R.EDGE_R2))


def case_edge_exponents():
    capi, O, R, hc = _child_setup(False)
    p, nor = R.edge_input("offset_1e3")
    cloud = capi.Cloud(p, nor)
    first = None
    for de, ae in EXPONENTS:
        a, b, w = capi.compute_neighborhood(cloud, R.EDGE_K, R.EDGE_R2, de, ae)
        if first is None:
            first = a, b
            _assert_edges_exact(R, hc.brute_rows(p, p, R.graph_radius(R.EDGE_R2), R.EDGE_K), a, b, len(p), "offset_1e3")
        assert (a == first[0]).all() and (b == first[1]).all()
        print(de, ae, "off by an ulp", _assert_weights(O, R, p, nor, a, b, w, R.EDGE_R2, de, ae))


def case_edge_k(name):
    """K on both sides of the rows' tiled / wave switch (k = 16); with coincident points K = 1 is itself a tie."""
    capi, O, R, hc = _child_setup(False)
    p, nor = R.edge_input(name)
    n, r = len(p), R.graph_radius(R.EDGE_R2)
    cloud = capi.Cloud(p, nor)
    full = hc.brute_rows(p, p, r, 17)
    cache = {}
    exact = 0
    for K in (1, 2, 8, 16, 17):
        a, b, w = capi.compute_neighborhood(cloud, K, R.EDGE_R2)
        tied = _assert_edge_rules(R, p, a, b, K, r, cache, (name, K))
        if not len(tied):
            _assert_edges_exact(R, hc.truncate(full, K), a, b, n, (name, K)); exact += 1
        _assert_weights(O, R, p, nor, a, b, w, R.EDGE_R2)
        print(name, K, "edges", len(a), "tied rows", len(tied))
    assert exact >= 1 if name == "offset_1e3" else len(tied) > 0


def case_edge_lattice():
    """27 <= K points within the radius: the set is defined despite the ties, and no pair at d² == r² may appear."""
    capi, O, R, hc = _child_setup(False)
    p = R.lattice()
    nor = np.tile(np.float32([0.0, 0.0, 1.0]), (len(p), 1))
    r2 = 0.015625
    r = R.graph_radius(r2)
    assert r == np.float32(0.125)
    a, b, w = capi.compute_neighborhood(capi.Cloud(p, nor), 32, r2)
    rows = hc.brute_rows(p, p, r, 32)
    assert rows[2].max() == 27
    _assert_edges_exact(R, rows, a, b, len(p), "lattice")
    assert len(_assert_edge_rules(R, p, a, b, 32, r, {}, "lattice")) == 0
    d2, _ = R.edge_inputs(p, nor, a, b)
    assert (d2 < hc.radius_sq(r)).all() and (hc.d2_rows(p, p[:64]) == hc.radius_sq(r)).sum() > 200
    _assert_weights(O, R, p, nor, a, b, w, r2)


def case_edge_seams():
    """k_edge_scan is one 1024-thread workgroup that slices n: sizes around its slice boundaries."""
    capi, O, R, hc = _child_setup(False)
    P, N = R.edge_input("offset_1e3")
    r = R.graph_radius(R.EDGE_R2)
    for n in (1, 2, 1023, 1024, 1025, 2049):
        p, nor = np.ascontiguousarray(P[:n]), np.ascontiguousarray(N[:n])
        a, b, w = capi.compute_neighborhood(capi.Cloud(p, nor), R.EDGE_K, R.EDGE_R2)
        tied = _assert_edge_rules(R, p, a, b, R.EDGE_K, r, {}, n)
        assert not len(tied)
        _assert_edges_exact(R, hc.brute_rows(p, p, r, R.EDGE_K), a, b, n, n)
        _assert_weights(O, R, p, nor, a, b, w, R.EDGE_R2)


def case_edge_normals():
    """A zero normal gives powf(0, e), a flipped one clamps to 0, a scaled one clamps to 1."""
    capi, O, R, hc = _child_setup(False)
    p, nor = R.edge_input("planar")
    nor = R.degenerate_normals(nor)
    a, b, w = capi.compute_neighborhood(capi.Cloud(p, nor), R.EDGE_K, R.EDGE_R2)
    _assert_edges_exact(R, hc.brute_rows(p, p, R.graph_radius(R.EDGE_R2), R.EDGE_K), a, b, len(p), "planar")
    _, dot = R.edge_inputs(p, nor, a, b)
    assert (dot == 0).sum() > 1000 and (dot < 0).sum() > 1000 and (dot > 1).sum() > 1000
    _assert_weights(O, R, p, nor, a, b, w, R.EDGE_R2)
    assert (w[dot <= 0] == 0).all() and (w[(dot > 1) & (a != b)] > 0).any()


# ---- label transfer --------------------------------------------------------------------------------------------------------

def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _assert_result(got, want, what, ids=False):
    keys = ("labels", "order") + (("class_ids", "instance_ids") if ids else ())
    for k in keys:
        bad = np.nonzero(np.asarray(got[k]) != np.asarray(want[k]))[0]
        assert not len(bad), (what, k, len(bad), int(bad[0]))
    bad = np.nonzero(_bits(got["min_dists"]) != _bits(want["min_dists"]))[0]
    assert not len(bad), (what, "min_dists", len(bad), int(bad[0]), got["min_dists"][bad[0]], want["min_dists"][bad[0]])


def _arrangement_args(objects, placements, clouds):
    poses = np.stack([np.ascontiguousarray(p["pose"], np.float32).ravel() for p in placements]) if placements else np.zeros((0, 16), np.float32)
    return (poses, [clouds[p["object_idx"]] for p in placements], [objects[p["object_idx"]]["is_static"] for p in placements],
            [objects[p["object_idx"]]["class_idx"] for p in placements], [p["uidx"] for p in placements])


def _assert_arrangement(capi, R, tmin, inverse, scene_pos, scene_nor, objects, placements, radius, what, modes=(False, True),
                        object_cells=(0.1, -1.0, 0.0), scene_cells=(-1.0, 0.05)):
    """capi.arrangement_to_labels and arrangement_to_ids equal the restatement for every layout of the object and scene clouds."""
    cache = {}
    want = {prio: R.arrangement(scene_pos, scene_nor, objects, placements, radius, int(prio), 37, tmin, inverse, cache) for prio in modes}
    for w in want.values():
        assert w["tie_dependent"] == 0
    for oc in object_cells:
        clouds = [capi.Cloud(o["pos"], o["nor"], cell_size=oc) for o in objects]
        poses, ocl, stat, cls, uidx = _arrangement_args(objects, placements, clouds)
        for sc in scene_cells:
            scn = capi.Cloud(scene_pos, scene_nor, cell_size=sc)
            for prio in modes:
                got = capi.arrangement_to_labels(scn, poses, ocl, stat, cls, radius, prio)
                _assert_result(got, want[prio], (what, oc, sc, prio, "labels"))
                got = capi.arrangement_to_ids(scn, poses, ocl, stat, cls, uidx, radius, prio, 37)
                _assert_result(got, want[prio], (what, oc, sc, prio, "ids"), ids=True)
            scn.close()
        for c in clouds:
            c.close()
    return want


def case_labels(name):
    capi, O, R, hc = _child_setup(False)
    tmin = R.gate_tmin(O.label_gate)
    f = R.family(name)
    objects, placements = R.six_placements(f)
    want = _assert_arrangement(capi, R, tmin, O.mat4_inverse, f["points"], f["normals"], objects, placements, 0.05, name)
    print(name, "labelled", int((want[False]["labels"] != 0).sum()), int((want[True]["labels"] != 0).sum()))
    assert (want[False]["labels"] != 0).sum() >= 2


def case_label_split(name):
    capi, O, R, hc = _child_setup(True)
    import torch
    tmin = R.gate_tmin(O.label_gate)
    f = R.family("contrast" if name == "contrast9000" else name)
    sp, sn = R.contrast_subset() if name == "contrast9000" else (f["points"], f["normals"])
    objects, placements = R.six_placements(f)
    ns = len(sp)
    cache = {}
    whole = R.arrangement(sp, sn, objects, placements, 0.05, 0, 37, tmin, O.mat4_inverse, cache)
    prio = R.arrangement(sp, sn, objects, placements, 0.05, 1, 37, tmin, O.mat4_inverse, cache)
    assert whole["tie_dependent"] == 0 and prio["tie_dependent"] == 0 and (whole["labels"] != 0).sum() > 30
    clouds = [capi.Cloud(o["pos"], o["nor"]) for o in objects]
    scn = capi.Cloud(sp, sn)
    poses, ocl, stat, cls, uidx = _arrangement_args(objects, placements, clouds)
    _assert_result(capi.arrangement_to_labels(scn, poses, ocl, stat, cls, 0.05, False), whole, (name, "whole"))
    _assert_result(capi.arrangement_to_labels(scn, poses, ocl, stat, cls, 0.05, True), prio, (name, "prioritised"))
    order, radii = R.sorted_radii(objects, placements, 0.05)
    assert (order == whole["order"]).all()
    sposes, sclouds = poses[order], [ocl[i] for i in order]
    n_plc = len(order)

    def same(labels, mind, what):
        _assert_result(dict(labels=labels, min_dists=mind, order=order), whole, (name, what))

    # the chain cut after placements 1 and 4: three calls with carried state
    labels = np.zeros(ns, np.int8); mind = np.full(ns, 1e9, np.float32)
    for k0, k1 in ((0, 1), (1, 4), (4, n_plc)):
        capi.assign_labels(scn, sposes[k0:k1], sclouds[k0:k1], radii[k0:k1], labels, mind, label_base=k0)
    same(labels, mind, "three assign_labels calls")
    # unary rows, then the ordered arg-min on the host
    rows = capi.label_rows(scn, sposes, sclouds, radii)
    labels = np.zeros(ns, np.int8); mind = np.full(ns, 1e9, np.float32)
    capi.combine_label_rows(rows, labels, mind)
    same(labels, mind, "label_rows + combine_label_rows")
    # rows left on the device, folded there: fresh, from carried state, and in the scene's query order
    dev = torch.zeros(n_plc * ns, dtype=torch.float32, device="cuda:0")
    offs = [k * ns for k in range(n_plc)]
    capi.label_rows(scn, sposes, sclouds, radii, out_device_ptr=dev.data_ptr()); capi.synchronize()
    assert (_bits(dev.cpu().numpy().reshape(n_plc, ns)) == _bits(rows)).all()
    l, m = capi.fold_label_rows_device(dev.data_ptr(), offs, ns)
    same(l, m, "fold, fresh")
    l, m = capi.fold_label_rows_device(dev.data_ptr(), offs[:2], ns)
    l, m = capi.fold_label_rows_device(dev.data_ptr(), offs[2:], ns, l, m, label_base=2)
    same(l, m, "fold, carried")
    capi.label_rows(scn, sposes, sclouds, radii, out_device_ptr=dev.data_ptr(), query_order=True); capi.synchronize()
    l, m = capi.fold_label_rows_device(dev.data_ptr(), offs, ns, query_order_of=scn)
    same(l, m, "fold, query order, fresh")
    l, m = capi.fold_label_rows_device(dev.data_ptr(), offs[:4], ns, query_order_of=scn)
    l, m = capi.fold_label_rows_device(dev.data_ptr(), offs[4:], ns, l, m, label_base=4, query_order_of=scn)
    same(l, m, "fold, query order, carried")


def case_label_shell():
    capi, O, R, hc = _child_setup(False)
    tmin = R.gate_tmin(O.label_gate)
    for shifted in (False, True):
        sp, sn, obj, pose = R.shell(shifted)
        plc = [dict(pose=pose, object_idx=0, uidx=5)]
        want = _assert_arrangement(capi, R, tmin, O.mat4_inverse, sp, sn, [obj], plc, R.SHELL_RADIUS, ("shell", shifted))
        assert (want[True]["labels"][:6] == 0).all() and (want[True]["labels"][14:20] == 1).all() and (want[True]["labels"][28:] == 0).all()
        # the placement loop itself at radius r and at 1.5 r, from a fresh state
        for radius in (np.float32(R.SHELL_RADIUS), np.float32(1.5) * np.float32(R.SHELL_RADIUS)):
            wl = np.zeros(len(sp), np.int8); wm = np.full(len(sp), 1e9, np.float32)
            R.label_chain(sp, sn, [dict(pose=pose, pos=obj["pos"], nor=obj["nor"], radius=radius)], wl, wm, 0, tmin, O.mat4_inverse)
            for oc in (0.1, -1.0, 0.0):
                for sc in (-1.0, 0.05):
                    gl = np.zeros(len(sp), np.int8); gm = np.full(len(sp), 1e9, np.float32)
                    capi.assign_labels(capi.Cloud(sp, sn, cell_size=sc), pose[None, :], [capi.Cloud(obj["pos"], obj["nor"], cell_size=oc)], [radius], gl, gm)
                    assert (gl == wl).all() and (_bits(gm) == _bits(wm)).all(), (shifted, float(radius), oc, sc)
        print("shell", shifted, "labelled at r", int((want[True]["labels"] != 0).sum()), "at 1.5 r", int((want[False]["labels"] != 0).sum()))


def case_label_ties():
    capi, O, R, hc = _child_setup(False)
    tmin = R.gate_tmin(O.label_gate)
    sp, sn, obj, pose, r = R.lattice_ties()
    want = _assert_arrangement(capi, R, tmin, O.mat4_inverse, sp, sn, [obj], [dict(pose=pose, object_idx=0, uidx=5)], r, "lattice ties")
    assert want[True]["tied"] > 500 and (want[True]["labels"] == 1).all()          # ties occurred, and none decided anything


def case_label_zero_normals():
    capi, O, R, hc = _child_setup(False)
    tmin = R.gate_tmin(O.label_gate)
    f = R.family("offset_1e3")
    objects, placements = R.six_placements(f)
    caches = {prio: {} for prio in (False, True)}
    base = {prio: R.arrangement(f["points"], f["normals"], objects, placements, 0.05, int(prio), 37, tmin, O.mat4_inverse, caches[prio]) for prio in caches}
    sn, zobjects = R.zero_normals(f["normals"], objects)
    want = _assert_arrangement(capi, R, tmin, O.mat4_inverse, f["points"], sn, zobjects, placements, 0.05, "zero normals")
    zero = ~sn.any(axis=1)
    assert (base[False]["labels"][zero] != 0).any()
    for prio, w in want.items():
        # never labelled: a point whose own normal is zero; unchanged: a point whose normal and whose winner's normal are intact;
        # and a label won on a zeroed object normal is lost.  (The device equals `w` exactly, asserted above.)
        keep = R.zero_normal_survivors(base[prio], caches[prio], sn)
        b = base[prio]
        assert (w["labels"][zero] == 0).all() and (w["labels"] != 0).sum() > 100
        assert (w["labels"][keep] == b["labels"][keep]).all() and (_bits(w["min_dists"])[keep] == _bits(b["min_dists"])[keep]).all()
        lost = ~keep & (b["labels"] != 0)
        assert lost.sum() > 20 and (w["labels"][lost] != b["labels"][lost]).all()
        assert (keep & (b["labels"] != 0)).sum() > 100


def case_label_cap():
    capi, O, R, hc = _child_setup(False)
    import ctypes as C
    tmin = R.gate_tmin(O.label_gate)
    sp, sn, objects, placements = R.cap_arrangement(128)
    want = _assert_arrangement(capi, R, tmin, O.mat4_inverse, sp, sn, objects[:127], placements[:127], 0.05, "127 placements",
                               modes=(False,), object_cells=(-1.0,), scene_cells=(-1.0,))
    assert (want[False]["labels"] == 127).sum() >= 8 and want[False]["labels"].min() >= 0
    # 128: refused on the host, outputs untouched
    clouds = [capi.Cloud(o["pos"], o["nor"]) for o in objects]
    scn = capi.Cloud(sp, sn)
    poses, ocl, stat, cls, uidx = _arrangement_args(objects, placements, clouds)
    n = len(placements)
    labels = np.full(len(sp), 77, np.int8); mind = np.full(len(sp), -3.5, np.float32); order = np.full(n, -9, np.int32)
    handles = (C.c_void_p * n)(*[o.handle for o in ocl])
    rc = capi.load().rs_hip_arrangement_to_labels(scn.handle, poses, C.addressof(handles), np.ascontiguousarray(stat, np.int32),
                                                  np.ascontiguousarray(cls, np.int32), n, 0.05, 0, labels, mind, order)
    assert rc == -4 and (labels == 77).all() and (mind == np.float32(-3.5)).all() and (order == -9).all()
    assert _refused(capi, lambda: capi.arrangement_to_labels(scn, poses, ocl, stat, cls, 0.05, False))
    assert _refused(capi, lambda: capi.arrangement_to_ids(scn, poses, ocl, stat, cls, uidx, 0.05, False, 37))
    radii = [np.float32(0.05)] * n
    assert _refused(capi, lambda: capi.assign_labels(scn, poses, ocl, radii, labels, mind))
    assert _refused(capi, lambda: capi.assign_labels(scn, poses[:100], ocl[:100], radii[:100], labels, mind, label_base=28))
    assert (labels == 77).all() and (mind == np.float32(-3.5)).all()
    # and the next call is served
    got = capi.arrangement_to_labels(scn, poses[:127], ocl[:127], stat[:127], cls[:127], 0.05, False)
    _assert_result(got, want[False], "127 after the refusal")


def case_label_sizes():
    capi, O, R, hc = _child_setup(False)
    tmin = R.gate_tmin(O.label_gate)
    f = R.family("outside")
    objects, placements = R.six_placements(f)
    labelled = 0
    for n in (0, 1, 63, 64, 65, 257):
        for what, sel in zip(("prefix", "nearest the cut"), R.tiny_scenes(f, n)):
            sp, sn = np.ascontiguousarray(f["points"][sel]), np.ascontiguousarray(f["normals"][sel])
            if n:
                want = _assert_arrangement(capi, R, tmin, O.mat4_inverse, sp, sn, objects, placements, 0.05, (what, n), object_cells=(-1.0, 0.0))
                labelled += int((want[False]["labels"] != 0).sum())
                continue
            clouds = [capi.Cloud(o["pos"], o["nor"]) for o in objects]
            scn = capi.Cloud(sp.reshape(0, 3), sn.reshape(0, 3))
            poses, ocl, stat, cls, uidx = _arrangement_args(objects, placements, clouds)
            got = capi.arrangement_to_labels(scn, poses, ocl, stat, cls, 0.05, False)
            assert got["labels"].shape == (0,) and got["min_dists"].shape == (0,) and list(got["order"]) == [4, 0, 1, 2, 3, 5]
            got = capi.arrangement_to_ids(scn, poses, ocl, stat, cls, uidx, 0.05, True, 37)
            assert got["class_ids"].shape == (0,) and got["instance_ids"].shape == (0,)
            e8, e32 = np.zeros(0, np.int8), np.zeros(0, np.float32)
            capi.assign_labels(scn, poses, ocl, [0.05] * 6, e8, e32)
            assert capi.label_rows(scn, poses, ocl, [0.05] * 6).shape == (6, 0)
    assert labelled > 300


CASES = {f.__name__[5:]: f for f in (case_levels, case_level_cap, case_level_of, case_edges, case_edge_exponents, case_edge_k,
                                     case_edge_lattice, case_edge_seams, case_edge_normals, case_labels, case_label_split,
                                     case_label_shell, case_label_ties, case_label_zero_normals, case_label_cap, case_label_sizes)}

# ================================================================================================================================
# pytest side
# ================================================================================================================================

@pytest.mark.parametrize("name", R_.LEVEL_FAMILIES + LEVEL_EXTRA)
def test_level_samples(name):
    """capi.level_samples == the restatement, index for index and increasing: families at levels 4, 1, 3, 2 on one cloud; the
    sorted, raster and repeated inputs at 4, 1, 2 (sorted collinear at levels 1 and 2: at least 100 rounds); both lattices."""
    run_child("levels", name)


def test_level_max_n_neigh_boundary():
    """Exactly max_n_neigh points within the radius is accepted, one more is RS_HIP_E_CAPACITY, the contrast family is refused at
    every level, and the call after each refusal is right."""
    run_child("level_cap")


@pytest.mark.parametrize("name", ["offset_1e4", "negative"])
def test_level_cloud(name):
    """Cloud.level_of: the restatement's indices, and radius-search rows equal to a host-built cloud of the same points."""
    run_child("level_of", name)


@pytest.mark.parametrize("name", R_.EDGE_TIE_FREE + R_.EDGE_TIED + ("repeated",))
def test_neighborhood(name):
    """capi.compute_neighborhood at K = 8, r² = 0.0025: the must / may rules on every input, pairs and orientation exactly the
    restatement's on the tie-free ones, weights within the project's bar."""
    run_child("edges", name)


def test_neighborhood_exponents():
    run_child("edge_exponents")


@pytest.mark.parametrize("name", ["offset_1e3", "repeated"])
def test_neighborhood_k(name):
    run_child("edge_k", name)


def test_neighborhood_lattice():
    run_child("edge_lattice")


def test_neighborhood_scan_seams():
    run_child("edge_seams")


def test_neighborhood_degenerate_normals():
    run_child("edge_normals")


@pytest.mark.parametrize("name", hc_.FAMILIES)
def test_labels(name):
    """The six-placement arrangement in both modes through arrangement_to_labels and arrangement_to_ids, object clouds with cell
    0.1, the default and brute tiles, scene clouds with the default and 0.05: labels, min_dists bits, order and ids."""
    run_child("labels", name)


@pytest.mark.parametrize("name", ["offset_1e4", "contrast9000"])
def test_label_split_invariance(name):
    run_child("label_split", name)


def test_label_shell():
    run_child("label_shell")


def test_label_exact_ties():
    run_child("label_ties")


def test_label_zero_normals():
    run_child("label_zero_normals")


def test_label_cap():
    run_child("label_cap")


def test_label_scene_sizes():
    run_child("label_sizes")


if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print("ok")
