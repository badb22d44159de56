"""GPU parity tests proper: the HIP path, called through the C ABI (ctypes -> librescan_hip.so),
against the golden vectors generated from the compiled reference and against the CPU oracle on
seeded inputs.  Bit-exact for indices / labels / distances; poses within 1e-4 Frobenius
(BASELINE.json north_star); scores within 2e-6 absolute (float result of an fp64 mean whose
summation order differs)."""
import numpy as np
import pytest

import os

from conftest import ROOT, golden_files, label_case, load_golden, rows_equal_up_to_ties

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4
SCORE_TOL = 2e-6
I4 = np.eye(4, dtype=np.float32).ravel()


@pytest.fixture(scope="module")
def capi():
    from rescan_amd import capi
    capi.init(0)
    return capi


@pytest.fixture(scope="module")
def scene_clouds(capi, gscene):
    """Scene at the two grid radii the reference uses (cell = 2*radius) + object clouds."""
    pts, nor = gscene["points"], gscene["normals"]
    clouds = {r: capi.Cloud(pts, nor, cell_size=2 * r) for r in (0.05, 0.1)}
    clouds[0.075] = capi.Cloud(pts, nor)                         # density-derived cell
    objs = [capi.Cloud(o["pos"], o["nor"], cell_size=0.1) for o in gscene["objects"]]
    return clouds, objs


# ---- radius-search rows ------------------------------------------------------------------

@pytest.mark.parametrize("fname", golden_files("rows_"))
def test_rows_vs_golden(capi, gscene, fname):
    g = load_golden(fname)
    for cell in (2 * float(g["grid_radius"]), 0.04, -1.0, 0.0):  # reference cell, a finer one, auto, brute-tile layout
        if cell == 0.0 and int(g["k"]) > 16:
            continue
        tgt = capi.Cloud(gscene["points"], None, cell_size=cell)
        d, i, nn, tot = capi.radius_search(tgt, g["query"], float(g["radius"]), int(g["k"]))
        rows_equal_up_to_ties(g["dists"], g["inds"], g["nn"], d, i, nn)
        assert tot == int(g["total"])
        tgt.close()


def test_rows_edge_cases(capi, oracle):
    rng = np.random.default_rng(5)
    tgt_pts = rng.uniform(0, 1, (500, 3)).astype(np.float32)
    tgt = capi.Cloud(tgt_pts, None, cell_size=0.1)
    # no queries
    d, i, nn, tot = capi.radius_search(tgt, np.zeros((0, 3), np.float32), 0.1, 4)
    assert tot == 0 and len(nn) == 0
    # k larger than the cloud, radius covering everything, ragged query count (not a multiple of 64)
    q = rng.uniform(-0.2, 1.2, (131, 3)).astype(np.float32)
    d, i, nn, tot = capi.radius_search(tgt, q, 5.0, 600)
    # (oracle grid with a cell big enough that the reference's 512-bin cap, msh_hash_grid.h:1101,1213,
    #  does not truncate the candidate set: the cap is a reference artefact the HIP path does not have)
    g = oracle.grid_create(tgt_pts, 2.0)
    od, oi, onn, otot = oracle.radius_search(g, q, 5.0, 600, 1)
    oracle.grid_destroy(g)
    rows_equal_up_to_ties(od, oi, onn, d, i, nn)
    assert (nn == 500).all() and tot == otot
    # duplicate points: equal distances everywhere; counts and distances still agree
    dup = np.repeat(tgt_pts[:50], 3, axis=0)
    t2 = capi.Cloud(dup, None, cell_size=0.1)
    d, i, nn, _ = capi.radius_search(t2, q, 0.3, 8)
    g = oracle.grid_create(dup, 0.05)
    od, oi, onn, _ = oracle.radius_search(g, q, 0.3, 8, 1)
    oracle.grid_destroy(g)
    assert (nn == onn).all()
    valid = np.arange(8)[None, :] < nn[:, None]
    assert (d[valid] == od[valid]).all()
    # single target point / empty target
    t3 = capi.Cloud(tgt_pts[:1], None, cell_size=0.1)
    d, i, nn, tot = capi.radius_search(t3, tgt_pts[:3], 0.5, 2)
    assert nn[0] == 1 and i[0, 0] == 0 and d[0, 0] == 0.0
    t4 = capi.Cloud(np.zeros((0, 3), np.float32), None, cell_size=0.1)
    d, i, nn, tot = capi.radius_search(t4, q, 0.5, 2)
    assert tot == 0


def test_rows_more_than_the_wave_kernels_list_can_hold(capi, oracle, gscene):
    """k_rows_wave keeps a query's hits in a 1 024-entry LDS list; a query with more points within the radius sends the whole
    call to the storage-free kernel.  Same rows either way (radius 0.4 m: thousands of points within reach)."""
    pts = gscene["points"]
    tgt = capi.Cloud(pts, None, cell_size=0.1)
    q = np.ascontiguousarray(pts[::997][:12])
    d, i, nn, tot = capi.radius_search(tgt, q, 0.4, 32)
    g = oracle.grid_create(pts, 0.2)
    dw, iw, nw, totw = oracle.radius_search(g, q, 0.4, 32, 1)
    oracle.grid_destroy(g)
    assert (nn == 32).all()
    rows_equal_up_to_ties(dw, iw, nw, d, i, nn.astype(np.int64))


# ---- ICP ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fname", golden_files("corrs_"))
def test_find_corrs_vs_golden(capi, gscene, scene_clouds, fname):
    g = load_golden(fname)
    clouds, objs = scene_clouds
    md = float(g["max_dist"])
    tgt = clouds[round(md, 3)]
    out = capi.icp_find_corrs(objs[int(g["obj"])], tgt, g["T1"], g["T2"], md, g["max_angle"])
    for a, name in zip(out, ("c_pts1", "c_nor1", "c_pts2", "c_nor2", "weights")):
        assert a.shape == g[name].shape, name
        assert (a == g[name]).all(), name


POLICY_TOL = 2e-5      # what the default estimator of object-sized sources is held to on the reference's fixtures (5 x inside north_star's 1e-4; measured <= 1.5e-5)


@pytest.mark.parametrize("fname", golden_files("icp_"))
def test_icp_align_vs_golden(capi, gscene, scene_clouds, fname):
    """The nine icp_align fixtures of the reference under the estimator POLICY (round 6, profiles/r06/estimator_policy.txt):
    the default at this size (<= 4 096 source points: the reference's own order) returns the reference's bits; the default of larger
    object-sized sources — lane chains: reference cut + reference centroid chains + fp64 moments, forced here by lowering the
    reference-order threshold — stays within POLICY_TOL of the reference's pose with the reference's iteration count; and the opt-in
    rs_hip_icp_reference_order_below( 65536 ) is bit-identical whatever the size."""
    g = load_golden(fname)
    clouds, objs = scene_clouds
    md = float(g["max_dist"])
    src, tgt = objs[int(g["obj"])], clouds[round(md, 3)]
    err, T, iters = capi.icp_align(src, tgt, g["T1"], g["T2"], md, g["max_angle"])
    assert np.linalg.norm(T.astype(np.float64) - g["T_out"].astype(np.float64)) < POSE_TOL
    assert abs(err - float(g["err"])) < 1e-5
    assert iters == int(g["iters"])
    if "RS_HIP_REF_ORDER_BELOW" not in os.environ and "RS_HIP_LANE_CHAINS_BELOW" not in os.environ:
        assert src.n <= capi.icp_reference_order_below(-1) and T.tobytes() == np.asarray(g["T_out"], np.float32).ravel().tobytes()
    prev = capi.icp_reference_order_below(0)
    try:
        e2, T2, it2 = capi.icp_align(src, tgt, g["T1"], g["T2"], md, g["max_angle"])                 # the lane chains
        assert np.linalg.norm(T2.astype(np.float64) - g["T_out"].astype(np.float64)) < POLICY_TOL and abs(e2 - float(g["err"])) < 1e-5 and it2 == int(g["iters"])
        capi.icp_reference_order_below(65536)
        e3, T3, it3 = capi.icp_align(src, tgt, g["T1"], g["T2"], md, g["max_angle"])                 # the opt-in
        assert T3.tobytes() == np.asarray(g["T_out"], np.float32).ravel().tobytes() and np.float32(e3) == np.float32(g["err"]) and it3 == int(g["iters"])
    finally:
        capi.icp_reference_order_below(prev)


@pytest.mark.parametrize("fname", golden_files("icp_"))
def test_icp_align_reference_order_is_bit_identical(capi, gscene, scene_clouds, fname):
    """Sources below the threshold run the estimator in the reference's own accumulation order: pose, error and
    iteration count are the reference's bits, not merely within tolerance (icp.h:136-148,210-298,393-402)."""
    g = load_golden(fname)
    clouds, objs = scene_clouds
    md = float(g["max_dist"])
    src = objs[int(g["obj"])]
    prev = capi.icp_reference_order_below(max(src.n, 65536))
    try:
        err, T, iters = capi.icp_align(src, clouds[round(md, 3)], g["T1"], g["T2"], md, g["max_angle"])
    finally:
        capi.icp_reference_order_below(prev)
    assert T.tobytes() == np.asarray(g["T_out"], np.float32).ravel().tobytes()
    assert np.float32(err).tobytes() == np.float32(g["err"]).tobytes()
    assert iters == int(g["iters"])


@pytest.mark.parametrize("fname", golden_files("icp_"))
def test_icp_parallel_reference_order_is_the_sequential_one(capi, gscene, scene_clouds, fname):
    """The reference-order estimator computed in parallel (replay: speculative segments + exact walk) returns the bits of the
    sequential chains (k_icp_faithful) — and so the reference's — on every ICP fixture."""
    g = load_golden(fname)
    clouds, objs = scene_clouds
    o = objs[int(g["obj"])]
    prev, prev_r = capi.icp_reference_order_below(-1), capi.icp_replay_below(-1)
    md = float(g["max_dist"])
    try:
        capi.icp_reference_order_below(1 << 30)
        e_s, T_s, it_s = capi.icp_align(o, clouds[round(md, 3)], g["T1"], g["T2"], md, g["max_angle"])
        capi.icp_reference_order_below(0); capi.icp_replay_below(1 << 30)
        e_p, T_p, it_p = capi.icp_align(o, clouds[round(md, 3)], g["T1"], g["T2"], md, g["max_angle"])
    finally:
        capi.icp_reference_order_below(prev); capi.icp_replay_below(prev_r)
    assert (T_p == T_s).all() and e_p == e_s and it_p == it_s
    assert T_p.tobytes() == np.asarray(g["T_out"], np.float32).ravel().tobytes() and it_p == int(g["iters"])


def test_icp_reference_order_vs_oracle_seeded(capi, oracle):
    """The same on fresh seeded scenes, as a batch (every problem of a batch is its own sequential chain), for
    whole scans with the threshold lifted, and for the estimator entry point; and the fp64 reduction, which larger
    sources get, stays within the pose tolerance of the same runs."""
    from rescan_amd import synth
    ang = np.float32(np.deg2rad(60.0))
    s0 = synth.make_scene(seed=21, density=1500, timestep=0)
    s1 = synth.make_scene(seed=21, density=1500, timestep=1)
    a = capi.Cloud(s0["points"], s0["normals"])
    rng = np.random.default_rng(8)
    prev = capi.icp_reference_order_below(-1)
    try:
        o = s1["objects"][1]
        oc = capi.Cloud(o["pos"], o["nor"])
        capi.icp_reference_order_below(65536)                 # (the opt-in: every call site of the reference in the reference's own order)
        T0s = np.stack([synth.perturbed_pose(o["pose"], rng, 0.05, 0.05) for _ in range(4)])
        errs, Ts, its = capi.icp_align_batch(oc, a, T0s, I4, 0.075, ang)
        for k in range(4):
            e_o, T_o, it_o = oracle.icp_align(o["pos"], o["nor"], s0["points"], s0["normals"], T0s[k], I4, 0.075, ang)
            assert Ts[k].tobytes() == T_o.tobytes() and np.float32(errs[k]).tobytes() == np.float32(e_o).tobytes() and its[k] == it_o
        # whole scan, threshold lifted / estimator forced to the fp64 reduction
        b = capi.Cloud(s1["points"], s1["normals"])
        T0 = synth.perturbed_pose(I4, rng, 0.03, 0.03)
        e_o, T_o, it_o = oracle.icp_align(s1["points"], s1["normals"], s0["points"], s0["normals"], T0, I4, 0.1, ang)
        capi.icp_reference_order_below(1 << 30)
        e_g, T_g, it_g = capi.icp_align(b, a, T0, I4, 0.1, float(ang))
        assert T_g.tobytes() == T_o.tobytes() and np.float32(e_g).tobytes() == np.float32(e_o).tobytes() and it_g == it_o
        c = oracle.icp_find_corrs(s1["points"], s1["normals"], s0["points"], s0["normals"], T0, I4, 0.1, ang)
        e_o2, T_o2 = oracle.icp_estimate_pt2pl(c[0], c[2], c[3], c[4], T0)
        e_g2, T_g2 = capi.icp_estimate_pt2pl(c[0], c[2], c[3], c[4], T0)
        assert T_g2.tobytes() == T_o2.tobytes() and np.float32(e_g2).tobytes() == np.float32(e_o2).tobytes()
        assert capi.icp_reference_order_below(0) == 1 << 30
        e_f, T_f, it_f = capi.icp_align(b, a, T0, I4, 0.1, float(ang))
        assert it_f == it_o and np.linalg.norm(T_f.astype(np.float64) - T_o) < POSE_TOL
        e_f2, T_f2 = capi.icp_estimate_pt2pl(c[0], c[2], c[3], c[4], T0)
        assert np.linalg.norm(T_f2.astype(np.float64) - T_o2) < POSE_TOL
    finally:
        capi.icp_reference_order_below(prev)


@pytest.mark.parametrize("estimator", ["sequential chains", "parallel chains", "fp64 moments"])
def test_icp_batch_matches_single(capi, gscene, scene_clouds, estimator):
    clouds, objs = scene_clouds
    rng = np.random.default_rng(3)
    from rescan_amd import synth
    o = gscene["objects"][1]
    T0s = np.stack([synth.perturbed_pose(o["pose"], rng) for _ in range(5)])
    prev, prev_r = capi.icp_reference_order_below(-1), capi.icp_replay_below(-1)
    try:
        capi.icp_reference_order_below(1 << 30 if estimator == "sequential chains" else 0)
        capi.icp_replay_below(1 << 30 if estimator == "parallel chains" else 0)
        errs, Ts, its = capi.icp_align_batch(objs[1], clouds[0.1], T0s, I4, 0.1, np.deg2rad(60.0))
        for k in range(5):
            e, T, it = capi.icp_align(objs[1], clouds[0.1], T0s[k], I4, 0.1, np.deg2rad(60.0))
            assert (T == Ts[k]).all() and e == errs[k] and it == its[k]
    finally:
        capi.icp_reference_order_below(prev); capi.icp_replay_below(prev_r)


def test_sequential_estimator_one_pass_statistics_and_centroids(capi, oracle, gscene, scene_clouds):
    """k_icp_faithful sums the dist² statistics (lib/rs/icp.h:393-402) and the weighted centroids (:136-148) in ONE pass, the 2.5
    sigma cut of the weights (:396-401) taken at a guess of sigma and checked afterwards.  Same bits as the three passes (switch
    0) and as the oracle, with the stop test on; a guess that is wrong on purpose (cut scaled by 0.5 / 2: points between the two
    cuts get the other weight) is caught by the check — the centroids are summed again (rs_hip_icp_faith_redone counts it) — and
    returns the same bits too; the guess as made is never redone here."""
    from rescan_amd import synth
    clouds, objs = scene_clouds
    rng = np.random.default_rng(23)
    pts, nor = gscene["points"], gscene["normals"]
    prev = capi.icp_faith_guess(-1)
    prev_ro = capi.icp_reference_order_below(65536)         # (the sequential estimator, whatever RS_HIP_REF_ORDER_BELOW the suite runs under)
    try:
        for k, o in enumerate(gscene["objects"]):
            for trial in range(2):
                T0 = synth.perturbed_pose(o["pose"], rng)
                got = {}
                for guess in (1000, 0, 500, 2000):
                    capi.icp_faith_guess(guess)
                    before = capi.icp_faith_redone()
                    e, T, it = capi.icp_align(objs[k], clouds[0.1], T0, I4, 0.1, np.deg2rad(60.0))
                    got[guess] = (np.float32(e).tobytes(), T.tobytes(), it, capi.icp_faith_redone() - before)
                assert got[1000][:3] == got[0][:3] == got[500][:3] == got[2000][:3], (k, trial)
                assert got[1000][3] == 0 and got[0][3] == 0, (k, trial, got[1000][3], got[0][3])
                assert got[500][3] > 0 or got[2000][3] > 0, (k, trial)          # (no dist² between a cut and half / twice it: not on these clouds)
                eo, To, ito = oracle.icp_align(o["pos"], o["nor"], pts, nor, T0, I4, 0.1, np.deg2rad(60.0))
                assert To.tobytes() == got[1000][1] and np.float32(eo).tobytes() == got[1000][0] and ito == got[1000][2], (k, trial)
    finally:
        capi.icp_faith_guess(prev); capi.icp_reference_order_below(prev_ro)


def test_icp_multi_source_batch_matches_single(capi, oracle, gscene, scene_clouds):
    """rs_hip_icp_align_multi: the per-placement refine loop (lib/rs/rs_database.h:220-230 — a DIFFERENT source per problem) as one
    call.  Every problem's pose, error and iteration count are those of its own rs_hip_icp_align — and, the sources being
    object-sized (reference-order estimator), the oracle's — bit for bit: sources of very different sizes (3 231 / 1 562 / 1 542
    points, a 700-point and a 9-point subset, a 30 k-point scan extract), the same source twice, with and without the stop test; a
    batch that holds a source above the estimator's range takes the problem-by-problem route and returns the same.  (Batches of
    more than 4 096 tiles — phase A + the cooperative kernel — are the headline suite's: test_strong_scaling_icp_units_vs_reference.)"""
    from rescan_amd import synth
    clouds, objs = scene_clouds
    rng = np.random.default_rng(17)
    pts, nor = gscene["points"], gscene["normals"]
    host = [(o["pos"], o["nor"]) for o in gscene["objects"]]
    poses = [o["pose"] for o in gscene["objects"]]
    sub = rng.permutation(len(host[0][0]))[:700]; host.append((host[0][0][sub], host[0][1][sub])); poses.append(poses[0])
    sub = rng.permutation(len(host[1][0]))[:9]; host.append((host[1][0][sub], host[1][1][sub])); poses.append(poses[1])
    big = np.sort(rng.permutation(len(pts))[:30000])
    host.append((np.ascontiguousarray(pts[big]), np.ascontiguousarray(nor[big]))); poses.append(I4)
    srcs = list(objs) + [capi.Cloud(p, n_, cell_size=0.1) for p, n_ in host[len(objs):]]
    order = [5, 0, 3, 1, 4, 2, 0]                                   # ragged, the big one first, source 0 twice
    T0s = np.stack([synth.perturbed_pose(poses[k], rng) for k in order])
    prev = capi.icp_reference_order_below(65536)                    # the opt-in: every problem in the reference's own order
    try:
        for md, ma, fixed, iters in ((0.1, 60.0, False, 100), (0.075, 50.0, True, 7)):
            ma = np.float32(np.deg2rad(np.float32(ma)))
            errs, Ts, its = capi.icp_align_multi([srcs[k] for k in order], clouds[0.1], T0s, I4, md, ma, max_iter=iters, fixed_iters=fixed)
            for j, k in enumerate(order):
                e, T, it = capi.icp_align(srcs[k], clouds[0.1], T0s[j], I4, md, ma, max_iter=iters, fixed_iters=fixed)
                assert (T == Ts[j]).all() and e == errs[j] and it == its[j], (j, k)
                if not fixed:
                    eo, To, ito = oracle.icp_align(host[k][0], host[k][1], pts, nor, T0s[j], I4, md, ma)
                    assert (To == Ts[j]).all() and np.float32(eo) == errs[j] and ito == its[j], (j, k)
        # Mixed batches: every problem gets the estimator its own call would get.  Threshold 2 000: the 30 k-point extract and the
        # 3 231-point table take the lane chains (one batch), the chairs and the subsets the reference's order (another); threshold
        # 20 000 with the lane chains off: the extract runs alone on the grid chains.  Same answers as the single calls, bit for bit.
        for ro, ln in ((2000, 65536), (20000, 0)):
            capi.icp_reference_order_below(ro); prev_l = capi.icp_lane_chains_below(ln)
            try:
                errs2, Ts2, its2 = capi.icp_align_multi([srcs[k] for k in order], clouds[0.1], T0s, I4, 0.1, np.deg2rad(60.0))
                for j, k in enumerate(order):
                    e, T, it = capi.icp_align(srcs[k], clouds[0.1], T0s[j], I4, 0.1, np.deg2rad(60.0))
                    assert (T == Ts2[j]).all() and e == errs2[j] and it == its2[j], (ro, ln, j, k)
            finally:
                capi.icp_lane_chains_below(prev_l)
    finally:
        capi.icp_reference_order_below(prev)
    # the DEFAULT policy on the same batch: within POLICY_TOL of the oracle (= the reference), equal iteration counts
    errs, Ts, its = capi.icp_align_multi([srcs[k] for k in order], clouds[0.1], T0s, I4, 0.1, np.deg2rad(60.0))
    for j, k in enumerate(order):
        eo, To, ito = oracle.icp_align(host[k][0], host[k][1], pts, nor, T0s[j], I4, 0.1, np.deg2rad(60.0))
        d = float(np.linalg.norm(Ts[j].astype(np.float64) - To))
        if k == 5:
            # The 30 k-point extract is a SUBSET OF ITS OWN TARGET: once aligned its residuals are the rounding noise of the coordinates
            # (error 3e-4, moving in the third digit with every rounding of the estimator), and the stop test |delta err| < 1e-5 fires two
            # iterations apart for any estimator that is not the reference's own order — including one that is exact everywhere
            # (oracle/price_estimators.py, mode 3).  Reported, held to 1e-3; the reference-order opt-in above returns the bits.
            print(f"self-alignment of a scan extract under the default estimator: {d:.2e} from the reference, {its[j]} vs {ito} iterations")
            assert d < 1e-3
            continue
        if len(host[k][0]) <= capi.icp_reference_order_below(-1):      # the reference's own order at this size: its bits
            assert d == 0.0 and its[j] == ito, (j, k, d)
            continue
        if len(host[k][0]) < 64:
            # (only under RS_HIP_REF_ORDER_BELOW=0 — tools/switch_matrix.sh — which puts the chains on the 9-point subset: six unknowns from
            #  nine correspondences, a system whose answer is its rounding noise; nothing but the reference's own order reproduces that)
            continue
        assert d < POLICY_TOL and its[j] == ito, (j, k, d)
    # an empty batch, a batch of one
    e0, T0, i0 = capi.icp_align_multi([], clouds[0.1], np.zeros((0, 16), np.float32))
    assert len(e0) == 0
    e1, T1, i1 = capi.icp_align_multi([srcs[1]], clouds[0.1], T0s[3:4])
    e, T, it = capi.icp_align(srcs[1], clouds[0.1], T0s[3])
    assert (T == T1[0]).all() and e == e1[0] and it == i1[0]


def test_icp_batch_of_scan_sized_sources_in_slices(capi, gscene):
    """Many start poses of a source above the reference-order range keep per-point records per problem; rs_hip_icp_align_batch runs
    them in slices of problems (RS_HIP_ICP_BATCH_BYTES).  The problems are independent: a batch cut into slices of one returns the
    bits of the batch run whole (a child process: the limit is read once)."""
    import subprocess, sys, json
    code = """
import sys, json, numpy as np
sys.path.insert(0, %r)
from rescan_amd import capi, synth
capi.init(0)
s = synth.make_scene(seed=5, density=1500.0, timestep=1)
a = capi.Cloud(s["points"], s["normals"]); 
rng = np.random.default_rng(2)
T0s = np.stack([synth.perturbed_pose(np.eye(4, dtype=np.float32).ravel(), rng, 0.01, 0.01) for _ in range(5)])
capi.icp_reference_order_below(0); capi.icp_replay_below(0)
errs, Ts, its = capi.icp_align_batch(a, a, T0s, max_iter=12)
print(json.dumps(dict(errs=errs.view(np.uint32).tolist(), Ts=Ts.view(np.uint32).ravel().tolist(), its=its.tolist())))
""" % ROOT
    outs = []
    for cap in ("4e9", "1"):
        env = dict(os.environ, RS_HIP_ICP_BATCH_BYTES=cap)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-600:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]
    assert max(outs[0]["its"]) > 3


CH_ROWS_TEST = 7


def test_exact_centroid_chains_are_the_sequential_sums(capi, gscene, scene_clouds):
    """Sources above the replay threshold centre the fp64 step on the reference's own centroid sums (Σw, Σw·p, Σw·q as
    sequential fp32 chains, icp.h:136-148).  Two implementations of those seven chains — pass 2 of the replay (itself held
    against the sequential kernel above) and the grid chains (integer sums per binade + a walk; the default) — must agree bit
    for bit: poses, errors and iteration counts of whole icp_align runs, on object-sized sources with both thresholds at zero
    (every fixture's start pose, batches included) and on whole scans."""
    from rescan_amd import synth
    clouds, objs = scene_clouds
    prev, prev_r, prev_c = capi.icp_reference_order_below(-1), capi.icp_replay_below(-1), capi.icp_exact_centroids(-1)
    prev_w = capi.icp_chains_retry_after(0)      # (every mode-1 call below tries the chains, also on a source that gave up before)
    prev_l = capi.icp_lane_chains_below(0)       # (the GRID chains at every size: object-sized sources would take the lane chains, test_lane_chains_are_the_sequential_sums)
    try:
        capi.icp_reference_order_below(0); capi.icp_replay_below(0)
        for fname in golden_files("icp_"):
            g = load_golden(fname)
            o = objs[int(g["obj"])]
            md = float(g["max_dist"])
            out = {}
            for mode in (1, 2):
                capi.icp_exact_centroids(mode)
                out[mode] = capi.icp_align(o, clouds[round(md, 3)], g["T1"], g["T2"], md, g["max_angle"])
            assert (out[1][1] == out[2][1]).all() and out[1][0] == out[2][0] and out[1][2] == out[2][2], fname
            assert np.linalg.norm(out[1][1].astype(np.float64) - g["T_out"]) < POSE_TOL, fname
        rng = np.random.default_rng(5)
        o = gscene["objects"][1]
        T0s = np.stack([synth.perturbed_pose(o["pose"], rng) for _ in range(4)])
        res = {}
        for mode in (1, 2):
            capi.icp_exact_centroids(mode)
            res[mode] = capi.icp_align_batch(objs[1], clouds[0.1], T0s, I4, 0.1, np.deg2rad(60.0))
        assert (res[1][1] == res[2][1]).all() and (res[1][0] == res[2][0]).all() and (res[1][2] == res[2][2]).all()
        # (2.6 M source points: more than the 512 blocks one round of the walks' forecasts covers — a second round, from the exact value so far)
        for n_pts, seed in ((70_000, 3), (330_000, 8), (2_600_000, 13)):
            s0 = synth.scene_for_point_count(n_pts, seed=seed, timestep=0)
            s1 = synth.scene_for_point_count(n_pts, seed=seed, timestep=1)
            # (one scan shifted so that its x coordinates straddle zero: a chain that changes sign on the way)
            shift = np.array([-float(np.median(s1["points"][:, 0])), 0.0, 0.0], np.float32) if seed == 3 else np.zeros(3, np.float32)
            a, b = capi.Cloud(s0["points"] + shift, s0["normals"]), capi.Cloud(s1["points"] + shift, s1["normals"])
            T0 = synth.perturbed_pose(I4, rng, 0.02, 0.01)
            out = {}
            gave_up = capi.icp_chains_gave_up()
            for mode in (1, 2):
                capi.icp_exact_centroids(mode)
                out[mode] = capi.icp_align(b, a, T0, I4, 0.1, np.deg2rad(60.0), **(dict(max_iter=6, fixed_iters=True) if n_pts > 1_000_000 else {}))
                if mode == 1:
                    print(f"{b.n} source points: segments the chain walks added one addend after the other in the last iteration: {capi.icp_replay_redone()}")
            assert (out[1][1] == out[2][1]).all() and out[1][0] == out[2][0] and out[1][2] == out[2][2], n_pts
            if n_pts == 330_000:
                # ... and as a batch of three start poses on the same scans: every problem its own walks, same bits as alone
                T0s = np.stack([T0] + [synth.perturbed_pose(I4, rng, 0.02, 0.01) for _ in range(2)])
                capi.icp_exact_centroids(1)
                eb, Tb, itb = capi.icp_align_batch(b, a, T0s, I4, 0.1, np.deg2rad(60.0), max_iter=5, fixed_iters=True)
                for k in range(3):
                    e1, T1, it1 = capi.icp_align(b, a, T0s[k], I4, 0.1, np.deg2rad(60.0), max_iter=5, fixed_iters=True)
                    assert (Tb[k] == T1).all() and eb[k] == e1 and itb[k] == it1, k
            # (a room in the positive octant: sums that grow steadily — the chains must not have handed the call to the replay;
            #  the shifted scan's x sums wander around zero: they may)
            assert seed == 3 or capi.icp_chains_gave_up() == gave_up, n_pts
            a.close(); b.close()
        # a scan that BEGINS with points that match nothing (a fifth of it moved 50 m away): its chains stay at exactly zero — no
        # binade — through 1 200 segments; they must be walked through as records, not added up addend by addend
        s0 = synth.scene_for_point_count(330_000, seed=21, timestep=0)
        s1 = synth.scene_for_point_count(330_000, seed=21, timestep=1)
        p1 = s1["points"].copy(); p1[: len(p1) // 5] += np.array([50.0, 0.0, 0.0], np.float32)
        a, b = capi.Cloud(s0["points"], s0["normals"]), capi.Cloud(p1, s1["normals"])
        T0 = synth.perturbed_pose(I4, rng, 0.02, 0.01)
        out = {}
        for mode in (1, 2):
            capi.icp_exact_centroids(mode)
            out[mode] = capi.icp_align(b, a, T0, I4, 0.1, np.deg2rad(60.0), max_iter=6, fixed_iters=True)
            if mode == 1:
                redone = capi.icp_replay_redone()
        assert (out[1][1] == out[2][1]).all() and out[1][0] == out[2][0] and out[1][2] == out[2][2]
        print(f"{b.n} source points, the first fifth unmatched: segments added one addend after the other over the six iterations: {redone}")
        assert redone < 6 * CH_ROWS_TEST * 60, redone
        a.close(); b.close()
        # both scans moved so that the median point is the origin: the x and z sums random-walk around zero and change binade
        # thousands of times — the chains give such a call up (a walk's budget), the library runs it again with the same seven sums
        # by pass 2 of the replay: same bits as asking for that directly
        s0 = synth.scene_for_point_count(330_000, seed=22, timestep=0)
        s1 = synth.scene_for_point_count(330_000, seed=22, timestep=1)
        shift = -np.median(s1["points"], axis=0).astype(np.float32)
        a, b = capi.Cloud(s0["points"] + shift, s0["normals"]), capi.Cloud(s1["points"] + shift, s1["normals"])
        gave_up = capi.icp_chains_gave_up()
        out = {}
        for mode in (1, 2):
            capi.icp_exact_centroids(mode)
            out[mode] = capi.icp_align(b, a, T0, I4, 0.1, np.deg2rad(60.0), max_iter=6, fixed_iters=True)
        assert (out[1][1] == out[2][1]).all() and out[1][0] == out[2][0] and out[1][2] == out[2][2]
        print(f"{b.n} source points around the origin: calls the chains gave up: {capi.icp_chains_gave_up() - gave_up}")
        a.close(); b.close()
    finally:
        capi.icp_reference_order_below(prev); capi.icp_replay_below(prev_r); capi.icp_exact_centroids(prev_c); capi.icp_chains_retry_after(prev_w); capi.icp_lane_chains_below(prev_l)


def test_lane_chains_are_the_sequential_sums(capi, gscene, scene_clouds):
    """Round 6: object-sized sources above the reference-order threshold take the LANE chains (one wave per centroid chain, 1 024 addends
    per stretch, sixteen per lane, on the integer grid of the sum's binade, fp32 one by one where that does not hold: rs_icp_chain.hip).  The seven sums
    must be the sequential fp32 sums whatever the input: whole icp_align runs against the same estimator with the sums by pass 2 of
    the replay (itself held against the sequential kernel) — poses, errors and iteration counts bit for bit — on every object
    fixture, batches, a scan whose x coordinates straddle zero (a chain that changes sign), a scan that begins with unmatched points
    (sums that stay exactly zero), scans centred on the origin (sums that hover: the fp32 stretches), and through
    rs_hip_icp_align_multi with sources of very different sizes; and every such pose within 1e-5 of the reference-order
    estimator's (the reference's bits) where that one is affordable."""
    from rescan_amd import synth
    clouds, objs = scene_clouds
    prev, prev_r, prev_c, prev_l = capi.icp_reference_order_below(-1), capi.icp_replay_below(-1), capi.icp_exact_centroids(-1), capi.icp_lane_chains_below(-1)
    prev_p = capi.icp_early_plain(0)      # (the replay route of a fixed-length call would run its early iterations without the sums this test is about)
    try:
        capi.icp_reference_order_below(0); capi.icp_replay_below(0)

        def both(fn):
            capi.icp_lane_chains_below(1 << 30); capi.icp_exact_centroids(1)
            a = fn()
            capi.icp_lane_chains_below(0); capi.icp_exact_centroids(2)
            b = fn()
            return a, b

        for fname in golden_files("icp_"):
            g = load_golden(fname)
            o = objs[int(g["obj"])]
            md = float(g["max_dist"])
            a, b = both(lambda: capi.icp_align(o, clouds[round(md, 3)], g["T1"], g["T2"], md, g["max_angle"]))
            assert (a[1] == b[1]).all() and a[0] == b[0] and a[2] == b[2], fname
            assert np.linalg.norm(a[1].astype(np.float64) - g["T_out"]) < 2e-5 and a[2] == int(g["iters"]), fname
        rng = np.random.default_rng(5)
        o = gscene["objects"][1]
        T0s = np.stack([synth.perturbed_pose(o["pose"], rng) for _ in range(4)])
        a, b = both(lambda: capi.icp_align_batch(objs[1], clouds[0.1], T0s, I4, 0.1, np.deg2rad(60.0)))
        assert (a[1] == b[1]).all() and (a[0] == b[0]).all() and (a[2] == b[2]).all()
        for n_pts, seed, centre in ((70_000, 3, "x"), (120_000, 8, None), (120_000, 22, "xyz"), (40_000, 23, "xyz")):
            s0 = synth.scene_for_point_count(n_pts, seed=seed, timestep=0)
            s1 = synth.scene_for_point_count(n_pts, seed=seed, timestep=1)
            shift = np.zeros(3, np.float32)
            if centre == "x":
                shift[0] = -float(np.median(s1["points"][:, 0]))
            if centre == "xyz":
                shift = -np.median(s1["points"], axis=0).astype(np.float32)
            p1 = s1["points"] + shift
            if seed == 8:
                p1 = p1.copy(); p1[: len(p1) // 5] += np.array([50.0, 0.0, 0.0], np.float32)      # (a fifth of it matches nothing, at the START of the chains)
            ca, cb = capi.Cloud(s0["points"] + shift, s0["normals"]), capi.Cloud(p1, s1["normals"])
            T0 = synth.perturbed_pose(I4, rng, 0.02, 0.01)
            seq0 = capi.icp_lane_chains_sequential()
            a, b = both(lambda: capi.icp_align(cb, ca, T0, I4, 0.1, np.deg2rad(60.0), max_iter=8, fixed_iters=True))
            print(f"{cb.n} source points (seed {seed}, centred {centre}): {capi.icp_lane_chains_sequential() - seq0} of {8 * 7 * cb.n} addends added one by one")
            assert (a[1] == b[1]).all() and a[0] == b[0] and a[2] == b[2], (n_pts, seed)
            capi.icp_reference_order_below(1 << 30)
            r = capi.icp_align(cb, ca, T0, I4, 0.1, np.deg2rad(60.0), max_iter=8, fixed_iters=True)
            capi.icp_reference_order_below(0)
            d = float(np.linalg.norm(a[1].astype(np.float64) - r[1].astype(np.float64)))
            print(f"   {d:.2e} from the reference-order estimator's pose")
            assert d < 1e-5
            ca.close(); cb.close()
        # rs_hip_icp_align_multi: problems of very different sizes side by side, each the bits of its own single call
        pts, nor = gscene["points"], gscene["normals"]
        host = [(o["pos"], o["nor"]) for o in gscene["objects"]]
        poses = [o["pose"] for o in gscene["objects"]]
        sub = rng.permutation(len(host[1][0]))[:9]; host.append((host[1][0][sub], host[1][1][sub])); poses.append(poses[1])
        big = np.sort(rng.permutation(len(pts))[:30000])
        host.append((np.ascontiguousarray(pts[big]), np.ascontiguousarray(nor[big]))); poses.append(I4)
        srcs = list(objs) + [capi.Cloud(p, n_, cell_size=0.1) for p, n_ in host[len(objs):]]
        order = [4, 0, 3, 1, 2, 0]
        T0m = np.stack([synth.perturbed_pose(poses[k], rng) for k in order])
        capi.icp_lane_chains_below(1 << 30); capi.icp_exact_centroids(1)
        for fixed, iters in ((False, 100), (True, 7)):
            errs, Ts, its = capi.icp_align_multi([srcs[k] for k in order], clouds[0.1], T0m, I4, 0.075, np.deg2rad(50.0), max_iter=iters, fixed_iters=fixed)
            for j, k in enumerate(order):
                e, T, it = capi.icp_align(srcs[k], clouds[0.1], T0m[j], I4, 0.075, np.deg2rad(50.0), max_iter=iters, fixed_iters=fixed)
                assert (T == Ts[j]).all() and e == errs[j] and it == its[j], (j, k)
    finally:
        capi.icp_reference_order_below(prev); capi.icp_replay_below(prev_r); capi.icp_exact_centroids(prev_c); capi.icp_lane_chains_below(prev_l); capi.icp_early_plain(prev_p)


def test_stop_test_guard_restores_the_reference_decision(capi, oracle):
    """Round 6.  An estimator that is not the reference's own order follows the reference's per-iteration errors to 1e-8 ... 6e-7; the stop
    test |err - prev_err| < 1e-5 (lib/rs/icp.h:489) decided by less than that falls the other way now and then — one iteration more or
    less, 1e-4 in the pose (2 of 49 object-sized runs in oracle/price_estimators.py's arithmetic).  The guard flags a problem whose
    decisive difference comes within 1.5e-6 of the threshold and runs it again in the reference's order.  Forty seeded object-to-scene
    runs with the lane chains forced on every size (3-9 k points: BELOW the default policy's range, where the reference's own rounding
    of a few thousand addends is largest — up to 2.4e-5 from an estimator that does not share it): with the guard OFF the poses are
    reported (flips show as ~1e-4); with it ON every run ends with the oracle's (= the reference's) iteration count, within 5e-5 of
    its pose, and some runs were redone."""
    from rescan_amd import synth
    prev, prev_r, prev_l, prev_g = capi.icp_reference_order_below(0), capi.icp_replay_below(0), capi.icp_lane_chains_below(1 << 30), capi.icp_stop_guard(-1.0)
    try:
        cases = []
        for seed in (21, 22, 23, 24, 25):
            s = synth.make_scene(seed=seed, density=2500, timestep=0, objects=("shelf", "chair", "table", "chair"))
            scn = capi.Cloud(s["points"], s["normals"])
            rng = np.random.default_rng(9)
            for o in s["objects"]:
                T0 = synth.perturbed_pose(o["pose"], rng)
                oc = capi.Cloud(o["pos"], o["nor"])
                for md, ma in ((0.1, 60.0), (0.075, 50.0)):
                    ma32 = np.float32(np.deg2rad(np.float32(ma)))
                    e_o, T_o, it_o = oracle.icp_align(o["pos"], o["nor"], s["points"], s["normals"], T0, I4, md, ma32)
                    cases.append((f"seed {seed} {o['kind']} r {md}", oc, scn, T0, md, ma32, T_o, it_o))
        report = {}
        for guard in (0.0, 1.5e-6):
            capi.icp_stop_guard(guard)
            redone0 = capi.icp_stop_guard_redone()
            worst, flips = 0.0, []
            for name, oc, scn, T0, md, ma32, T_o, it_o in cases:
                e, T, it = capi.icp_align(oc, scn, T0, I4, md, ma32)
                d = float(np.linalg.norm(T.astype(np.float64) - T_o))
                worst = max(worst, d)
                if it != it_o or d >= 5e-5:
                    flips.append((name, it, it_o, d))
            report[guard] = (worst, flips, capi.icp_stop_guard_redone() - redone0)
            print(f"\nstop-test guard {guard:g}: worst pose distance {worst:.2e}, runs off the reference's decision: {flips}, runs redone in reference order: {report[guard][2]} of {len(cases)}")
        assert report[0.0][2] == 0
        assert not report[1.5e-6][1] and report[1.5e-6][0] < 5e-5
        assert 0 < report[1.5e-6][2] < len(cases) // 2
    finally:
        capi.icp_reference_order_below(prev); capi.icp_replay_below(prev_r); capi.icp_lane_chains_below(prev_l); capi.icp_stop_guard(prev_g)


def test_icp_no_correspondences(capi, scene_clouds):
    clouds, objs = scene_clouds
    far = I4.copy(); far[12] = 100.0
    err, T, it = capi.icp_align(objs[0], clouds[0.1], far, I4, 0.1, np.deg2rad(60.0))
    assert err == np.float32(1e6) and (T == far).all() and it == 1      # icp.h:441-442,455-459


def test_icp_estimate_vs_oracle(capi, oracle, gscene):
    g = load_golden(golden_files("corrs_")[0])
    e_o, T_o = oracle.icp_estimate_pt2pl(g["c_pts1"], g["c_pts2"], g["c_nor2"], g["weights"], g["T1"])
    e_g, T_g = capi.icp_estimate_pt2pl(g["c_pts1"], g["c_pts2"], g["c_nor2"], g["weights"], g["T1"])
    assert np.linalg.norm(T_o.astype(np.float64) - T_g) < 1e-5 and abs(e_o - e_g) < 1e-6


# ---- alignment score ---------------------------------------------------------------------

@pytest.mark.parametrize("fname", golden_files("scores_"))
def test_scores_vs_golden(capi, scene_clouds, fname):
    g = load_golden(fname)
    clouds, objs = scene_clouds
    for cell in (0.05, 0.1):
        sc = capi.alignment_scores(objs[int(g["obj"])], clouds[cell], g["poses"], 0.1, int(g["k"]))
        assert np.abs(sc.astype(np.float64) - g["scores"]).max() < SCORE_TOL


@pytest.mark.parametrize("fname", golden_files("scores_"))
def test_scores_scene_space_route_vs_golden(capi, scene_clouds, fname):
    """The same fixtures through the scene-space route (queries sorted by scene block and normal direction, k_score_scene), which
    batches this small would not take by themselves: the reference's scores, and the object-space route's bits."""
    g = load_golden(fname)
    clouds, objs = scene_clouds
    for cell in (0.05, 0.1, 0.075):
        a = capi.alignment_scores(objs[int(g["obj"])], clouds[cell], g["poses"], 0.1, int(g["k"]))
        prev = capi.score_scene_space_from(0)
        try:
            b = capi.alignment_scores(objs[int(g["obj"])], clouds[cell], g["poses"], 0.1, int(g["k"]))
        finally:
            capi.score_scene_space_from(prev)
        assert np.abs(b.astype(np.float64) - g["scores"]).max() < SCORE_TOL
        assert (a == b).all()


def test_scores_scene_space_route_edge_cases(capi, scene_clouds):
    """Poses that put the object outside the scene, far outside, and non-finite poses: both routes agree bit for bit (NaN scores
    included)."""
    clouds, objs = scene_clouds
    rng = np.random.default_rng(7)
    I4 = np.eye(4, dtype=np.float32)
    poses = []
    for shift in (0.0, 0.3, 3.0, 50.0, 1e6):
        m = I4.copy(); m[3, :3] = rng.uniform(-1, 1, 3) * shift; poses.append(m.ravel())
    m = I4.copy(); m[3, 0] = np.nan; poses.append(m.ravel())
    m = I4.copy(); m[3, 1] = np.inf; poses.append(m.ravel())
    poses = np.stack(poses).astype(np.float32)
    for cell in (0.05, 0.1, 0.075):
        a = capi.alignment_scores(objs[0], clouds[cell], poses, 0.1, 64)
        prev = capi.score_scene_space_from(0)
        try:
            b = capi.alignment_scores(objs[0], clouds[cell], poses, 0.1, 64)
            c = capi.alignment_scores(objs[0], clouds[cell], poses[:1], 0.05, 32)
        finally:
            capi.score_scene_space_from(prev)
        assert (a.view(np.uint32) == b.view(np.uint32)).all(), (a, b)
        assert (c == capi.alignment_scores(objs[0], clouds[cell], poses[:1], 0.05, 32)).all()


# ---- label transfer ----------------------------------------------------------------------

@pytest.mark.parametrize("fname", golden_files("labels_"))
def test_labels_vs_golden(capi, gscene, scene_clouds, fname):
    d, objs, plcs = label_case(gscene, fname)
    clouds, _ = scene_clouds
    oc = [capi.Cloud(o["pos"], o["nor"], cell_size=0.1) for o in objs]
    poses = np.stack([p["pose"] for p in plcs])
    prio = bool(int(d["prioritize_static"]))
    res = capi.arrangement_to_labels(clouds[0.05], poses, [oc[p["object_idx"]] for p in plcs],
                                     [objs[p["object_idx"]]["is_static"] for p in plcs],
                                     [objs[p["object_idx"]]["class_idx"] for p in plcs], 0.05, prio)
    assert (res["order"] == d["order"]).all()
    assert (res["labels"] == d["labels"]).all()
    assert (res["min_dists"] == d["min_dists"]).all()
    ids = capi.arrangement_to_ids(clouds[0.05], poses, [oc[p["object_idx"]] for p in plcs],
                                  [objs[p["object_idx"]]["is_static"] for p in plcs], [objs[p["object_idx"]]["class_idx"] for p in plcs],
                                  [p["uidx"] for p in plcs], 0.05, prio, 0)
    assert (ids["class_ids"] == d["class_ids"]).all() and (ids["instance_ids"] == d["instance_ids"]).all()
    if prio:
        return        # the rows below model the shared min_dists of the default mode (rs_pointcloud_filters.cpp:841-848)
    # the sharded route: unary rows per placement, then the ordered arg-min, gives the same answer
    order = res["order"]
    first_static = next((k for k, oi in enumerate(order) if objs[plcs[oi]["object_idx"]]["is_static"]), 0)
    radii = [0.05 if k < first_static else np.float32(1.5) * np.float32(0.05) for k in range(len(order))]
    rows = capi.label_rows(clouds[0.05], poses[order], [oc[plcs[oi]["object_idx"]] for oi in order], radii)
    labels = np.zeros(len(gscene["points"]), np.int8); mind = np.full(len(gscene["points"]), 1e9, np.float32)
    capi.combine_label_rows(rows, labels, mind)
    assert (labels == d["labels"]).all() and (mind == d["min_dists"]).all()


def test_labels_prioritize_static_vs_oracle(capi, oracle, gscene, scene_clouds):
    d, objs, plcs = label_case(gscene, "labels_mixed.npz")
    clouds, _ = scene_clouds
    want = oracle.arrangement_to_labels(gscene["points"], gscene["normals"], objs, plcs, 0.05, 1, 0)
    oc = [capi.Cloud(o["pos"], o["nor"], cell_size=0.1) for o in objs]
    res = capi.arrangement_to_labels(clouds[0.05], np.stack([p["pose"] for p in plcs]),
                                     [oc[p["object_idx"]] for p in plcs],
                                     [objs[p["object_idx"]]["is_static"] for p in plcs],
                                     [objs[p["object_idx"]]["class_idx"] for p in plcs], 0.05, True)
    assert (res["labels"] == want["labels"]).all() and (res["min_dists"] == want["min_dists"]).all()


@pytest.mark.parametrize("fname", golden_files("labels_"))
@pytest.mark.parametrize("prioritize", [False, True])
def test_class_and_instance_ids_vs_oracle(capi, oracle, gscene, scene_clouds, fname, prioritize):
    """The tail of rspf_arrangement_to_labels (lib/rs/rs_pointcloud_filters.cpp:851-869), mapped on the device: the class of
    the labelled placement's object, the placement's uidx, (unlabelled class, 1024) where nothing was assigned."""
    d, objs, plcs = label_case(gscene, fname)
    clouds, _ = scene_clouds
    unl = 37
    want = oracle.arrangement_to_labels(gscene["points"], gscene["normals"], objs, plcs, 0.05, int(prioritize), unl)
    oc = [capi.Cloud(o["pos"], o["nor"], cell_size=0.1) for o in objs]
    res = capi.arrangement_to_ids(clouds[0.05], np.stack([p["pose"] for p in plcs]), [oc[p["object_idx"]] for p in plcs],
                                  [objs[p["object_idx"]]["is_static"] for p in plcs], [objs[p["object_idx"]]["class_idx"] for p in plcs],
                                  [p["uidx"] for p in plcs], 0.05, prioritize, unl)
    assert (res["class_ids"] == want["class_ids"]).all() and (res["instance_ids"] == want["instance_ids"]).all()
    assert (res["labels"] == want["labels"]).all() and (res["min_dists"] == want["min_dists"]).all()
    assert (res["instance_ids"][res["labels"] == 0] == 1024).all() and (res["class_ids"][res["labels"] == 0] == unl).all()


def test_level_attribute_gathers(capi, gscene):
    """rs_pointcloud.h:1090-1099: every per-point array of level 0 at the level's sample indices."""
    g = load_golden("level.npz")
    pts = gscene["points"]
    rng = np.random.default_rng(5)
    col = rng.random((len(pts), 3)).astype(np.float32); rad = rng.random(len(pts)).astype(np.float32)
    cls = rng.integers(0, 40, len(pts)).astype(np.int32)
    idx = g["own_l2"]
    out = capi.gather_attributes(idx, [pts, gscene["normals"], col, rad, cls])
    for got, src in zip(out, [pts, gscene["normals"], col, rad, cls]):
        assert np.array_equal(got, src[idx])
    assert capi.gather_attributes(np.zeros(0, np.int32), [rad])[0].shape == (0,)


# ---- neighbourhood graph -------------------------------------------------

def _edges_sorted(a, b, w, n):
    key = np.maximum(a, b).astype(np.int64) * n + np.minimum(a, b)
    o = np.argsort(key, kind="stable")
    return key[o], a[o], b[o], w[o]


def _weights_match(got, want):
    """Edge weights: the reference's value is (1 - pow(..)) * powf(..) from the host libm, and glibc's
    powf is only good to 0.82 ulp, so the float weight is defined up to its last bit.  The GPU
    evaluates both powers correctly rounded; bar: never more than 1 float ulp apart, and bit-identical
    on all but a sliver of the edges."""
    du = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert du.max() <= 1
    assert (du == 0).mean() > 0.998
    return int((du != 0).sum())


def test_neighborhood_vs_golden(capi, gscene):
    from oracle.pyoracle import edge_digest
    for fname in golden_files("neighborhood_obj"):
        d = load_golden(fname)
        o = gscene["objects"][int(d["obj"])]
        n = len(o["pos"])
        a, b, w = capi.compute_neighborhood(capi.Cloud(o["pos"], o["nor"]))
        kg, ag, bg, wg = _edges_sorted(a, b, w, n)
        kw, aw, bw, ww = _edges_sorted(d["idx1"], d["idx2"], d["weight"], n)
        assert (kg == kw).all() and (ag == aw).all() and (bg == bw).all()       # same pairs, same orientation
        _weights_match(wg, ww)
    a, b, w = capi.compute_neighborhood(capi.Cloud(gscene["points"], gscene["normals"]))
    want = load_golden("neighborhood_scene.npz")["digest"]       # [count, sum of pair keys, sum of weight bit patterns]
    got = edge_digest(a, b, w)
    assert got[0] == want[0] and got[1] == want[1]
    assert abs(int(got[2]) - int(want[2])) <= 0.002 * got[0]       # at most that many last-bit differences


def test_neighborhood_exponents_and_large(capi, oracle):
    from rescan_amd import synth
    s = synth.make_scene(seed=5, density=1500, timestep=0)
    pts, nor = s["points"][:40000].copy(), s["normals"][:40000].copy()
    c = capi.Cloud(pts, nor)
    n = len(pts)
    # integer exponents are evaluated exactly-then-rounded; fractional ones go through the device's double pow, rounded once
    for de, ae, exact in ((2.0, 3.0, True), (15.0, 16.0, True), (1.5, 0.5, False)):
        a, b, w = capi.compute_neighborhood(c, 8, 0.0025, de, ae)
        wa, wb, ww = oracle.compute_neighborhood(pts, nor, 8, 0.0025, de, ae)
        kg, ag, bg, wg = _edges_sorted(a, b, w, n)
        kw, aw, bw, wwt = _edges_sorted(wa, wb, ww, n)
        assert (kg == kw).all() and (ag == aw).all() and (bg == bw).all()
        if exact:
            _weights_match(wg, wwt)
        else:
            assert np.abs(wg - wwt).max() < 1e-6
    # other K / radius
    a, b, w = capi.compute_neighborhood(c, 4, 0.03 * 0.03)
    wa, wb, ww = oracle.compute_neighborhood(pts, nor, 4, 0.03 * 0.03)
    assert (_edges_sorted(a, b, w, n)[0] == _edges_sorted(wa, wb, ww, n)[0]).all()
    # n > 46340: the reference's int32 key max*n+min wraps and drops colliding pairs; the GPU keeps
    # every pair, so its edge set contains the reference's (same weights on the common pairs)
    big = synth.make_scene(seed=6, density=3000, timestep=0)
    bp, bn = big["points"], big["normals"]
    nb = len(bp)
    assert nb > 46340
    a, b, w = capi.compute_neighborhood(capi.Cloud(bp, bn))
    wa, wb, ww = oracle.compute_neighborhood(bp, bn)
    kg, _, _, wg = _edges_sorted(a, b, w, nb)
    kw, _, _, wwt = _edges_sorted(wa, wb, ww, nb)
    assert len(np.unique(kg)) == len(kg) and (np.bincount(a, minlength=nb) <= 8).all()
    pos = np.searchsorted(kg, kw)
    assert (pos < len(kg)).all() and (kg[pos] == kw).all()
    _weights_match(wg[pos], wwt)


# ---- scene-coverage term --------------------------------------------------

def test_level_builder_vs_golden(capi, gscene):
    """rs_pointcloud__compute_level_poisson: the sample indices are the reference's, exactly, for the
    scene's own point order (a few propagation steps) and a raster order (hundreds)."""
    from oracle.pyoracle import LEVEL_VOXEL, level_max_n_neigh
    g = load_golden("level.npz")
    pts = gscene["points"]
    for name, p in (("own", pts), ("raster", np.ascontiguousarray(pts[g["raster"]]))):
        cloud = capi.Cloud(p, None)
        steps = []
        for level in (1, 2, 3, 4):
            got, rounds = capi.level_samples(cloud, LEVEL_VOXEL[level], level_max_n_neigh(level))
            want = g[f"{name}_l{level}"]
            assert len(got) == len(want) and (got == want).all(), (name, level)
            steps.append(rounds)
        assert max(steps) >= 2
        cloud.close()


def test_level_cloud_built_on_the_device(capi, oracle, gscene):
    """rs_hip_cloud_create_level: samples, gather and index without a host round trip — the level cloud answers searches
    exactly like a cloud created from the same points on the host, and ICP against it returns the same bits."""
    from oracle.pyoracle import LEVEL_VOXEL, level_max_n_neigh
    g = load_golden("level.npz")
    pts, nor = gscene["points"], gscene["normals"]
    base = capi.Cloud(pts, nor)
    lvl, idx = capi.Cloud.level_of(base, LEVEL_VOXEL[2], level_max_n_neigh(2))
    assert (idx == g["own_l2"]).all() and lvl.n == len(idx)
    host = capi.Cloud(pts[idx], nor[idx])
    q = pts[::37] + np.float32(0.003)
    a = capi.radius_search(lvl, q, 0.05, 8); b = capi.radius_search(host, q, 0.05, 8)
    assert all((x == y).all() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    o = gscene["objects"][1]
    oc = capi.Cloud(o["pos"], o["nor"])
    r1 = capi.icp_align(oc, lvl, o["pose"], I4, 0.1, np.deg2rad(60.0)); r2 = capi.icp_align(oc, host, o["pose"], I4, 0.1, np.deg2rad(60.0))
    assert r1[1].tobytes() == r2[1].tobytes() and r1[2] == r2[2]
    c = capi.icp_find_corrs(oc, lvl, o["pose"], I4, 0.1, np.deg2rad(60.0)); d = capi.icp_find_corrs(oc, host, o["pose"], I4, 0.1, np.deg2rad(60.0))
    assert all(x.shape == y.shape and (x == y).all() for x, y in zip(c, d))          # host copies of the level were downloaded correctly


def test_level_builder_edge_cases(capi, oracle):
    from oracle.pyoracle import LEVEL_VOXEL, level_max_n_neigh
    rng = np.random.default_rng(12)
    base = rng.uniform(0, 0.5, (4000, 3)).astype(np.float32)
    cases = {
        "one": base[:1], "two close": np.array([[0, 0, 0], [0.001, 0, 0]], np.float32), "coincident": np.repeat(base[:4], 50, axis=0),
        "volume": base, "line": np.stack([np.linspace(0, 1, 3000), np.zeros(3000), np.zeros(3000)], 1).astype(np.float32),
        "exactly on the radius": np.array([[0, 0, 0], [0.02, 0, 0], [0.04, 0, 0], [0.0400001, 0, 0]], np.float32),
    }
    for name, p in cases.items():
        cloud = capi.Cloud(np.ascontiguousarray(p), None)
        for level in (2, 3):
            r, k = LEVEL_VOXEL[level], level_max_n_neigh(level)
            want = oracle.level_poisson(p, r, k)
            got, _ = capi.level_samples(cloud, r, k)
            assert len(got) == len(want) and (got == want).all(), (name, level)
        cloud.close()
    # empty cloud
    e = capi.Cloud(np.zeros((0, 3), np.float32), None)
    got, _ = capi.level_samples(e, 0.02, 512)
    assert len(got) == 0
    # a search the reference would truncate (more than max_n_neigh points within the radius) is refused, not approximated
    dense = capi.Cloud(rng.uniform(0, 0.01, (600, 3)).astype(np.float32), None)
    with pytest.raises(RuntimeError):
        capi.level_samples(dense, 0.02, 512)


def test_coverage_vs_golden(capi, gscene):
    from conftest import coverage_case
    d, objs, static, arrangements = coverage_case(gscene)
    cov = capi.Coverage(d["bbox_min"], d["bbox_max"], gscene["points"], d["quality"], 0.05, 0.5)
    assert tuple(cov.res) == tuple(d["res"]) and cov.n_cells == int(d["n_cells"]) and (cov.origin == d["origin"]).all()
    want_grid = np.unpackbits(d["scene_grid"])[:cov.n_cells]
    assert (cov.scene_grid() == want_grid).all() and cov.valid_cells == int(want_grid.sum())
    clouds = [capi.Cloud(p, np.zeros_like(p)) for p in objs]
    batch = [[(clouds[k], pose, static[k]) for k, pose in plc] for plc in arrangements]
    sc, agree = cov.scores(batch)                      # all 24 arrangements in one launch
    assert (sc == d["scores"]).all()
    one, _ = cov.scores(batch[5:6])                    # and one at a time, as the SA loop calls it
    assert one[0] == d["scores"][5]


def test_coverage_edge_cases(capi, oracle):
    from rescan_amd import synth
    s = synth.make_scene(seed=31, density=900, timestep=0)
    pts = s["points"]
    bmin, bmax = pts.min(0), pts.max(0)
    rng = np.random.default_rng(2)
    cov = capi.Coverage(bmin, bmax, pts, None, 0.07)
    g = oracle.voxgrid(bmin, bmax, 0.07)
    sd = oracle.rasterize_scene(g, pts)
    assert (cov.scene_grid() == sd).all()
    clouds = [capi.Cloud(o["pos"], o["nor"]) for o in s["objects"]]
    arrs, want = [], []
    for a in range(10):
        poses = [synth.perturbed_pose(o["pose"], rng, 1.5 if a % 2 else 0.1, 0.3) for o in s["objects"]]     # far moves push points out of the grid
        stat = [int(rng.uniform() < 0.3) for _ in s["objects"]]
        arrs.append([(clouds[k], poses[k], stat[k]) for k in range(len(clouds))])
        ad = oracle.rasterize_arrangement(g, [o["pos"] for o in s["objects"]], poses, stat)
        want.append(oracle.coverage_score(sd, ad))
    arrs.append([]); want.append((np.float32(0), 0, int(sd.sum())))                                           # empty arrangement
    sc, agree = cov.scores(arrs)
    assert (sc == np.array([w[0] for w in want], np.float32)).all() and (agree == [w[1] for w in want]).all()
    # a scene with no point above the quality threshold: empty grid, score 0 (not NaN)
    empty = capi.Coverage(bmin, bmax, pts, np.zeros(len(pts), np.float32), 0.07)
    assert empty.valid_cells == 0 and (empty.scores(arrs[:2])[0] == 0).all()


# ---- fresh seeded inputs against the oracle (sizes the oracle finishes in seconds) --------

def test_seeded_scene_vs_oracle(capi, oracle):
    from rescan_amd import synth
    s = synth.make_scene(seed=21, density=2500, timestep=0, objects=("shelf", "chair", "table", "chair"))
    pts, nor = s["points"], s["normals"]
    rng = np.random.default_rng(9)
    scn = capi.Cloud(pts, nor)                                   # density-derived cell (the default)
    scn_brute = capi.Cloud(pts[::7].copy(), nor[::7].copy(), cell_size=0.0)
    for o in s["objects"]:
        oc = capi.Cloud(o["pos"], o["nor"])
        T0 = synth.perturbed_pose(o["pose"], rng)
        want = oracle.icp_find_corrs(o["pos"], o["nor"], pts, nor, T0, I4, 0.1, np.float32(np.deg2rad(60.0)))
        got = capi.icp_find_corrs(oc, scn, T0, I4, 0.1, np.deg2rad(60.0))
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(want, got))
        e_o, T_o, it_o = oracle.icp_align(o["pos"], o["nor"], pts, nor, T0, I4, 0.1, np.float32(np.deg2rad(60.0)))
        e_g, T_g, it_g = capi.icp_align(oc, scn, T0, I4, 0.1, np.deg2rad(60.0))
        assert np.linalg.norm(T_o.astype(np.float64) - T_g) < POSE_TOL and it_o == it_g
        poses = np.stack([synth.perturbed_pose(o["pose"], rng, 0.4, 0.1) for _ in range(6)])
        sc_o = oracle.alignment_scores(pts, nor, o["pos"], o["nor"], poses, 64)
        sc_g = capi.alignment_scores(oc, scn, poses, 0.1, 64)
        assert np.abs(sc_o.astype(np.float64) - sc_g).max() < SCORE_TOL
        # brute-tile layout gives the same correspondences as the grid layout
        w_b = oracle.icp_find_corrs(o["pos"], o["nor"], pts[::7], nor[::7], T0, I4, 0.1, np.float32(np.deg2rad(60.0)))
        g_b = capi.icp_find_corrs(oc, scn_brute, T0, I4, 0.1, np.deg2rad(60.0))
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(w_b, g_b))


def test_quarter_million_points_vs_oracle(capi, oracle):
    """Scan-to-scan ICP on ~280 k points each: large enough for every mechanism of the search to engage
    (hand-off to the cooperative kernel, certificates, slow-tile lists, chunked device-side loop), small
    enough for the oracle (~15 s).  Correspondences bit-exact, pose within the north-star tolerance,
    same number of iterations."""
    from rescan_amd import synth
    s0 = synth.scene_for_point_count(250_000, seed=23, timestep=0)
    s1 = synth.scene_for_point_count(250_000, seed=23, timestep=1)
    a, b = capi.Cloud(s0["points"], s0["normals"]), capi.Cloud(s1["points"], s1["normals"])
    T0 = synth.perturbed_pose(I4, np.random.default_rng(3), 0.02, 0.02)
    ang = np.float32(np.deg2rad(60.0))
    want = oracle.icp_find_corrs(s1["points"], s1["normals"], s0["points"], s0["normals"], T0, I4, 0.1, ang)
    got = capi.icp_find_corrs(b, a, T0, I4, 0.1, np.deg2rad(60.0))
    assert all(x.shape == y.shape and (x == y).all() for x, y in zip(want, got))
    e_o, T_o, it_o = oracle.icp_align(s1["points"], s1["normals"], s0["points"], s0["normals"], T0, I4, 0.1, ang)
    e_g, T_g, it_g = capi.icp_align(b, a, T0, I4, 0.1, np.deg2rad(60.0))
    assert it_o == it_g and np.linalg.norm(T_o.astype(np.float64) - T_g) < POSE_TOL and abs(float(e_o) - float(e_g)) < 1e-6
    # scores (good and bad poses of a 10 k-point table) and the label transfer of 8 placements, same scene
    rng = np.random.default_rng(8)
    op, on = synth.make_object("table", 77, density=3800.0)
    tbl = [o for o in s1["objects"] if o["kind"] == "table"][0]
    poses = np.stack([synth.perturbed_pose(tbl["pose"], rng, 0.02 if k < 4 else 0.5, 0.02 if k < 4 else 0.25) for k in range(16)])
    sc_o = oracle.alignment_scores(s1["points"], s1["normals"], op, on, poses, 64)
    sc_g = capi.alignment_scores(capi.Cloud(op, on), b, poses, 0.1, 64)
    assert np.abs(sc_o.astype(np.float64) - sc_g).max() < SCORE_TOL
    objs, plcs = [], []
    for k, o in enumerate(s1["objects"][:8]):
        objs.append(dict(pos=o["pos"], nor=o["nor"], class_idx=o["class_idx"], is_static=int(k % 3 == 0)))
        plcs.append(dict(pose=synth.perturbed_pose(o["pose"], rng, 0.01, 0.005), object_idx=k, uidx=o["uidx"]))
    want = oracle.arrangement_to_labels(s1["points"], s1["normals"], objs, plcs, 0.05, 0, 0)
    res = capi.arrangement_to_labels(b, np.stack([p["pose"] for p in plcs]), [capi.Cloud(o["pos"], o["nor"]) for o in objs],
                                     [o["is_static"] for o in objs], [o["class_idx"] for o in objs], 0.05, False)
    assert (res["labels"] == want["labels"]).all() and (res["min_dists"] == want["min_dists"]).all() and (res["order"] == want["order"]).all()


def test_certificates_change_nothing(capi, monkeypatch):
    """The gate certificates and the rank certificates (rs_icp_search.hip: icp_certificate) only decide which source
    points are searched again; the poses and errors must be the same bits with either of them switched off
    (the fp64 estimator sums in a fixed order, the dist² statistics are integer sums).  The same holds for the per-row
    sweep of the warm tiles (sweep_by_rows): which lanes test which candidates is no part of the result."""
    from rescan_amd import synth
    s0 = synth.scene_for_point_count(250_000, seed=29, timestep=0)
    s1 = synth.scene_for_point_count(250_000, seed=29, timestep=1)
    a, b = capi.Cloud(s0["points"], s0["normals"]), capi.Cloud(s1["points"], s1["normals"])
    T0 = synth.perturbed_pose(I4, np.random.default_rng(4), 0.01, 0.01)
    runs = []
    for switch in (None, "RS_HIP_NO_RANK_CERT", "RS_HIP_NO_CERT", "RS_HIP_NO_BY_ROWS"):
        if switch:
            monkeypatch.setenv(switch, "1")
        e, T, it = capi.icp_align(b, a, T0, I4, 0.1, np.deg2rad(60.0), max_iter=12, fixed_iters=True)
        if switch:
            monkeypatch.delenv(switch)
        runs.append((np.float32(e).tobytes(), T.tobytes(), it))
    assert runs[0] == runs[1] == runs[2] == runs[3]


# ---- size-independent properties at BASELINE.json's full size (~1M-point clouds) -----------

def test_full_size_properties(capi):
    from rescan_amd import synth
    s = synth.scene_for_point_count(1_000_000, seed=11, timestep=0)
    pts, nor = s["points"], s["normals"]
    scn = capi.Cloud(pts, nor)
    rng = np.random.default_rng(1)
    # (1) self-search: every point's nearest neighbour within r is itself at distance 0
    sub = rng.integers(0, len(pts), 200_000)
    d, i, nn, _ = capi.radius_search(scn, pts[sub], 0.05, 1)
    assert (nn == 1).all() and (d[:, 0] == 0).all()
    same = i[:, 0] == sub
    assert same.all() or (pts[i[~same, 0]] == pts[sub[~same]]).all()       # exact duplicates may swap
    # (2) rows are sorted and within the radius; k-prefix property: rows(k=4) == rows(k=16)[:, :4]
    q = pts[sub[:50_000]] + rng.normal(0, 0.01, (50_000, 3)).astype(np.float32)
    d16, i16, nn16, _ = capi.radius_search(scn, q, 0.05, 16)
    d4, i4, nn4, _ = capi.radius_search(scn, q, 0.05, 4)
    valid = np.arange(16)[None, :] < nn16[:, None]
    assert (np.diff(d16, axis=1)[valid[:, 1:]] >= 0).all() and (d16[valid] < np.float32(0.05) ** 2).all()
    assert (nn4 == np.minimum(nn16, 4)).all()
    v4 = np.arange(4)[None, :] < nn4[:, None]
    assert (d4[v4] == d16[:, :4][v4]).all() and (i4[v4] == i16[:, :4][v4]).all()
    # (3) labels: a scene labelled by copies of its own instances recovers those instances
    inst = s["instance_idx"]
    objs, poses, stat, cls = [], [], [], []
    for o in s["objects"][:6]:
        objs.append(capi.Cloud(o["pos"], o["nor"], cell_size=0.1)); poses.append(o["pose"]); stat.append(0); cls.append(o["class_idx"])
    res = capi.arrangement_to_labels(scn, np.stack(poses), objs, stat, cls, 0.05, False)
    lab = res["labels"]
    for k, oi in enumerate(res["order"]):
        uid = s["objects"][oi]["uidx"]
        mine = inst == uid
        assert (lab[mine] == k + 1).mean() > 0.88           # its own scan points (fresh sampling; edge points fail the 70° gate)
        assert (lab[~mine & (inst >= 3)] != k + 1).mean() > 0.999
    # (4) ICP from a perturbed pose returns to the true pose; idempotent when restarted there
    o = s["objects"][3]
    oc = capi.Cloud(o["pos"], o["nor"], cell_size=0.1)
    T0 = synth.perturbed_pose(o["pose"], rng)
    e1, T1, _ = capi.icp_align(oc, scn, T0, I4, 0.1, np.deg2rad(60.0))
    assert np.abs(T1 - o["pose"]).max() < 5e-3
    e2, T2, _ = capi.icp_align(oc, scn, T1, I4, 0.1, np.deg2rad(60.0))
    assert np.linalg.norm(T2 - T1) < 2e-3 and abs(e2 - e1) < 1e-4


# ---- determinism ------------------------------------------------------------------------------

def test_icp_is_bit_reproducible_and_thread_safe(capi):
    """Run to run, and issued from several host threads at once, an ICP run returns the same bits (the
    cooperative kernel's waves must agree on which lanes a certificate lets them skip: a regression here
    showed up as 1-ulp pose differences between runs)."""
    from concurrent.futures import ThreadPoolExecutor
    from rescan_amd import synth
    s0 = synth.scene_for_point_count(300_000, seed=11, timestep=0)
    s1 = synth.scene_for_point_count(300_000, seed=11, timestep=1)
    a, b = capi.Cloud(s0["points"], s0["normals"]), capi.Cloud(s1["points"], s1["normals"])
    T0 = synth.perturbed_pose(I4, np.random.default_rng(16), 0.01, 0.01)
    run = lambda: capi.icp_align(b, a, T0, I4, 0.10, np.deg2rad(60.0), max_iter=10, fixed_iters=True)   # noqa: E731
    key = lambda r: (np.float32(r[0]).tobytes(), np.asarray(r[1], np.float32).tobytes())                  # noqa: E731
    ref = key(run())
    assert all(key(run()) == ref for _ in range(8))
    with ThreadPoolExecutor(max_workers=3) as pool:
        for _ in range(3):
            assert all(key(f.result()) == ref for f in [pool.submit(run) for _ in range(3)])


def test_cu_masked_stream_keeps_to_its_cus_and_changes_no_result(capi):
    """rs_hip_stream_cu_mask (bench.py keeps the score batch off the ICP chain's CUs with it): a worker thread's stream is
    confined to the mask bits [0, n/2); the probe's workgroups then run on half of the CUs of every XCD and on no other (bit i
    is CU slot i / 8 of XCD i % 8 — profiles/r02/cu_mask_probe.txt), and an ICP run issued on that stream returns the bits of
    an unmasked one."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from rescan_amd import synth
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    s0 = synth.scene_for_point_count(120_000, seed=5, timestep=0)
    s1 = synth.scene_for_point_count(120_000, seed=5, timestep=1)
    a, b = capi.Cloud(s0["points"], s0["normals"]), capi.Cloud(s1["points"], s1["normals"])
    T0 = synth.perturbed_pose(I4, np.random.default_rng(3), 0.01, 0.01)
    run = lambda: capi.icp_align(b, a, T0, I4, 0.10, np.deg2rad(60.0), max_iter=6, fixed_iters=True)   # noqa: E731
    key = lambda r: (np.float32(r[0]).tobytes(), np.asarray(r[1], np.float32).tobytes())                # noqa: E731
    ref = key(run())

    def placement():
        import os, sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
        import benchaux
        xcc, se, sh, cu = benchaux.probe_placement(8192)
        return set(zip(xcc.tolist(), se.tolist(), sh.tolist(), cu.tolist()))

    with ThreadPoolExecutor(max_workers=1) as pool:                 # (the mask belongs to the calling thread's stream)
        everywhere = pool.submit(placement).result()
        pool.submit(capi.stream_cu_mask, [1] * (n_cu // 2) + [0] * (n_cu - n_cu // 2)).result()
        half = pool.submit(placement).result()
        masked = key(pool.submit(run).result())
        pool.submit(capi.stream_cu_mask, None).result()             # back to an unrestricted stream
        again = pool.submit(placement).result()
    assert again == everywhere
    assert len(everywhere) == n_cu
    assert half < everywhere and len(half) == n_cu // 2
    assert len({x for x, _, _, _ in half}) == len({x for x, _, _, _ in everywhere})     # every XCD keeps CUs: the mask is per XCD
    assert masked == ref


def test_cloud_build_edge_cases(capi, oracle):
    """The device-side index build on degenerate inputs: tiny clouds, coincident points, a NaN coordinate,
    a huge sparse extent — searches on them still agree with the oracle."""
    rng = np.random.default_rng(5)
    base = rng.uniform(0, 1, (500, 3)).astype(np.float32)
    nor = np.tile(np.array([0, 0, 1], np.float32), (500, 1))
    cases = {
        "one": (base[:1], nor[:1]),
        "two": (base[:2], nor[:2]),
        "coincident": (np.repeat(base[:1], 300, axis=0), nor[:300]),
        "line": (np.stack([np.linspace(0, 1, 400), np.zeros(400), np.zeros(400)], 1).astype(np.float32), nor[:400]),
        "sparse_far": (np.concatenate([base[:200], base[:200] + np.float32(60.0)]), nor[:400]),
    }
    q = np.concatenate([base[:64], base[:8] + np.float32(60.0)])
    for name, (p, n) in cases.items():
        c = capi.Cloud(p.copy(), n.copy())
        g = oracle.grid_create(p, 0.5)                       # big cells: the reference's 512-bin cap stays out of the way
        for k, r in ((1, 0.05), (8, 0.3)):
            d, i, nn, _ = capi.radius_search(c, q, r, k)
            want = oracle.radius_search(g, q, r, k, 1)
            rows_equal_up_to_ties(d, i, nn, want[0], want[1], want[2].astype(nn.dtype))
        oracle.grid_destroy(g)
    # an extent of 1e5 m (the trial grids for the cell size do not fit; the table is capped): every point still finds itself
    p = np.concatenate([base[:200], base[:200] + np.float32(1.0e5)])
    c = capi.Cloud(p, nor[:400].copy())
    d, i, nn, _ = capi.radius_search(c, p, 0.05, 1)
    assert (nn == 1).all() and (d[:, 0] == 0).all()
    # a NaN coordinate never matches anything and breaks nothing
    p = base.copy(); p[7, 1] = np.nan
    c = capi.Cloud(p, nor.copy())
    d, i, nn, _ = capi.radius_search(c, base[:32], 0.2, 4)
    valid = np.arange(4)[None, :] < nn[:, None]
    assert (i[valid] != 7).all() and np.isfinite(d[valid]).all()
    assert capi.Cloud(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)).n == 0
