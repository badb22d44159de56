"""GPU parity of the HEADLINE workload and of the multi-GPU route, through the C ABI.

* bench.py's 1 M-point step (BASELINE.json configs[1]) against tests/golden/bench_seed11.npz, and the same step on a second
  synthetic room against bench_seed23.npz — what the compiled reference
  computes for the same inputs (oracle/gen_golden_bench.py): pose / error after the 10 fixed ICP iterations, per-iteration
  correspondence counts, the 256 alignment scores; labels / min_dists / class and instance ids of the reference's own label
  loops (rs_pointcloud_filters.cpp:738-879 compiled from its text, oracle/_ref/libref_filters.so).
* 24 scan-to-scan icp_align runs on >= 100 k-point scans against tests/golden/sweep_icp.npz (the reference's own icp_align):
  the fp64-moment estimator used for sources above RS_HIP_REF_ORDER_BELOW, and the reference-order estimator.
* the sharded route of bench.py (--shard / --gpus N): world of one, and a 2-way split simulated on one device, bit-identical
  to the unsharded entry points.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4
SCORE_TOL = 2e-6
I4 = np.eye(4, dtype=np.float32).ravel()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def capi():
    from rescan_amd import capi
    capi.init(0)
    return capi


@pytest.fixture(scope="module")
def bench_mod():
    sys.path.insert(0, ROOT)
    import bench
    return bench


@pytest.fixture(scope="module", params=[11, 23], ids=["seed11-the-bench-workload", "seed23"])
def headline(request, capi, bench_mod):
    """The bench workload (seed 11) and a second room of the same size (seed 23), each uploaded once for this module, and
    the fixture that pins it."""
    g = load_golden("bench_seed%d.npz" % request.param)
    w = bench_mod.build_workload(int(g["n_points"]), seed=int(g["seed"]), knn="hash")
    s0, s1 = w["s0"], w["s1"]
    op, on = w["obj_score_np"]
    got = [sha(s0["points"]), sha(s0["normals"]), sha(s1["points"]), sha(s1["normals"]), sha(op), sha(on),
           sha(w["score_poses"]), sha(w["plc_poses"]), sha(w["icp_T0"])]
    assert got == [str(x) for x in g["in_sha"]], "the generator no longer produces the inputs the fixture was made for"
    return w, g


def test_headline_icp_vs_reference(capi, bench_mod, headline):
    """The step's ICP (978 k -> 978 k points, 10 fixed iterations) ends within 1e-4 Frobenius of the reference's pose."""
    w, g = headline
    err, T, it = capi.icp_align(w["scan1"], w["scan0"], w["icp_T0"], I4, 0.10, np.deg2rad(60.0), max_iter=bench_mod.ICP_ITERS, fixed_iters=True)
    dist = np.linalg.norm(T.astype(np.float64) - g["icp_pose"].astype(np.float64))
    print(f"headline ICP: pose distance to the reference {dist:.3e}, err {err:.7f} vs {float(g['icp_err']):.7f}")
    assert it == bench_mod.ICP_ITERS
    assert dist < POSE_TOL
    assert abs(err - float(g["icp_err"])) < 1e-5


def test_headline_first_search_counts(capi, headline):
    """Iteration 0 searches from the same pose as the reference: the number of correspondences is the reference's."""
    w, g = headline
    out = capi.icp_find_corrs(w["scan1"], w["scan0"], w["icp_T0"], I4, 0.10, np.deg2rad(60.0))
    assert len(out[-1]) == int(g["icp_n_corrs"][0])


def test_headline_scores_vs_reference(capi, headline):
    w, g = headline
    sc = capi.alignment_scores(w["obj_score"], w["scan1"], w["score_poses"], 0.1, 64)
    d = np.abs(sc.astype(np.float64) - g["scores"].astype(np.float64)).max()
    print(f"headline scores: max abs error {d:.3e}")
    assert d < SCORE_TOL


def test_headline_labels_vs_reference(capi, headline):
    """Label transfer at the headline's size against the reference's own loops (rs_pointcloud_filters.cpp:738-879 compiled from
    its text, oracle/gen_golden_bench.py --labels-only): temporary labels, min_dists, class and instance ids, bit-exact."""
    w, g = headline
    assert "reference" in str(g["labels_source"])
    res = capi.arrangement_to_labels(w["scan1"], w["plc_poses"], [p["cloud"] for p in w["plc"]], [0] * len(w["plc"]),
                                     [p["cls"] for p in w["plc"]], 0.05, False)
    assert (res["order"] == g["order"]).all()
    assert (res["labels"] == g["labels"]).all()
    assert sha(res["min_dists"]) == str(g["min_dists_sha"])
    ids = capi.arrangement_to_ids(w["scan1"], w["plc_poses"], [p["cloud"] for p in w["plc"]], [0] * len(w["plc"]),
                                  [p["cls"] for p in w["plc"]], list(range(len(w["plc"]))), 0.05, False, 0)
    assert sha(ids["class_ids"]) == str(g["class_ids_sha"]) and sha(ids["instance_ids"]) == str(g["instance_ids_sha"])


def test_headline_labels_with_static_placements_vs_reference(capi, bench_mod, headline):
    """Label transfer at the headline's size WITH static placements — the second pass of rspf_arrangement_to_labels (1.5 x radius, shared
    or reset min_dists), the (static << 10 | class) ordering, static objects of 0.1 - 0.3 M points cut from the scan — against the
    reference's own loops (oracle/gen_golden_bench.py --static-labels: tests/golden/bench_labels_static_seed11.npz), both values of
    prioritize_static: temporary labels, min_dists, class and instance ids, bit-exact."""
    w, g0 = headline
    if int(g0["seed"]) != 11:
        pytest.skip("the static-arrangement fixture was made for seed 11")
    from conftest import static_label_case
    g, objs, plcs = static_label_case(w)
    assert "reference" in str(g["labels_source"])
    clouds = [p["cloud"] for p in w["plc"][:8]]
    made = [capi.Cloud(o["pos"], o["nor"]) for o in objs[8:]]
    clouds += made
    try:
        args = (w["scan1"], g["plc_pose"], [clouds[p["object_idx"]] for p in plcs], [objs[p["object_idx"]]["is_static"] for p in plcs],
                [objs[p["object_idx"]]["class_idx"] for p in plcs])
        for prio in (0, 1):
            res = capi.arrangement_to_ids(*args, [p["uidx"] for p in plcs], 0.05, bool(prio), 0)
            assert (res["order"] == g[f"order_prio{prio}"]).all()
            assert int((res["labels"] > 0).sum()) == int(g["n_labelled"][prio])
            for k in ("labels", "min_dists", "class_ids", "instance_ids"):
                assert sha(res[k]) == str(g[f"{k}_prio{prio}"]), (k, prio)
    finally:
        for c in made:
            c.close()


def test_headline_sharded_route_is_bit_identical(capi, bench_mod, headline):
    """bench.py's sharded route (rescan_amd.dist.shard_*) at world 1, and a 2-way split simulated on this device (both
    ranks' send buffers computed one after the other, concatenated as the all-gather would, folded), return the same
    bits as the unsharded entry points."""
    import torch
    from rescan_amd import dist as rd
    w, g = headline
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n_plc = len(w["plc"])
    order, _, radii = rd.arrangement_plan([0] * n_plc, [p["cls"] for p in w["plc"]], 0.05)
    T0s = np.stack([w["icp_T0"], w["icp_T0"]])                     # two ICP problems, so that a 2-way split gives each rank one
    units = dict(icp=(w["scan1"], w["scan0"], T0s, 0.10, np.deg2rad(60.0), bench_mod.ICP_ITERS),
                 score=(w["obj_score"], w["scan1"], w["score_poses"], 0.1, 64),
                 label=(w["scan1"], w["plc_poses"][order], [w["plc"][i]["cloud"] for i in order], radii))
    # unsharded
    err0, T0, it0 = capi.icp_align(w["scan1"], w["scan0"], w["icp_T0"], I4, 0.10, np.deg2rad(60.0), max_iter=bench_mod.ICP_ITERS, fixed_iters=True)
    sc0 = capi.alignment_scores(w["obj_score"], w["scan1"], w["score_poses"], 0.1, 64)
    lab0 = capi.arrangement_to_labels(w["scan1"], w["plc_poses"], [p["cloud"] for p in w["plc"]], [0] * n_plc, [p["cls"] for p in w["plc"]], 0.05, False)
    for world in (1, 2, 3):                                          # (3: ragged slices — 2 ICP problems, 256 poses, 8 placements over 3 ranks)
        lay = rd.ShardLayout(world, len(T0s), len(w["score_poses"]), n_plc, w["n_scan1"])
        recv = torch.zeros(world * lay.words, dtype=torch.float32, device=dev)
        for rank in range(world):
            send = recv[rank * lay.words:(rank + 1) * lay.words]   # "all-gather": rank r's buffer lands in slot r
            small = torch.zeros(lay.small_words, dtype=torch.float32)
            rd.shard_compute(capi, lay, rank, units, send, small)
            rd.shard_publish(lay, send, small)
        torch.cuda.synchronize()
        errs, Ts, its, scores, labels, mind = rd.shard_fold(capi, lay, recv, scene=w["scan1"])
        assert (Ts[0] == T0).all() and (Ts[1] == T0).all() and errs[0] == np.float32(err0) and its[0] == it0, f"world {world}: ICP"
        assert (scores == sc0).all(), f"world {world}: scores"
        assert (labels == lab0["labels"]).all() and (mind == lab0["min_dists"]).all(), f"world {world}: labels"


def test_many_problem_batches_take_the_narrow_cooperative_tiles(capi, bench_mod):
    """Round 6: a batch of more than eight ICP problems runs its cooperative searches at 4 waves per queued tile from 32 768 tiles in
    all, at 2 from 131 072 (rs_icp_api.hip: icp_coop_waves — such launches are throughput-bound; 512 refines: 33.8 -> 28.9 ms per step).
    Ten start poses of the headline scan (156 k tiles: 2 waves) — the eight of the units fixture, two of them twice — end where the
    reference's ten iterations end and where the single calls end, bit for bit; nine start poses of every fourth point of the scan
    (~35 k tiles: 4 waves) where their single calls end."""
    g = load_golden("bench_seed11_units.npz")
    w = bench_mod.build_workload(1_000_000, seed=11, knn="hash", units=8)
    try:
        assert np.array_equal(w["icp_T0s"], g["icp_T0s"][:8])
        T0s = np.concatenate([w["icp_T0s"], w["icp_T0s"][:2]])
        assert len(T0s) * (w["scan1"].n // 64) >= 131072          # (a tile holds at most 64 points: at least this many tiles)
        errs, Ts, its = capi.icp_align_batch(w["scan1"], w["scan0"], T0s, I4, 0.10, np.deg2rad(60.0), max_iter=bench_mod.ICP_ITERS, fixed_iters=True)
        ref = np.concatenate([g["icp_pose"][:8], g["icp_pose"][:2]]).astype(np.float64).reshape(-1, 16)
        d = np.linalg.norm(Ts.astype(np.float64).reshape(-1, 16) - ref, axis=1)
        print(f"ten start poses of the headline scan as one batch: pose distances from the reference's {d.max():.2e}")
        assert (d < 1e-5).all() and (its == bench_mod.ICP_ITERS).all()
        assert (Ts[8] == Ts[0]).all() and (Ts[9] == Ts[1]).all() and errs[8] == errs[0]
        for j in (0, 5):
            e, T, it = capi.icp_align(w["scan1"], w["scan0"], T0s[j], I4, 0.10, np.deg2rad(60.0), max_iter=bench_mod.ICP_ITERS, fixed_iters=True)
            assert (T == Ts[j]).all() and e == errs[j], j
        sub = capi.Cloud(np.ascontiguousarray(w["s1"]["points"][::4]), np.ascontiguousarray(w["s1"]["normals"][::4]))
        try:
            T9 = np.concatenate([w["icp_T0s"], w["icp_T0s"][:1]])
            assert 32768 <= len(T9) * (sub.n // 64) and len(T9) * (sub.n // 32) < 131072
            errs, Ts, its = capi.icp_align_batch(sub, w["scan0"], T9, I4, 0.10, np.deg2rad(60.0), max_iter=6, fixed_iters=True)
            for j in (0, 3, 8):
                e, T, it = capi.icp_align(sub, w["scan0"], T9[j], I4, 0.10, np.deg2rad(60.0), max_iter=6, fixed_iters=True)
                assert (T == Ts[j]).all() and e == errs[j] and it == its[j], j
        finally:
            sub.close()
    finally:
        _close_workload(w)


@pytest.mark.parametrize("n_ranks", [2, 4, 8])
def test_weak_scaling_unit_lists_vs_reference(capi, bench_mod, n_ranks):
    """Round 6 (missing 1a): what bench.py --gpus N computes at N > 1 under weak scaling — N ICP start poses, 256 N score
    poses, 8 N placements of the one scene — against the reference build's results for exactly those unit lists
    (tests/golden/bench_seed11_units.npz, oracle/gen_golden_bench.py --units): through the sharded route with the N ranks simulated
    on this device (every rank's send buffer computed in turn, concatenated as the all-gather would, the (min_dist, label) partials
    folded in rank order) AND through bench.parity_block, the function the bench line's `parity` comes from.  Every pose within
    1e-4 (measured ~1e-6), every score within 2e-6, labels / min_dists of the whole 8 N-placement arrangement bit for bit."""
    import torch
    from rescan_amd import dist as rd
    g = load_golden("bench_seed11_units.npz")
    w = bench_mod.build_workload(1_000_000, seed=11, knn="hash", units=n_ranks)
    try:
        assert [sha(w["s0"]["points"]), sha(w["s1"]["points"])] == [str(x) for x in g["in_sha"][:2]]
        assert np.array_equal(w["icp_T0s"], g["icp_T0s"][:n_ranks])
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        n_plc = len(w["plc"])
        assert n_plc == 8 * n_ranks
        order, _, radii = rd.arrangement_plan([0] * n_plc, [p["cls"] for p in w["plc"]], 0.05)
        assert (np.asarray(order) == g["order_u%d" % n_ranks]).all()
        units = dict(icp=(w["scan1"], w["scan0"], w["icp_T0s"], 0.10, np.deg2rad(60.0), bench_mod.ICP_ITERS),
                     score=(w["obj_score"], w["scan1"], w["score_poses"], 0.1, 64),
                     label=(w["scan1"], w["plc_poses"][order], [w["plc"][i]["cloud"] for i in order], radii))
        lay = rd.ShardLayout(n_ranks, n_ranks, len(w["score_poses"]), n_plc, w["n_scan1"], prefold=True)
        recv = torch.zeros(n_ranks * lay.words, dtype=torch.float32, device=dev)
        for rank in range(n_ranks):
            send = recv[rank * lay.words:(rank + 1) * lay.words]
            small = torch.zeros(lay.small_words, dtype=torch.float32)
            rd.shard_compute(capi, lay, rank, units, send, small)
            rd.shard_publish(lay, send, small)
        torch.cuda.synchronize()
        errs, Ts, its, scores, labels, mind = rd.shard_fold(capi, lay, recv, scene=w["scan1"])
        d = np.linalg.norm(Ts.astype(np.float64).reshape(-1, 16) - g["icp_pose"][:n_ranks].astype(np.float64).reshape(-1, 16), axis=1)
        print(f"N = {n_ranks}: pose distances {d.tolist()}, scores max abs {np.abs(scores.astype(np.float64) - g['scores'][:256 * n_ranks]).max():.2e}")
        assert (d < POSE_TOL).all() and (its == bench_mod.ICP_ITERS).all()
        assert np.abs(scores.astype(np.float64) - g["scores"][:256 * n_ranks].astype(np.float64)).max() < SCORE_TOL
        assert sha(labels) == str(g["labels_sha_u%d" % n_ranks]) and sha(mind) == str(g["min_dists_sha_u%d" % n_ranks])
        blk = bench_mod.parity_block(dict(err=errs[0], T=Ts[0], scores=scores, labels=labels, min_dists=mind, Ts=Ts, errs=errs), 1_000_000, 11, "hash", n_ranks)
        assert blk["label_mismatches"] == 0 and blk["min_dists_identical"] and blk["pose_dist_all_units"] < POSE_TOL and blk["score_max_abs_err_all_units"] < SCORE_TOL, blk
    finally:
        _close_workload(w)


def test_brute_tile_step_vs_reference(capi, bench_mod):
    """BASELINE.json configs[1] names the brute-tile k-NN: one full-size step with every target — both scans and the eight placed
    models — stored as ONE cell (bench.py --knn brute; every tile streams the whole target through LDS: ~3.4 s), against the
    reference's fixture: the same bars as the hash-cell layout."""
    g = load_golden("bench_seed11.npz")
    w = bench_mod.build_workload(int(g["n_points"]), seed=11, knn="brute")
    try:
        out = bench_mod.run_step(w, None, False)
        d = np.linalg.norm(np.asarray(out["T"], np.float64) - g["icp_pose"].astype(np.float64))
        print(f"brute-tile step: pose {d:.3e} from the reference, scores max abs {np.abs(out['scores'].astype(np.float64) - g['scores']).max():.2e}")
        assert d < POSE_TOL and np.abs(out["scores"].astype(np.float64) - g["scores"].astype(np.float64)).max() < SCORE_TOL
        assert (out["labels"] == g["labels"]).all() and sha(out["min_dists"]) == str(g["min_dists_sha"])
    finally:
        _close_workload(w)


def test_strong_scaling_split_is_bit_identical(capi, bench_mod, headline):
    """bench.py --scaling strong: ONE fixed scene — 8 per-placement ICP problems (model -> scan, lib/rs/rs_database.h:220-230),
    256 score poses, 8 placements — sharded over a simulated world of 1, 2, 3 and 8 ranks on this device (every rank's send
    buffer computed in turn, concatenated as the all-gather would, folded): every split returns the bits of the unsharded
    entry points."""
    import torch
    from rescan_amd import dist as rd
    w, g = headline
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n_plc = bench_mod.N_PLACEMENTS
    plc = w["plc"][:n_plc]
    order, _, radii = rd.arrangement_plan([0] * n_plc, [p["cls"] for p in plc], 0.05)
    si = w["strong_icp"]
    units = dict(icp=([p["cloud"] for p in plc], w["scan1"], si["T0s"], si["max_dist"], si["max_angle"], bench_mod.ICP_ITERS),
                 score=(w["obj_score"], w["scan1"], w["score_poses"][:bench_mod.N_POSES], 0.1, 64),
                 label=(w["scan1"], w["plc_poses"][order], [plc[i]["cloud"] for i in order], radii))
    ref = [capi.icp_align(plc[k]["cloud"], w["scan1"], si["T0s"][k], I4, si["max_dist"], si["max_angle"], max_iter=bench_mod.ICP_ITERS, fixed_iters=True) for k in range(n_plc)]
    sc0 = capi.alignment_scores(w["obj_score"], w["scan1"], w["score_poses"][:bench_mod.N_POSES], 0.1, 64)
    lab0 = capi.arrangement_to_labels(w["scan1"], w["plc_poses"][:n_plc], [p["cloud"] for p in plc], [0] * n_plc, [p["cls"] for p in plc], 0.05, False)
    for world, prefold in ((1, False), (2, False), (3, False), (8, False), (1, True), (3, True), (8, True), (12, True)):
        # (prefold: every rank sends the partial of its own run — 5 B per scene point — instead of its rows; 12 ranks: some without a placement)
        lay = rd.ShardLayout(world, n_plc, bench_mod.N_POSES, n_plc, w["n_scan1"], prefold=prefold)
        recv = torch.zeros(world * lay.words, dtype=torch.float32, device=dev)
        for rank in range(world):
            send = recv[rank * lay.words:(rank + 1) * lay.words]
            small = torch.zeros(lay.small_words, dtype=torch.float32)
            rd.shard_compute(capi, lay, rank, units, send, small)
            rd.shard_publish(lay, send, small)
        torch.cuda.synchronize()
        errs, Ts, its, scores, labels, mind = rd.shard_fold(capi, lay, recv, scene=w["scan1"])
        for k in range(n_plc):
            assert (Ts[k] == ref[k][1]).all() and errs[k] == np.float32(ref[k][0]) and its[k] == ref[k][2], f"world {world}: ICP problem {k}"
        assert (scores == sc0).all(), f"world {world}: scores"
        assert (labels == lab0["labels"]).all() and (mind == lab0["min_dists"]).all(), f"world {world} prefold {prefold}: labels"


def test_strong_scaling_icp_units_vs_reference(capi, bench_mod, headline):
    """The ICP units of bench.py --scaling strong — each placement's ~50 k-point model refined against the ~0.98 M-point scan with
    rsdb_refine_alignment_of_objects_to_scene's parameters (lib/rs/rs_database.h:220-230), ten fixed iterations — as ONE
    rs_hip_icp_align_multi call (8 sources, 6 000+ tiles: phase A and the cooperative kernel on per-problem source views) against
    the reference's own ten iterations of each (oracle/gen_golden_bench.py --strong-only): object-sized sources take the
    reference-order estimator, so the poses and errors are the reference's bit for bit; and against the eight single calls."""
    w, g = headline
    if "strong_icp_pose" not in g:
        pytest.skip("this room's fixture holds no --scaling strong units (bench_seed11.npz does)")
    n_plc = bench_mod.N_PLACEMENTS
    plc = w["plc"][:n_plc]
    si = w["strong_icp"]
    assert [sha(p["np"][0]) for p in plc] + [sha(si["T0s"])] == [str(x) for x in g["strong_icp_sha"]], "the generator no longer produces the fixture's inputs"
    # the DEFAULT estimator at this size (round 6: lane chains) against the bar; then the opt-in, bit for bit
    for opt_in in (False, True):
        prev = capi.icp_reference_order_below(65536 if opt_in else -1)
        try:
            errs, Ts, its = capi.icp_align_multi([p["cloud"] for p in plc], w["scan1"], si["T0s"], I4, si["max_dist"], si["max_angle"],
                                                 max_iter=bench_mod.ICP_ITERS, fixed_iters=True)
            d = np.linalg.norm(Ts.astype(np.float64).reshape(-1, 16) - g["strong_icp_pose"].astype(np.float64).reshape(-1, 16), axis=1)
            print("strong-scaling ICP units,", "reference order (opt-in):" if opt_in else "default estimator:", "pose distance from the reference's", d.tolist(),
                  "errors", errs.tolist(), g["strong_icp_err"].tolist())
            assert (its == bench_mod.ICP_ITERS).all()
            if opt_in:
                assert (d == 0.0).all() and (errs == g["strong_icp_err"]).all()
            else:
                assert (d < 1e-5).all() and np.abs(errs - g["strong_icp_err"]).max() < 1e-6
            for k in range(n_plc):
                e, T, it = capi.icp_align(plc[k]["cloud"], w["scan1"], si["T0s"][k], I4, si["max_dist"], si["max_angle"], max_iter=bench_mod.ICP_ITERS, fixed_iters=True)
                assert (T == Ts[k]).all() and e == errs[k] and it == its[k]
        finally:
            capi.icp_reference_order_below(prev)


MORE_SEEDS = list(range(31, 39))


def _close_workload(w):
    seen = set()
    for c in [w["scan0"], w["scan1"], w["obj_score"]] + [p["cloud"] for p in w["plc"]]:      # (units > 1: further placements share their model's cloud)
        if id(c) not in seen:
            seen.add(id(c)); c.close()


@pytest.mark.parametrize("seed", MORE_SEEDS)
def test_more_headline_rooms_vs_reference(capi, bench_mod, seed):
    """Eight more rooms of the headline's size (round 3: oracle/gen_golden_bench.py --more), each through the DEFAULT path
    at that size.  Every one must hold north_star's bar — no budget of exceptions: the step's ICP (10 fixed iterations) and
    the reference's own icp_align WITH its stop test (lib/rs/icp.h:489; the three call sites' parameters in turn, start poses
    from 5 mm / 0.3 deg to 3 cm / 2 deg) end within 1e-4 Frobenius of the reference's pose, the 256 scores within 2e-6,
    labels / min_dists bit for bit."""
    g = load_golden("bench_seed%d.npz" % seed)
    w = bench_mod.build_workload(int(g["n_points"]), seed=int(g["seed"]), knn="hash")
    try:
        s0, s1 = w["s0"], w["s1"]
        op, on = w["obj_score_np"]
        got = [sha(s0["points"]), sha(s0["normals"]), sha(s1["points"]), sha(s1["normals"]), sha(op), sha(on),
               sha(w["score_poses"]), sha(w["plc_poses"]), sha(w["icp_T0"])]
        assert got == [str(x) for x in g["in_sha"]], "the generator no longer produces the inputs the fixture was made for"
        err, T, it = capi.icp_align(w["scan1"], w["scan0"], w["icp_T0"], I4, 0.10, np.deg2rad(60.0), max_iter=bench_mod.ICP_ITERS, fixed_iters=True)
        d_fixed = np.linalg.norm(T.astype(np.float64) - g["icp_pose"].astype(np.float64))
        md, ma = float(g["stop_params"][0]), float(g["stop_params"][1])
        e2, T2, it2 = capi.icp_align(w["scan1"], w["scan0"], g["stop_T0"], I4, md, ma)
        d_stop = np.linalg.norm(T2.astype(np.float64) - g["stop_pose"].astype(np.float64))
        sc = capi.alignment_scores(w["obj_score"], w["scan1"], w["score_poses"], 0.1, 64)
        d_sc = np.abs(sc.astype(np.float64) - g["scores"].astype(np.float64)).max()
        res = capi.arrangement_to_labels(w["scan1"], w["plc_poses"], [p["cloud"] for p in w["plc"]], [0] * len(w["plc"]),
                                         [p["cls"] for p in w["plc"]], 0.05, False)
        print(f"seed {seed}: 10 fixed iterations {d_fixed:.3e} from the reference (err {err:.7f} vs {float(g['icp_err']):.7f}); "
              f"icp_align r {md:.3f}: {d_stop:.3e}, {it2} vs {int(g['stop_iters'])} iterations, err {e2:.7f} vs {float(g['stop_err']):.7f}; "
              f"scores max abs {d_sc:.2e}, {int((sc == g['scores']).sum())} of {len(sc)} bit-identical")
        assert it == bench_mod.ICP_ITERS and d_fixed < POSE_TOL and abs(err - float(g["icp_err"])) < 1e-5
        assert d_stop < POSE_TOL, f"icp_align with the stop test: {d_stop:.3e} from the reference ({it2} vs {int(g['stop_iters'])} iterations)"
        assert it2 == int(g["stop_iters"]), f"icp_align with the stop test: {it2} vs the reference's {int(g['stop_iters'])} iterations"
        assert d_sc < SCORE_TOL
        assert (res["order"] == g["order"]).all()
        assert "reference" in str(g["labels_source"])
        assert sha(res["labels"]) == str(g["labels_sha"]) and sha(res["min_dists"]) == str(g["min_dists_sha"])
    finally:
        _close_workload(w)


def test_traced_icp_is_the_same_call(capi, headline):
    """rs_hip_icp_align_traced (behind the shim's icp_align( ..., verbose = true ), lib/rs/icp.h:482-486): the per-iteration errors of the
    headline's ten fixed iterations against the reference's (fixture icp_errs), the result the untraced call's bit for bit; and an
    object-sized source with the stop test on."""
    w, g = headline
    e0, T0, it0 = capi.icp_align(w["scan1"], w["scan0"], w["icp_T0"], I4, 0.10, np.deg2rad(60.0), max_iter=10, fixed_iters=True)
    e1, T1, it1, errs = capi.icp_align_traced(w["scan1"], w["scan0"], w["icp_T0"], I4, 0.10, np.deg2rad(60.0), max_iter=10, fixed_iters=True)
    assert it1 == it0 == 10 and e1 == e0 and (T1 == T0).all() and len(errs) == 10 and errs[-1] == e1
    # (whole scans: the fp64-moment estimator evaluates the residual algebraically where the reference sums fp32 terms — 4e-5 apart in the
    #  first two iterations, where the error is 5e-3 ... 2e-2 and no stop test looks at it, 1e-6 once it has settled.  Round 6: a
    #  fixed-length call runs the PLAIN step — its own fp64 centroids — until two iterations before its end (rs_hip_icp_early_plain):
    #  those iterations' errors are the plain step's, 1.3e-3 ... 2e-6 from the reference's (of errors of 2e-2 ... 1e-3); the last two are the
    #  chains', and the plain one before them has settled as far)
    d = np.abs(errs.astype(np.float64) - g["icp_errs"].astype(np.float64))
    assert d.max() < 5e-3 and d[-3:].max() < 1e-5, d
    prev_p = capi.icp_early_plain(0)
    try:
        e2, T2, it2, errs2 = capi.icp_align_traced(w["scan1"], w["scan0"], w["icp_T0"], I4, 0.10, np.deg2rad(60.0), max_iter=10, fixed_iters=True)
        d2 = np.abs(errs2.astype(np.float64) - g["icp_errs"].astype(np.float64))
        assert d2.max() < 1e-4 and d2[5:].max() < 1e-5, d2      # the chains in every iteration: the round-5 bounds
    finally:
        capi.icp_early_plain(prev_p)
    p = w["plc"][0]
    a = capi.icp_align(p["cloud"], w["scan1"], p["pose"], I4, 0.075, np.deg2rad(50.0))
    b = capi.icp_align_traced(p["cloud"], w["scan1"], p["pose"], I4, 0.075, np.deg2rad(50.0))
    assert a[0] == b[0] and (a[1] == b[1]).all() and a[2] == b[2] == len(b[3]) and b[3][-1] == b[0]
    assert (np.diff(b[3]) < 1e-3).all()      # (the error settles)


def _check_room(capi, bench_mod, g, w, with_stop):
    s0, s1 = w["s0"], w["s1"]
    op, on = w["obj_score_np"]
    got = [sha(s0["points"]), sha(s0["normals"]), sha(s1["points"]), sha(s1["normals"]), sha(op), sha(on),
           sha(w["score_poses"]), sha(w["plc_poses"]), sha(w["icp_T0"])]
    assert got == [str(x) for x in g["in_sha"]], "the generator no longer produces the inputs the fixture was made for"
    gave_up = capi.icp_chains_gave_up()
    err, T, it = capi.icp_align(w["scan1"], w["scan0"], w["icp_T0"], I4, 0.10, np.deg2rad(60.0), max_iter=bench_mod.ICP_ITERS, fixed_iters=True)
    d_fixed = np.linalg.norm(T.astype(np.float64) - g["icp_pose"].astype(np.float64))
    msg = f"10 fixed iterations {d_fixed:.3e} from the reference (err {err:.7f} vs {float(g['icp_err']):.7f})"
    assert it == bench_mod.ICP_ITERS and d_fixed < POSE_TOL and abs(err - float(g["icp_err"])) < 1e-5, msg
    if with_stop:
        md, ma = float(g["stop_params"][0]), float(g["stop_params"][1])
        e2, T2, it2 = capi.icp_align(w["scan1"], w["scan0"], g["stop_T0"], I4, md, ma)
        d_stop = np.linalg.norm(T2.astype(np.float64) - g["stop_pose"].astype(np.float64))
        msg += f"; icp_align r {md:.3f}: {d_stop:.3e}, {it2} vs {int(g['stop_iters'])} iterations"
        assert d_stop < POSE_TOL, msg
        assert it2 == int(g["stop_iters"]), msg
    sc = capi.alignment_scores(w["obj_score"], w["scan1"], w["score_poses"], 0.1, 64)
    d_sc = np.abs(sc.astype(np.float64) - g["scores"].astype(np.float64)).max()
    res = capi.arrangement_to_labels(w["scan1"], w["plc_poses"], [p["cloud"] for p in w["plc"]], [0] * len(w["plc"]),
                                     [p["cls"] for p in w["plc"]], 0.05, False)
    print(msg + f"; scores max abs {d_sc:.2e}, {int((sc == g['scores']).sum())} of {len(sc)} bit-identical; calls the centroid chains gave up: {capi.icp_chains_gave_up() - gave_up}")
    assert d_sc < SCORE_TOL
    assert (res["order"] == g["order"]).all()
    assert "reference" in str(g["labels_source"])
    assert sha(res["labels"]) == str(g["labels_sha"]) and sha(res["min_dists"]) == str(g["min_dists_sha"])


@pytest.mark.parametrize("seed", [11, 31, 32])
def test_centred_rooms_vs_reference(capi, bench_mod, seed):
    """Round 5: rooms moved so that the scan's median point is the ORIGIN — coordinates of both signs, as real scans have; the
    reference's fp32 centroid sums then hover around zero (the regime in which the grid chains fall back on the replay) —
    against the reference build's own results for exactly these inputs (oracle/gen_golden_bench.py --centre): the step's ten fixed
    iterations, icp_align with its stop test, the 256 scores, labels / min_dists."""
    g = load_golden("bench_seed%d_centre.npz" % seed)
    w = bench_mod.build_workload(int(g["n_points"]), seed=int(g["seed"]), knn="hash", centre=True)
    try:
        _check_room(capi, bench_mod, g, w, with_stop=True)
    finally:
        _close_workload(w)


@pytest.mark.parametrize("t0", [1, 2])
def test_further_scan_pairs_vs_reference(capi, bench_mod, t0):
    """bench.py --timesteps 4 (BASELINE configs[3]): the pairs (1, 2) and (2, 3) of the sequence against the reference build's results
    (oracle/gen_golden_bench.py --pair)."""
    g = load_golden("bench_seed11_t%d.npz" % t0)
    w = bench_mod.build_workload(int(g["n_points"]), seed=int(g["seed"]), knn="hash", t0=t0)
    try:
        _check_room(capi, bench_mod, g, w, with_stop=False)
    finally:
        _close_workload(w)


def test_label_rows_in_all_three_forms(capi, headline):
    """rs_hip_label_rows: host rows (input order), device rows in input order, device rows in the scene's query order — the
    last folded by rs_hip_fold_label_rows_device with the scene cloud — all give the rows / labels of the placement loop."""
    import torch
    from rescan_amd import dist as rd
    w, g = headline
    n_plc, ns = len(w["plc"]), w["n_scan1"]
    order, _, radii = rd.arrangement_plan([0] * n_plc, [p["cls"] for p in w["plc"]], 0.05)
    poses, clouds = w["plc_poses"][order], [w["plc"][i]["cloud"] for i in order]
    host = capi.label_rows(w["scan1"], poses, clouds, radii)
    dev = torch.zeros(n_plc * ns, dtype=torch.float32, device="cuda:0")
    capi.label_rows(w["scan1"], poses, clouds, radii, out_device_ptr=dev.data_ptr()); capi.synchronize()
    assert np.array_equal(dev.cpu().numpy().reshape(n_plc, ns), host)
    labels = np.zeros(ns, np.int8); mind = np.full(ns, 1e9, np.float32)
    capi.combine_label_rows(host, labels, mind)
    assert (labels == g["labels"]).all() and sha(mind) == str(g["min_dists_sha"])
    capi.label_rows(w["scan1"], poses, clouds, radii, out_device_ptr=dev.data_ptr(), query_order=True); capi.synchronize()
    offs = [k * ns for k in range(n_plc)]
    l2, m2 = capi.fold_label_rows_device(dev.data_ptr(), offs, ns, query_order_of=w["scan1"])
    assert (l2 == labels).all() and (m2 == mind).all()
    # continued from a caller's state: the first three rows, then the rest
    l3, m3 = capi.fold_label_rows_device(dev.data_ptr(), offs[:3], ns, query_order_of=w["scan1"])
    l3, m3 = capi.fold_label_rows_device(dev.data_ptr(), offs[3:], ns, l3, m3, label_base=3, query_order_of=w["scan1"])
    assert (l3 == labels).all() and (m3 == mind).all()


# ---- scan-sized sources: which estimator ---------------------------------------------------------------------------

def _sweep_case(seed):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from gen_golden_bench import sweep_inputs
    return sweep_inputs(seed)


def test_scan_sized_icp_sweep_vs_reference(capi):
    """24 scan-to-scan icp_align runs on ~134 k-point scans (the reference's three parameter sets in turn) against the
    reference's own results.  Reference-order estimator (RS_HIP_REF_ORDER_BELOW lifted): pose, error and iteration count
    bit for bit.  The default at this size (round 6: grid chains — reference cut + reference centroid chains + fp64 moments): within
    1e-5 of the reference, same iteration count, every run.  Plain fp64 moments (nobody's default): the distances are REPORTED and
    counted — the moments are exact where the reference's fp32 chains carry their own rounding, so a run may end
    farther than 1e-4 from the reference without either being wrong."""
    g = load_golden("sweep_icp.npz")
    prev = capi.icp_reference_order_below(-1); prev_replay = capi.icp_replay_below(-1)
    over, worst, iter_diff, exact, replay_exact, redone, worst_default = [], 0.0, 0, 0, 0, [], 0.0
    try:
        for k, seed in enumerate(g["seeds"]):
            s0, s1, T0, md, ma = _sweep_case(int(seed))
            assert sha(s1["points"]) + sha(s0["points"]) == str(g["in_sha"][k])
            assert np.array_equal(T0, g["T0"][k])
            a, b = capi.Cloud(s0["points"], s0["normals"]), capi.Cloud(s1["points"], s1["normals"])
            capi.icp_reference_order_below(prev); capi.icp_replay_below(prev_replay)      # the DEFAULT at this size (round 6: grid chains)
            ed, Td, itd = capi.icp_align(b, a, T0, I4, float(md), float(ma))
            dd = float(np.linalg.norm(Td.astype(np.float64) - g["pose"][k].astype(np.float64)))
            worst_default = max(worst_default, dd)
            assert dd < 1e-5 and itd == int(g["iters"][k]), f"seed {seed}: the default estimator {dd:.2e} from the reference, {itd} vs {int(g['iters'][k])} iterations"
            capi.icp_reference_order_below(0); capi.icp_replay_below(0); prev_ec = capi.icp_exact_centroids(0)         # plain fp64 moments
            e64, T64, it64 = capi.icp_align(b, a, T0, I4, float(md), float(ma))
            capi.icp_exact_centroids(prev_ec)
            capi.icp_replay_below(1 << 30)                          # the reference's sums, computed in parallel
            ep, Tp, itp = capi.icp_align(b, a, T0, I4, float(md), float(ma))
            replay_exact += int((Tp == g["pose"][k]).all() and itp == int(g["iters"][k]) and np.float32(ep) == g["err"][k])
            redone.append(capi.icp_replay_redone())
            capi.icp_reference_order_below(1 << 30)                 # reference order
            er, Tr, itr = capi.icp_align(b, a, T0, I4, float(md), float(ma))
            d64 = float(np.linalg.norm(T64.astype(np.float64) - g["pose"][k].astype(np.float64)))
            dr = float(np.linalg.norm(Tr.astype(np.float64) - g["pose"][k].astype(np.float64)))
            print(f"sweep seed {int(seed):2d}: r {float(md):.3f}  fp64 moments {d64:.2e} ({it64} vs {int(g['iters'][k])} it)   reference order {dr:.2e} ({itr} it)")
            worst = max(worst, d64)
            if d64 >= POSE_TOL:
                over.append((int(seed), d64))
            iter_diff += int(it64 != int(g["iters"][k]))
            exact += int(dr == 0.0 and itr == int(g["iters"][k]) and np.float32(er) == g["err"][k])
            assert dr < POSE_TOL and itr == int(g["iters"][k]), f"seed {seed}: reference-order estimator {dr:.2e}, {itr} iterations"
            a.close(); b.close()
    finally:
        capi.icp_reference_order_below(prev); capi.icp_replay_below(prev_replay)
    print(f"parallel reference order (replay): {replay_exact} of {len(g['seeds'])} bit-identical to the reference; segments re-added in the last iteration: {redone}")
    assert replay_exact == exact
    print(f"fp64 moments: {len(over)} of {len(g['seeds'])} runs end >= 1e-4 from the reference (worst {worst:.2e}); {iter_diff} stop an iteration apart")
    print(f"reference order: {exact} of {len(g['seeds'])} bit-identical (pose, error, iterations)")
    assert exact >= len(g["seeds"]) - 1              # (an exact fp32 distance tie may cost one run a few 1e-5)
    print(f"default estimator (grid chains at this size): worst {worst_default:.2e} from the reference, every iteration count the reference's")
    # The DEFAULT estimator for sources of this size is held to 1e-5 and to the reference's iteration count in every run above
    # (round 6; up to round 5 it was the replay — the reference's bits at 0.7 ms per iteration instead of 0.12 — which stays an opt-in,
    # bit for bit: replay_exact == exact).  The plain fp64 moments (RS_HIP_EXACT_CENTROIDS=0) are nobody's default; their distances
    # are data for DESIGN.md §4's policy.
