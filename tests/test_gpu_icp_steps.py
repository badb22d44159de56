"""GPU: every traced ICP iteration against an fp64 restatement of the step the device says it ran (tests/icp_restate.py).

rs_hip_icp_trace_begin records, per problem and iteration, the pose after the step, its error and the estimator kind.  For
iteration i the restatement starts from the DEVICE's pose T_i (the start pose, or row i-1), takes the oracle's correspondences
(pinned bit for bit to the device's searches) at that iteration's max_dist, and must land on row i:

* reference order / replay: the oracle's own icp_estimate_pt2pl — bit for bit;
* lane chains, grid chains, the chains' sums from records, plain, k_icp_moments: the reference's fp32 centroid chains (or fp64
  centroids) and the centred fp64 normal equations.  The device forms the same system from UNcentred fp64 moments: the
  centring subtracts terms ~|c1|²/spread² larger than the result (coordinates of a few metres, spreads of a metre: 10-100),
  and its reductions add 10^4-10^6 fp64 terms in another order — together ~1e-13 relative in the 6x6 system and in x.  The
  fp32 pose composed from x then agrees exactly unless a component of x (or a centroid) sits within that distance of a
  float rounding boundary, where it moves by one ulp: ~1e-7 in an entry of the composed pose.  Bound: every pose entry within
  max(1e-6, 4 ulp of the entry) and the error within 4 ulp — 20x tighter than POLICY_TOL (2e-5), and far below what a
  skipped block of 1 024 points or a step centred on the wrong weights moves (1e-5 ... 1e-3 per iteration).
* the device's 2.5 sigma cut comes from integer-quantised dist² sums; where the modelled cut cannot decide a correspondence
  (`ambiguous`, reported) that iteration is held to POLICY_TOL / 10 instead.
* the same where the device's search (rs_hip_icp_find_corrs from the same pose) and the oracle's disagree — which must be
  nothing but EXACT dist² ties between two target points, taken in another order than the reference's sort (found by these
  tests: a 70 k-point source, one correspondence of 65 735; reported as `search ties`).

The kinds must follow the policy of DESIGN.md §4 / include/rescan_hip.h, encoded once in `policy_kind`; tracing must not
change a single bit of any call's results; problems the stop test's guard runs again must end with the oracle's icp_align
bits.  Each test prints, per kind, the iterations checked and the largest deviation."""
import os
import subprocess
import sys

import numpy as np
import pytest

import icp_restate as R
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

I4 = np.eye(4, dtype=np.float32).ravel()
MA = np.float32(np.deg2rad(60.0))
POLICY_TOL = 2e-5

# ---- the estimator policy (include/rescan_hip.h; rs_icp_api.hip) at the default thresholds -------------------
REF_ORDER_BELOW = 16384          # rs_hip_icp_reference_order_below
LANE_BELOW = 65536               # rs_hip_icp_lane_chains_below (batches)
LANE_SINGLE_CAP = 28672          # ... a call with one problem: the grid chains from here on
PLAIN_ABOVE = 65536              # early plain iterations only for scan-sized sources
STOP_PLAIN_ABOVE = 262144        # ... and with the stop test only above this (below: the guard wants the reference's errors)


def policy_kind(n, n_call, fixed_iters, max_iter, i, redone=False):
    """The estimator iteration i of a problem with n source points runs, in a call (or slice, or multi-source group) of
    n_call problems.  GRID_CHAINS also stands for RECORDS (the same sums after the chains gave up)."""
    if redone:
        return R.STEP_REF_ORDER if n <= 65536 else R.STEP_REPLAY
    if n <= REF_ORDER_BELOW:
        return R.STEP_REF_ORDER
    if n <= (LANE_BELOW if n_call > 1 else LANE_SINGLE_CAP):
        return R.STEP_LANE_CHAINS
    n_plain = 0
    if n > PLAIN_ABOVE:
        if fixed_iters:
            n_plain = max(0, max_iter - 2)
        elif n > STOP_PLAIN_ABOVE:
            n_plain = min(max(0, 7 - 3), max(0, max_iter - 3))
    return R.STEP_PLAIN if i < n_plain else R.STEP_GRID_CHAINS


def test_policy_table_matches_the_sources():
    """The thresholds above are the ones the library reports, and the prose of DESIGN.md §4 / the header still says them."""
    from rescan_amd import capi
    capi.init(0)
    assert capi.icp_reference_order_below(-1) == REF_ORDER_BELOW
    assert capi.icp_lane_chains_below(-1) == LANE_BELOW
    assert capi.icp_replay_below(-1) == 0 and capi.icp_exact_centroids(-1) == 1 and capi.icp_early_plain(-1) == 1
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    hdr = open(os.path.join(ROOT, "include", "rescan_hip.h")).read()
    for s in ("≤ 16 384 points reference order", "≤ 65 536 the lane chains", "28 672", "TWO before its end", "above 262 144 points"):
        assert s in design, s
    assert "from 28672 points on" in hdr and "sources up to 262144 points" in hdr and "Default 16384" in hdr


# ---- checking one traced problem ------------------------------------------------------------------------------------

def ulp(x):
    return np.spacing(np.abs(np.float32(x))).astype(np.float64)


class Stats:
    def __init__(self):
        self.k = {}

    def add(self, kind, dpose, derr_ulp, ambiguous, ties):
        c = self.k.setdefault(kind, [0, 0.0, 0.0, 0, 0])
        c[0] += 1; c[1] = max(c[1], dpose); c[2] = max(c[2], derr_ulp); c[3] += ambiguous; c[4] += ties

    def report(self, what):
        from rescan_amd import capi
        for kind, (n, dp, de, amb, ties) in sorted(self.k.items()):
            print(f"[{what}] {capi.ICP_STEP_NAMES[kind]:>11}: {n:4d} iterations, max pose deviation {dp:.2e}, max err deviation "
                  f"{de:.1f} ulp, ambiguous cut corrs {amb}, search ties {ties}")


def search_ties(dev, c, T, md):
    """Correspondences where the device's search (rs_hip_icp_find_corrs) took another target point than the oracle's; each
    must be an exact dist² tie (same query, same float dist², same count).  Returns how many."""
    from rescan_amd import capi
    d = capi.icp_find_corrs(dev[0], dev[1], T, I4, md, MA)
    assert len(d[0]) == len(c) and (d[0] == c.p1).all() and (d[1] == c.n1).all(), "the searches found other correspondences"
    bad = np.nonzero((d[2] != c.p2).any(axis=1) | (d[3] != c.n2).any(axis=1) | (d[4] != c.w_ref))[0]
    for i in bad:
        v = (d[2][i] - c.p1[i]).astype(np.float32)
        d2 = np.float32(np.float32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        assert d2 == c.d2[i], f"correspondence {i}: the device's target point is not a dist² tie ({d2!r} vs {c.d2[i]!r})"
    return len(bad)


def check_problem(O, grid, src, tgt, T0, md0, rows_T, rows_e, rows_k, iters, T_out, e_out, stats, expect=None, label="", dev=None):
    """Holds every recorded iteration of one problem to the restatement.  expect(i) -> the policy's kind (or None); dev: the
    (source, target) clouds, for the search-tie check."""
    ran = np.nonzero(rows_k != -1)[0]
    assert len(ran) == iters and (ran == np.arange(iters)).all(), (label, rows_k, iters)
    assert rows_T[iters - 1].tobytes() == np.asarray(T_out, np.float32).tobytes() and rows_e[iters - 1] == e_out, label
    md = np.float32(md0)
    T_prev, e_prev = np.asarray(T0, np.float32).ravel(), np.float32(1e6)
    for i in range(iters):
        kind = int(rows_k[i])
        if expect is not None:
            want = expect(i)
            ok = kind == want or (want == R.STEP_GRID_CHAINS and kind == R.STEP_RECORDS)
            assert ok, f"{label}: iteration {i} ran estimator {kind}, the policy says {want}"
        c = R.Corrs(O, grid, src[0], src[1], tgt[0], tgt[1], T_prev, I4, md, MA)
        T_r, e_r, info = R.restate_step(O, kind, c, T_prev)
        e_r = e_prev if e_r is None else e_r
        ties = search_ties(dev, c, T_prev, md) if dev is not None and len(c) else 0
        T_d, e_d = rows_T[i], rows_e[i]
        dpose = float(np.abs(T_d.astype(np.float64) - T_r).max())
        derr = abs(float(e_d) - float(e_r)) / float(ulp(max(e_d, e_r)))
        stats.add(kind, dpose, derr, info["ambiguous"], ties)
        where = f"{label}: iteration {i} ({kind}), {len(c)} corrs, pose {dpose:.3e}, err {e_d!r} vs {e_r!r}, search ties {ties}"
        if ties:
            assert dpose < POLICY_TOL / 10, where
        elif kind in R.REF_KINDS:
            assert T_d.tobytes() == T_r.tobytes() and e_d == e_r, where
        elif info["ambiguous"]:
            assert dpose < POLICY_TOL / 10, where
        else:
            tol = np.maximum(1e-6, 4 * np.maximum(ulp(T_d), ulp(T_r)))
            assert (np.abs(T_d.astype(np.float64) - T_r) <= tol).all() and derr <= 4, where
        T_prev, e_prev, md = T_d, e_d, R.next_max_dist(md)


def traced(fn, max_iter, n_prob):
    """fn() untraced, then traced: the same bits; returns (result, trace)."""
    from rescan_amd import capi
    a = fn()
    with capi.IcpTrace(max_iter, n_prob) as tr:
        b = fn()
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), "tracing changed a result"
    return b, tr


@pytest.fixture(scope="module")
def capi():
    from rescan_amd import capi
    capi.init(0)
    return capi


@pytest.fixture(scope="module")
def room():
    """A scan pair of ~300 k points (the policy's edges are exact-size subsets of its second scan)."""
    from rescan_amd import synth
    s0 = synth.scene_for_point_count(300_000, seed=41, timestep=0)
    s1 = synth.scene_for_point_count(300_000, seed=41, timestep=1)
    return s0, s1


def subset(s, n, seed=0):
    idx = np.sort(np.random.default_rng(seed + n).choice(len(s["points"]), n, replace=False))
    return np.ascontiguousarray(s["points"][idx]), np.ascontiguousarray(s["normals"][idx])


EDGES = [4096, 16384, 16385, 28672, 28673, 65536, 65537, 262144, 262145]


def test_single_calls_at_the_policy_edges(capi, oracle, room):
    """One problem per call at every threshold of the policy (exact sizes, most not multiples of 64 / 128 / 1 024): 8 fixed
    iterations and the stop test, every iteration against the restatement."""
    from rescan_amd import synth
    s0, s1 = room
    assert len(s1["points"]) > EDGES[-1]
    tgt = (s0["points"], s0["normals"])
    tc = capi.Cloud(*tgt)
    grid = O_grid = oracle.grid_create(tgt[0], 0.1)
    stats = Stats()
    prev_g = capi.icp_stop_guard(0.0)       # (the guard's reruns have their own test; here: the policy's estimators throughout)
    try:
        for n in EDGES:
            src = subset(s1, n)
            sc = capi.Cloud(*src)
            T0 = synth.perturbed_pose(I4, np.random.default_rng(n), 0.02, 0.01)
            for fixed, mi in ((True, 8), (False, 40)):
                (e, T, it), tr = traced(lambda: capi.icp_align(sc, tc, T0, I4, 0.1, MA, max_iter=mi, fixed_iters=fixed), mi, 1)
                check_problem(oracle, grid, src, tgt, T0, 0.1, tr.poses[0], tr.errs[0], tr.kinds[0], it, T, e, stats,
                              expect=lambda i: policy_kind(n, 1, fixed, mi, i), label=f"n {n} fixed {fixed}", dev=(sc, tc))
                assert tr.redone[0] == 0
            sc.close()
    finally:
        capi.icp_stop_guard(prev_g)
        oracle.grid_destroy(O_grid); tc.close()
    stats.report("edges")


def test_headline_room_traced_once(capi, oracle):
    """The benchmark's own call (bench_seed11: 10 fixed iterations, 8 plain + 2 grid chains) — traced once at 1 M points."""
    sys.path.insert(0, ROOT)
    import bench
    g = load_golden("bench_seed11.npz")
    w = bench.build_inputs(int(g["n_points"]), int(g["seed"]), 1, False, 0)
    s0, s1 = w["s0"], w["s1"]
    tgt, src = (s0["points"], s0["normals"]), (s1["points"], s1["normals"])
    a, b = capi.Cloud(*tgt), capi.Cloud(*src)
    grid = oracle.grid_create(tgt[0], 0.1)
    stats = Stats()
    try:
        (e, T, it), tr = traced(lambda: capi.icp_align(b, a, w["icp_T0"], I4, 0.10, MA, max_iter=bench.ICP_ITERS, fixed_iters=True),
                                bench.ICP_ITERS, 1)
        n = len(src[0])
        check_problem(oracle, grid, src, tgt, w["icp_T0"], 0.1, tr.poses[0], tr.errs[0], tr.kinds[0], it, T, e, stats,
                      expect=lambda i: policy_kind(n, 1, True, bench.ICP_ITERS, i), label="headline", dev=(b, a))
        assert (tr.kinds[0] == R.STEP_PLAIN).sum() == 8
    finally:
        oracle.grid_destroy(grid); a.close(); b.close()
    stats.report("headline")


def test_centred_room_from_records(capi, oracle):
    """A room centred on its median (sums that hover around zero): the chains' sums by pass 2 of the replay from the
    searches' records — the path the grid chains fall back on — forced (rs_hip_icp_exact_centroids( 2 )), after plain steps."""
    from rescan_amd import synth
    s0 = synth.scene_for_point_count(330_000, seed=22, timestep=0)
    s1 = synth.scene_for_point_count(330_000, seed=22, timestep=1)
    sh = -np.median(s1["points"], axis=0).astype(np.float32)
    tgt, src = (s0["points"] + sh, s0["normals"]), (s1["points"] + sh, s1["normals"])
    a, b = capi.Cloud(*tgt), capi.Cloud(*src)
    grid = oracle.grid_create(tgt[0], 0.1)
    stats = Stats()
    prev = capi.icp_exact_centroids(2)
    try:
        T0 = synth.perturbed_pose(I4, np.random.default_rng(5), 0.02, 0.01)
        (e, T, it), tr = traced(lambda: capi.icp_align(b, a, T0, I4, 0.1, MA, max_iter=6, fixed_iters=True), 6, 1)
        check_problem(oracle, grid, src, tgt, T0, 0.1, tr.poses[0], tr.errs[0], tr.kinds[0], it, T, e, stats, label="centred", dev=(b, a))
        assert list(tr.kinds[0]) == [R.STEP_PLAIN] * 4 + [R.STEP_RECORDS] * 2
    finally:
        capi.icp_exact_centroids(prev)
        oracle.grid_destroy(grid); a.close(); b.close()
    stats.report("records")


def _start_poses(k, seed, far=None):
    from rescan_amd import synth
    rng = np.random.default_rng(seed)
    T = np.stack([synth.perturbed_pose(I4, rng, 0.02, 0.01) for _ in range(k)])
    if far is not None:
        T[far][12] = 100.0                      # no correspondences: inactive after its first iteration (icp.h:455-459)
    return T


@pytest.mark.parametrize("n_src", [20_000, 70_000], ids=["lane", "grid"])
def test_batches(capi, oracle, room, n_src):
    """icp_align_batch with 1, 8 and 9 problems (8 fixed iterations; in the larger batches one problem without
    correspondences goes inactive at once), every problem's every iteration against the restatement."""
    s0, s1 = room
    tgt, src = (s0["points"], s0["normals"]), subset(s1, n_src, 3)
    a, b = capi.Cloud(*tgt), capi.Cloud(*src)
    grid = oracle.grid_create(tgt[0], 0.1)
    stats = Stats()
    try:
        for k in (1, 8, 9):
            T0 = _start_poses(k, k, far=k - 1 if k > 1 else None)
            (e, T, it), tr = traced(lambda: capi.icp_align_batch(b, a, T0, I4, 0.1, MA, max_iter=8, fixed_iters=True), 8, k)
            for p in range(k):
                check_problem(oracle, grid, src, tgt, T0[p], 0.1, tr.poses[p], tr.errs[p], tr.kinds[p], it[p], T[p], e[p], stats,
                              expect=lambda i: policy_kind(n_src, k, True, 8, i), label=f"batch {k} problem {p}", dev=(b, a))
            if k > 1:
                assert it[k - 1] == 1 and e[k - 1] == np.float32(1e6) and (T[k - 1] == T0[k - 1]).all()
    finally:
        oracle.grid_destroy(grid); a.close(); b.close()
    stats.report(f"batch {n_src}")


def test_multi_ragged_sources(capi, oracle, room):
    """icp_align_multi over sources of 9, 700, ~3 k, ~30 k and ~70 k points (three estimator groups) and a ~3 k one without
    correspondences, 8 fixed iterations."""
    s0, s1 = room
    tgt = (s0["points"], s0["normals"])
    sizes = [9, 700, 3001, 30_011, 70_003, 2999]
    srcs = [subset(s1, n, 7) for n in sizes]
    a = capi.Cloud(*tgt)
    cl = [capi.Cloud(*s) for s in srcs]
    grid = oracle.grid_create(tgt[0], 0.1)
    stats = Stats()
    try:
        T0 = _start_poses(len(sizes), 11, far=len(sizes) - 1)
        (e, T, it), tr = traced(lambda: capi.icp_align_multi(cl, a, T0, I4, 0.1, MA, max_iter=8, fixed_iters=True), 8, len(sizes))
        for p, n in enumerate(sizes):
            # (one problem per estimator class beyond the reference order: each runs as a single call)
            check_problem(oracle, grid, srcs[p], tgt, T0[p], 0.1, tr.poses[p], tr.errs[p], tr.kinds[p], it[p], T[p], e[p], stats,
                          expect=lambda i: policy_kind(n, 1, True, 8, i), label=f"multi problem {p} ({n} points)", dev=(cl[p], a))
    finally:
        oracle.grid_destroy(grid); a.close()
        for c in cl:
            c.close()
    stats.report("multi")


def lattice(n, seed):
    """n points 0.25 apart (more than the 0.1 search radius: each point's only neighbour is itself), random unit normals."""
    k = int(np.ceil(n ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n] * 0.25 + 0.5
    nr = np.random.default_rng(seed).normal(0, 1, (n, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    return np.ascontiguousarray(g, np.float32), np.ascontiguousarray(nr, np.float32)


def test_degenerate_systems(capi, oracle):
    """A source that is its own target, at the identity, its points further apart than the radius: every correspondence is
    the point itself — dist² all 0, sd 0 (no cut), a zero right-hand side.  Every estimator the threshold setters can force
    on it must leave the pose exactly unchanged with error 0, and all seven kinds must have been met."""
    small, mid, big = lattice(4096, 1), lattice(30_000, 2), lattice(70_000, 3)
    saved = (capi.icp_replay_below(-1), capi.icp_exact_centroids(-1), capi.icp_lane_chains_below(-1))
    seen = set()
    try:
        for pts, setup in ((small, None), (mid, "lane"), (mid, None), (mid, "replay"), (mid, "moments"), (big, None), (big, "records")):
            if setup == "lane":
                capi.icp_lane_chains_below(1 << 20)
            elif setup == "replay":
                capi.icp_replay_below(1 << 20)
            elif setup == "moments":
                capi.icp_exact_centroids(0)
            elif setup == "records":
                capi.icp_exact_centroids(2)
            c = capi.Cloud(*pts)
            (e, T, it), tr = traced(lambda: capi.icp_align(c, c, I4, I4, 0.1, MA, max_iter=3, fixed_iters=True), 3, 1)
            c.close()
            capi.icp_replay_below(saved[0]); capi.icp_exact_centroids(saved[1]); capi.icp_lane_chains_below(saved[2])
            assert it == 3 and (tr.kinds[0] >= 0).all()
            seen |= set(tr.kinds[0].tolist())
            assert (tr.poses[0] == I4).all() and (tr.errs[0] == 0).all() and (T == I4).all() and e == 0, (setup, tr.kinds[0], tr.errs[0])
    finally:
        capi.icp_replay_below(saved[0]); capi.icp_exact_centroids(saved[1]); capi.icp_lane_chains_below(saved[2])
    assert seen == set(range(7)), seen


def _check_redone(oracle, src, tgt, T0, e, T, it, label):
    e_o, T_o, it_o = oracle.icp_align(src[0], src[1], tgt[0], tgt[1], T0, I4, 0.1, MA)
    assert T.tobytes() == T_o.tobytes() and e == np.float32(e_o) and it == it_o, (label, it, it_o, e, e_o)


def test_stop_guard_inside_a_multi_lane_group(capi, oracle, room):
    """The guard's reruns in an icp_align_multi lane-chain group (stop test on, the guard widened so that they certainly
    happen): every redone problem ends with the oracle's icp_align bits, its rows are the rerun's (reference order), the
    others keep their estimator and their untraced bits."""
    s0, s1 = room
    tgt = (s0["points"], s0["normals"])
    sizes = [17_001, 20_000, 24_577, 30_000, 20_001]
    srcs = [subset(s1, n, 13) for n in sizes]
    a = capi.Cloud(*tgt)
    cl = [capi.Cloud(*s) for s in srcs]
    grid = oracle.grid_create(tgt[0], 0.1)
    stats = Stats()
    prev_g = capi.icp_stop_guard(1e-5)
    try:
        T0 = _start_poses(len(sizes), 17, far=len(sizes) - 1)
        r0 = capi.icp_stop_guard_redone()
        (e, T, it), tr = traced(lambda: capi.icp_align_multi(cl, a, T0, I4, 0.1, MA, max_iter=40), 40, len(sizes))
        assert tr.redone.sum() > 0 and capi.icp_stop_guard_redone() - r0 >= 2 * tr.redone.sum()
        assert tr.redone[-1] == 0
        for p, n in enumerate(sizes):
            red = bool(tr.redone[p])
            check_problem(oracle, grid, srcs[p], tgt, T0[p], 0.1, tr.poses[p], tr.errs[p], tr.kinds[p], it[p], T[p], e[p], stats,
                          expect=lambda i: policy_kind(n, len(sizes), False, 40, i, red), label=f"multi guard problem {p}", dev=(cl[p], a))
            if red:
                _check_redone(oracle, srcs[p], tgt, T0[p], e[p], T[p], it[p], f"problem {p}")
        print(f"redone: {tr.redone.tolist()}")
    finally:
        capi.icp_stop_guard(prev_g)
        oracle.grid_destroy(grid); a.close()
        for c in cl:
            c.close()
    stats.report("multi guard")


_CHILD = r"""
import sys, json, numpy as np
sys.path.insert(0, sys.argv[1])
from rescan_amd import capi
capi.init(0)
d = np.load(sys.argv[2])
a, b = capi.Cloud(d["tp"], d["tn"]), capi.Cloud(d["sp"], d["sn"])
capi.icp_stop_guard(float(d["guard"]))
fixed, mi = bool(d["fixed"]), int(d["max_iter"])
e0, T0, i0 = capi.icp_align_batch(b, a, d["T0"], max_dist=0.1, max_angle=float(d["ma"]), max_iter=mi, fixed_iters=fixed)
with capi.IcpTrace(mi, len(d["T0"])) as tr:
    e, T, it = capi.icp_align_batch(b, a, d["T0"], max_dist=0.1, max_angle=float(d["ma"]), max_iter=mi, fixed_iters=fixed)
np.savez(sys.argv[3], e0=e0, T0=T0, i0=i0, e=e, T=T, it=it, poses=tr.poses, errs=tr.errs, kinds=tr.kinds, redone=tr.redone)
print("ok")
"""


@pytest.mark.parametrize("n_src,fixed", [(70_000, True), (100_003, False)], ids=["fixed", "stop-guard"])
def test_sliced_batch_in_a_child(capi, oracle, room, tmp_path, n_src, fixed):
    """A batch of a scan-sized source cut into slices (a small RS_HIP_ICP_BATCH_BYTES, read once per process: a child):
    every iteration against the restatement; with the stop test and a widened guard, the reruns in the reference's order
    (its replay above 65 536 points) end with the oracle's icp_align bits and the untraced call's."""
    s0, s1 = room
    tgt, src = (s0["points"], s0["normals"]), subset(s1, n_src, 5)
    k = 5
    T0 = _start_poses(k, 23, far=2)
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    mi = 8 if fixed else 40
    np.savez(inp, tp=tgt[0], tn=tgt[1], sp=src[0], sn=src[1], T0=T0, guard=np.float32(0.0 if fixed else 1e-5),
             fixed=fixed, max_iter=mi, ma=MA)
    env = dict(os.environ, RS_HIP_ICP_BATCH_BYTES=str(96 * n_src * 2))       # slices of two problems
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, inp, out], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
    d = dict(np.load(out))
    for x, y in (("e0", "e"), ("T0", "T"), ("i0", "it")):
        assert d[x].tobytes() == d[y].tobytes(), "tracing changed a result"
    grid = oracle.grid_create(tgt[0], 0.1)
    a, b = capi.Cloud(*tgt), capi.Cloud(*src)
    stats = Stats()
    try:
        for p in range(k):
            red = bool(d["redone"][p])
            check_problem(oracle, grid, src, tgt, T0[p], 0.1, d["poses"][p], d["errs"][p], d["kinds"][p], d["it"][p], d["T"][p],
                          d["e"][p], stats, expect=lambda i: policy_kind(n_src, 2, fixed, mi, i, red), label=f"slice problem {p}",
                          dev=(b, a))
            if red:
                _check_redone(oracle, src, tgt, T0[p], d["e"][p], d["T"][p], d["it"][p], f"problem {p}")
        if not fixed:
            assert d["redone"].sum() > 0 and d["redone"][2] == 0
        print(f"redone: {d['redone'].tolist()}")
    finally:
        oracle.grid_destroy(grid); a.close(); b.close()
    stats.report(f"sliced {n_src}")
