"""GPU: the end of an ICP iteration on hostile systems (tests/hard_systems.py; the families are held to their claims in
tests/test_hard_systems_cpu.py): a pivot that is exactly zero, pivots of rounding noise and steps of thousands of radians, a second
search that finds nothing, weights whose sum lies on either side of the double 1e-7, negative weights.

* the reference order and the replay through icp_align (stop test on, 100 iterations allowed, traced) and through
  rs_hip_icp_estimate_pt2pl: pose, error, iteration count and every traced row are the oracle's, bit for bit (a non-finite entry by its
  class);
* the fp64 kinds (lane chains, grid chains, RECORDS, k_icp_moments, PLAIN) on the axis families: the bound of test_gpu_icp_steps.py
  (check_problem) per iteration, the oracle's iteration count, axis_x's pose kept bit for bit, both hand-overs of the wide launch;
* the fp64 kinds on tilted_jitter, where no value is defined: the call returns, the kinds are the ones asked for, tracing and the
  hand-over change no bit; the deviation from the oracle is printed;
* the vanish cases and free weights: which side of the break, by the double compare;
* a batch of three problems of one source — the identity, the garbage pose a tilted_jitter step leaves, a start a kilometre away —
  each with its single call's bits.

Every test runs in a child process under its own time limit; the thresholds it sets are restored in `finally` (the `thresholds`
context of test_gpu_hard_sums.py's prelude).  Nothing is skipped: a route that did not run, by the kinds a traced call reports, is a
failure."""
import os
import subprocess
import sys

import pytest

import hard_systems as S
from conftest import ROOT
from test_gpu_hard_sums import PRELUDE as SUMS_PRELUDE

pytestmark = pytest.mark.gpu

PRELUDE = SUMS_PRELUDE + r"""
import hard_systems as S
from test_gpu_icp_steps import check_problem, Stats
np.seterr(all="ignore")
KINDS = {0: dict(icp_reference_order_below=BIG),
         1: dict(icp_reference_order_below=0, icp_lane_chains_below=0, icp_replay_below=BIG),
         2: dict(icp_reference_order_below=0, icp_replay_below=0, icp_lane_chains_below=BIG, icp_exact_centroids=1),
         3: dict(icp_reference_order_below=0, icp_replay_below=0, icp_lane_chains_below=0, icp_exact_centroids=1),
         5: dict(icp_reference_order_below=0, icp_replay_below=0, icp_lane_chains_below=0, icp_exact_centroids=2),
         6: dict(icp_reference_order_below=0, icp_replay_below=0, icp_lane_chains_below=0, icp_exact_centroids=0)}
FP64_SIZES = ((2, S.LANE_SIZES), (3, S.GRID_SIZES), (5, S.GRID_SIZES), (6, (S.MOMENTS_SIZE,)))
WIDE = (3, 5)                                   # the kinds whose iterations end in k_icp_update_wide
def forced(kind):
    return thresholds(icp_chains_retry_after=0, **KINDS[kind])
def align(src, tgt, T0, max_iter=100, fixed=False, ma=MA):
    # the call untraced, then traced: the same bits; ((e, T, it), trace)
    fn = lambda: capi.icp_align(src, tgt, T0, I4, S.RADIUS, ma, max_iter=max_iter, fixed_iters=fixed)
    a = fn()
    with capi.IcpTrace(max_iter, 1) as tr:
        b = fn()
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), "tracing changed a result"
    return b, tr
def both_handovers(fn):
    assert capi.icp_update_fenced(-1) == 0
    out = []
    try:
        for on in (0, 1):
            capi.icp_update_fenced(on)
            out.append(fn())
    finally:
        capi.icp_update_fenced(0)
    ((ea, Ta, ia), tra), ((eb, Tb, ib), trb) = out
    assert Ta.tobytes() == Tb.tobytes() and F(ea).tobytes() == F(eb).tobytes() and ia == ib, "the two hand-overs part: result"
    assert tra.poses.tobytes() == trb.poses.tobytes() and tra.errs.tobytes() == trb.errs.tobytes() and (tra.kinds == trb.kinds).all(), "the two hand-overs part: rows"
    return out[0]
def ran_kinds(tr, it):
    k = tr.kinds[0].tolist()
    assert all(v != capi.ICP_STEP_NONE for v in k[:it]) and all(v == capi.ICP_STEP_NONE for v in k[it:]), (k, it)
    return k[:it]
def rows_differ(tr, it, e, T, poses, errs):
    # the call's result and every traced row against the oracle's rows: indices that differ in bits (or in non-finite class)
    if it != len(errs):
        return ["iterations", it, len(errs)]
    got = np.concatenate([tr.poses[0, :it].ravel(), tr.errs[0, :it], np.asarray(T, F), [F(e)]])
    want = np.concatenate([poses.ravel(), errs, poses[-1], [errs[-1]]])
    return H.bits_or_class_differ(got, want).tolist()
"""

FAULTED = []        # a child that ended by a fault, an abort or its time limit: nothing more of this module is started on the GPU after it


def run_child(body, *args, limit=120):
    assert not FAULTED, f"not started: an earlier child of this module ended abnormally ({FAULTED[0]})"
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT] + [str(a) for a in args],
                         capture_output=True, text=True, env=dict(os.environ))
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139) or "illegal memory access" in out.stderr:
        FAULTED.append(out.returncode)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    print(out.stdout.strip())
    return out.stdout


@pytest.mark.parametrize("name", S.CLOUDS)
def test_reference_order_and_replay_have_the_oracles_rows(name):
    """k_icp_faithful and the replay (icp_solve_ref_order behind both) at 3, 7, 64, 129 and 1 025 points (tilted_jitter: where it
    holds its claim), the whole loop with the stop test: the oracle's iteration count, and its pose and error after EVERY iteration,
    bit for bit — through a zero pivot, through sinf / cosf of thousands of radians (rs_sincosf_model's large-argument reduction),
    through the n_corr == 0 and Σw breaks.  The first iteration's correspondences also go through rs_hip_icp_estimate_pt2pl."""
    run_child(r"""
name = sys.argv[2]
calls = 0
for n in [n for n in S.REF_SIZES if n in S.sizes_of(name)]:
    src, tgt, nor = S.cloud(name, n)
    poses, errs, ncs = S.oracle_rows(O, src, nor, tgt, nor, I4)
    sc, tc = capi.Cloud(src, nor), capi.Cloud(tgt, nor)
    for kind in (0, 1):
        with forced(kind):
            (e, T, it), tr = align(sc, tc, I4)
        assert set(ran_kinds(tr, it)) == {kind}, (name, n, kind, tr.kinds[0][:it])
        bad = rows_differ(tr, it, e, T, poses, errs)
        assert not bad, (name, n, kind, "differs from the oracle at", bad[:12], "iterations", it, len(errs))
        calls += 1
    g = O.grid_create(tgt, S.RADIUS)
    try:
        p1, n1, p2, n2, w = O.icp_find_corrs_uncut(g, src, nor, tgt, nor, I4, I4, S.RADIUS, MA)[:5]
    finally:
        O.grid_destroy(g)
    for T1 in (I4, TURN):
        for route in ("ref_order", "replay"):
            check_bits(route, (p1, p2, n2, w), T1, (name, n))
    print(f"{name} n {n}: {len(errs)} iterations, n_corr {ncs[:3].tolist()}, largest |pose entry| {np.abs(poses).max():.3g}")
    sc.close(); tc.close()
print(f"{name}: {calls} traced calls with the oracle's rows")
print("ok")
""", name)


def test_steps_of_thousands_of_radians_have_libms_bits():
    """big_step — well-conditioned free systems whose step, in the reference's own arithmetic, runs to 1e2 ... 2e5 radians — through
    k_icp_faithful and the replay at 7, 64, 129 and 1 025 correspondences, 48 seeds each, from the identity and a turned pose: the
    oracle's pose and error bit for bit.  The oracle composes with the host's sinf / cosf, the device with rs_sincosf_model: this is
    the large-argument reduction on the device (the double-precision fallback it replaced differed on 1.3 % of such arguments)."""
    run_child(r"""
calls = 0
for n in S.BIG_STEP_SIZES:
    for seed in S.BIG_STEP_SEEDS:
        arrays = S.big_step(n, seed)
        for T1 in (I4, TURN):
            for route in ("ref_order", "replay"):
                assert check_bits(route, arrays, T1, ("big_step", n, seed)), ("the oracle's pose is not finite", n, seed)
                calls += 1
print(f"big_step: {calls} calls with the oracle's bits")
print("ok")
""")


@pytest.mark.parametrize("name", S.AXIS_FAMILIES)
def test_fp64_kinds_on_a_dead_pivot(name):
    """The lane chains (64, 1 025 points), the grid chains and RECORDS (65, 4 097), k_icp_moments + k_icp_update (257) with the stop
    test, and PLAIN + the grid chains at 65 537 points (five fixed iterations; every iteration there ends in k_icp_update_wide) under
    both hand-overs: every iteration within check_problem's bound of the restatement — whose unpivoted solve stops at the same pivot —
    the oracle's iteration count, no rerun by the stop guard, and on axis_x every row the start pose bit for bit."""
    run_child(r"""
name = sys.argv[2]
seen = set()
stats = Stats()
def check(n, kind, expect, max_iter=100, fixed=False):
    # kind None: the thresholds as they are
    src, tgt, nor = S.cloud(name, n)
    sc, tc = capi.Cloud(src, nor), capi.Cloud(tgt, nor)
    g = O.grid_create(tgt, S.RADIUS)
    run = lambda: align(sc, tc, I4, max_iter=max_iter, fixed=fixed)
    try:
        with forced(kind) if kind is not None else thresholds():
            (e, T, it), tr = both_handovers(run) if (kind is None or kind in WIDE) else run()
        kinds = ran_kinds(tr, it)
        seen.update(kinds)
        assert tr.redone[0] == 0, (name, n, kind)
        check_problem(O, g, (src, nor), (tgt, nor), I4, S.RADIUS, tr.poses[0], tr.errs[0], tr.kinds[0], it, T, e, stats,
                      expect=expect, label=f"{name} n {n} kind {kind}", dev=(sc, tc))
        if not fixed:
            e_o, T_o, it_o = O.icp_align(src, nor, tgt, nor, I4, I4, S.RADIUS, MA)
            assert it == it_o, (name, n, kind, "iterations", it, "the oracle's", it_o)
        if name == "axis_x":
            assert (tr.poses[0, :it] == I4).all() and np.asarray(T, F).tobytes() == I4.tobytes(), (name, n, kind, "the pose moved")
    finally:
        O.grid_destroy(g); sc.close(); tc.close()
for kind, sizes in FP64_SIZES:
    for n in sizes:
        check(n, kind, lambda i, kind=kind: kind)
mi = S.PLAIN_ITERS
check(S.PLAIN_SIZE, None, lambda i: capi.ICP_STEP_PLAIN if i < mi - 2 else capi.ICP_STEP_GRID_CHAINS, max_iter=mi, fixed=True)
assert seen == {2, 3, 4, 5, 6}, seen
stats.report(name)
print("ok")
""", name, limit=180)


def test_fp64_kinds_on_tilted_jitter():
    """Pivots of rounding noise: the fp64 kinds' x is whatever their own rounding gives (thousands of radians, like the reference's,
    but not its values), so no value is asserted.  Each call returns within max_iter iterations, runs the kind asked for in every
    iteration, gives the same bits traced and untraced and under both hand-overs.  The deviation from the oracle is printed."""
    run_child(r"""
name = "tilted_jitter"
seen = set()
for kind, sizes in FP64_SIZES:
    for n in sizes:
        src, tgt, nor = S.cloud(name, n)
        poses, errs, ncs = S.oracle_rows(O, src, nor, tgt, nor, I4)
        sc, tc = capi.Cloud(src, nor), capi.Cloud(tgt, nor)
        with forced(kind):
            (e, T, it), tr = both_handovers(lambda: align(sc, tc, I4))
        kinds = ran_kinds(tr, it)
        seen.update(kinds)
        assert 1 <= it <= 100 and set(kinds) <= ({kind, 0, 1} if tr.redone[0] else {kind}), (n, kind, kinds)
        m = min(it, len(errs))
        dev = [float(np.abs(tr.poses[0, i].astype(np.float64) - poses[i]).max()) for i in range(m)]
        print(f"[tilted_jitter] {capi.ICP_STEP_NAMES[kind]:>11} n {n}: {it} iterations (oracle {len(errs)}), redone {int(tr.redone[0])}, first row "
              f"{dev[0]:.3g} from the oracle's (largest entry {np.abs(poses[0]).max():.3g}), last common row {dev[-1]:.3g}, error {float(e):.6g} vs {float(errs[-1]):.6g}")
        sc.close(); tc.close()
assert {2, 3, 5, 6} <= seen, seen
print("ok")
""", limit=180)


def test_weights_on_either_side_of_1e_7():
    """The vanish cases (max_angle 1.6) through every kind that runs one to three points, and the free single weights — f32(1e-7), its
    two neighbours, 2^-24, 2^-23 — through the three routes of rs_hip_icp_estimate_pt2pl.  Σw <= 1e-7 IN DOUBLE keeps the pose and
    the previous error (icp_align: 1e6, after one counted search; the estimate: error 0); anything above goes on to the estimator, and
    the reference-order kinds then have the oracle's bits."""
    run_child(r"""
for case in S.VANISH_CASES:
    src, sn, tgt, tn = S.vanish(case)
    gone = S.vanished(H.seq(S.vanish_weights(case))[-1])
    poses, errs, ncs = S.oracle_rows(O, src, sn, tgt, tn, I4, max_angle=S.VANISH_MAX_ANGLE)
    assert (len(errs) == 1 and errs[0] == F(1e6)) == gone, case
    sc, tc = capi.Cloud(src, sn), capi.Cloud(tgt, tn)
    for kind in (0, 1, 2, 3, 5, 6):
        with forced(kind):
            (e, T, it), tr = align(sc, tc, I4, ma=S.VANISH_MAX_ANGLE)
        assert set(ran_kinds(tr, it)) == {kind}, (case, kind, tr.kinds[0][:it])
        if gone:
            assert it == 1 and F(e) == F(1e6) and np.asarray(T, F).tobytes() == I4.tobytes(), (case, kind, it, e, T)
            assert tr.poses[0, 0].tobytes() == I4.tobytes() and tr.errs[0, 0] == F(1e6), (case, kind)
        elif kind in (0, 1):
            bad = rows_differ(tr, it, e, T, poses, errs)
            assert not bad, (case, kind, bad[:12])
        else:
            assert F(e) != F(1e6) and tr.errs[0, 0] != F(1e6), (case, kind, "the estimator did not run", e)
    sc.close(); tc.close()
    print(f"{case}: vanished {gone}, the oracle's iterations {len(errs)}")
for case in S.FREE_WEIGHTS:
    arrays = S.free_system(case)
    gone = S.vanished(H.seq(arrays[3])[-1])
    assert gone == vanishing(arrays[3])
    assert gone == (case in ("below", "2^-24")), case
    for T1 in (I4, TURN):
        for route in ("ref_order", "replay"):
            finite = check_bits(route, arrays, T1, case)                     # (vanished: T1 itself and error 0 — reference_estimate)
            if case in S.NEGATIVE:
                assert not finite, (case, "the reference's error is sqrt of a negative sum: NaN")
        with thresholds(**ROUTES["moments"]):
            assert estimate_route(len(arrays[3])) == "moments"
            e_d, T_d = capi.icp_estimate_pt2pl(*arrays, T1)
        if gone:
            assert T_d.tobytes() == np.asarray(T1, F).tobytes() and e_d == 0.0, (case, T_d, e_d)
        else:
            assert not (T_d.tobytes() == np.asarray(T1, F).tobytes() and e_d == 0.0) or len(arrays[3]) == 1, (case, "the estimator did not run")
        if case in S.NEGATIVE:
            # icp_solve clamps Σw·s² < 0 to 0 where the reference returns NaN: error 0, and a pose from pivots of either sign
            assert e_d == 0.0, (case, e_d)
            print(f"[free] {case}: k_icp_moments + icp_solve: error {e_d}, pose finite {bool(np.isfinite(T_d).all())}, largest entry {np.abs(T_d).max():.3g}")
print("ok")
""")


def test_a_batch_has_each_problems_single_call_bits():
    """Three problems of the axis_x source at 1 025 points: from the identity, from the pose tilted_jitter's fp64 step composes
    (a translation of hundreds of metres, a rotation composed from thousands of radians), and from a kilometre away — through the
    reference order, the replay, the lane chains, the grid chains and k_icp_moments, under both hand-overs: every problem has its
    single call's pose, error and iteration count, bit for bit, and the two far ones stop after one search with their start pose."""
    run_child(r"""
n = 1025
src, tgt, nor = S.cloud("axis_x", n)
x = S.first_step(O, "tilted_jitter", n)["x"]                    # the fp64 step of tilted_jitter: thousands of radians and metres
tj = R.compose(O, x, S.BASE.astype(F), I4)
assert np.isfinite(tj).all() and np.abs(x[:3]).min() >= 120 and np.abs(tj[12:15]).max() > 100
far = I4.copy(); far[12] = F(1000.0)
T0 = np.stack([I4, tj, far])
sc, tc = capi.Cloud(src, nor), capi.Cloud(tgt, nor)
for kind in (0, 1, 2, 3, 6):
    with forced(kind):
        for on in (0, 1):
            capi.icp_update_fenced(on)
            try:
                with capi.IcpTrace(100, 3) as tr:
                    e, T, it = capi.icp_align_batch(sc, tc, T0, I4, S.RADIUS, MA, max_iter=100, fixed_iters=False)
                for p in range(3):
                    e1, T1, it1 = capi.icp_align(sc, tc, T0[p], I4, S.RADIUS, MA, max_iter=100, fixed_iters=False)
                    assert T[p].tobytes() == T1.tobytes() and F(e[p]) == F(e1) and it[p] == it1, (kind, on, p, "not its single call's bits", it[p], it1, e[p], e1)
            finally:
                capi.icp_update_fenced(0)
            assert it[0] > 6 and (T[0] == I4).all(), (kind, it)
            assert it[1] == 1 and it[2] == 1 and T[1].tobytes() == tj.tobytes() and T[2].tobytes() == far.tobytes(), (kind, it)
            ran = set(tr.kinds[0][:it[0]].tolist())
            assert ran == {kind} or (kind == 3 and ran == {5}), (kind, ran)
sc.close(); tc.close()
print("ok")
""")
