"""CPU: the hostile systems of tests/hard_systems.py are what they claim — conditions on the INPUTS and on the reference's own loop,
checked with the oracle and numpy alone (no GPU): which pivot each family kills, in the centred system and in icp_solve's uncentred
algebra; the step angles of tilted_jitter; the margin by which the oracle's own stop test is decided; the fp32 Σw of the vanish cases;
and that f32(1e-7) has NOT vanished for the helpers, as it has not for the reference."""
import numpy as np
import pytest

import hard_sums as H
import hard_systems as S
import icp_restate as R

F = np.float32


def align_both_ways(oracle, name, n):
    src, tgt, nor = S.cloud(name, n)
    poses, errs, ncs = S.oracle_rows(oracle, src, nor, tgt, nor, S.I4)
    e, T, it = oracle.icp_align(src, nor, tgt, nor, S.I4, S.I4, S.RADIUS, S.MA)
    assert it == len(errs) and T.tobytes() == poses[-1].tobytes() and F(e).tobytes() == errs[-1].tobytes(), (name, n, "oracle_rows is not icp_align")
    return poses, errs, ncs


@pytest.mark.parametrize("name", S.AXIS_FAMILIES)
def test_axis_families_kill_their_pivot(oracle, name):
    """The designed pivot is exactly 0, and the first that is, in R.ldlt6_solve's factorisation of the centred system and of the
    uncentred one (hard_systems.uncentred_system: rs_math.h:icp_solve op for op); every x from it on is 0, the ones before it are not
    all 0 (a right-hand side that is not zero); axis_x never moves the oracle's pose."""
    k = S.DEAD_PIVOT[name]
    for n in S.sizes_of(name):
        if n < 7 or n > S.STOP_TEST_UP_TO:          # (three points: the 2.5 sigma cut may leave no weight at all — see the loop test)
            continue
        fs = S.first_step(oracle, name, n)
        assert fs["n_corr"] == n, (name, n)
        for what, C, x in (("centred", fs["C"], fs["x"]), ("uncentred", fs["Cu"], fs["xu"])):
            pv = S.pivots(C)
            assert len(pv) == k + 1 and pv[-1] == 0 and all(p != 0 for p in pv[:-1]), (name, n, what, pv)
            assert (C[k, :] == 0).all() and (C[:, k] == 0).all(), (name, n, what, "row / column not structurally zero")
            assert (x[k:] == 0).all() and (k == 0 or (x[:k] != 0).any()), (name, n, what, x)
        assert (fs["b"] != 0).any()
    for n in S.sizes_of("axis_x")[:6]:
        poses, errs, ncs = align_both_ways(oracle, "axis_x", n)
        assert (poses == S.I4).all(), n


def test_axis_z_keeps_tz_although_the_target_is_shifted_in_z(oracle):
    """The reference's quirk: the source lies 2^-9 and more from the target in z on average, the z row of the system and its
    right-hand side are not zero, and the stop at pivot 2 leaves tz = 0 all the same: only rx and ry move."""
    src, tgt, nor = S.cloud("axis_z", 1025)
    assert (src[:, 2].astype(np.float64) - tgt[:, 2]).mean() > 2.0 ** -9
    fs = S.first_step(oracle, "axis_z", 1025)
    assert fs["b"][5] != 0 and fs["C"][5, 5] > 100 and fs["x"][5] == 0 and fs["x"][2] == 0 and fs["x"][0] != 0 and fs["x"][1] != 0


def test_tilted_jitter_steps_by_hundreds_of_radians(oracle):
    """At every size the family is used at: no exact zero among the pivots, all three step angles of the fp64 restatement in
    [120, 1e6), and a finite pose from the oracle's own loop.  Pivots of either sign are met over the sizes."""
    signs = set()
    for n in S.TILTED_SIZES:
        fs = S.first_step(oracle, "tilted_jitter", n)
        pv = S.pivots(fs["C"])
        assert len(pv) == 6 and all(p != 0 for p in pv), (n, pv)
        signs |= {np.sign(p) for p in pv}
        a = np.abs(fs["x"][:3])
        print(f"tilted_jitter n {n}: pivots {np.array2string(np.array(pv), precision=2)}, step angles {np.array2string(fs['x'][:3], precision=1)} rad")
        assert ((a >= 120) & (a < 1e6)).all(), (n, fs["x"])
        poses, errs, ncs = align_both_ways(oracle, "tilted_jitter", n)
        assert np.isfinite(poses).all() and np.isfinite(errs).all(), n
    assert signs == {1.0, -1.0}, signs


def test_big_step_turns_by_thousands_of_radians_in_the_references_own_arithmetic(oracle):
    """Well conditioned (cond < 1e5), so the fp64 restatement's x is the reference's to rounding: every case has a step angle of at
    least 120 rad, none reaches 1e6, two thirds of all angles are beyond 120, and the oracle's pose is finite.  The family has teeth:
    in several of its cases an angle's sine or cosine by the double-precision function rounded once — what rs_sincosf_model used to
    return beyond 120 — is not the host's sinf / cosf."""
    import ctypes as C
    libm = C.CDLL("libm.so.6")
    for fn in (libm.sinf, libm.cosf):
        fn.restype = C.c_float; fn.argtypes = [C.c_float]
    beyond, total, parted = 0, 0, 0
    for n in S.BIG_STEP_SIZES:
        for seed in S.BIG_STEP_SEEDS:
            p1, p2, n2, w = S.big_step(n, seed)
            c1, c2, _ = R.seq_centroids(p1, p2, w)
            C, b, _, _ = R.centred_system(p1, p2, n2, w, c1, c2)
            x = R.ldlt6_solve(C, b)[:3]
            a = np.abs(x)
            big = [float(v) for v in x.astype(F) if abs(v) >= 120]
            parted += any(F(np.sin(v)) != F(libm.sinf(v)) or F(np.cos(v)) != F(libm.cosf(v)) for v in big)
            assert np.linalg.cond(C) < 1e5 and a.max() >= 120 and a.max() < 1e6, (n, seed, a)
            beyond += int((a >= 120).sum()); total += 3
            e, T = oracle.icp_estimate_pt2pl(p1, p2, n2, w, S.I4)
            assert np.isfinite(T).all() and np.isfinite(e), (n, seed)
    assert 3 * beyond >= 2 * total, (beyond, total)
    print(f"big_step: {beyond} of {total} angles beyond 120 rad; rounding the double-precision function once parts from libm in {parted} of {total // 3} cases")
    assert parted >= 4, parted


@pytest.mark.parametrize("name", S.CLOUDS)
def test_the_oracles_stop_test_is_decided_by_a_margin(oracle, name):
    """Every |err_i - err_{i-1}| with i > 5 of the oracle's own icp_align lies outside [0.5e-5, 2e-5] at every size the stop test is
    met at: an fp64 estimator that follows the reference's errors to ~1e-7 decides like the reference, and no decision falls inside
    the guard (1.5e-6 around 1e-5)."""
    met = 0
    for n in S.sizes_of(name):
        if n > S.STOP_TEST_UP_TO:
            continue
        poses, errs, ncs = align_both_ways(oracle, name, n)
        d = S.stop_deltas(errs)
        met += len(d)
        assert not ((d >= 0.5e-5) & (d <= 2e-5)).any(), (name, n, d)
    assert met > 0 or name == "tilted_jitter", name


def test_breaks_are_met_in_iteration_0_and_in_iteration_1(oracle):
    """What the loop's two breaks meet over the families: a first search whose every weight the 2.5 sigma cut zeroes (Σw = 0 exactly, in
    iteration 0, three points of axes_yz), and a second search that finds nothing after a step of thousands of radians
    (tilted_jitter at 257 points: n_corr == 0 in iteration 1, not 0)."""
    poses, errs, ncs = align_both_ways(oracle, "axes_yz", 3)
    assert len(errs) == 1 and ncs[0] == 3 and errs[0] == F(1e6) and (poses[0] == S.I4).all()
    poses, errs, ncs = align_both_ways(oracle, "tilted_jitter", 257)
    assert len(errs) == 2 and ncs[0] == 257 and ncs[1] == 0 and errs[1] == errs[0] and poses[1].tobytes() == poses[0].tobytes()


def test_vanish_cases_sum_to_what_was_designed(oracle):
    """The oracle's search gives every vanish case the designed weights bit for bit; their sequential fp32 sum lies on the designed side
    of the DOUBLE 1e-7, and both sides are met with 1, 2 and 3 points."""
    sides = {}
    for case, d in S.VANISH_CASES.items():
        src, sn, tgt, tn = S.vanish(case)
        g = oracle.grid_create(tgt, S.RADIUS)
        try:
            w = oracle.icp_find_corrs_uncut(g, src, sn, tgt, tn, S.I4, S.I4, S.RADIUS, S.VANISH_MAX_ANGLE)[4]
        finally:
            oracle.grid_destroy(g)
        want = S.vanish_weights(case)
        assert len(w) == len(d) and w.tobytes() == want.tobytes(), (case, w, want)
        dots = np.maximum(np.array(d), 0)
        assert ((want <= dots.astype(F)) & (want >= dots.astype(F) * F(0.99))).all()
        sides[case] = S.vanished(H.seq(w)[-1])
        poses, errs, ncs = S.oracle_rows(oracle, src, sn, tgt, tn, S.I4, max_angle=S.VANISH_MAX_ANGLE)
        e, T, it = oracle.icp_align(src, sn, tgt, tn, S.I4, S.I4, S.RADIUS, S.VANISH_MAX_ANGLE)
        assert it == len(errs) and T.tobytes() == poses[-1].tobytes()
        if sides[case]:
            assert it == 1 and e == F(1e6) and (T == S.I4).all(), case
        else:
            assert it > 1 or e != F(1e6), case
    assert sides == {"one_2^-24": True, "one_2^-23": False, "two_2^-24": False, "2^-24_and_0": True, "three_2^-24": False,
                     "2^-24_2^-23_0": False}, sides


def test_f32_1e_7_has_not_vanished():
    """The reference (icp.h:466) and the library compare the float total with the DOUBLE 1e-7.  f32(1e-7) = 1.0000000116860974e-07 lies
    above it: a total of exactly that value goes on to the estimator.  The helpers decide the same: hard_systems.vanished and
    icp_restate.restate_step (which used to compare in fp32 and kept the pose there)."""
    t = S.F32_1E7
    assert float(t) == 1.0000000116860974e-07 and float(t) > 1e-7 and bool(t <= F(1e-7))       # (what the fp32 compare said)
    assert not S.vanished(t) and S.vanished(np.nextafter(t, F(0))) and not S.vanished(np.nextafter(t, F(1)))
    assert S.vanished(F(2.0 ** -24)) and not S.vanished(F(2.0 ** -23)) and S.vanished(F(0)) and S.vanished(F(-1))

    class One:
        def __init__(self, w):
            self.p1, self.p2, self.n2, _ = S.free_system("f32(1e-7)")
            self.w_ref = self.w_uncut = np.array([w], F)
            self.d2 = np.zeros(1, F); self.max_dist = F(1.0)

        def __len__(self):
            return 1

    class Est:                                   # the estimator is asked exactly when the total has not vanished
        asked = 0

        def icp_estimate_pt2pl(self, p1, p2, n2, w, T1):
            Est.asked += 1
            return F(0.5), np.asarray(T1, F).copy()
    for w, goes_on in ((t, True), (np.nextafter(t, F(0)), False), (np.nextafter(t, F(1)), True)):
        before = Est.asked
        T, e, info = R.restate_step(Est(), R.STEP_REF_ORDER, One(w), S.I4)
        assert (Est.asked - before == 1) == goes_on and (e is not None) == goes_on, (w, e)


def test_negative_weights_part_the_estimators():
    """Negative weights with Σw > 1e-7 in the free systems: pivots of the system are negative and Σw·s² < 0 — icp_solve clamps it to 0
    (error 0), the reference takes the square root (NaN)."""
    for case in S.NEGATIVE:
        p1, p2, n2, w = S.free_system(case)
        assert not S.vanished(H.seq(w)[-1]) and (w < 0).any()
        C, b, err, c1, clamped = S.uncentred_system(S.moments(p1, p2, n2, w))
        print(f"{case}: pivots {np.array2string(np.array(S.pivots(C)), precision=2)}, clamped {clamped}, icp_solve's error {err}")
        assert any(p < 0 for p in S.pivots(C)), case
        assert clamped and err == 0, case
