"""CPU: the hostile addend families of tests/hard_sums.py are what they claim — conditions on the INPUTS, checked with the sequential
reference alone (no GPU) — and the comparisons tests/test_gpu_hard_sums.py makes can fail: the same streams summed pairwise, or with
ties rounded away from zero, trip them."""
import numpy as np
import pytest

import hard_sums as H
import icp_restate as R

F = np.float32
I4 = np.eye(4, dtype=np.float32).ravel()
MA = np.float32(np.deg2rad(60.0))
STREAM_SIZES = (1, 2, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 16385)
LANE_SIZES = (5, 64, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 20000)
GRID_SIZES = (65, 4095, 4096, 4097, 49153, 70001)
TIE_SIZES = tuple(sorted({n for n in STREAM_SIZES + LANE_SIZES + GRID_SIZES + (70001,) if n >= 1024}))


def cloud_rows(name, n):
    pos, sn, tn = H.cloud(name, n)
    p1, p2, w, _ = H.expected_corrs(name, pos, sn, tn)
    return H.addend_rows(p1, p2, w)


def test_dyadic_families_are_full_of_ties():
    """At least n / 32 ties in at least two of the three Σw·p chains at every size from 1 024 on, the first within 256 addends."""
    report = {}
    for n in TIE_SIZES:
        p1, p2, _, w = H.stream("dyadic", n)
        for what, rows in (("dyadic", H.addend_rows(p1, p2, w)), ("dyadic_lattice", cloud_rows("dyadic_lattice", n))):
            ties = [H.tie_count(rows[k]) for k in (1, 2, 3)]
            report[(what, n)] = ties
            assert sum(t >= n // 32 for t in ties) >= 2, (what, n, ties)
            first = min(int(np.nonzero(H.tie_mask(rows[k]))[0][0]) for k in (1, 2, 3))
            assert first < 256, (what, n, first)
            # ... and they matter: the sequential sum is neither the fp64 sum rounded nor the pairwise sum
            assert any(H.seq(rows[k])[-1] != F(rows[k].astype(np.float64).sum()) for k in (1, 2, 3)), (what, n)
            assert any(H.seq(rows[k])[-1] != H.pairwise_sum(rows[k]) for k in (1, 2, 3)), (what, n)
    for n in (20000, 70001):
        print(f"ties in Σw·x, Σw·y, Σw·z at n = {n}: dyadic {report[('dyadic', n)]}, dyadic_lattice {report[('dyadic_lattice', n)]}")


def test_pow2_families_change_binade_on_every_power_of_two():
    for n in sorted(set(STREAM_SIZES + LANE_SIZES + GRID_SIZES)):
        p1, p2, _, w = H.stream("pow2_steps", n)
        for what, rows in (("pow2_steps", H.addend_rows(p1, p2, w)), ("pow2_plane", cloud_rows("pow2_plane", n))):
            powers = [1 << k for k in range(20) if (1 << k) < n]           # addend i meets the sum of the i addends before it
            for row in (0, 1):
                at = set(H.binade_changes(rows[row]).tolist())
                assert at == set(powers), (what, n, row)
        rows = H.addend_rows(p1, p2, w)
        if n >= 64:
            between = H.binade_changes(rows[3])                          # Σw·z = 0.75 i
            assert len(between) >= len(powers) - 1 and all(b & (b - 1) for b in between[2:].tolist()), n
        if n >= 4096:
            assert H.tie_count(rows[4]) >= 2040, (n, H.tie_count(rows[4]))     # Σw·q.x: every addend is a tie while the sum is in [2^11, 2^12)
    print(f"pow2_steps at 16 385: {len(H.binade_changes(rows[0]))} binade changes of Σw on powers of two, {H.tie_count(rows[4])} ties in Σw·q.x")


def test_alternating_and_straddle_return_to_exactly_zero():
    for n in sorted(set(STREAM_SIZES + LANE_SIZES + GRID_SIZES)):
        p1, p2, _, w = H.stream("alternating", n)
        for what, rows, chains in (("alternating", H.addend_rows(p1, p2, w), (1,)), ("straddle", cloud_rows("straddle", n), (1, 2, 3, 4, 5, 6))):
            for k in chains:
                S = H.seq(rows[k])
                assert (S[1::2] == 0).all() and (S[0::2] != 0).all(), (what, n, k)
                assert H.sign_changes(rows[k]) >= n // 2 - 1, (what, n, k)
        if n >= 1023:
            rows = H.addend_rows(p1, p2, w)
            hover = H.binade_changes(rows[2])                            # y: back and forth across 2^10
            assert len(hover) >= n // 8, (n, len(hover))
            assert H.sign_changes(rows[3]) >= n // 64, n                 # z: a walk that keeps coming back through zero
    print(f"alternating at 70 001: {H.sign_changes(rows[1])} sign changes in Σw·x, {len(hover)} binade changes in Σw·y, "
          f"{H.sign_changes(rows[3])} sign changes in Σw·z")


def test_range_rises_eight_binades_inside_a_segment():
    for n in STREAM_SIZES:
        p1, p2, _, w = H.stream("range", n)
        rows = H.addend_rows(p1, p2, w)
        big = np.nonzero(np.abs(p1[:, 0]) == F(2.0 ** 30))[0].tolist()
        assert big == [k for k in (0, 63, 64, 127, 128) if k < n - 1] + ([n - 1] if len([k for k in (0, 63, 64, 127, 128) if k < n - 1]) % 2 else []), (n, big)
        for k in (1, 2, 3):                                              # every +2^30 is cancelled: the sums end small
            assert abs(H.seq(rows[k])[-1]) < 1.0, (n, k)
        if n >= 1023:
            assert H.binade_rise_in_segment(rows[3], 64) >= 8 and H.binade_rise_in_segment(rows[3], 128) >= 8, n
    print(f"range at 16 385: Σw·z rises {H.binade_rise_in_segment(rows[3], 64)} binades inside one segment of 64")


def test_tiny_sums_stay_tiny():
    for n in STREAM_SIZES:
        p1, p2, _, w = H.stream("tiny", n)
        rows = H.addend_rows(p1, p2, w)
        y = H.seq(rows[2])[-1]
        assert y != 0 and abs(y) < np.finfo(F).tiny, (n, y)              # non-zero and subnormal
        x = H.seq(rows[1])
        assert np.abs(x).max() < F(2.0 ** -63), n
        if n >= 127:
            assert x[-1] != 0, n
    for n in LANE_SIZES + GRID_SIZES:
        z = H.seq(cloud_rows("tiny_axis", n)[3])
        assert np.abs(z).max() < F(2.0 ** -63) and (n < 64 or z[-1] != 0), n


def test_zero_runs_are_where_they_claim():
    for n in STREAM_SIZES:
        i = np.arange(n)
        for name, zero in (("zeros_first", i < 640), ("zeros_middle", (i >= n // 3) & (i < 2 * n // 3)), ("zeros_all_but_first", i != 0),
                           ("zeros_all_but_last", i != n - 1)):
            p1, p2, _, w = H.stream(name, n)
            assert ((w == 0) == zero).all(), (name, n)
            if zero.sum() >= 64:
                assert np.signbit(w[zero]).any() and not np.signbit(w[zero]).all(), (name, n)


@pytest.mark.parametrize("name", H.CLOUDS)
def test_clouds_match_themselves(oracle, name):
    """The oracle's search at the identity finds exactly the designed correspondences: the points whose normals pass the gate, in source
    order, d² = 0 (`shifted`: all equal), the designed weights, no correspondence on the uncertain side of the device's cut; and the
    points lie further apart than the search radius."""
    for n in (5, 64, 1025, 4097, 20000):
        pos, sn, tn = H.cloud(name, n)
        tp = H.target_positions(name, pos)
        assert H.min_distance(pos) > H.RADIUS and H.min_distance(tp) > H.RADIUS, (name, n)
        g = oracle.grid_create(tp, H.RADIUS)
        try:
            p1, n1, p2, n2, w_ref, d2, wu = oracle.icp_find_corrs_uncut(g, pos, sn, tp, tn, I4, I4, H.RADIUS, MA)
        finally:
            oracle.grid_destroy(g)
        e1, e2, ew, ed2 = H.expected_corrs(name, pos, sn, tn)
        assert len(wu) == len(ew) == n - int(H.gated_mask(name, n).sum()), (name, n, len(wu))
        assert p1.tobytes() == e1.tobytes() and p2.tobytes() == e2.tobytes(), (name, n)
        assert d2.tobytes() == ed2.tobytes() and (d2 == ed2[:1].sum()).all() and (name == "shifted" or (d2 == 0).all()), (name, n)
        assert wu.tobytes() == ew.tobytes() and w_ref.tobytes() == ew.tobytes(), (name, n)
        assert R.device_cut(d2, H.RADIUS)[2] == 0 and not R.device_cut(d2, H.RADIUS)[0], (name, n)
        if name == "shifted":
            s = H.seq_sums(p1, p2, wu)
            assert s[1] != s[4] and s[3] != s[6], n                     # the Σw·q chains are not the Σw·p chains (the shift has no y)


@pytest.mark.parametrize("name", H.STREAMS)
def test_the_oracle_centres_on_the_sequential_sums(oracle, name):
    """seq_sums is the reference's icp__compute_weighted_centroid: c = Σw·p * (1.0f / Σw) from its sums has the oracle's bits (and
    icp_restate.seq_centroids'), so a device that prints seq_sums' bits centres where the reference does."""
    for n in STREAM_SIZES:
        p1, p2, n2, w = H.stream(name, n)
        s = H.seq_sums(p1, p2, w)
        if not s[0] > F(1e-7):
            continue                                                    # (weights that vanish: the reference divides by zero)
        with np.errstate(all="ignore"):
            inv = F(1.0) / s[0]
            c1, c2 = (s[1:4] * inv).astype(F), (s[4:7] * inv).astype(F)
        r1, r2, tw = R.seq_centroids(p1, p2, w)
        assert tw == s[0] and r1.tobytes() == c1.tobytes() and r2.tobytes() == c2.tobytes(), (name, n)
        assert oracle.weighted_centroid(p1, w).tobytes() == c1.tobytes() and oracle.weighted_centroid(p2, w).tobytes() == c2.tobytes(), (name, n)
        err, T = oracle.icp_estimate_pt2pl(p1, p2, n2, w, I4)
        if np.isfinite(T).all() and np.isfinite(err):
            # the pose is a rotation about c1: with x = 0 it is the identity; nothing more can be read from it without the solve, which
            # tests/test_icp_restate.py holds against this oracle
            assert T.shape == (16,)


def test_the_comparisons_can_fail():
    """What a subtly wrong chain would print trips the device tests' comparisons: the dyadic stream summed pairwise, and with ties
    rounded away from zero, at every size from 1 024 on; one ulp, a NaN for an infinity, a +0 for a -0 in a pose."""
    for n in (1024, 1025, 4097, 16385):
        p1, p2, _, w = H.stream("dyadic", n)
        rows = H.addend_rows(p1, p2, w)
        want = H.totals_words(H.seq_sums(p1, p2, w))
        assert want == H.totals_words([H.seq(r)[-1] for r in rows])
        pair = H.totals_words([H.pairwise_sum(r) for r in rows])
        away = H.totals_words([H.seq_half_away(r) for r in rows])
        assert pair != want and away != want, n
        assert sum(a != b for a, b in zip(pair[1:4], want[1:4])) >= 1 and sum(a != b for a, b in zip(away[1:4], want[1:4])) >= 2, (n, pair, away, want)
    line = "[rs_hip totals] mode 1 problem 0: " + " ".join(want) + "\n"
    assert H.parse_totals("noise\n" + line.replace(want[2], pair[2]) + line) == {0: want}
    T = np.arange(16, dtype=F)
    assert len(H.bits_or_class_differ(T, T)) == 0
    U = T.copy(); U[5] = np.nextafter(U[5], F(100))
    assert H.bits_or_class_differ(U, T).tolist() == [5]
    U = T.copy(); U[0] = F(-0.0)
    assert H.bits_or_class_differ(U, T).tolist() == [0]
    W = T.copy(); W[3] = np.inf; W[4] = np.nan
    U = W.copy(); U[3] = np.nan; U[4] = -np.inf
    assert H.bits_or_class_differ(W, W).tolist() == [] and H.bits_or_class_differ(U, W).tolist() == [3, 4]
    U = W.copy(); U[3] = -np.inf
    assert H.bits_or_class_differ(U, W).tolist() == [3]
