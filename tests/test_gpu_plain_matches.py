"""GPU: plain ICP iterations whose search writes no records (rs_hip_icp_plain_from_records( 0 ), the default).

A plain step of a scan-sized source forms its fp64 moments from what the search leaves per query slot — matched target slot,
dist², dot — in the source's tile order (k_plain_moments), instead of from 48-byte records at the points' original indices
(k_chain_moments).  The addends are the same floats and doubles; the order of the fp64 additions differs, and is fixed.  So:

* every traced iteration lands within the restatement's bound (tests/test_gpu_icp_steps.py: check_problem — per pose entry
  max(1e-6, 4 ulp), error within 4 ulp; POLICY_TOL / 10 where the cut is ambiguous or the search had a tie), with and without
  records, in single calls, batches, before the chains' own iterations and before the RECORDS estimator's;
* two runs give the same bits; tracing (one iteration per chunk: the records come and go per iteration) changes nothing;
* the two paths agree with each other within twice that bound after one step from the same pose.

Shapes: sources just above the 65 536-point threshold of the plain policy (no multiples of 64 or 1 024) and one just above
262 144 (the stop test's plain iterations)."""
import numpy as np
import pytest

import icp_restate as R
from test_gpu_icp_steps import I4, MA, POLICY_TOL, Stats, check_problem, lattice, policy_kind, search_ties, subset, traced, ulp

pytestmark = pytest.mark.gpu

N_SRC = 70_001          # 1 094 tiles' worth: not a multiple of 64 or 1 024
N_BATCH = 66_003
N_STOP = 262_147


@pytest.fixture(scope="module")
def capi():
    from rescan_amd import capi
    capi.init(0)
    assert capi.icp_plain_from_records(-1) == 0, "the default is the step from the matches"
    return capi


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(capi, oracle):
    """One scan pair, its target cloud and oracle grid, and the ~70 k-point source most tests use."""
    from rescan_amd import synth
    c = Ctx()
    c.s0 = synth.scene_for_point_count(275_000, seed=43, timestep=0)
    c.s1 = synth.scene_for_point_count(275_000, seed=43, timestep=1)
    assert len(c.s1["points"]) > N_STOP
    c.tgt = (c.s0["points"], c.s0["normals"])
    c.tc = capi.Cloud(*c.tgt)
    c.grid = oracle.grid_create(c.tgt[0], 0.1)
    c.src = subset(c.s1, N_SRC, 1)
    c.sc = capi.Cloud(*c.src)
    c.T0 = synth.perturbed_pose(I4, np.random.default_rng(N_SRC), 0.02, 0.01)
    yield c
    c.sc.close(); c.tc.close(); oracle.grid_destroy(c.grid)


def run5(capi, c):
    return traced(lambda: capi.icp_align(c.sc, c.tc, c.T0, I4, 0.1, MA, max_iter=5, fixed_iters=True), 5, 1)


@pytest.fixture(scope="module")
def from_matches(capi, ctx):
    """The fixed-length call of tests 1-3, untraced and traced (the same bits: `traced`)."""
    return run5(capi, ctx)


def check5(oracle, c, run, label):
    (e, T, it), tr = run
    stats = Stats()
    assert list(tr.kinds[0]) == [R.STEP_PLAIN] * 3 + [R.STEP_GRID_CHAINS] * 2, tr.kinds[0]
    check_problem(oracle, c.grid, c.src, c.tgt, c.T0, 0.1, tr.poses[0], tr.errs[0], tr.kinds[0], it, T, e, stats,
                  expect=lambda i: policy_kind(N_SRC, 1, True, 5, i), label=label, dev=(c.sc, c.tc))
    stats.report(label)


def test_fixed_call_without_records(capi, oracle, ctx, from_matches):
    """Three plain iterations from the matches, then the chains' two (their records written by their own searches)."""
    check5(oracle, ctx, from_matches, "from matches")


def test_against_the_step_from_records(capi, oracle, ctx, from_matches):
    """The same call with the records back: within the bound too; after iteration 0 (same pose, same correspondences) the two
    paths are within twice the bound of each other, at the end within POLICY_TOL / 10."""
    prev = capi.icp_plain_from_records(1)
    try:
        assert prev == 0
        rec = run5(capi, ctx)
    finally:
        capi.icp_plain_from_records(prev)
    check5(oracle, ctx, rec, "from records")
    (e_m, T_m, _), tr_m = from_matches
    (e_r, T_r, _), tr_r = rec
    c = R.Corrs(oracle, ctx.grid, ctx.src[0], ctx.src[1], ctx.tgt[0], ctx.tgt[1], ctx.T0, I4, np.float32(0.1), MA)
    _, _, info = R.restate_step(oracle, R.STEP_PLAIN, c, ctx.T0)
    loose = info["ambiguous"] or search_ties((ctx.sc, ctx.tc), c, ctx.T0, np.float32(0.1))
    a, b = tr_m.poses[0][0], tr_r.poses[0][0]
    d0 = np.abs(a.astype(np.float64) - b)
    print(f"[matches vs records] iteration 0: max pose difference {d0.max():.3e}, err {tr_m.errs[0][0]!r} vs {tr_r.errs[0][0]!r}; "
          f"final pose difference {np.abs(T_m.astype(np.float64) - T_r).max():.3e}")
    if loose:
        assert d0.max() < 2 * POLICY_TOL / 10
    else:
        assert (d0 <= 2 * np.maximum(1e-6, 4 * np.maximum(ulp(a), ulp(b)))).all(), d0.max()
        assert abs(float(tr_m.errs[0][0]) - float(tr_r.errs[0][0])) <= 2 * 4 * float(ulp(max(tr_m.errs[0][0], tr_r.errs[0][0])))
    assert np.abs(T_m.astype(np.float64) - T_r).max() < POLICY_TOL / 10


def test_twice_in_a_row(capi, ctx, from_matches):
    """The order of the additions is a function of the problem's size alone: pose, error and trace repeat bit for bit."""
    (e0, T0, it0), tr0 = from_matches
    (e1, T1, it1), tr1 = run5(capi, ctx)
    assert T0.tobytes() == T1.tobytes() and e0 == e1 and it0 == it1
    assert tr0.poses.tobytes() == tr1.poses.tobytes() and tr0.errs.tobytes() == tr1.errs.tobytes() and (tr0.kinds == tr1.kinds).all()


def test_batch_of_two_start_poses(capi, oracle, ctx):
    """Two start poses of one ~66 k-point source (blockIdx.y, rows at prob * n): each problem's bits are its single call's;
    the second pose moves half of the source out of the target's reach — many points without a match, an active cut."""
    from rescan_amd import synth
    src = subset(ctx.s1, N_BATCH, 2)
    sc = capi.Cloud(*src)
    stats = Stats()
    try:
        T0 = np.stack([synth.perturbed_pose(I4, np.random.default_rng(s), 0.02, 0.01) for s in (3, 4)])
        lo, hi = ctx.tgt[0][:, 0].min(), ctx.tgt[0][:, 0].max()
        T0[1][12] += np.float32(hi - np.median(src[0][:, 0]))          # the source's median x on the target's far wall
        moved = src[0] @ T0[1].reshape(4, 4)[:3, :3] + T0[1][12:15]
        outside = float(((moved[:, 0] > hi + 0.1) | (moved[:, 0] < lo - 0.1)).mean())
        assert 0.4 < outside < 0.6, outside
        (e, T, it), tr = traced(lambda: capi.icp_align_batch(sc, ctx.tc, T0, I4, 0.1, MA, max_iter=5, fixed_iters=True), 5, 2)
        for p in range(2):
            e1, T1, it1 = capi.icp_align(sc, ctx.tc, T0[p], I4, 0.1, MA, max_iter=5, fixed_iters=True)
            assert T[p].tobytes() == T1.tobytes() and e[p] == e1 and it[p] == it1, f"problem {p}: not its single call's bits"
            check_problem(oracle, ctx.grid, src, ctx.tgt, T0[p], 0.1, tr.poses[p], tr.errs[p], tr.kinds[p], it[p], T[p], e[p], stats,
                          expect=lambda i: policy_kind(N_BATCH, 2, True, 5, i), label=f"batch problem {p}", dev=(sc, ctx.tc))
        c = R.Corrs(oracle, ctx.grid, src[0], src[1], ctx.tgt[0], ctx.tgt[1], T0[1], I4, np.float32(0.1), MA)
        print(f"[batch] problem 1: {len(c)} of {N_BATCH} source points matched in iteration 0, {outside:.2f} outside the target's box")
        assert 0 < len(c) < 0.6 * N_BATCH
    finally:
        sc.close()
    stats.report("batch of two")


def test_records_estimator_after_plain_steps(capi, oracle, ctx):
    """rs_hip_icp_exact_centroids( 2 ): the RECORDS estimator's iterations read records — their own searches' — after three
    searches that wrote none."""
    stats = Stats()
    prev = capi.icp_exact_centroids(2)
    try:
        (e, T, it), tr = run5(capi, ctx)
    finally:
        capi.icp_exact_centroids(prev)
    assert list(tr.kinds[0]) == [R.STEP_PLAIN] * 3 + [R.STEP_RECORDS] * 2, tr.kinds[0]
    check_problem(oracle, ctx.grid, ctx.src, ctx.tgt, ctx.T0, 0.1, tr.poses[0], tr.errs[0], tr.kinds[0], it, T, e, stats,
                  label="records after plain", dev=(ctx.sc, ctx.tc))
    stats.report("records after plain")


def test_source_equal_to_its_target(capi):
    """A cloud aligned to itself at the identity, its points further apart than the radius: dist² all 0, sd 0 — the branch
    without a cut — and a right-hand side of exact zeros.  Three fixed iterations (the first one plain), from matches and from
    records: the same bits."""
    pts = lattice(N_SRC, 5)
    c = capi.Cloud(*pts)
    out = []
    try:
        for on in (0, 1):
            prev = capi.icp_plain_from_records(on)
            try:
                (e, T, it), tr = traced(lambda: capi.icp_align(c, c, I4, I4, 0.1, MA, max_iter=3, fixed_iters=True), 3, 1)
            finally:
                capi.icp_plain_from_records(prev)
            assert list(tr.kinds[0]) == [R.STEP_PLAIN] + [R.STEP_GRID_CHAINS] * 2 and it == 3
            out.append((e, T, tr))
    finally:
        c.close()
    (e0, T0, tr0), (e1, T1, tr1) = out
    assert T0.tobytes() == T1.tobytes() and e0 == e1
    assert tr0.poses.tobytes() == tr1.poses.tobytes() and tr0.errs.tobytes() == tr1.errs.tobytes()
    assert (tr0.poses[0] == I4).all() and (tr0.errs[0] == 0).all()


def test_stop_test_call_above_262144(capi, oracle, ctx):
    """With the stop test a source above 262 144 points runs plain in iterations 0-3 (no guard covers that size: the
    iteration count is not compared with the records path)."""
    from rescan_amd import synth
    src = subset(ctx.s1, N_STOP, 3)
    sc = capi.Cloud(*src)
    stats = Stats()
    try:
        T0 = synth.perturbed_pose(I4, np.random.default_rng(N_STOP), 0.02, 0.01)
        (e, T, it), tr = traced(lambda: capi.icp_align(sc, ctx.tc, T0, I4, 0.1, MA, max_iter=8, fixed_iters=False), 8, 1)
        assert it >= 7 and list(tr.kinds[0][:4]) == [R.STEP_PLAIN] * 4
        check_problem(oracle, ctx.grid, src, ctx.tgt, T0, 0.1, tr.poses[0], tr.errs[0], tr.kinds[0], it, T, e, stats,
                      expect=lambda i: policy_kind(N_STOP, 1, False, 8, i), label="stop test", dev=(sc, ctx.tc))
    finally:
        sc.close()
    stats.report("stop test")
