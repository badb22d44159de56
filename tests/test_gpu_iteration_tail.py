"""GPU: the end of an ICP iteration of a scan-sized source, and the edges of a call.

k_icp_update_wide — 35 workgroups sum the moments' partials, the last one to finish solves — hands its 35 sums over by
agent-scope atomic stores, a relaxed ticket and atomic loads; rs_hip_icp_update_fenced( 1 ) brings back the hand-over by two
full fences.  The additions and their order are the same, so:

* every estimator that ends in that launch (plain from the matches, plain from records, the grid chains, RECORDS) gives the
  same pose, error, iteration count and trace bit for bit under both hand-overs, with 512-capped and 4 n_blk partial counts,
  fixed length and stop test;
* the ticket is per problem and returns to zero: a batch with a problem that goes inactive in iteration 0 gives every problem
  its single call's bits, and a call repeats bit for bit, also right after that batch;
* the initial loop state of up to 1 KB rides in the fill launch's argument block, larger ones are copied: a problem's bits do
  not depend on which;
* k_plain_moments holds the restatement's bound at the smallest plain sizes, where the waves of the last XCD class hold
  fewer tiles than the others (a load pipeline for it was built and dropped in the same round: the cases stay).

The scan pair, `subset`, `traced`, `check_problem` and the fixed five-iteration call are those of test_gpu_plain_matches.py /
test_gpu_icp_steps.py."""
import numpy as np
import pytest

import icp_restate as R
from test_gpu_icp_steps import I4, MA, Stats, check_problem, policy_kind, subset, traced
from test_gpu_plain_matches import N_BATCH, N_STOP, capi, ctx, run5  # noqa: F401  (capi, ctx: fixtures)

pytestmark = pytest.mark.gpu


def same_bits(a, b, what):
    (ea, Ta, ia), tra = a
    (eb, Tb, ib), trb = b
    assert np.asarray(Ta).tobytes() == np.asarray(Tb).tobytes(), f"{what}: pose"
    assert np.asarray(ea).tobytes() == np.asarray(eb).tobytes() and np.asarray(ia).tobytes() == np.asarray(ib).tobytes(), f"{what}: error / iterations"
    assert tra.poses.tobytes() == trb.poses.tobytes() and tra.errs.tobytes() == trb.errs.tobytes(), f"{what}: traced iterations"
    assert (tra.kinds == trb.kinds).all(), f"{what}: estimator kinds"


def both_handovers(capi, fn):
    """fn() under the atomics and under the fences; the switch is back at its default afterwards."""
    assert capi.icp_update_fenced(-1) == 0, "the default is the hand-over by atomics"
    out = []
    try:
        for on in (0, 1):
            capi.icp_update_fenced(on)
            out.append(fn())
    finally:
        capi.icp_update_fenced(0)
    return out


@pytest.fixture(scope="module")
def stop_cloud(capi, ctx):
    sc = capi.Cloud(*subset(ctx.s1, N_STOP, 3))
    yield sc
    sc.close()


@pytest.mark.parametrize("case", ["from_matches", "from_records", "records_estimator", "stop_test"])
def test_publish_against_fences(capi, ctx, stop_cloud, case):
    """Three plain iterations and two of the chains (partial counts 512-capped and 4 n_blk), the same from records, the RECORDS
    estimator's own iterations, and a stop-test call on the 262 147-point source."""
    from rescan_amd import synth
    kinds = None
    if case == "stop_test":
        T0 = synth.perturbed_pose(I4, np.random.default_rng(N_STOP), 0.02, 0.01)
        fn = lambda: traced(lambda: capi.icp_align(stop_cloud, ctx.tc, T0, I4, 0.1, MA, max_iter=8, fixed_iters=False), 8, 1)
    else:
        fn = lambda: run5(capi, ctx)
        kinds = [R.STEP_PLAIN] * 3 + [R.STEP_RECORDS if case == "records_estimator" else R.STEP_GRID_CHAINS] * 2
    prev_rec = capi.icp_plain_from_records(1 if case == "from_records" else 0)
    prev_cen = capi.icp_exact_centroids(2) if case == "records_estimator" else None
    try:
        atomics, fenced = both_handovers(capi, fn)
    finally:
        capi.icp_plain_from_records(prev_rec)
        if prev_cen is not None:
            capi.icp_exact_centroids(prev_cen)
    same_bits(atomics, fenced, case)
    (_, _, it), tr = atomics
    if kinds is not None:
        assert it == 5 and list(tr.kinds[0]) == kinds, tr.kinds[0]
    else:
        assert it >= 7 and list(tr.kinds[0][:4]) == [R.STEP_PLAIN] * 4, (it, tr.kinds[0])


@pytest.fixture(scope="module")
def batch(capi, ctx):
    """Three start poses of one 66 003-point source; the third is a kilometre away: no correspondence in iteration 0."""
    from rescan_amd import synth
    src = subset(ctx.s1, N_BATCH, 2)
    sc = capi.Cloud(*src)
    T0 = np.stack([synth.perturbed_pose(I4, np.random.default_rng(s), 0.02, 0.01) for s in (3, 4, 5)])
    T0[2][12] += np.float32(1000.0)
    yield sc, T0
    sc.close()


def run_batch(capi, ctx, batch):
    sc, T0 = batch
    return capi.icp_align_batch(sc, ctx.tc, T0, I4, 0.1, MA, max_iter=5, fixed_iters=True)


def test_batch_with_a_problem_that_goes_inactive(capi, ctx, batch):
    """Per-problem ticket and done[prob]: every problem of the batch has its single call's bits — the two that run all five
    iterations and the one that stops in iteration 0 — under both hand-overs."""
    sc, T0 = batch
    for e, T, it in both_handovers(capi, lambda: run_batch(capi, ctx, batch)):
        for p in range(3):
            e1, T1, it1 = capi.icp_align(sc, ctx.tc, T0[p], I4, 0.1, MA, max_iter=5, fixed_iters=True)
            assert T[p].tobytes() == T1.tobytes() and e[p] == e1 and it[p] == it1, f"problem {p}: not its single call's bits"
        assert it[0] == 5 and it[1] == 5 and it[2] == 1, it
        assert T[2].tobytes() == T0[2].tobytes(), "a problem without correspondences keeps its start pose"


def test_twice_in_a_row_and_after_the_batch(capi, ctx, batch):
    """Nothing of the ticket or the state's upload outlives a call."""
    call = lambda: capi.icp_align(ctx.sc, ctx.tc, ctx.T0, I4, 0.1, MA, max_iter=5, fixed_iters=True)
    e0, T0, it0 = call()
    e1, T1, it1 = call()
    run_batch(capi, ctx, batch)
    e2, T2, it2 = call()
    assert T0.tobytes() == T1.tobytes() == T2.tobytes() and e0 == e1 == e2 and it0 == it1 == it2 == 5


def test_state_in_the_argument_block_and_by_copy(capi, ctx, batch):
    """The largest batch whose state block fits in the fill launch's argument block, and one problem more (a copy): the
    common problems' bits are the same, and problem 0's are its single call's (one problem: the argument block)."""
    from rescan_amd import synth
    sc, _ = batch
    state_words, launch_max_words = capi.icp_state_layout()      # the library's own numbers: 39 words per problem, 256 words = 1 KB
    assert state_words >= 34 and launch_max_words * 4 == 1024, (state_words, launch_max_words)
    fits = launch_max_words // state_words
    assert fits >= 1
    T0 = np.stack([synth.perturbed_pose(I4, np.random.default_rng(100 + s), 0.02, 0.01) for s in range(fits + 1)])
    e_a, T_a, it_a = capi.icp_align_batch(sc, ctx.tc, T0[:fits], I4, 0.1, MA, max_iter=5, fixed_iters=True)
    e_c, T_c, it_c = capi.icp_align_batch(sc, ctx.tc, T0, I4, 0.1, MA, max_iter=5, fixed_iters=True)
    assert T_a.tobytes() == T_c[:fits].tobytes() and e_a.tobytes() == e_c[:fits].tobytes() and it_a.tobytes() == it_c[:fits].tobytes()
    e1, T1, it1 = capi.icp_align(sc, ctx.tc, T0[0], I4, 0.1, MA, max_iter=5, fixed_iters=True)
    assert T1.tobytes() == T_c[0].tobytes() and e1 == e_c[0] and it1 == it_c[0] == 5
    assert not (T_c[fits] == T0[fits]).all(), "the problem beyond the argument block ran"


@pytest.mark.parametrize("n", [65_537, 65_601])
def test_smallest_plain_sizes(capi, oracle, ctx, n):
    """The smallest sources that run plain iterations: the tiles do not divide evenly among the XCD classes and waves; five
    iterations, each within the restatement's bound (check_problem, as test_fixed_call_without_records)."""
    from rescan_amd import synth
    src = subset(ctx.s1, n, 4)
    sc = capi.Cloud(*src)
    stats = Stats()
    try:
        T0 = synth.perturbed_pose(I4, np.random.default_rng(n), 0.02, 0.01)
        (e, T, it), tr = traced(lambda: capi.icp_align(sc, ctx.tc, T0, I4, 0.1, MA, max_iter=5, fixed_iters=True), 5, 1)
        assert list(tr.kinds[0]) == [R.STEP_PLAIN] * 3 + [R.STEP_GRID_CHAINS] * 2, tr.kinds[0]
        check_problem(oracle, ctx.grid, src, ctx.tgt, T0, 0.1, tr.poses[0], tr.errs[0], tr.kinds[0], it, T, e, stats,
                      expect=lambda i: policy_kind(n, 1, True, 5, i), label=f"{n} points", dev=(sc, ctx.tc))
    finally:
        sc.close()
    stats.report(f"{n} points")


def test_call_without_iterations_returns_its_own_start(capi, ctx, batch):
    """max_iter = 0 enqueues no iteration and copies nothing back: the call returns ITS start pose, error 1e6 and 0 iterations,
    not what an earlier call (here: a batch from other poses) left in the pinned state block."""
    run_batch(capi, ctx, batch)
    e, T, it = capi.icp_align(ctx.sc, ctx.tc, ctx.T0, I4, 0.1, MA, max_iter=0, fixed_iters=True)
    assert np.asarray(T, np.float32).tobytes() == np.asarray(ctx.T0, np.float32).tobytes() and e == np.float32(1e6) and it == 0, (T, e, it)
