"""GPU: the ICP estimators' sums on hostile addends (tests/hard_sums.py; the families are held to their claims in
tests/test_hard_sums_cpu.py): exact ties, binade changes on segment / stretch / block boundaries, sums that return to exactly zero,
sums below 2^-63 and denormal ones, values that rise 40 binades inside one segment.

* free streams through rs_hip_icp_estimate_pt2pl: k_icp_faithful and the replay against the oracle's icp_estimate_pt2pl, pose and
  error bit for bit (a non-finite entry by its class); k_icp_moments against the fp64 restatement, within the bound of
  test_gpu_icp_steps.py;
* self-matching clouds through icp_align: the seven sums the lane chains, the grid chains and the records route used
  (RS_HIP_DEBUG_TOTALS) against the sequential fp32 sums of the oracle's correspondences, bit for bit, and against each other;
* streams with a NaN or an overflow, and weights that vanish.

Every test runs in a child process under its own time limit; the thresholds it sets are restored in `finally`.  Nothing is skipped: a
route that did not run — by the kinds a traced call reports, or by the thresholds the library reads back — is a failure."""
import os
import subprocess
import sys

import pytest

import hard_sums as H
from conftest import ROOT

pytestmark = pytest.mark.gpu

PRELUDE = r"""
import os, sys, tempfile
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from rescan_amd import capi
from oracle.pyoracle import Oracle
import hard_sums as H, icp_restate as R
capi.init(0)
O = Oracle()
F = np.float32
I4 = np.eye(4, dtype=F).ravel()
MA = F(np.deg2rad(60.0))
BIG = 1 << 30
STREAM_SIZES = (1, 2, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 16385)
MOMENT_SIZES = (257, 4097, 16385, 70001)
LANE_SIZES = (5, 64, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 20000)
GRID_SIZES = (65, 4095, 4096, 4097, 49153, 70001)          # 49 153: twelve blocks of 4 096 and one point
# a pose that is not the identity: a turn of 0.3 rad about (0, 0, 1) and a shift, by the oracle's own helpers
TURN = O.rotate(O.translate(I4, np.array([0.5, -0.25, 2.0], F)), F(0.3), np.array([0.0, 0.0, 1.0], F))
assert not (TURN == I4).all()
SETTERS = ("icp_reference_order_below", "icp_replay_below", "icp_lane_chains_below", "icp_exact_centroids", "icp_chains_retry_after")
class thresholds:
    # with thresholds(icp_replay_below=BIG, ...): sets them, reads them back, restores what was there
    def __init__(self, **kw): self.kw = kw
    def __enter__(self):
        self.prev = {k: getattr(capi, k)(-1) for k in SETTERS}
        for k, v in self.kw.items():
            getattr(capi, k)(v)
            assert getattr(capi, k)(-1) == v, k
        return self
    def __exit__(self, *exc):
        for k, v in self.prev.items(): getattr(capi, k)(v)
        return False
def estimate_route(n):
    # rs_hip_icp_estimate_pt2pl's choice (rs_icp_api.hip), from the thresholds the library reads back now
    ref, rep, lane, mode = (getattr(capi, k)(-1) for k in SETTERS[:4])
    seq_below = max(ref, lane if mode != 0 else 0)
    if n <= max(seq_below, rep):
        return "ref_order" if (n <= seq_below or n > rep) else "replay"
    return "moments"
ROUTES = {"ref_order": dict(icp_reference_order_below=BIG),
          "replay": dict(icp_reference_order_below=0, icp_lane_chains_below=0, icp_replay_below=BIG),
          "moments": dict(icp_reference_order_below=0, icp_lane_chains_below=0, icp_replay_below=0, icp_exact_centroids=0)}
def vanishing(w):
    # the weights' sequential fp32 sum is <= 1e-7 (icp.h:466-470: icp_align keeps the pose; include/rescan_hip.h: so does the estimate)
    # (compared in DOUBLE as the reference and the library do: a sum of exactly f32(1e-7) = 1.0000000116860974e-07 has not vanished)
    return bool(float(H.seq(w)[-1]) <= 1e-7)
def reference_estimate(p1, p2, n2, w, T1):
    if vanishing(w):
        return F(0.0), np.asarray(T1, F).copy()
    with np.errstate(all="ignore"):
        e, T = O.icp_estimate_pt2pl(p1, p2, n2, w, T1)
    return F(e), T
def check_bits(route, arrays, T1, what):
    # one call through `route` against the oracle: every entry of the pose and the error, bit for bit or by its non-finite class
    e_o, T_o = reference_estimate(*arrays, T1)
    with thresholds(**ROUTES[route]):
        assert estimate_route(len(arrays[3])) == route, (what, route)
        e_d, T_d = capi.icp_estimate_pt2pl(*arrays, T1)
    bad = H.bits_or_class_differ(np.concatenate([T_d, [e_d]]), np.concatenate([T_o, [e_o]]))
    assert not len(bad), (what, route, "entries", bad.tolist(), "device", np.concatenate([T_d, [e_d]])[bad], "oracle", np.concatenate([T_o, [e_o]])[bad])
    return bool(np.isfinite(T_o).all() and np.isfinite(e_o))
class stderr_text:
    # what the library writes to file descriptor 2 inside the block (RS_HIP_DEBUG_TOTALS' lines)
    def __enter__(self):
        sys.stderr.flush()
        self.f = tempfile.TemporaryFile(); self.saved = os.dup(2); os.dup2(self.f.fileno(), 2)
        return self
    def __exit__(self, *exc):
        os.dup2(self.saved, 2); os.close(self.saved)
        self.f.seek(0); self.text = self.f.read().decode(errors="replace"); self.f.close()
        return False
def ulp(x): return np.spacing(np.abs(np.asarray(x, F))).astype(np.float64)
"""


FAULTED = []        # a child that ended by a fault, an abort or its time limit: nothing more of this module is started on the GPU after it


def run_child(body, *args, limit=120):
    assert not FAULTED, f"not started: an earlier child of this module ended abnormally ({FAULTED[0]})"
    env = dict(os.environ, RS_HIP_DEBUG_TOTALS="1")
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT] + [str(a) for a in args],
                         capture_output=True, text=True, env=env)
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139) or "illegal memory access" in out.stderr:
        FAULTED.append(out.returncode)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    print(out.stdout.strip())
    return out.stdout


@pytest.mark.parametrize("name", H.STREAMS)
def test_reference_order_and_replay_have_the_oracles_bits(name):
    """k_icp_faithful and the replay (segments of 128, four mantissa classes, k_replay_walk) on every free stream at sizes around the
    segment (128), superblock (8 192) and stretch boundaries, from the identity and from a turned pose: the oracle's pose and error,
    bit for bit; a non-finite entry must be non-finite of the same class.  Weights that vanish keep the pose (include/rescan_hip.h)."""
    run_child(r"""
name = sys.argv[2]
finite = 0
for n in STREAM_SIZES:
    arrays = H.stream(name, n)
    for T1 in (I4, TURN):
        for route in ("ref_order", "replay"):
            finite += check_bits(route, arrays, T1, (name, n))
print(f"{name}: {4 * len(STREAM_SIZES)} calls, {finite} with a finite reference")
print("ok")
""", name)


@pytest.mark.parametrize("name", H.MOMENT_STREAMS)
def test_moments_route_follows_the_fp64_restatement(name):
    """k_icp_moments (all three thresholds 0, rs_hip_icp_exact_centroids( 0 )) against icp_restate.restate_step( STEP_MOMENTS ) fed
    with the stream through a Corrs-like object: every pose entry within max(1e-6, 4 ulp), the error within 4 ulp — the bound of
    test_gpu_icp_steps.py.  It rests on coordinates of a few metres there; at offsets of 1e4 the uncentred fp64 algebra of icp_solve,
    restated in numpy and summed in three orders, moved x by at most 2e-11 from the centred solve (20 000 and 70 000
    correspondences), so the bound carries over.  The largest deviation per family is printed (DESIGN.md §4 keeps the figures)."""
    run_child(r"""
name = sys.argv[2]
class Stream:
    def __init__(self, p1, p2, n2, w):
        self.p1, self.p2, self.n2, self.w_ref, self.w_uncut = p1, p2, n2, w, w
        self.d2 = np.zeros(len(w), F); self.max_dist = F(1.0)              # no dist² statistics: no cut (device_cut: sd = 0)
    def __len__(self): return len(self.w_ref)
worst_pose, worst_err = 0.0, 0.0
for n in MOMENT_SIZES:
    arrays = H.stream(name, n)
    for T1 in (I4, TURN):
        T_r, e_r, info = R.restate_step(O, R.STEP_MOMENTS, Stream(*arrays), T1)
        assert e_r is not None and info["ambiguous"] == 0
        with thresholds(**ROUTES["moments"]):
            assert estimate_route(n) == "moments"
            e_d, T_d = capi.icp_estimate_pt2pl(*arrays, T1)
        dpose = np.abs(T_d.astype(np.float64) - T_r.astype(np.float64))
        derr = abs(float(e_d) - float(e_r)) / float(ulp(max(F(e_d), F(e_r))))
        print(f"{name} n {n}: pose {dpose.max():.3e} ({(dpose / np.maximum(ulp(T_d), ulp(T_r))).max():.2f} ulp of its entry), err {derr:.2f} ulp")
        worst_pose, worst_err = max(worst_pose, float(dpose.max())), max(worst_err, derr)
        tol = np.maximum(1e-6, 4 * np.maximum(ulp(T_d), ulp(T_r)))
        assert (dpose <= tol).all() and derr <= 4, (name, n, dpose.max(), derr)
print(f"[moments] {name}: largest pose deviation {worst_pose:.3e}, largest err deviation {worst_err:.2f} ulp")
print("ok")
""", name)


CHAINS = r"""
def corrs_of(name, pos, sn, tn):
    tp = H.target_positions(name, pos)
    g = O.grid_create(tp, H.RADIUS)
    try:
        p1, n1, p2, n2, w_ref, d2, wu = O.icp_find_corrs_uncut(g, pos, sn, tp, tn, I4, I4, H.RADIUS, MA)
    finally:
        O.grid_destroy(g)
    use, cut, ambiguous = R.device_cut(d2, H.RADIUS)
    assert not use and ambiguous == 0
    return p1, p2, wu
CHAIN_ROUTES = (("lane_chains", LANE_SIZES, dict(icp_lane_chains_below=BIG, icp_exact_centroids=1), capi.ICP_STEP_LANE_CHAINS),
                ("grid_chains", GRID_SIZES, dict(icp_lane_chains_below=0, icp_exact_centroids=1), capi.ICP_STEP_GRID_CHAINS),
                ("records", GRID_SIZES, dict(icp_lane_chains_below=0, icp_exact_centroids=2), capi.ICP_STEP_RECORDS))
def traced_align(src, tgt, T0s, max_iter):
    n = len(T0s)
    with capi.IcpTrace(max_iter, n) as tr, stderr_text() as err:
        if n == 1:
            e, T, it = capi.icp_align(src, tgt, T0s[0], I4, H.RADIUS, MA, max_iter=max_iter, fixed_iters=True)
            e, T, it = np.array([e], F), T[None, :], np.array([it])
        else:
            e, T, it = capi.icp_align_batch(src, tgt, T0s, I4, H.RADIUS, MA, max_iter=max_iter, fixed_iters=True)
    return e, T, it, tr, H.parse_totals(err.text)
"""


@pytest.mark.parametrize("name", H.CLOUDS)
def test_chain_routes_print_the_sequential_sums(name):
    """icp_align of a self-matching cloud from the identity (three fixed iterations; `shifted`: one), through the lane chains
    (stretches of 16 addends x 64 lanes), the grid chains (segments of 64, blocks of 64 segments, forecast walks, a budget after which
    a call is given up to the records route) and the records route (pass 2 of the replay): the kind every iteration ran is the one
    asked for (RECORDS after a give-up; the first of three iterations of a source above 65 536 points is the policy's PLAIN step), the
    seven sums of the last iteration are the sequential fp32 sums of the oracle's correspondences, the three routes print the same
    words, the pose stays the identity with error 0, and no family but `straddle` makes the grid chains give a call up."""
    run_child(CHAINS + r"""
name = sys.argv[2]
mi = H.cloud_max_iter(name)
gave_up_total = 0
for n in sorted(set(LANE_SIZES + GRID_SIZES)):
    pos, sn, tn = H.cloud(name, n)
    src, tgt = capi.Cloud(pos, sn), capi.Cloud(H.target_positions(name, pos), tn)
    p1, p2, wu = corrs_of(name, pos, sn, tn)
    want = H.totals_words(H.seq_sums(p1, p2, wu))
    printed = {}
    for route, sizes, setting, kind in CHAIN_ROUTES:
        if n not in sizes:
            continue
        with thresholds(icp_reference_order_below=0, icp_replay_below=0, icp_chains_retry_after=0, **setting):
            before = capi.icp_chains_gave_up()
            e, T, it, tr, totals = traced_align(src, tgt, I4[None, :], mi)
            gave_up = capi.icp_chains_gave_up() - before
        where = (name, n, route)
        gave_up_total += gave_up
        assert gave_up == 0 or (route == "grid_chains" and name == "straddle"), where
        kinds = tr.kinds[0].tolist()
        if len(wu) == 0:
            # every normal gated: the first search finds nothing, the call ends there with the pose it came with (icp.h:455-459)
            assert it[0] == 1 and kinds[1:] == [capi.ICP_STEP_NONE] * (mi - 1) and T[0].tobytes() == I4.tobytes(), where + (kinds,)
            if 0 in totals:
                assert totals[0] == want, where
            continue
        ran = capi.ICP_STEP_RECORDS if gave_up else kind
        n_plain = max(0, mi - 2) if (n > 65536 and route != "lane_chains") else 0          # (DESIGN.md §4: early plain iterations)
        assert it[0] == mi and kinds == [capi.ICP_STEP_PLAIN] * n_plain + [ran] * (mi - n_plain), where + (kinds,)
        assert 0 in totals, where + ("no [rs_hip totals] line",)
        assert totals[0] == want, where + (totals[0], want)
        printed[route] = totals[0]
        if name != "shifted":
            assert (tr.poses[0, :mi] == I4).all() and (tr.errs[0, :mi] == 0).all() and (T[0] == I4).all() and e[0] == 0, where + (tr.errs[0],)
        else:
            assert np.isfinite(T[0]).all() and e[0] > 0 and not (T[0] == I4).all(), where
    assert len(set(map(tuple, printed.values()))) <= 1, (name, n, printed)
    src.close(); tgt.close()
print(f"{name}: calls the grid chains gave up: {gave_up_total}")
print("ok")
""", name)


def test_a_batch_prints_the_single_calls_sums():
    """Three start poses, all the identity, through icp_align_batch on dyadic_lattice at 20 000 points (the lane chains, a walk per
    problem side by side): every problem prints the totals of the single call, which are the sequential sums."""
    run_child(CHAINS + r"""
name, n = "dyadic_lattice", 20000
pos, sn, tn = H.cloud(name, n)
src, tgt = capi.Cloud(pos, sn), capi.Cloud(pos, tn)
p1, p2, wu = corrs_of(name, pos, sn, tn)
want = H.totals_words(H.seq_sums(p1, p2, wu))
with thresholds(icp_reference_order_below=0, icp_replay_below=0, icp_chains_retry_after=0):
    e1, T1, it1, tr1, single = traced_align(src, tgt, I4[None, :], 3)
    e3, T3, it3, tr3, batch = traced_align(src, tgt, np.stack([I4, I4, I4]), 3)
assert single == {0: want}, (single, want)
assert batch == {0: want, 1: want, 2: want}, (batch, want)
assert (tr1.kinds == capi.ICP_STEP_LANE_CHAINS).all() and (tr3.kinds == capi.ICP_STEP_LANE_CHAINS).all(), (tr1.kinds, tr3.kinds)
assert (T3 == I4).all() and (e3 == 0).all() and (it3 == 3).all()
print("ok")
""")


def test_weights_that_vanish_keep_the_pose():
    """All-zero weights (some of them -0.0) at n = 1, 128 and 4 097: the reference's estimator divides by their sum and returns NaN; its
    caller tests the sum first and keeps the pose (icp.h:466-470).  rs_hip_icp_estimate_pt2pl does what the caller does on all three of
    its routes (include/rescan_hip.h): T1 comes back as it went in, the error is 0."""
    run_child(r"""
for n in (1, 128, 4097):
    p1, p2, n2, w = H.stream("dyadic", n)
    w = np.where(np.arange(n) % 3 == 1, F(-0.0), F(0.0)).astype(F)
    with np.errstate(all="ignore"):
        e_o, T_o = O.icp_estimate_pt2pl(p1, p2, n2, w, I4)
    assert not np.isfinite(T_o).all()                                     # (the reference itself: NaN)
    for T1 in (I4, TURN):
        for route in ("ref_order", "replay", "moments"):
            with thresholds(**ROUTES[route]):
                assert estimate_route(n) == route
                e_d, T_d = capi.icp_estimate_pt2pl(p1, p2, n2, w, T1)
            assert T_d.tobytes() == np.asarray(T1, F).tobytes() and e_d == 0.0, (n, route, T_d, e_d)
print("ok")
""")


def test_zz_nonfinite_streams_end_with_the_oracles_classes():
    """Last, alone in its own child: `dyadic` with one NaN coordinate at index 130, and with two 3e38 addends of one sign (a chain that
    overflows), through k_icp_faithful and the replay at n = 257, 4 097 and 16 385: every entry of the pose and the error is non-finite
    of the oracle's class (NaN, +inf, -inf) or equal to it in bits.

    Why every loop of those routes ends whatever the values are (rescan_amd/csrc/rs_icp_faithful.hip) — all of them are counted loops
    over chunks, segments and addends; no exit rests on a comparison of summed values, which a NaN would make false for ever:
      k_icp_faithful     faith_pass steps k0 = 0 .. n_chunks by FAITH_AHEAD (:250), n_chunks from n alone (:236); a chain wave adds a
                         chunk by two fully unrolled loops over FAITH_CHUNK / 16 groups (:187, :208); the guess of sigma strides
                         i < n (:323); the comparisons on sums (cnt == 0 :341, total <= 1e-7 :363, the band test :351) select a
                         straight-line branch each — with a NaN total the pass goes on to the normal equations and the counted
                         6x6 solve;
      k_replay_run       replay_terms strides t < REPLAY_SEG (:503); replay_run_chain adds t = 0 .. REPLAY_SEG - 1 (:647) — a NaN or
                         infinite guess or value only clears `valid` (:639, :653), which keeps the shifts defined (:654) and marks
                         the record unusable (:667);
      k_replay_walk      replay_walk_row walks s0 < n_super (:848), js < n_sup (:853), j < n_here (:860) and re-adds a segment by
                         t4 < REPLAY_SEG / 4 (:871); an unusable record costs one re-added segment, never a retry;
      between them       k_replay_sums (:571), k_replay_scan (:592, :595, :603) and replay_compose_chain (s < n, :718) are
                         counted as well, and replay_params' tests (:452-:472) only choose whether a pass runs at all.
    Nothing had to be changed for this test."""
    run_child(r"""
checked = 0
for kind in ("nan", "inf"):
    for n in (257, 4097, 16385):
        arrays = H.nonfinite_stream(kind, n)
        for route in ("ref_order", "replay"):
            finite = check_bits(route, arrays, I4, (kind, n))
            assert not finite, (kind, n, "the oracle's result is finite: the stream is not hostile")
            checked += 1
print(f"{checked} non-finite calls")
print("ok")
""")
