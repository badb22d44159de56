"""GPU: the switches still reach the code they steer after rs_switches.h took over the reads.

* the LIVE flags of the ICP searches, flipped through os.environ between two calls of one process, are seen (rs_hip_switch_get) and
  leave pose and error bit-identical;
* the estimator thresholds' setters reach icp_choose: every iteration's trace kind is the estimator they asked for;
* rs_hip_icp_update_fenced( 1 ) against ( 0 ) on the grid chains: the same bits;
* the routes of the full-rows search (RS_HIP_ROWS_TILED_FROM, RS_HIP_NO_ROWS_WAVE) return the same rows.

Clouds from rescan_amd/synth.py: a ~3 000-point source (more than one tile: a warm start has something to reuse) against a
~20 000-point room (cells enough for certificates and a slow-tile list), six fixed iterations (1 to 5 are warm)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I4 = np.eye(4, dtype=np.float32).ravel()
MA = np.float32(np.deg2rad(60.0))
N_ITER = 6
LIVE_FLAGS = ["RS_HIP_NO_WARM", "RS_HIP_NO_CERT", "RS_HIP_NO_RANK_CERT", "RS_HIP_NO_SEED", "RS_HIP_NO_LPT", "RS_HIP_NO_BY_ROWS",
              "RS_HIP_NO_BOUNDED_ONLY"]


@pytest.fixture(scope="module")
def capi():
    from rescan_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def pair(capi):
    """(source cloud, target cloud, start pose, the room's points)"""
    from rescan_amd import synth
    s = synth.make_scene(seed=3, density=860.0, timestep=1)
    pos, nor = synth.make_object("table", 3 * 7919, 1125.0, 1.0, 0.0)
    assert 2500 <= len(pos) <= 3500 and 17000 <= len(s["points"]) <= 23000, (len(pos), len(s["points"]))
    src = capi.Cloud(np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(nor, np.float32), cell_size=0.1)
    tgt = capi.Cloud(s["points"], s["normals"], cell_size=0.1)
    T0 = synth.perturbed_pose(s["objects"][0]["pose"], np.random.default_rng(5))
    yield src, tgt, T0, s["points"]
    src.close(); tgt.close()


@pytest.fixture()
def clean_env():
    """None of the library's names in the environment during the test; whatever was there is back afterwards."""
    saved = {k: v for k, v in os.environ.items() if k.startswith(("RS_HIP_", "RS_DROPIN_")) and k != "RS_HIP_LIB"}
    for k in saved:
        del os.environ[k]
    yield
    for k in [k for k in os.environ if k.startswith(("RS_HIP_", "RS_DROPIN_")) and k != "RS_HIP_LIB"]:
        del os.environ[k]
    os.environ.update(saved)


def align(capi, pair):
    src, tgt, T0, _ = pair
    err, T, it = capi.icp_align(src, tgt, T0, I4, 0.1, MA, max_iter=N_ITER, fixed_iters=True)
    assert it == N_ITER and np.isfinite(err) and err < 1e5, (err, it)
    return np.float32(err).tobytes() + np.asarray(T, np.float32).tobytes()


def test_live_flags_are_seen_and_leave_the_bits_alone(capi, pair, clean_env):
    base = align(capi, pair)
    assert align(capi, pair) == base, "a call repeats bit for bit"
    for flag in LIVE_FLAGS:
        assert capi.switch_get(flag) == 0.0, flag
        os.environ[flag] = "0"                     # (set at all)
        try:
            assert capi.switch_get(flag) == 1.0, flag
            assert align(capi, pair) == base, flag
        finally:
            del os.environ[flag]
        assert capi.switch_get(flag) == 0.0, flag
    os.environ.update({f: "1" for f in LIVE_FLAGS})
    try:
        assert align(capi, pair) == base, "all of them"
    finally:
        for f in LIVE_FLAGS:
            del os.environ[f]


def traced(capi, pair):
    with capi.IcpTrace(N_ITER, 1) as tr:
        bits = align(capi, pair)
    return bits, tr


@pytest.fixture()
def thresholds(capi):
    """The estimator policy at its defaults for the test (whatever the environment said when the library was loaded), restored afterwards."""
    fns = capi.icp_reference_order_below, capi.icp_replay_below, capi.icp_lane_chains_below, capi.icp_update_fenced, capi.icp_exact_centroids
    prev = [fn(v) for fn, v in zip(fns, (16384, 0, 65536, 0, 1))]
    yield
    for fn, v in zip(fns, prev):
        fn(v)


def test_setters_reach_the_estimator_choice(capi, pair, clean_env, thresholds):
    _, tr = traced(capi, pair)
    assert (tr.kinds[0] == capi.ICP_STEP_REF_ORDER).all(), tr.kinds
    capi.icp_reference_order_below(0)
    assert capi.switch_get("RS_HIP_REF_ORDER_BELOW") == 0.0
    _, tr = traced(capi, pair)
    assert (tr.kinds[0] == capi.ICP_STEP_LANE_CHAINS).all(), tr.kinds
    capi.icp_lane_chains_below(0)
    assert capi.switch_get("RS_HIP_LANE_CHAINS_BELOW") == 0.0
    grid, tr = traced(capi, pair)
    assert (tr.kinds[0] == capi.ICP_STEP_GRID_CHAINS).all(), tr.kinds
    # the launch that ends a grid-chain iteration, by fences instead of atomics: the same bits
    assert capi.icp_update_fenced(1) == 0 and capi.switch_get("RS_HIP_UPDATE_FENCED") == 1.0
    fenced, trf = traced(capi, pair)
    assert capi.icp_update_fenced(0) == 1
    assert fenced == grid and trf.poses.tobytes() == tr.poses.tobytes() and trf.errs.tobytes() == tr.errs.tobytes()
    assert (trf.kinds[0] == capi.ICP_STEP_GRID_CHAINS).all()


def test_rows_routes_give_the_same_rows(capi, pair, clean_env):
    _, tgt, _, pts = pair
    rng = np.random.default_rng(9)
    q = (pts[rng.choice(len(pts), 2000, replace=False)] + rng.normal(0.0, 0.01, (2000, 3))).astype(np.float32)
    assert capi.switch_get("RS_HIP_ROWS_TILED_FROM") == 4096.0
    wave = capi.radius_search(tgt, q, 0.08, 8)            # 2 000 queries of k = 8: below the threshold, one wave per query
    os.environ["RS_HIP_ROWS_TILED_FROM"] = "0"
    try:
        assert capi.switch_get("RS_HIP_ROWS_TILED_FROM") == 0.0
        tiled = capi.radius_search(tgt, q, 0.08, 8)
    finally:
        del os.environ["RS_HIP_ROWS_TILED_FROM"]
    os.environ["RS_HIP_NO_ROWS_WAVE"] = "1"
    try:
        assert capi.switch_get("RS_HIP_NO_ROWS_WAVE") == 1.0
        no_wave = capi.radius_search(tgt, q, 0.08, 8)
    finally:
        del os.environ["RS_HIP_NO_ROWS_WAVE"]
    assert wave[3] > 8 * 1000, "most rows are full: the k-cap is exercised"
    held = np.arange(8)[None, :] < wave[2][:, None]           # (what a row holds beyond its count is nobody's)
    for other, what in ((tiled, "RS_HIP_ROWS_TILED_FROM=0"), (no_wave, "RS_HIP_NO_ROWS_WAVE=1")):
        assert (other[2] == wave[2]).all() and other[3] == wave[3], what
        assert other[0][held].tobytes() == wave[0][held].tobytes() and (other[1][held] == wave[1][held]).all(), what
