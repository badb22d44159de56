"""CPU: the host planner of the pose search (rs_hip_pose_grid_plan) against the NumPy restatement written from the reference's loops
(tests/propose_restate.py) and against the reference's own translations (tests/golden/propose_floor.npz, written by
mgs__propose_poses_at_level / mgs_propose_poses: tools/propose_fixture); its counts-only pass and refusals; the restated bookkeeping
over the fixtures' recorded lists; the fixtures' sizes and conditions; the new symbols.

The yaw table's yardstick is the restatement, not the reference's output: a last yaw step that never wins a cell does not show in
any list the reference returns, so only the restatement of :219-221 in explicit float32 / float64 can say how many steps there are.
(Where a rotation does win, the fixtures' poses carry its bits, and those are compared too.)"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden
import propose_restate as R

LIB = os.path.join(ROOT, "rescan_amd", "librescan_hip.so")
E_ARG, E_CAPACITY = -2, -4
F = np.float32
CASES = ("room", "wide", "floor", "empty")
SYMBOLS = ("rs_hip_pose_grid_plan", "rs_hip_propose_poses", "rs_hip_cell_best", "rs_hip_verify_marks", "rs_hip_propose_release")
DEFAULT_DELTA = F(np.float64(6.2831853072) / np.float64(F(10.0)))          # (float)( MSH_TWO_PI / 10.0f ), pose_proposal.cpp:28
# the sweep
LENGTHS = (0.0, 0.05, 1.0, 1.2, 1.6, 2.0, 3.2, 3.3000002, 8.0, 12.7)
SPACINGS = (0.1, 0.07, 0.15, 0.25, 0.3)
DELTAS = (DEFAULT_DELTA, F(np.float64(6.2831853072) / 6.0), F(np.float64(6.2831853072) / 12.0), F(1.0), F(6.2831855), F(7.0), F(0.01))


@pytest.fixture(scope="module")
def lib():
    from rescan_amd import build
    build.build()
    lib = C.CDLL(LIB)
    lib.rs_hip_pose_grid_plan.restype = C.c_int
    lib.rs_hip_pose_grid_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
    return lib


def plan(lib, lo, hi, spacing, delta, caps=None, tables=True):
    lo, hi = np.ascontiguousarray(lo, F), np.ascontiguousarray(hi, F)
    n = np.full(3, -7, np.int32)
    args = [lo.ctypes.data, hi.ctypes.data, float(spacing), float(delta), n.ctypes.data, n.ctypes.data + 4, n.ctypes.data + 8]
    if not tables:
        return lib.rs_hip_pose_grid_plan(*args, None, 0, None, 0, None, 0), n, None
    if caps is None:
        rc, n, _ = plan(lib, lo, hi, spacing, delta, tables=False)
        assert rc == 0
        caps = n.tolist()
    ox, oz, yaw = np.full(max(caps[0], 1), -7, F), np.full(max(caps[1], 1), -7, F), np.full((max(caps[2], 1), 16), -7, F)
    rc = lib.rs_hip_pose_grid_plan(*args, ox.ctypes.data, caps[0], oz.ctypes.data, caps[1], yaw.ctypes.data, caps[2])
    return rc, n, (ox[:caps[0]], oz[:caps[1]], yaw[:caps[2]])


def test_planner_counts_the_issue_names(lib):
    """Fails on a library without rs_hip_pose_grid_plan.  10 yaws at the default delta; 22, 18, 35 and 83 steps for 2.0, 1.6, 3.2, 8.0."""
    for length, want in ((2.0, 22), (1.6, 18), (3.2, 35), (8.0, 83)):
        rc, n, _ = plan(lib, (0, 0, 0), (length, 1, length), 0.1, DEFAULT_DELTA, tables=False)
        assert rc == 0 and n.tolist() == [want, want, 10], (length, n)
    assert len(R.offsets(3.2, 0.1)) == 35 and int(np.ceil((np.float64(F(3.2)) + 2 * np.float64(F(0.1))) / np.float64(F(0.1)))) == 34


def test_planner_equals_the_restatement_over_the_sweep(lib):
    n_cases = 0
    for k, length in enumerate(LENGTHS):
        for spacing in SPACINGS:
            delta = DELTAS[(k + n_cases) % len(DELTAS)]
            lo = np.array([0.3 * k - 1.0, -0.5, 0.1 * k], F)
            hi = np.array([lo[0] + F(length), 0.5, lo[2] + F(0.5 * length)], F)
            rc, n, (ox, oz, yaw) = plan(lib, lo, hi, spacing, delta)
            wx, wz, wy = R.grid_plan(lo, hi, spacing, delta)
            assert rc == 0 and n.tolist() == [len(wx), len(wz), len(wy)], (length, spacing, delta, n)
            assert ox.tobytes() == wx.tobytes() and oz.tobytes() == wz.tobytes() and yaw.tobytes() == wy.tobytes(), (length, spacing, delta)
            n_cases += 1
    for delta in DELTAS:        # every yaw table of the sweep, whatever the rotation above picked
        rc, n, (_, _, yaw) = plan(lib, (0, 0, 0), (1, 1, 1), 0.1, delta)
        assert rc == 0 and yaw.tobytes() == R.grid_plan((0, 0, 0), (1, 1, 1), 0.1, delta)[2].tobytes(), delta
    assert len(R.yaw_angles(F(7.0))) == 1 and len(R.yaw_angles(F(6.2831855))) == 1 and len(R.yaw_angles(DEFAULT_DELTA)) == 10


def test_planner_translations_are_the_references(lib):
    """Every cell of the floor fixture proposes, so the recorded poses show the reference's ox and oz tables; the winning rotations
    show rows of its yaw table."""
    g = load_golden("propose_floor.npz")
    for r in range(int(g["n_runs"])):
        rc, n, (ox, oz, yaw) = plan(lib, g["bbox"][:3], g["bbox"][3:], g[f"run{r}_spacing"], g[f"run{r}_angle_delta"])
        assert rc == 0
        P = g[f"run{r}_obj0_poses"]
        assert len(P) == n[0] * n[1]
        tx, tz = P[:, 12].reshape(n[0], n[1]), P[:, 14].reshape(n[0], n[1])
        assert (tx == (g["bbox"][0] + ox)[:, None]).all() and (tz == (g["bbox"][2] + oz)[None, :]).all()
        assert (P[:, 13] == g["height"]).all() and (P[:, 15] == 1).all()
        rows = {y[:12].tobytes() for y in yaw}
        assert all(p[:12].tobytes() in rows for p in P)


def test_planner_counts_only_short_tables_and_refusals(lib):
    lo, hi = (0, 0, 0), (2.0, 1.0, 1.6)
    rc, n, _ = plan(lib, lo, hi, 0.1, DEFAULT_DELTA, tables=False)
    assert rc == 0 and n.tolist() == [22, 18, 10]
    for caps in ([21, 18, 10], [22, 17, 10], [22, 18, 9]):
        rc, n, (ox, oz, yaw) = plan(lib, lo, hi, 0.1, DEFAULT_DELTA, caps=caps)
        assert rc == E_CAPACITY and n.tolist() == [22, 18, 10]
        assert (ox == -7).all() and (oz == -7).all() and (yaw == -7).all(), "a refused call wrote a table"
    for bad_lo, bad_hi, sp, de in (((np.nan, 0, 0), hi, 0.1, 0.6), (lo, (np.inf, 1, 1), 0.1, 0.6), (lo, (2, np.nan, 1), 0.1, 0.6),
                                   (lo, hi, 0.0, 0.6), (lo, hi, -0.1, 0.6), (lo, hi, np.nan, 0.6), (lo, hi, 0.1, 0.0), (lo, hi, 0.1, -1.0),
                                   (lo, hi, 0.1, np.nan), (lo, hi, np.inf, 0.6),
                                   ((-3e38, 0, 0), (3e38, 1, 1), 0.1, 0.6)):
        rc, n, _ = plan(lib, bad_lo, bad_hi, sp, de, tables=False)
        assert rc == E_ARG and (n == -7).all(), (bad_lo, bad_hi, sp, de, rc)
    for bad_hi, sp, de in (((1e6, 1, 1), 0.25, 0.6), (hi, 1e-9, 0.6), (hi, 0.1, 1e-9)):       # more than 2^20 steps in a table
        rc, n, _ = plan(lib, lo, bad_hi, sp, de, tables=False)
        assert rc == E_CAPACITY and (n == -7).all(), (bad_hi, sp, de, rc)
    assert lib.rs_hip_pose_grid_plan(None, None, 0.1, 0.6, None, None, None, None, 0, None, 0, None, 0) == E_ARG


@pytest.mark.parametrize("case", CASES)
def test_restated_bookkeeping_gives_the_fixtures_lists(case):
    """Stage by stage over the recorded storage: marks keep entries <= 0, turn the others into a score > threshold or -1, and the
    final copy of the last stage is mgs_propose_poses' own list, -1 entries included."""
    g = load_golden(f"propose_{case}.npz")
    thr = g["thresholds"]
    for r in range(int(g["n_runs"])):
        for o in range(int(g["n_objects"])):
            P, s = g[f"run{r}_obj{o}_poses"], [g[f"run{r}_obj{o}_s{k}"] for k in range(3)]
            assert (s[0] > thr[0]).all()
            for k in (1, 2):
                # what the reference scored is lost where it wrote -1: any value that fails the threshold stands in for it
                new = np.where(s[k] == -1, thr[k], s[k]).astype(F)
                assert R.verify_marks(s[k - 1], new, thr[k]).tobytes() == s[k].tobytes()
                assert ((s[k] > thr[k]) | (s[k] == -1)).all() and (s[k][s[k - 1] == -1] == -1).all()
            fp, fs = R.final_copy(P, s[2])
            assert fp.tobytes() == g[f"run{r}_obj{o}_final_poses"].tobytes() and fs.tobytes() == g[f"run{r}_obj{o}_final_scores"].tobytes()
            assert len(fs) == len(s[0]), "every stored proposal is copied: |score| > 1e-6 holds for kept and for -1 alike"
            # the poses are grid poses in cell order
            ox, oz, yaw = R.grid_plan(g["bbox"][:3], g["bbox"][3:], g[f"run{r}_spacing"], g[f"run{r}_angle_delta"])
            if len(P):
                ix = np.searchsorted(g["bbox"][0] + ox, P[:, 12]); iz = np.searchsorted(g["bbox"][2] + oz, P[:, 14])
                assert ((g["bbox"][0] + ox)[ix] == P[:, 12]).all() and ((g["bbox"][2] + oz)[iz] == P[:, 14]).all()
                assert (np.diff(ix * len(oz) + iz) > 0).all(), "cell order"


def test_fixture_sizes_and_conditions():
    import importlib.util
    spec = importlib.util.spec_from_file_location("propose_gen", os.path.join(ROOT, "tools", "propose_fixture", "gen.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    for case in CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"propose_{case}.npz")) <= 757075
        gen.conditions(case, load_golden(f"propose_{case}.npz"))
    g = load_golden("propose_room.npz")
    assert [int(g[f"obj{o}_static"]) for o in range(3)] == [0, 0, 1] and len(g["run0_obj2_final_scores"]) == 0


def test_new_symbols_are_exported_and_bound(lib):
    from rescan_amd import capi
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in capi.SIGNATURES, s
    hdr = open(os.path.join(ROOT, "include", "rescan_hip.h")).read()
    assert all(s + "(" in hdr for s in SYMBOLS)
    assert all(callable(getattr(capi, f)) for f in ("pose_grid_plan", "propose_poses", "cell_best", "verify_marks", "propose_release"))
    ox, oz, yaw = capi.pose_grid_plan((0, 0, 0), (3.2, 1, 1.6), 0.1, DEFAULT_DELTA)
    assert (len(ox), len(oz), yaw.shape) == (35, 18, (10, 16)) and capi.pose_grid_plan((0, 0, 0), (3.2, 1, 1.6), 0.1, DEFAULT_DELTA, tables=False) == (35, 18, 10)
    lib.rs_hip_propose_release.restype = C.c_int
    assert lib.rs_hip_propose_release() == 0              # nothing held by this thread: nothing to free, no device needed
    dropin = C.CDLL(os.path.join(ROOT, "rescan_amd", "librescan_dropin.so"))
    assert hasattr(dropin, "rsd_propose_poses")
