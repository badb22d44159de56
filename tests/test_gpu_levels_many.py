"""GPU: all levels of many clouds in one call -- rs_hip_level_samples_many, rs_hip_cloud_create_levels_many (rescan_amd/csrc/rs_levels.hip)
and the shim's rsd_levels_poisson -- on the hostile inputs of tests/hard_clouds.py and tests/rows_restate.py.

Expected samples are rows_restate.level_samples (numpy, held to the CPU oracle by tests/test_hard_rows_cpu.py), never the code under
test; every case asserts within <= cap for the restatement, so the reference's answer is defined.  Expected cloud bytes are
Cloud.level_of's of the same base, compared through layout(), the host copies and the reported size.  Every comparison is equality.

The GPU work runs in child processes (this file, run as a script with a case name), each under its own time limit; the session stops
at the first abort, fault or time limit.  No case provokes a fault: every refusal is decided on the host, the caps after the counting
pass (which writes counts and a word) and before anything is written through the counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rows_restate as R_

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

pytestmark = pytest.mark.gpu

E_CAPACITY = "error -4"                                       # RS_HIP_E_CAPACITY, as capi reports it


def run_child(case, *args, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), case, *[str(a) for a in args]],
                         capture_output=True, text=True)
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139) or "illegal memory access" in out.stderr:
        # a time limit, an abort or a fault: nothing more is started on this GPU, the evidence is what the child printed
        pytest.exit(f"{case} {args}: the child ended with {out.returncode}; the session stops here\n{out.stdout[-3000:]}\n{out.stderr[-3000:]}", 3)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


# ================================================================================================================================
# child side
# ================================================================================================================================

def _setup():
    for p in (HERE, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    from rescan_amd import capi
    import build_restate as B
    import rows_restate as R
    capi.init(0)
    return capi, R, B


def _levels(numbers):
    from oracle.pyoracle import LEVEL_VOXEL, level_max_n_neigh
    return [(LEVEL_VOXEL[lv], level_max_n_neigh(lv)) for lv in numbers]


def _want(R, p, levels):
    out = []
    for r, cap in levels:
        idx, within = R.level_samples(p, r)
        assert within <= cap, (r, cap, within)
        out.append(idx)
    return out


def _assert_samples(got, want, what):
    assert got.dtype == np.int32 and len(got) == len(want), (what, len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (what, len(bad), int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def _host_points(capi, cloud, with_nor):
    p = np.zeros((cloud.n, 3), np.float32); n = np.zeros((cloud.n, 3), np.float32)
    capi._check(capi.load().rs_hip_cloud_points(cloud.handle, p.ctypes.data, n.ctypes.data if with_nor else None))
    return p.tobytes() + (n.tobytes() if with_nor else b"")


def _assert_cloud(capi, B, got, base, r, cap, cell, what):
    """got == Cloud.level_of(base, r, cap, cell) to the byte: both layouts, the host copies, the reported sizes."""
    twin, idx = capi.Cloud.level_of(base, r, cap, cell)
    a, b = got.layout(), twin.layout()
    assert sorted(a) == sorted(b) and ("nor" in a) == (base._nor is not None), (what, sorted(a), sorted(b))
    assert B.layout_bytes(a) == B.layout_bytes(b), (what, [k for k in a if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()])
    with_nor = base._nor is not None
    assert _host_points(capi, got, with_nor) == _host_points(capi, twin, with_nor), what
    assert got.n == twin.n and got.n_tiles == twin.n_tiles and got.nbytes == twin.nbytes, what
    twin.close()
    return idx


def _assert_batch(capi, R, B, clouds, levels, what, cell=-1.0, want=None):
    """Both entry points on the batch: samples == the restatement, clouds == level_of's.  clouds: [(points, normals or None)]."""
    bases = [capi.Cloud(p, n) for p, n in clouds]
    want = want or [_want(R, p, levels) for p, _ in clouds]
    got, rounds = capi.level_samples_many(bases, levels)
    made = capi.Cloud.levels_many(bases, levels, cell)
    assert len(got) == len(bases) == len(made)
    for c, base in enumerate(bases):
        assert len(got[c]) == len(levels) == len(made[c])
        for l, (r, cap) in enumerate(levels):
            _assert_samples(got[c][l], want[c][l], (what, c, l, "samples"))
            _assert_samples(made[c][l][1], want[c][l], (what, c, l, "cloud's samples"))
            cells = cell if np.ndim(cell) == 0 else cell[l]
            idx = _assert_cloud(capi, B, made[c][l][0], base, r, cap, cells, (what, c, l))
            _assert_samples(idx, want[c][l], (what, c, l, "level_of"))
            made[c][l][0].close()
    for b in bases:
        b.close()
    return got, rounds


def case_one_level(name):
    """1. one cloud, one level == the single call."""
    capi, R, B = _setup()
    f = R.family(name)
    levels = _levels((2,))
    got, rounds = _assert_batch(capi, R, B, [(f["points"], f["normals"])], levels, name)
    base = capi.Cloud(f["points"], None)
    single, _ = capi.level_samples(base, *levels[0])
    _assert_samples(got[0][0], single, (name, "single call"))
    print(name, "samples", len(single), "rounds", rounds)


def case_four_levels():
    """2. levels (4, 1, 3, 2) in that order; equal radii with different caps."""
    capi, R, B = _setup()
    f = R.family("offset_1e3")
    p, nor = f["points"], f["normals"]
    _assert_batch(capi, R, B, [(p, nor)], _levels((4, 1, 3, 2)), "4132", cell=[-1.0, 0.05, 0.0, -1.0])
    r = 0.01
    want, within = R.level_samples(p, r)
    assert within <= 256
    base = capi.Cloud(p, None)
    got, _ = capi.level_samples_many([base], [(r, 256), (r, 512)])
    _assert_samples(got[0][0], want, "equal radii, 256"); _assert_samples(got[0][1], want, "equal radii, 512")
    got, _ = capi.level_samples_many([base], [(r, 512), (0.04, 768), (r, 256)])
    _assert_samples(got[0][0], want, "equal radii around a larger one"); _assert_samples(got[0][2], want, "equal radii around a larger one")
    _assert_samples(got[0][1], R.level_samples(p, 0.04)[0], "the larger one")


def case_threshold(shuffled):
    """3. both radii are exact lattice distances: the strict < decides the class of a pair."""
    capi, R, B = _setup()
    p = R.lattice(shuffled=shuffled == "1")
    levels = [(0.0625, 256), (0.125, 512)]
    from hard_clouds import d2_rows, radius_sq
    d2 = d2_rows(p, p[:64])
    assert (d2 == radius_sq(0.0625)).sum() > 200 and (d2 == radius_sq(0.125)).sum() > 200      # pairs exactly at each threshold
    _assert_batch(capi, R, B, [(p, None)], levels, ("lattice", shuffled))
    _assert_batch(capi, R, B, [(p, None)], levels[::-1], ("lattice, reversed", shuffled))


def case_sizes():
    """4. sizes around a tile and a block in one batch, prefixes of one family, two levels."""
    capi, R, B = _setup()
    f = R.family("negative")
    clouds = [(np.ascontiguousarray(f["points"][:n]), np.ascontiguousarray(f["normals"][:n])) for n in (0, 1, 2, 63, 64, 65, 255, 256, 257)]
    got, _ = _assert_batch(capi, R, B, clouds, _levels((3, 1)), "sizes")
    assert [len(g[0]) for g in got][:2] == [0, 1]
    # the near points of the family, so that a tile holds neighbours: the first 257 by distance to the first point
    d = ((f["points"].astype(np.float64) - f["points"][0]) ** 2).sum(1)
    near = np.sort(np.argsort(d, kind="stable")[:257])
    clouds = [(np.ascontiguousarray(f["points"][near[:n]]), None) for n in (0, 1, 2, 63, 64, 65, 255, 256, 257)]
    got, _ = _assert_batch(capi, R, B, clouds, _levels((3, 1)), "near sizes")
    assert len(got[-1][0]) < 257


def case_crosstalk():
    """5. a family, the same points shuffled, the first again: problems do not see each other."""
    capi, R, B = _setup()
    f = R.family("outside")
    p = f["points"]
    o = np.random.default_rng(11).permutation(len(p))
    q = np.ascontiguousarray(p[o])
    levels = _levels((2, 4))
    wp, wq = _want(R, p, levels), _want(R, q, levels)
    got, _ = _assert_batch(capi, R, B, [(p, None), (q, None), (p, None)], levels, "crosstalk", want=[wp, wq, wp])
    for l in range(len(levels)):
        assert (got[0][l] == got[2][l]).all()
    # the same base object listed twice
    base = capi.Cloud(p, None)
    got, _ = capi.level_samples_many([base, base], levels)
    for l in range(len(levels)):
        _assert_samples(got[0][l], wp[l], "listed twice"); _assert_samples(got[1][l], wp[l], "listed twice")


def case_depth_mix():
    """6. chains of several hundred steps beside shallow problems."""
    capi, R, B = _setup()
    extra = R.level_extra_inputs()
    levels = _levels((1, 2, 4))
    clouds = [(extra[k][0], None) for k in ("collinear_sorted", "planar_raster", "repeated")] + [(R.family("offset_1e4")["points"], None)]
    stats = {}
    _, within = R.level_samples(clouds[0][0], levels[0][0], stats)
    assert stats["depth"] > 100
    bases = [capi.Cloud(p, n) for p, n in clouds]
    got, rounds = capi.level_samples_many(bases, levels)
    for c, (p, _) in enumerate(clouds):
        for l, w in enumerate(_want(R, p, levels)):
            _assert_samples(got[c][l], w, ("depth mix", c, l))
    assert rounds >= 100, rounds
    print("rounds", rounds, "depth of the sorted line at level 1", stats["depth"])


def case_normals_mix():
    """7. a base with normals and one without: the first one's level has them, gathered exactly."""
    capi, R, B = _setup()
    f, g = R.family("planar"), R.family("two_far")
    levels = _levels((2,))
    bases = [capi.Cloud(f["points"], f["normals"]), capi.Cloud(g["points"], None), capi.Cloud(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))]
    made = capi.Cloud.levels_many(bases, levels)
    wf, wg = _want(R, f["points"], levels)[0], _want(R, g["points"], levels)[0]
    _assert_samples(made[0][0][1], wf, "with normals"); _assert_samples(made[1][0][1], wg, "without")
    assert made[2][0][0].n == 0
    for c, base in enumerate(bases):
        _assert_cloud(capi, B, made[c][0][0], base, levels[0][0], levels[0][1], -1.0, ("normals mix", c))
    pn = np.zeros((len(wf), 3), np.float32); nn = np.zeros((len(wf), 3), np.float32)
    capi._check(capi.load().rs_hip_cloud_points(made[0][0][0].handle, pn.ctypes.data, nn.ctypes.data))
    assert pn.tobytes() == f["points"][wf].tobytes() and nn.tobytes() == f["normals"][wf].tobytes()
    L = made[1][0][0].layout()
    assert "nor" not in L and "nor" in made[0][0][0].layout() and "nor" in made[2][0][0].layout()


def case_caps():
    """8. exactly the cap is accepted; one more refuses the whole call and names the problem; the next call is right."""
    import ctypes as C
    capi, R, B = _setup()
    room = R.family("offset_1e3")["points"]
    levels = _levels((1, 3))
    want = _want(R, room, levels)
    rc = capi.Cloud(room, None)

    def good_batch(what):
        got, _ = capi.level_samples_many([rc, rc], levels)
        for c in range(2):
            for l in range(2):
                _assert_samples(got[c][l], want[l], (what, c, l))

    def refused(call, cloud, level):
        try:
            call()
        except capi.RescanHipError as e:
            assert E_CAPACITY in str(e) and "max_n_neigh" in str(e) and f"cloud {cloud}, level {level}" in str(e), str(e)
            return True
        return False

    c256, c257 = capi.Cloud(R.cluster(256, 0.01), None), capi.Cloud(R.cluster(257, 0.01), None)
    got, _ = capi.level_samples_many([rc, c256], [(0.01, 256)])
    assert list(got[1][0]) == [0]
    _assert_samples(got[0][0], want[0], "beside the cluster")
    assert refused(lambda: capi.level_samples_many([rc, c256, c257, c257], [(0.01, 256)]), 2, 0)
    good_batch("after the sample refusal")
    # out untouched, nothing made
    bases = (C.c_void_p * 2)(rc.handle, c257.handle)
    radii = np.array([0.04, 0.01], np.float32); caps = np.array([768, 256], np.int32)
    out = (C.c_void_p * 4)(0x11, 0x22, 0x33, 0x44); counts = np.full(4, -7, np.int32)
    code = capi.load().rs_hip_cloud_create_levels_many(C.addressof(bases), 2, radii.ctypes.data, caps.ctypes.data, None, 2, C.addressof(out), None, counts.ctypes.data)
    assert code == -4 and list(out) == [0x11, 0x22, 0x33, 0x44] and (counts == -7).all()
    assert b"cloud 1, level 1" in capi.load().rs_hip_last_error()
    assert refused(lambda: capi.Cloud.levels_many([rc, c257], [(0.04, 768), (0.01, 256)]), 1, 1)
    good_batch("after the cloud refusal")
    # only the largest radius is over: the cluster's 257 points fill a ball of diameter 0.005, a ball of radius 0.001 holds fewer
    assert R.level_samples(R.cluster(257, 0.01), 0.001)[1] <= 256
    assert refused(lambda: capi.level_samples_many([rc, c257], [(0.001, 256), (0.02, 256)]), 1, 1)
    assert refused(lambda: capi.level_samples_many([c257], [(0.02, 256), (0.001, 256)]), 0, 0)
    good_batch("after the largest-radius refusal")
    got, _ = capi.level_samples_many([c257], [(0.01, 257)])
    assert list(got[0][0]) == [0]


def case_shim():
    """9. rsd_levels_poisson for levels 1-4 == four rsd_level_poisson calls."""
    import ctypes as C
    capi, R, B = _setup()
    from oracle.pyoracle import LEVEL_VOXEL
    dropin = C.CDLL(os.path.join(ROOT, "rescan_amd", "librescan_dropin.so"))
    dropin.rsd_level_poisson.restype = C.c_int32
    dropin.rsd_level_poisson.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p]
    dropin.rsd_levels_poisson.restype = C.c_int32
    dropin.rsd_levels_poisson.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    pts = np.ascontiguousarray(R.family("offset_1e3")["points"])
    voxel = np.array(LEVEL_VOXEL, np.float32)
    idx = [np.full(len(pts), -1, np.int32) for _ in range(4)]
    ptrs = (C.c_void_p * 4)(*[a.ctypes.data for a in idx]); counts = np.zeros(4, np.int32)
    assert dropin.rsd_levels_poisson(pts.ctypes.data, len(pts), voxel.ctypes.data, 1, 4, C.addressof(ptrs), counts.ctypes.data) == 0
    one = np.zeros(len(pts), np.int32)
    for k, level in enumerate((1, 2, 3, 4)):
        m = dropin.rsd_level_poisson(pts.ctypes.data, len(pts), float(voxel[level]), level, one.ctypes.data)
        assert m > 0 and m == counts[k] and (one[:m] == idx[k][:m]).all(), (level, m, counts[k])
        want, _ = R.level_samples(pts, LEVEL_VOXEL[level])
        _assert_samples(idx[k][:m], want, ("shim", level))


CASES = {f.__name__[5:]: f for f in (case_one_level, case_four_levels, case_threshold, case_sizes, case_crosstalk, case_depth_mix,
                                     case_normals_mix, case_caps, case_shim)}

# ================================================================================================================================
# pytest side
# ================================================================================================================================

@pytest.mark.parametrize("name", R_.LEVEL_FAMILIES)
def test_one_cloud_one_level(name):
    run_child("one_level", name)


def test_one_cloud_four_levels_in_caller_order_and_equal_radii():
    run_child("four_levels")


@pytest.mark.parametrize("shuffled", [0, 1])
def test_threshold_classification_on_the_exact_lattice(shuffled):
    run_child("threshold", shuffled)


def test_sizes_around_a_tile_and_a_block():
    run_child("sizes")


def test_problems_do_not_see_each_other():
    run_child("crosstalk")


def test_deep_and_shallow_problems_in_one_batch():
    run_child("depth_mix")


def test_bases_with_and_without_normals():
    run_child("normals_mix")


def test_caps_refuse_the_whole_call_and_name_the_problem():
    run_child("caps")


def test_shim_levels_equal_four_single_calls():
    run_child("shim")


if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print("ok")
