"""GPU: the two layouts of a cloud as the device build leaves them (capi.Cloud.layout(), rs_hip_cloud_layout) against the numpy
restatement of the build (tests/build_restate.py, tied to the kernels' own expressions in tests/test_hard_build_cpu.py) on the clouds
of tests/hard_builds.py and tests/hard_clouds.py.  Every comparison is equality of integers or of bits; there is no tolerance.  The
GPU work runs in child processes, each under its own time limit.  Nothing here is meant to provoke a fault: before a non-finite or far
cloud is created the test asserts, on the host, that the restated build keeps every index inside its table."""
import subprocess
import sys

import pytest

import hard_builds as H
import hard_clouds as hc
from conftest import ROOT

pytestmark = pytest.mark.gpu

PRELUDE = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from rescan_amd import capi
import build_restate as R
import hard_builds as H
import hard_clouds as hc
capi.init(0)
F = np.float32
SCALE, EXTENT_MAX = R.switches()

def check(f, what=None, keep=False):
    # every layout of the family against the restatement; returns the clouds when keep
    out = {}
    for ln, c in f["cells"]:
        cloud = capi.Cloud(f["points"], f["normals"], c)
        L = cloud.layout()
        want = R.plan(f["points"], c, f["normals"], SCALE, EXTENT_MAX)
        if want["n"] and want["inv_cell"] == 0:
            # the brute layout (asked for, or an extent that overflows a float): its occupied estimate goes through pow, so the limit
            # is held to its range and the tiling to the reported limit
            assert F(0.25) <= L["extent_limit"] <= EXTENT_MAX, (f["name"], L["extent_limit"])
            want = R.plan(f["points"], c, f["normals"], SCALE, EXTENT_MAX, limit=L["extent_limit"])
            R.assert_layout(L, want, (f["name"], ln), skip=("occupied",))
        else:
            R.assert_layout(L, want, (f["name"], ln))
        assert L["n_tiles"] == cloud.n_tiles
        if keep: out[ln] = (cloud, L)
        else: cloud.close()
    return out
"""


def run_child(body, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


@pytest.mark.parametrize("shape", H.SHAPES)
def test_layout_and_tiling_at_every_size(shape):
    """Every scalar and array of the layout, under every cell size, at the sizes around a tile (64), a block of the tiling kernels
    (256) and 4096; the tiling is the sequential greedy one; a line of points further apart than the limit has a tile per point."""
    run_child(r"""
shape = sys.argv[2]
for n in H.SIZES:
    f = H.shape(shape, n)
    got = check(f, keep=True)
    for ln, (cloud, L) in got.items():
        if shape == "stones": assert L["n_tiles"] == n, (n, ln, L["n_tiles"])
        if shape == "blob": assert L["n_tiles"] == (n + 63) // 64, (n, ln, L["n_tiles"])
        cloud.close()
print("ok")
""".replace("sys.argv[2]", repr(shape)))


def test_extent_edge_pairs():
    """Two points whose separation on one axis is exactly the extent limit share a tile (the kernel's test is a strict >); one float32
    step more and they do not."""
    run_child(r"""
probe = capi.Cloud(H.extent_pair(0.3, 0, 0), None, 0.1)
limit = probe.layout()["extent_limit"]
assert F(0.25) <= limit <= EXTENT_MAX
for axis in range(3):
    for ulps, tiles in ((0, 1), (1, 2)):
        p = H.extent_pair(limit, axis, ulps)
        c = capi.Cloud(p, None, 0.1)
        L = c.layout()
        assert L["extent_limit"].view(np.uint32) == limit.view(np.uint32), "the pair is cut with the limit it was made for"
        assert L["n_tiles"] == tiles and L["tiles"].tolist() == ([0, 2] if tiles == 1 else [0, 1, 2]), (axis, ulps, L["tiles"])
        R.assert_layout(L, R.plan(p, 0.1, None, SCALE, EXTENT_MAX), (axis, ulps))
print("ok")
""")


@pytest.mark.parametrize("name", H.CELL_EDGES)
def test_cell_edges(name):
    run_child(r"""
check(H.make(sys.argv[2]))
print("ok")
""".replace("sys.argv[2]", repr(name)))


@pytest.mark.parametrize("name", hc.FAMILIES)
def test_layout_on_the_hard_clouds(name):
    run_child(r"""
check(H.from_hc(sys.argv[2]))
print("ok")
""".replace("sys.argv[2]", repr(name)))


@pytest.mark.parametrize("name", H.HOSTILE)
def test_non_finite_and_far_clouds(name):
    """The create call succeeds, the layout is the restatement's (a point with a non-finite coordinate is stored and counted, in its
    clamped cell), every finite point finds itself, rows of 8 equal the brute force and no non-finite point is in any row."""
    run_child(r"""
f = H.make(sys.argv[2])
p = f["points"]
# on the host first: the restated build keeps every index inside its table (a regression is a failed assertion, not a device write)
mn, mx = R.bounds(p)
trials = []
R.auto_cell(p, mn, mx, SCALE, clamped=True, trace=trials)
for _, _, g, ids in trials:
    assert min(ids) >= 0 and max(ids) < g["cells"] and (max(ids) >> 5) < g["words"], sys.argv[2]
for ln, c in f["cells"]:
    P = R.plan(p, c, None, SCALE, EXTENT_MAX)                 # (asserts its cell ids and keys in range)
    assert P["n_cells"] <= R.TABLE_CELLS_MAX and (P["dims"] <= R.TABLE_DIM_MAX).all()
got = check(f, keep=True)
fin = H.finite_rows(p)
q = np.ascontiguousarray(p[fin])
for ln, (cloud, L) in got.items():
    assert L["n"] == len(p)
    back = np.zeros_like(p); capi._check(capi.load().rs_hip_cloud_points(cloud.handle, back.ctypes.data, None))
    assert back.tobytes() == p.tobytes(), "a non-finite point is still stored"
    if len(q):
        d, i, nn, tot = capi.radius_search(cloud, q, 0.05, 1)
        assert (nn == 1).all() and (d[:, 0] == 0).all(), (ln, "every finite point finds itself at distance 0", int((nn != 1).sum()), int((d[:, 0] != 0).sum()))
        # (itself, or a point whose float32 distance to it is 0 as well — coincident points, denormal offsets whose squares vanish: among
        #  equal distances the search may return any, tests/hard_clouds.py: assert_rows)
        assert fin[i[:, 0]].all() and (hc.d2_rows(p[i[:, 0]], q).diagonal() == 0).all(), (ln, "the point found is not at distance 0")
        want = hc.brute_rows(p, q, 0.05, 8)
        rows = capi.radius_search(cloud, q, 0.05, 8)
        hc.assert_rows(want, rows, p, q)
        valid = np.arange(8)[None, :] < rows[2][:, None]
        assert fin[rows[1][valid]].all(), (ln, "a non-finite point in a row")
    cloud.close()
print("ok")
""".replace("sys.argv[2]", repr(name)))


def test_device_built_clouds_have_the_layout_of_their_points():
    """Cloud.level_of, Cloud.resampled and Cloud.from_mesh index on the device what they made there: the layout is, to the byte, that
    of a cloud created from their points (and normals) with the same cell size."""
    run_child(r"""
g = dict(np.load(os.path.join(sys.argv[1], "tests", "golden", "normals_patch.npz")))
f = hc.make("planar")
base = capi.Cloud(f["points"], f["normals"])
made = []
for cell in (-1.0, 0.1, 0.0):
    made.append(("level_of", cell, capi.Cloud.level_of(base, 0.01, 256, cell)[0]))
    made.append(("resampled", cell, capi.Cloud.resampled(g["pos"], g["nor_loader"], g["faces"], cell)))
    made.append(("resampled, no normals", cell, capi.Cloud.resampled(g["pos"], None, g["faces"], cell)))
    made.append(("from_mesh", cell, capi.Cloud.from_mesh(g["pos"], g["faces"], cell)))
for what, cell, cloud in made:
    assert cloud.n > 500, (what, cloud.n)
    twin = capi.Cloud(cloud._pos, cloud._nor, cell)
    a, b = cloud.layout(), twin.layout()
    assert sorted(a) == sorted(b) and ("nor" in a) == (cloud._nor is not None)
    assert R.layout_bytes(a) == R.layout_bytes(b), (what, cell, [k for k in a if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()])
    cloud.close(); twin.close()
print("ok")
""")


def test_repeats_give_the_same_bytes():
    """The same cloud twice, and large / small / large (the workspace's bit table and scratch arrays are reused, and the doubling
    rounds mark concurrently): the layouts are equal to the byte."""
    run_child(r"""
big, small = hc.make("contrast"), H.extent_pair(0.3, 1, 1)
for cell in (-1.0, 0.1):
    a = capi.Cloud(big["points"], big["normals"], cell); La = R.layout_bytes(a.layout())
    b = capi.Cloud(big["points"], big["normals"], cell); Lb = R.layout_bytes(b.layout())
    assert La == Lb, ("twice", cell)
    s = capi.Cloud(small, None, cell); Ls = s.layout()
    R.assert_layout(Ls, R.plan(small, cell, None, SCALE, EXTENT_MAX), ("small after large", cell))
    c = capi.Cloud(big["points"], big["normals"], cell); Lc = R.layout_bytes(c.layout())
    assert Lc == La, ("large, small, large", cell)
    assert R.layout_bytes(a.layout()) == La, "reading a layout changes nothing"
    for x in (a, b, c, s): x.close()
print("ok")
""")
