"""GPU: capi.Cloud.many (rs_hip_cloud_create_many) against the single build and against the numpy restatement of the build
(tests/build_restate.py) on the clouds of tests/hard_builds.py and tests/hard_clouds.py.  For every cloud of every batch: the layout
is, to the byte, that of capi.Cloud on the same points, normals and cell size; it is the restatement's; the host copies, the number
of tiles and the reported size are equal.  Every comparison is equality of integers or of bits; there is no tolerance.  The GPU work
runs in child processes, each under its own time limit.  Nothing here is meant to provoke a fault: every input is a cloud the
single build already takes, and before a non-finite or far cloud is created the test asserts, on the host, that the restated build
keeps every index inside its table."""
import subprocess
import sys

import pytest

import hard_builds as H
from conftest import ROOT

pytestmark = pytest.mark.gpu

PRELUDE = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from rescan_amd import capi
import build_restate as R
import hard_builds as H
import hard_clouds as hc
capi.init(0)
F = np.float32
SCALE, EXTENT_MAX = R.switches()
lib = capi.load()

def points_of(cloud):
    pos = np.zeros((cloud.n, 3), F); nor = np.zeros((cloud.n, 3), F) if cloud._nor is not None else None
    capi._check(lib.rs_hip_cloud_points(cloud.handle, pos.ctypes.data, None if nor is None else nor.ctypes.data))
    return pos.tobytes() + (b"" if nor is None else nor.tobytes())

def restated(L, p, nor, c, what):
    # the layout against the numpy restatement (the brute layout as check() of tests/test_gpu_hard_build.py takes it)
    want = R.plan(p, c, nor, SCALE, EXTENT_MAX)
    if want["n"] and want["inv_cell"] == 0:
        assert F(0.25) <= L["extent_limit"] <= EXTENT_MAX, (what, L["extent_limit"])
        want = R.plan(p, c, nor, SCALE, EXTENT_MAX, limit=L["extent_limit"])
        R.assert_layout(L, want, what, skip=("occupied",))
    else:
        R.assert_layout(L, want, what)

def same_as_single(cloud, L, p, nor, c, what, single=None):
    # the batch's cloud against capi.Cloud on the same arguments; returns the single build's layout bytes
    one = single if single is not None else capi.Cloud(p, nor, c)
    S = one.layout()
    assert sorted(L) == sorted(S), what
    a, b = R.layout_bytes(L), R.layout_bytes(S)
    assert a == b, (what, [k for k in L if np.asarray(L[k]).tobytes() != np.asarray(S[k]).tobytes()])
    assert cloud.n == one.n and cloud.n_tiles == one.n_tiles == L["n_tiles"] and cloud.nbytes == one.nbytes, (what, cloud.n_tiles, one.n_tiles, cloud.nbytes, one.nbytes)
    assert points_of(cloud) == points_of(one) == (p.tobytes() + (b"" if nor is None else nor.tobytes())), (what, "host copies")
    if single is None: one.close()
    return b

def check_batch(items, what, restate=True, single_every=1, cells="list", whole_nor=True, keep=False):
    # items: (points, normals or None, cell size).  Every cloud against the restatement, every single_every-th against its single build.
    pairs = [(p, n) for p, n, c in items]
    many = capi.Cloud.many(pairs, [c for _, _, c in items]) if cells == "list" else capi.Cloud.many(pairs) if cells is None else capi.Cloud.many(pairs, cells)
    assert len(many) == len(items)
    out = []
    for k, ((p, n, c), cloud) in enumerate(zip(items, many)):
        L = cloud.layout()
        assert ("nor" in L) == (n is not None), (what, k)
        if restate: restated(L, p, n, c, (what, k))
        b = same_as_single(cloud, L, p, n, c, (what, k)) if k % single_every == 0 else R.layout_bytes(L)
        out.append(b)
    if keep: return many, out
    for cloud in many: cloud.close()
    return out
"""


def run_child(body, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


@pytest.mark.parametrize("shape", H.SHAPES)
def test_every_size_under_every_cell_in_one_batch(shape):
    """One batch of every size around a tile (64), a block (256) and 4096, each under each cell size of the shape: empty clouds
    first (the four of size 0), in the middle and last, the single-point clouds next to each other.  The same batch reversed gives
    every cloud the same bytes: they do not depend on its place."""
    run_child(r"""
shape = sys.argv[2]
items = []
for n in H.SIZES:
    f = H.shape(shape, n)
    items += [(f["points"], f["normals"], c) for _, c in f["cells"]]
empty = np.zeros((0, 3), F)
items.insert(len(items) // 2, (empty, None, -1.0)); items.append((empty, None, 0.1))
assert [len(p) for p, _, _ in items[:4]] == [0] * 4 and [len(p) for p, _, _ in items[4:8]] == [1] * 4 and len(items[-1][0]) == 0
fwd = check_batch(items, shape)
many = capi.Cloud.many([(p, n) for p, n, c in reversed(items)], [c for _, _, c in reversed(items)])
back = [R.layout_bytes(c.layout()) for c in many]
assert back == fwd[::-1], [k for k in range(len(fwd)) if back[k] != fwd[::-1][k]]
for c in many: c.close()
print("ok")
""".replace("sys.argv[2]", repr(shape)))


def test_mixed_normals_and_cells():
    """Clouds with and without normals and auto, 0.1 and brute cells in one batch; no normals for the whole call (nor == NULL); no
    cell sizes (cell_sizes == NULL)."""
    run_child(r"""
fams = [hc.make("planar"), H.make("cell_edges"), H.shape("clusters", 257), hc.make("contrast"), H.make("coincident"), H.shape("stones", 129)]
assert any(f["normals"] is not None for f in fams) and any(f["normals"] is None for f in fams)
items = [(f["points"], f["normals"], c) for k, f in enumerate(fams) for c in ((-1.0, 0.1, 0.0)[k % 3], (0.1, 0.0, -1.0)[k % 3])]
check_batch(items, "mixed")
bare = [(p, None, c) for p, _, c in items[:6]]
check_batch(bare, "nor == NULL")
auto = [(p, n, -1.0) for p, n, _ in items[:6]]
check_batch(auto, "cell_sizes == NULL", cells=None)
check_batch([(p, n, 0.1) for p, n, _ in items[:4]], "one cell size for all", cells=0.1)
print("ok")
""")


@pytest.mark.parametrize("name", H.HOSTILE)
def test_a_hostile_cloud_between_two_clean_ones(name):
    """A non-finite, denormal or far cloud between two copies of a clean one: the clean copies have the bytes of the clean cloud built
    alone, the hostile one those of its own single build, and rows of 8 over its finite points equal the brute force."""
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
clean = H.shape("clusters", 257)
fin = H.finite_rows(p)
q = np.ascontiguousarray(p[fin])
alone = {}
for ln, c in f["cells"]:
    if c not in alone:
        one = capi.Cloud(clean["points"], None, c); alone[c] = R.layout_bytes(one.layout()); one.close()
    items = [(clean["points"], None, c), (p, f["normals"], c), (clean["points"], None, c)]
    many, got = check_batch(items, (sys.argv[2], ln), keep=True)
    assert got[0] == alone[c] and got[2] == alone[c], (ln, "the clean cloud's bytes depend on its neighbour")
    if len(q):
        want = hc.brute_rows(p, q, 0.05, 8)
        rows = capi.radius_search(many[1], q, 0.05, 8)
        hc.assert_rows(want, rows, p, q)
        valid = np.arange(8)[None, :] < rows[2][:, None]
        assert fin[rows[1][valid]].all(), (ln, "a non-finite point in a row")
    for c_ in many: c_.close()
print("ok")
""".replace("sys.argv[2]", repr(name)))


def test_trial_attempts_that_differ():
    """One batch holds a cloud whose cell is decided by the first trial grid, one that is coarsened several times and one whose first
    grids are too fine to count: the clouds leave the lock-step attempts at different times, and each equals its single build."""
    run_child(r"""
far = H.make("far_1e10")
nearer = dict(far, points=far["points"].copy()); nearer["points"][3, 0] = F(1e6)      # the same box, its far point at 1e6 instead of 1e10
fams = [H.make("coincident"), H.shape("stones", 4096), far, nearer]
traces = []
for f in fams:
    t = []
    R.auto_cell(f["points"], *R.bounds(f["points"]), SCALE, clamped=True, trace=t)
    traces.append([a for a, _, _, _ in t])
    # on the host first, as for the hostile clouds: every trial cell inside its bit table, every cell id and key inside its range
    for _, _, g, ids in t:
        assert min(ids) >= 0 and max(ids) < g["cells"] and (max(ids) >> 5) < g["words"], f["name"]
    P = R.plan(f["points"], -1.0, None, SCALE, EXTENT_MAX)
    assert P["n_cells"] <= R.TABLE_CELLS_MAX and (P["dims"] <= R.TABLE_DIM_MAX).all()
first, several, never, late = traces
assert first == [0], first                                       # decided at the first attempt
assert several[0] == 0 and len(several) >= 3, several            # counted from the first attempt on, coarsened at least twice
assert never == [], never                                        # no grid is countable: decided at the last attempt, without a count
assert late and late[0] >= 1, late                               # the first grids are not countable, a later one is
assert len({tuple(t) for t in traces}) == 4
for order in ((0, 1, 2, 3), (3, 2, 0, 1), (1, 3, 2, 0)):
    check_batch([(fams[k]["points"], fams[k]["normals"], -1.0) for k in order], ("attempts", order), restate=order == (0, 1, 2, 3))
print("ok")
""")


def test_many_tiny_clouds():
    """1500 clouds of 1 .. 5 points, some coincident, some on cell edges: more clouds than a block of any per-cloud kernel has lanes,
    several times over.  Every cloud against the restatement, every 50th against its single build as well."""
    run_child(r"""
rng = np.random.default_rng(5)
edges = np.concatenate([H.make(k)["points"] for k in H.CELL_EDGES])
cells = (-1.0, 0.1, 0.25, 0.0)
items = []
for k in range(1500):
    n = 1 + k % 5
    kind = k % 3
    if kind == 0: p = edges[rng.integers(0, len(edges), n)]
    elif kind == 1: p = np.tile(edges[rng.integers(0, len(edges))], (n, 1))          # coincident
    else: p = rng.uniform(-1.0, 1.0, (n, 3)).astype(F)
    nor = hc._unit(rng, n) if k % 4 == 1 else None
    items.append((np.ascontiguousarray(p, F), nor, cells[(k // 5) % 4]))
check_batch(items, "tiny", single_every=50)
print("ok")
""", limit=240)


def test_both_routes_give_the_same_bytes():
    """With the threshold at 100 a batch of sizes 64 .. 4096 takes the batched and the single route in one call, at 0 every cloud is
    built alone: the bytes are those of the default.  A batch of one equals the single build.  The setter is restored."""
    run_child(r"""
items = []
for n in (64, 65, 100, 101, 255, 257, 4096):
    f = H.shape("clusters", n)
    items += [(f["points"], None, c) for c in (-1.0, 0.1)]
default = capi.cloud_many_single_above()
want = check_batch(items, "default")
try:
    for limit in (100, 0):
        assert capi.cloud_many_single_above(limit) in (default, 100)
        got = check_batch(items, ("single above", limit), restate=False, single_every=5)
        assert got == want, limit
finally:
    capi.cloud_many_single_above(default)
assert capi.cloud_many_single_above() == default
for p, n, c in items[-2:]:
    check_batch([(p, n, c)], "a batch of one")
print("ok")
""")


def test_lifetime_of_the_shared_allocation():
    """A batch of 8; clouds 0, 2, 4 and 6 are closed, an unrelated large cloud is created (freed memory would be reused): the remaining
    layouts are unchanged to the byte and their searches still right.  The rest is closed in reverse order.  The same batch again gives
    the same bytes (the workspaces are reused)."""
    run_child(r"""
fams = [hc.make(k) for k in ("planar", "contrast", "lattice", "negative")] + [H.shape(s, n) for s, n in (("blob", 4097), ("clusters", 4095), ("stones", 257), ("clusters", 65))]
items = [(f["points"], f["normals"], (-1.0, 0.1)[k % 2]) for k, f in enumerate(fams)]
many, first = check_batch(items, "batch of 8", keep=True)
for k in (0, 2, 4, 6): many[k].close()
rng = np.random.default_rng(3)
big = capi.Cloud(rng.uniform(0.0, 4.0, (400000, 3)).astype(F), None, -1.0)
for k in (1, 3, 5, 7):
    assert R.layout_bytes(many[k].layout()) == first[k], k
    p = items[k][0]; q = np.ascontiguousarray(p[:: max(1, len(p) // 256)])
    hc.assert_rows(hc.brute_rows(p, q, 0.05, 8), capi.radius_search(many[k], q, 0.05, 8), p, q)
for k in (7, 5, 3, 1): many[k].close()
big.close()
again = check_batch(items, "the same batch again", restate=False, single_every=4)
assert again == first
print("ok")
""")


def test_refusals_leave_out_untouched():
    """n_clouds < 0, a negative n[k], points without an array and out == NULL are refused with RS_HIP_E_ARG and `out` stays as it
    was; a batch of no clouds is RS_HIP_OK."""
    run_child(r"""
fn = lib.rs_hip_cloud_create_many
pts = np.zeros((4, 3), F)
pos = (C.c_void_p * 2)(pts.ctypes.data, pts.ctypes.data)
out = (C.c_void_p * 2)(0x1234, 0x5678)
def call(pos_, n_, k, out_):
    n_ = (C.c_int32 * 2)(*n_)
    return fn(C.addressof(pos_), None, C.addressof(n_), None, k, None if out_ is None else C.addressof(out_))
assert call(pos, (4, 4), -1, out) == -2 and b"create_many" in lib.rs_hip_last_error()
assert call(pos, (4, -1), 2, out) == -2
assert call((C.c_void_p * 2)(pts.ctypes.data, None), (4, 4), 2, out) == -2
assert call(pos, (4, 4), 2, None) == -2
assert call(pos, (4, 4), 0, out) == 0
assert out[0] == 0x1234 and out[1] == 0x5678
assert capi.Cloud.many([]) == []
# ... and an empty cloud may come without an array
a, b = capi.Cloud.many([(pts, None), (np.zeros((0, 3), F), None)])
assert call((C.c_void_p * 2)(pts.ctypes.data, None), (4, 0), 2, out) == 0
made = [capi.Cloud.__new__(capi.Cloud), capi.Cloud.__new__(capi.Cloud)]
for k, c in enumerate(made): c.handle = out[k]; c.n = (4, 0)[k]; c._pos = pts[:c.n]; c._nor = None
assert R.layout_bytes(made[0].layout()) == R.layout_bytes(a.layout()) and R.layout_bytes(made[1].layout()) == R.layout_bytes(b.layout())
print("ok")
""")


def test_split_objects_are_the_clouds_of_their_points():
    """Cloud.split_objects on the fixtures of tests/golden/split_*.npz: every object's layout is that of a cloud created from its
    points and normals with the same cell size (this holds before the batched build too: it pins that the consumers did not change)."""
    run_child(r"""
import hard_split as HS
def golden(name): return dict(np.load(os.path.join(sys.argv[1], "tests", "golden", f"split_{name}.npz")))
g = golden("room"); cases = [("room", g["scan_pos"], g["scan_nor"], g["scan_cls"], g["scan_inst"], g["static_classes"])]
q = golden("quirks")
for name in q["names"].tolist():
    s = f"case_{name}_scan_"
    cases.append((name, q[s + "pos"], q[s + "nor"], q[s + "cls"], q[s + "inst"], q["static_classes"]))
h = golden("hostile")
for name in h["names"].tolist():
    pos, nor, cls, inst = HS.scan(name)
    if np.isfinite(pos).all() and np.abs(pos).max() < 2.0 ** 24: cases.append((name, pos, nor, cls, inst, h["static_classes"]))
made = 0
for name, pos, nor, cls, inst, static in cases:
    scan = capi.Cloud(pos, nor)
    for cell in (-1.0, 0.1):
        clouds, info = scan.split_objects(cls, inst, static, cell)
        for k, c in enumerate(clouds):
            same_as_single(c, c.layout(), c._pos, c._nor, cell, (name, cell, k)); made += 1
            c.close()
    scan.close()
assert made > 20, made
print("ok")
""")


def test_fused_arrangement_results_are_the_clouds_of_their_points():
    """The same for every result of Cloud.fuse_arrangement on tests/golden/fuse_arrangement.npz."""
    run_child(r"""
g = dict(np.load(os.path.join(sys.argv[1], "tests", "golden", "fuse_arrangement.npz")))
made = 0
for cell in (-1.0, 0.1):
    scan = capi.Cloud(g["scan_pos"], g["scan_nor"])
    pls = []
    for p in range(len(g["uidx"])):
        frm = int(g["model_from"][p])
        pls.append(dict(uidx=int(g["uidx"][p]), pose=g["poses"][p], refine=not int(g["is_static"][p]), model_from=frm,
                        model=capi.Cloud(g[f"p{p}_model_pos"], g[f"p{p}_model_nor"]) if frm < 0 else None))
    res = capi.Cloud.fuse_arrangement(scan, g["scan_inst"], pls, max_dist=float(g["max_dist"]), max_angle=float(g["max_angle"]), cell_size=cell)
    for k, (c, info) in enumerate(res):
        if c is None: continue
        same_as_single(c, c.layout(), c._pos, c._nor, cell, ("fused", cell, k)); made += 1
        c.close()
assert made >= 2, made
print("ok")
""")
