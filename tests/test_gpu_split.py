"""GPU: rs_hip_instance_table, rs_hip_split_by_instance, rs_hip_scan_to_objects, rs_hip_cloud_split_objects and rsd_scan_to_objects
against the reference's fixtures (tests/golden/split_*.npz) and against the host plan that reproduces them (rs_hip_split_plan, checked
in tests/test_split_cpu.py), bit for bit, on both routes of the partition; the partition against rs_hip_select_by_ids per id; tile,
wave and instance-count edges.  The GPU work runs in child processes, each under its own time limit; nothing here provokes a fault:
every refusal is decided on the host or from the table, before a launch that could depend on it.

The streams of the hostile fixture with an Inf or NaN coordinate, and the two whose coordinates reach 2^30 and 2^40 (tie, cancel), go
through rs_hip_scan_to_objects only: rs_hip_cloud_create's grid counts its cells in an int and is not defined on coordinates that are
not finite, so no such scan cloud is made here (`indexable` in cases())."""
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PRELUDE = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from rescan_amd import capi
import split_restate as R
import hard_split as H
capi.init(0)
KEYS = R.KEYS
LAY = capi.split_layout()
T, LDS, MAXI = LAY["tile"], LAY["lds_ranks"], LAY["max_instances"]
def golden(name): return dict(np.load(os.path.join(sys.argv[1], "tests", "golden", f"split_{name}.npz")))
def cases():
    # (name, pos, nor, cls, inst, static classes, finite) of every fixture case
    g = golden("room"); out = [("room", g["scan_pos"], g["scan_nor"], g["scan_cls"], g["scan_inst"], g["static_classes"], True)]
    q = golden("quirks")
    for name in q["names"].tolist():
        p = f"case_{name}_scan_"
        out.append((name, q[p + "pos"], q[p + "nor"], q[p + "cls"], q[p + "inst"], q["static_classes"], True))
    h = golden("hostile")
    for name in h["names"].tolist():
        pos, nor, cls, inst = H.scan(name)
        assert R.same_bits(pos, h[f"stream_{name}_pos"])
        out.append((name, pos, nor, cls, inst, h["static_classes"], bool(np.isfinite(pos).all() and np.abs(pos).max() < 2.0 ** 24)))
    return out
PLAN_KEYS = ("inst_ids", "counts", "first", "offsets", "order", "class_of", "is_static", "sums", "centroids", "xforms", "poses")
def same(got, want, what, points=True):
    assert got["n_instances"] == want["n_instances"], what
    for k in PLAN_KEYS + (("out_pos", "out_nor") if points else ()):
        assert R.same_bits(got[k], want[k]), (what, k)
def both_routes(fn):
    # fn() on the LDS route and on the sort route; the setter is back at its default afterwards
    out = []
    for ranks in (LDS, 0):
        before = capi.split_lds_ranks(ranks)
        try:
            out.append(fn())
        finally:
            capi.split_lds_ranks(before)
    return out
def by_selection(ids):
    # (inst_ids, offsets, order) from rs_hip_select_by_ids, one id at a time, in order of first appearance
    inst = R.table(ids)[0]
    segs = [capi.select_by_ids(ids, [int(v)]) for v in inst]
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    return inst, off, (np.concatenate(segs) if segs else np.zeros(0, np.int32)).astype(np.int32)
"""


def run_child(body, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


def test_every_fixture_through_scan_to_objects_on_both_routes():
    """Against the plan, bit for bit (the plan against the fixtures: tests/test_split_cpu.py, test_hard_split_cpu.py), and against the
    fixtures' transformed arrays directly.  The room's chains are all order-free; the cancellation stream's are not."""
    run_child(r"""
room, quirks, hostile = golden("room"), golden("quirks"), golden("hostile")
for name, pos, nor, cls, inst, static, finite in cases():
    want = capi.split_plan(pos, nor, cls, inst, static)
    for got in both_routes(lambda: capi.scan_to_objects(pos, nor, cls, inst, static)):
        same(got, want, name)
        fx = room["out_pos"] if name == "room" else quirks[f"case_{name}_out_pos"] if f"case_{name}_out_pos" in quirks else hostile[f"stream_{name}_out_pos"]
        assert R.same_bits(got["out_pos"], fx), name
    seq = capi.split_chains_sequential()
    if name == "room": assert seq == 0, seq
    if name == "cancel": assert seq > 0
    # the other five arrays follow through order and the device gather
    got = capi.scan_to_objects(pos, nor, cls, inst, static)
    ids2 = capi.gather_attributes(got["order"], [inst])[0]
    assert (ids2 == np.repeat(got["inst_ids"], got["counts"])).all(), name
# without normals: positions alone
g = room
got = capi.scan_to_objects(g["scan_pos"], None, g["scan_cls"], g["scan_inst"], g["static_classes"])
assert R.same_bits(got["out_pos"], g["out_pos"]) and "out_nor" not in got
print("ok")
""")


def test_every_finite_fixture_through_cloud_split_objects():
    run_child(r"""
for name, pos, nor, cls, inst, static, finite in cases():
    if not finite: continue
    want = capi.split_plan(pos, nor, cls, inst, static)
    scan = capi.Cloud(pos, nor)
    for clouds, info in both_routes(lambda: scan.split_objects(cls, inst, static)):
        same(info, want, name, points=False)
        assert [c.n for c in clouds] == want["counts"].tolist(), name
        got_pos = np.concatenate([c._pos for c in clouds]); got_nor = np.concatenate([c._nor for c in clouds])
        assert R.same_bits(got_pos, want["out_pos"]) and R.same_bits(got_nor, want["out_nor"]), name
        for c in clouds: c.close()
    scan.close()
# an object made this way is a cloud like any other: a search on the chair finds its own points
g = golden("room")
scan = capi.Cloud(g["scan_pos"], g["scan_nor"])
clouds, info = scan.split_objects(g["scan_cls"], g["scan_inst"], g["static_classes"])
chair = clouds[0]
d, i, nn, tot = capi.radius_search(chair, chair._pos[:64], 0.02, 4)
assert (nn >= 1).all() and (d[:, 0] == 0).all() and (i[:, 0] == np.arange(64)).all()
print("ok")
""")


def test_table_and_partition_against_select_by_ids():
    run_child(r"""
for name, pos, nor, cls, inst, static, finite in cases():
    want = R.table(inst)
    got = capi.instance_table(inst)
    assert all((a == b).all() and a.dtype == b.dtype for a, b in zip(got, want)), name
    sel = by_selection(inst)
    for got in both_routes(lambda: capi.split_by_instance(inst)):
        assert all((a == b).all() for a, b in zip(got, sel)), name
print("ok")
""")


def test_tile_and_wave_edges():
    """n around a wave, a tile and two tiles; one id, two ids alternating, ids that change exactly at a wave or tile boundary with one
    point after it, a run that spans three tiles — each on both routes, against a plain selection per id.  A partition that is stable
    only inside a wave or a tile fails here."""
    run_child(r"""
def patterns(n):
    k = np.arange(n)
    yield "one", np.full(n, 7)
    yield "alternating", np.where(k % 2 == 0, -5, 9)
    for b in (64, T):
        yield f"change_at_{b}", np.where(k < b, 3, np.where(k == b, 8, 3))          # a new id at the boundary, the old one after it
        yield f"blocks_of_{b}", (k // b) % 3 - 1                                      # ids change exactly at every boundary, and return
    yield "three_tiles", np.where((k >= T // 2) & (k < T // 2 + 3 * T), 1, np.where(k % 3 == 0, 2, 0))
for n in (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 4 * T + 5):
    for what, ids in patterns(n):
        ids = ids.astype(np.int32)
        inst, counts, first = R.table(ids)
        want_order = np.concatenate([np.flatnonzero(ids == v) for v in inst]).astype(np.int32) if n else np.zeros(0, np.int32)
        for got in both_routes(lambda: capi.split_by_instance(ids)):
            assert (got[0] == inst).all() and (got[1] == np.concatenate([[0], np.cumsum(counts)])).all() and (got[2] == want_order).all(), (n, what)
        t = capi.instance_table(ids)
        assert (t[0] == inst).all() and (t[1] == counts).all() and (t[2] == first).all(), (n, what)
print("ok")
""")


def test_instance_counts_around_the_routes_and_the_cap():
    """lds_ranks - 1, lds_ranks, lds_ranks + 1 and max_instances distinct ids pass on whichever route serves them; max_instances + 1 are
    refused with the outputs untouched."""
    run_child(r"""
rng = np.random.default_rng(7)
for count in (LDS - 1, LDS, LDS + 1, MAXI):
    n = count + 3 * T + 17
    ids = (rng.permutation(n) % count).astype(np.int32) * 7 - 1000        # every id present, in no order
    inst, counts, first = R.table(ids)
    assert len(inst) == count
    lut = {int(v): k for k, v in enumerate(inst)}
    rank = np.array([lut[int(v)] for v in ids])
    want_order = np.argsort(rank, kind="stable").astype(np.int32)
    for got in both_routes(lambda: capi.split_by_instance(ids)):
        assert (got[0] == inst).all() and (got[2] == want_order).all(), count
    pos = rng.uniform(-1, 1, (n, 3)).astype(np.float32); cls = np.full(n, 5, np.int32)
    same(capi.scan_to_objects(pos, pos, cls, ids, (1, 2, 0)), capi.split_plan(pos, pos, cls, ids, (1, 2, 0)), count)
# one too many: refused, nothing written
n = MAXI + 1
ids = np.arange(n, dtype=np.int32)[::-1].copy()
lib = capi.load()
inst = np.full(n, -7, np.int32); counts = np.full(n, -7, np.int64); first = np.full(n, -7, np.int64); order = np.full(n, -7, np.int32); off = np.full(n + 1, -7, np.int64)
k = C.c_int32(-7)
assert lib.rs_hip_instance_table(ids.ctypes.data, n, inst.ctypes.data, counts.ctypes.data, first.ctypes.data, C.byref(k)) == -4 and b"distinct" in lib.rs_hip_last_error()
assert lib.rs_hip_split_by_instance(ids.ctypes.data, n, inst.ctypes.data, off.ctypes.data, order.ctypes.data, C.byref(k)) == -4
assert k.value == -7 and all((a == -7).all() for a in (inst, counts, first, order, off))
pos = np.zeros((n, 3), np.float32); cls = np.zeros(n, np.int32)
try:
    capi.scan_to_objects(pos, pos, cls, ids, ())
    raise SystemExit("max_instances + 1 ids were not refused")
except capi.RescanHipError as e:
    assert "distinct" in str(e)
# and the library still works after the refusal
assert capi.instance_table(ids[:5])[0].tolist() == ids[:5].tolist()
print("ok")
""")


def test_two_runs_give_identical_bytes_and_the_shim_agrees():
    run_child(r"""
g = golden("room")
args = (g["scan_pos"], g["scan_nor"], g["scan_cls"], g["scan_inst"], g["static_classes"])
a, b = capi.scan_to_objects(*args), capi.scan_to_objects(*args)
for k in PLAN_KEYS + ("out_pos", "out_nor"):
    assert a[k].tobytes() == b[k].tobytes(), k
h = golden("hostile")
for name in ("cancel", "range", "one_nan"):
    x = H.scan(name)
    a, b = capi.scan_to_objects(*x, ()), capi.scan_to_objects(*x, ())
    for k in PLAN_KEYS + ("out_pos", "out_nor"):
        assert a[k].tobytes() == b[k].tobytes(), (name, k)
# the lone-lane form of the chains gives the same doubles
before = capi.split_chains_form(1)
try:
    c = capi.scan_to_objects(*args)
finally:
    capi.split_chains_form(before)
assert c["sums"].tobytes() == capi.scan_to_objects(*args)["sums"].tobytes()
# the shim, on the device
d = C.CDLL(os.path.join(sys.argv[1], "rescan_amd", "librescan_dropin.so"))
f = d.rsd_scan_to_objects
f.restype = C.c_int32
f.argtypes = [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 8
n = len(g["scan_pos"]); static = np.ascontiguousarray(g["static_classes"])
inst = np.zeros(8, np.int32); cls = np.zeros(8, np.int32); off = np.zeros(9, np.int64); order = np.zeros(n, np.int32)
pos = np.zeros((n, 3), np.float32); nor = np.zeros((n, 3), np.float32); x = np.zeros((8, 16), np.float32); p = np.zeros((8, 16), np.float32)
assert f(*[g["scan_" + k].ctypes.data for k in ("pos", "nor", "cls", "inst")], n, static.ctypes.data, len(static), 8,
         *[v.ctypes.data for v in (inst, cls, off, order, pos, nor, x, p)]) == 4
d.rsd_device_failures.restype = C.c_ulonglong
assert d.rsd_device_failures() == 0
assert R.same_bits(pos, g["out_pos"]) and R.same_bits(nor, g["out_nor"]) and R.same_bits(p[:4], g["poses"]) and (inst[:4] == g["inst_ids"]).all()
print("ok")
""")
