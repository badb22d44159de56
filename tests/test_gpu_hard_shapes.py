"""GPU: rs_hip_overlap_factors and rs_hip_nms on the hostile shapes of tests/hard_shapes.py — grid widths around every word
seam up to the 4096-cell limit, walls and combs on the seams, boundary in the first and last cell of every axis, tiny and empty
clouds, one call that mixes disjoint, LDS-route and global-route pairs — IDENTICALLY to the reference's numbers in
tests/golden/isect_hard.npz (int32 counts, float32 overlap bits, marks) at four LDS budgets: the default, 0 (every pair through
global memory), the exact byte size of one pair's planes, and that size minus 4.  The seeded "random" family is compared with
tests/isect_restate.py, which tests/test_hard_shapes_cpu.py holds against the same fixture.
The GPU work runs in child processes, each under its own time limit; nothing here provokes a fault: the refusals are decided on
the host from the boxes, or flagged by the kernel's own in-bounds check.
Not tested: the chunking of the global route's slab beyond 256 MB of planes in one launch — it would need grids far too large for a
test of a few seconds."""
import subprocess
import sys
import time

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PRELUDE = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from rescan_amd import capi
import hard_shapes as H, isect_restate as R
capi.init(0)
G = dict(np.load(os.path.join(sys.argv[1], "tests", "golden", "isect_hard.npz")))
DEFAULT = 61440
def bits(a): return np.ascontiguousarray(a, np.float32).view(np.uint32)
def clouds(c): return [(capi.Cloud(b, None, 0.0), capi.Cloud(e, None, 0.0)) for b, e in c.shapes]
def rows(j): return slice(int(G["case_first"][j]), int(G["case_first"][j + 1]))
def run(c, cl, sel=slice(None)):
    return capi.overlap_factors(cl, c.ia[sel], c.pose_a[sel], c.ib[sel], c.pose_b[sel], c.voxel, c.inside, c.by_smaller)
def fit_of(c, k):
    ba, bb = R.box(c.pose_a[k], c.shapes[c.ia[k]][1]), R.box(c.pose_b[k], c.shapes[c.ib[k]][1])
    return H.plane_bytes(R.grid_of(ba, bb, c.voxel)[1], c.inside) if R.boxes_intersect(ba, bb) else 0
def raw(c, cl, fill=-7):
    L = capi.load(); arr = capi._isect_shapes(cl); n = len(c)
    ov = np.full(n, fill, np.float32); cnt = np.full((n, 3), fill, np.int32)
    rc = L.rs_hip_overlap_factors(C.addressof(arr), len(cl), c.ia.ctypes.data, c.pose_a.ctypes.data, c.ib.ctypes.data, c.pose_b.ctypes.data, n,
                                  float(c.voxel), int(c.inside), int(c.by_smaller), ov.ctypes.data, cnt.ctypes.data)
    return rc, ov, cnt, L.rs_hip_last_error().decode()
"""


def run_child(body, limit=240):
    t0 = time.perf_counter()
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True)
    print(f"child: {time.perf_counter() - t0:.2f} s")
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


def test_every_fixture_row_at_four_budgets():
    run_child(r"""
cases = H.fixture_cases()
assert [c.name for c in cases] == [n.decode() for n in G["case_name"]]
seen = 0
for j, c in enumerate(cases):
    assert (c.crcs() == G["shape_crc"][G["shape_first"][j]:G["shape_first"][j + 1]]).all(), c.name      # the clouds the reference saw
    if c.expect != "ok":
        continue
    cl = clouds(c)
    fit = next(f for f in (fit_of(c, k) for k in range(len(c))) if f)
    want_cnt, want_ov = G["counts"][rows(j)], G["overlap"][rows(j)]
    for budget in (DEFAULT, 0, fit, fit - 4):
        capi.isect_lds_budget(budget)
        ov, cnt = run(c, cl)
        assert cnt.dtype == np.int32 and (cnt == want_cnt).all(), (c.name, budget, np.flatnonzero((cnt != want_cnt).any(1))[:8], cnt[(cnt != want_cnt).any(1)][:3], want_cnt[(cnt != want_cnt).any(1)][:3])
        assert (bits(ov) == bits(want_ov)).all(), (c.name, budget)
        ov2, cnt2 = run(c, cl)
        assert (cnt2 == cnt).all() and (bits(ov2) == bits(ov)).all(), (c.name, budget)                # two calls, identical bits
    seen += len(c)
capi.isect_lds_budget(DEFAULT)
assert seen == int((G["case_reference"][np.searchsorted(G["case_first"], np.arange(len(G["overlap"])), "right") - 1] == 1).sum())
print("ok")
""")


def test_routes_call_equals_its_pairs_sent_alone():
    run_child(r"""
cases = H.fixture_cases()
j = [c.name for c in cases].index("routes"); c = cases[j]; cl = clouds(c)
named = fit_of(c, H.ROUTES_NAMED)
assert 0 < named <= DEFAULT
for budget in (DEFAULT, named, named - 4):
    capi.isect_lds_budget(budget)
    ov, cnt = run(c, cl)                                          # ONE call: disjoint, LDS, global, LDS, disjoint, ...
    assert (cnt == G["counts"][rows(j)]).all() and (bits(ov) == bits(G["overlap"][rows(j)])).all(), budget
    for k in range(len(c)):                                       # a batch of one agrees with its row of the batch
        o1, c1 = run(c, cl, slice(k, k + 1))
        assert (c1[0] == cnt[k]).all() and bits(o1)[0] == bits(ov[k:k + 1])[0], (budget, k)
capi.isect_lds_budget(DEFAULT)
print("ok")
""")


def test_nms_list_is_the_references():
    run_child(r"""
lib = C.CDLL(os.path.join(sys.argv[1], "rescan_amd", "librescan_dropin.so"))
vp, i32, f = C.c_void_p, C.c_int32, C.c_float
lib.rsd_non_maxima_suppression.restype = C.c_int
lib.rsd_non_maxima_suppression.argtypes = [vp, i32, vp, i32, vp, vp, vp, i32, f, vp, vp, vp]
L = H.nms_list()
assert (G["nms_shape_crc"] == [len(L["shape"][0]), H.crc(L["shape"][0]), len(L["shape"][1]), H.crc(L["shape"][1])]).all()
shape = (capi.Cloud(L["shape"][0], None, 0.0), capi.Cloud(L["shape"][1], None, 0.0))
cen, poses, scores, thr, want = G["nms_centroid"], G["nms_poses"], G["nms_scores"], G["nms_dist_threshold"], G["nms_marks"]
capi.isect_pairs(reset=True)
for budget in (DEFAULT, 0):
    capi.isect_lds_budget(budget)
    marks, keep, rounds = capi.nms(shape, cen, poses, scores, thr)
    assert (marks == want).all(), (budget, np.flatnonzero(marks != want)[:8])
    assert (keep == np.flatnonzero(want == 1)).all() and rounds == len(keep)
    m2, k2, r2 = capi.nms(shape, cen, poses, scores, thr)
    assert (m2 == marks).all() and (k2 == keep).all() and r2 == rounds
capi.isect_lds_budget(DEFAULT)
ev, sk = capi.isect_pairs()
assert ev > 0 and sk > 0
b, e, c = (np.ascontiguousarray(a, np.float32) for a in (L["shape"][0], L["shape"][1], cen))
p, s = np.ascontiguousarray(poses, np.float32), np.ascontiguousarray(scores, np.float32)
ms, ks, nk = np.zeros(len(s), np.int32), np.zeros(len(s), np.int32), i32()
rc = lib.rsd_non_maxima_suppression(b.ctypes.data, len(b), e.ctypes.data, len(e), c.ctypes.data, p.ctypes.data, s.ctypes.data, len(s), float(thr),
                                    ms.ctypes.data, ks.ctypes.data, C.addressof(nk))
assert rc == 0 and (ms == want).all() and nk.value == int((want == 1).sum()) and (ks[:nk.value] == np.flatnonzero(want == 1)).all(), rc
print("ok")
""")


def test_refusals_name_their_pair_and_write_nothing():
    run_child(r"""
small = next(c for c in H.fixture_cases() if c.name == "edges_touch_z")
for name in ("widths_x4097", "widths_z4097"):
    big = next(c for c in H.fixture_cases() if c.name == name)
    # pair 1 of 3 has a line of 4097 cells
    c = H.Case("refused", "widths", small.shapes + big.shapes, [(0, H.I16, 0, H.I16), (1, H.I16, 2, H.I16), (0, H.I16, 0, H.I16)])
    cl = clouds(c)
    for budget in (DEFAULT, 0):
        capi.isect_lds_budget(budget)
        rc, ov, cnt, msg = raw(c, cl)
        assert rc == -4 and "pair 1" in msg and "4097" in msg and (ov == -7.0).all() and (cnt == -7).all(), (name, rc, msg)
    capi.isect_lds_budget(DEFAULT)
    ov, cnt = run(small, cl[:1])                                   # the next call still answers
    assert (cnt[:, 0] > 0).all()
# one NaN point in a boundary cloud: the kernel's own in-bounds check (in fp32, so that a NaN fails it) flags pair 1
c = H.nan_case(); cl = clouds(c)
for budget in (DEFAULT, 0):
    capi.isect_lds_budget(budget)
    rc, ov, cnt, msg = raw(c, cl)
    assert rc == -2 and "pair 1" in msg and (ov == -7.0).all() and (cnt == -7).all(), (rc, msg)
capi.isect_lds_budget(DEFAULT)
good = H.Case("good", "edges", c.shapes, [(0, H.I16, 0, H.I16)])
rc, ov, cnt, msg = raw(good, cl)
assert rc == 0 and ov[0] == 1.0 and cnt[0, 0] == cnt[0, 1] == cnt[0, 2] == 1800
print("ok")
""")


def test_random_unions_match_the_restatement():
    run_child(r"""
for c in H.random_pairs():
    want = [R.overlap(c.shapes[c.ia[k]], c.pose_a[k], c.shapes[c.ib[k]], c.pose_b[k], c.voxel, c.inside, c.by_smaller) for k in range(len(c))]
    want_ov, want_cnt = np.array([w[0] for w in want], np.float32), np.array([w[1] for w in want], np.int32)
    assert (want_cnt[:, 2] > 0).sum() >= 20, c.name
    cl = clouds(c)
    for budget in (DEFAULT, 0):
        capi.isect_lds_budget(budget)
        ov, cnt = run(c, cl)
        assert (cnt == want_cnt).all(), (c.name, budget, np.flatnonzero((cnt != want_cnt).any(1))[:8])
        assert (bits(ov) == bits(want_ov)).all(), (c.name, budget)
capi.isect_lds_budget(DEFAULT)
print("ok")
""")
