"""GPU: rs_hip_overlap_factors and rs_hip_nms against every pair and every list of the reference's fixtures
(tests/golden/nms_*.npz), IDENTICALLY: int32 equality of the counts, bit equality of the float32 overlap, equal marks /
keep_idx / n_keep — on the LDS route and on the global-scratch route, through the C ABI and through the drop-in shim.
The GPU work runs in child processes, each under its own time limit; nothing here provokes a fault: the refusals are
decided from the boxes on the host or flagged by an in-bounds check of the kernel."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PRELUDE = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from rescan_amd import capi
capi.init(0)
G = {n: dict(np.load(os.path.join(sys.argv[1], "tests", "golden", f"nms_{n}.npz"))) for n in ("chair", "table", "crate")}
CL = {n: (capi.Cloud(g["boundary"], None, 0.0), capi.Cloud(g["extent"], None, 0.0)) for n, g in G.items()}
def bits(a): return np.ascontiguousarray(a, np.float32).view(np.uint32)
def groups(g):
    key = np.stack([bits(g["voxel"]), g["inside"].astype(np.uint32), g["by_smaller"].astype(np.uint32)], 1)
    for k in np.unique(key, axis=0):
        yield np.flatnonzero((key == k[None, :]).all(1))
def run_pairs(name, sel):
    g = G[name]; z = np.zeros(len(sel), np.int32)
    return capi.overlap_factors([CL[name]], z, g["pose_a"][sel], z, g["pose_b"][sel], g["voxel"][sel[0]], int(g["inside"][sel[0]]), int(g["by_smaller"][sel[0]]))
"""


def run_child(body, limit=300):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


def test_every_pair_is_the_references_on_both_routes():
    run_child(r"""
for budget in (61440, 0):                   # the default routes (case g alone goes to global memory), then every pair through global memory
    capi.isect_lds_budget(budget)
    for name, g in G.items():
        seen = 0
        for sel in groups(g):
            ov, cnt = run_pairs(name, sel)
            assert (cnt == g["counts"][sel]).all(), (budget, name, sel[(cnt != g["counts"][sel]).any(1)][:5])
            assert (bits(ov) == bits(g["overlap"][sel])).all(), (budget, name)
            seen += len(sel)
        assert seen == len(g["overlap"])
capi.isect_lds_budget(61440)
# case g does not fit the LDS route: with the default budget it was evaluated through the slab (same bits as above)
print("ok")
""")


def test_three_shapes_in_one_call_and_one_pair_against_a_thousand():
    run_child(r"""
names = list(G)
shapes = [CL[n] for n in names]
rng = np.random.default_rng(5)
ia, ib, pa, pb, want = [], [], [], [], []
for s, n in enumerate(names):                      # pairs of one shape with itself, from the fixtures: 0.1 m, inside, larger count
    g = G[n]
    sel = np.flatnonzero((g["voxel"] == np.float32(0.1)) & (g["inside"] == 1) & (g["by_smaller"] == 0))
    for k in sel:
        ia.append(s); ib.append(s); pa.append(g["pose_a"][k]); pb.append(g["pose_b"][k]); want.append((g["counts"][k], g["overlap"][k]))
order = rng.permutation(len(ia))[:1000]
while len(order) < 1000: order = np.concatenate([order, order])[:1000]
ia, ib, pa, pb = np.array(ia, np.int32)[order], np.array(ib, np.int32)[order], np.stack(pa)[order], np.stack(pb)[order]
ov, cnt = capi.overlap_factors(shapes, ia, pa, ib, pb, 0.1, True, False)
ov2, cnt2 = capi.overlap_factors(shapes, ia, pa, ib, pb, 0.1, True, False)
assert (bits(ov) == bits(ov2)).all() and (cnt == cnt2).all()                    # two runs, identical bits
for j, k in enumerate(order):
    assert (cnt[j] == want[k][0]).all() and bits(ov[j:j + 1])[0] == bits(np.float32(want[k][1]).reshape(1))[0], j
for j in range(0, 1000, 37):                                                    # a batch of one agrees with its row of the batch of 1000
    o1, c1 = capi.overlap_factors(shapes, ia[j:j + 1], pa[j:j + 1], ib[j:j + 1], pb[j:j + 1], 0.1, True, False)
    assert bits(o1)[0] == bits(ov[j:j + 1])[0] and (c1[0] == cnt[j]).all(), j
# mixed shapes in one pair: symmetric in the counts
o_ab, c_ab = capi.overlap_factors(shapes, [0], pa[:1], [1], pb[:1], 0.1, True, False)
o_ba, c_ba = capi.overlap_factors(shapes, [1], pb[:1], [0], pa[:1], 0.1, True, False)
assert c_ab[0, 0] == c_ba[0, 1] and c_ab[0, 1] == c_ba[0, 0] and c_ab[0, 2] == c_ba[0, 2] and bits(o_ab)[0] == bits(o_ba)[0]
print("ok")
""")


def test_nms_lists_are_the_references():
    run_child(r"""
lib = C.CDLL(os.path.join(sys.argv[1], "rescan_amd", "librescan_dropin.so"))
vp, i32, f = C.c_void_p, C.c_int32, C.c_float
lib.rsd_non_maxima_suppression.restype = C.c_int
lib.rsd_non_maxima_suppression.argtypes = [vp, i32, vp, i32, vp, vp, vp, i32, f, vp, vp, vp]
for budget in (61440, 0):
    capi.isect_lds_budget(budget)
    for name, g in G.items():
        for li in (0, 1):
            poses, scores, want = g[f"list{li}_poses"], g[f"list{li}_scores"], g[f"list{li}_marks"]
            marks, keep, rounds = capi.nms(CL[name], g["centroid"], poses, scores, float(g["dist_threshold"]))
            assert (marks == want).all(), (budget, name, li, np.flatnonzero(marks != want)[:8])
            assert (keep == np.flatnonzero(want == 1)).all() and rounds == len(keep)
            m2, k2, r2 = capi.nms(CL[name], g["centroid"], poses, scores, float(g["dist_threshold"]))
            assert (m2 == marks).all() and (k2 == keep).all() and r2 == rounds
            if budget:                       # ... and through the shim, on host arrays
                b, e, c = (np.ascontiguousarray(g[k], np.float32) for k in ("boundary", "extent", "centroid"))
                p, s = np.ascontiguousarray(poses, np.float32), np.ascontiguousarray(scores, np.float32)
                ms, ks, nk = np.zeros(len(s), np.int32), np.zeros(len(s), np.int32), i32()
                rc = lib.rsd_non_maxima_suppression(b.ctypes.data, len(b), e.ctypes.data, len(e), c.ctypes.data, p.ctypes.data, s.ctypes.data, len(s),
                                                    float(g["dist_threshold"]), ms.ctypes.data, ks.ctypes.data, C.addressof(nk))
                assert rc == 0 and (ms == want).all() and nk.value == len(keep) and (ks[:nk.value] == keep).all(), (name, li, rc)
capi.isect_lds_budget(61440)
ev, sk = capi.isect_pairs()
assert ev > 0 and sk > 0
# the shim's single-pair call
lib.rsd_overlap_factor.restype = C.c_int
lib.rsd_overlap_factor.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, i32, vp, f, C.c_int, C.c_int, vp]
g = G["crate"]; b, e = np.ascontiguousarray(g["boundary"]), np.ascontiguousarray(g["extent"])
for k in (0, 5, 20, 100):
    o = C.c_float(-1.0); pa, pb = np.ascontiguousarray(g["pose_a"][k]), np.ascontiguousarray(g["pose_b"][k])
    rc = lib.rsd_overlap_factor(b.ctypes.data, len(b), e.ctypes.data, len(e), pa.ctypes.data, b.ctypes.data, len(b), e.ctypes.data, len(e), pb.ctypes.data,
                                float(g["voxel"][k]), int(g["inside"][k]), int(g["by_smaller"][k]), C.addressof(o))
    assert rc == 0 and bits(np.float32(o.value).reshape(1))[0] == bits(g["overlap"][k:k + 1])[0], k
print("ok")
""")


def test_refusals_return_their_code_and_write_nothing():
    run_child(r"""
L = capi.load()
g = G["crate"]; shape = CL["crate"]
I = np.eye(4, dtype=np.float32).ravel()
arr = capi._isect_shapes([shape])
def call(arr, pa, pb, n, inside=1):
    z = np.zeros(n, np.int32); ov = np.full(n, -7.0, np.float32); cnt = np.full((n, 3), -7, np.int32)
    pa, pb = np.ascontiguousarray(pa, np.float32), np.ascontiguousarray(pb, np.float32)
    rc = L.rs_hip_overlap_factors(C.addressof(arr), 1, z.ctypes.data, pa.ctypes.data, z.ctypes.data, pb.ctypes.data, n, 0.1, inside, 0, ov.ctypes.data, cnt.ctypes.data)
    return rc, ov, cnt, L.rs_hip_last_error().decode()
# a line of more than 4096 cells: pair 1 of 3 is stretched a thousandfold along x
wide = I.copy(); wide[0] = 1000.0
rc, ov, cnt, msg = call(arr, np.stack([I, wide, I]), np.stack([I, I, I]), 3)
assert rc == -4 and "pair 1" in msg and (ov == -7.0).all() and (cnt == -7).all(), (rc, msg)
# (without the fill there is no scanline to overflow: the pair is rasterised — through global memory — and then fails the reference's
#  other condition, its level-1 points lying up to 40 m, not 4 cm, from the stretched level-3 points)
rc, ov, cnt, msg = call(arr, np.stack([I, wide, I]), np.stack([I, I, I]), 3, inside=0)
assert rc == -2 and "pair 1" in msg and (ov == -7.0).all() and (cnt == -7).all(), (rc, msg)
# a boundary point outside the grid: an extent cloud far smaller than the boundary cloud
tiny = capi.Cloud(g["extent"][:4] * np.float32(0.01), None, 0.0)
arr2 = capi._isect_shapes([(shape[0], tiny)])
for budget in (61440, 0):
    capi.isect_lds_budget(budget)
    rc, ov, cnt, msg = call(arr2, np.stack([I, I]), np.stack([I, I]), 2)
    assert rc == -2 and "pair 0" in msg and (ov == -7.0).all() and (cnt == -7).all(), (rc, msg)
capi.isect_lds_budget(61440)
# ... and the library still answers afterwards
rc, ov, cnt, msg = call(arr, I[None], I[None], 1)
assert rc == 0 and ov[0] == 1.0 and cnt[0, 0] == cnt[0, 1] == cnt[0, 2] > 0
# nms: the same shape refuses, marks untouched
marks = np.full(3, -7, np.int32); keep = np.full(3, -7, np.int32); nk = C.c_int32(-7)
sc = np.array([0.5, 0.4, 0.3], np.float32); po = np.stack([I, I, I]); cen = np.zeros(3, np.float32)
# (threshold 0: no distance is below it, so the overlap of the coincident proposals has to be evaluated)
rc = L.rs_hip_nms(C.addressof(arr2), cen.ctypes.data, po.ctypes.data, sc.ctypes.data, 3, 0.0, marks.ctypes.data, keep.ctypes.data, C.addressof(nk), None)
assert rc == -2 and (marks == -7).all() and nk.value == -7
rc = L.rs_hip_nms(C.addressof(arr), cen.ctypes.data, po.ctypes.data, sc.ctypes.data, 0, 0.2, marks.ctypes.data, keep.ctypes.data, C.addressof(nk), None)
assert rc == 0 and nk.value == 0
print("ok")
""")
