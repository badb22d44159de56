"""CPU: the voxel-overlap / non-maximum-suppression fixtures (tests/golden/nms_*.npz, written by the reference's own
isect_get_overlap_factor and mgs_non_maxima_suppresion: tools/nms_fixture) are reproduced IDENTICALLY by the NumPy
restatement of what include/rescan_hip.h documents (tests/isect_restate.py) — every pair, every list; the new entry points
exist, check their arguments before they touch a device and fail loudly without one."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
import isect_restate as R

SHAPES = ("chair", "table", "crate")
LIB = os.path.join(ROOT, "rescan_amd", "librescan_hip.so")
DROPIN = os.path.join(ROOT, "rescan_amd", "librescan_dropin.so")


@pytest.fixture(scope="module")
def built():
    from rescan_amd import build
    build.build()


def test_fixtures_hold_every_case():
    biggest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                  if f.endswith(".npz") and not f.startswith("nms_"))
    for name in SHAPES:
        g = load_golden(f"nms_{name}.npz")
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"nms_{name}.npz")) <= biggest
        cases = [c.decode() for c in g["case"]]
        assert set(cases) == set("abcdefg") and cases.count("d") >= 200
        assert {(int(i), int(s)) for c, i, s in zip(cases, g["inside"], g["by_smaller"]) if c == "f"} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        for li in (0, 1):
            s, m = g[f"list{li}_scores"], g[f"list{li}_marks"]
            assert 40 <= len(s) <= 300 and set(np.unique(m)) == {1, 2}
            assert (np.unique(s, return_counts=True)[1] > 1).any() and (s < 0.01).any() and (s == 10.0).any()


@pytest.mark.parametrize("name", SHAPES)
def test_restatement_reproduces_every_pair(name):
    g = load_golden(f"nms_{name}.npz")
    shape = (g["boundary"], g["extent"])
    bad = []
    for k in range(len(g["overlap"])):
        ov, cnt = R.overlap(shape, g["pose_a"][k], shape, g["pose_b"][k], g["voxel"][k], int(g["inside"][k]), int(g["by_smaller"][k]))
        if tuple(cnt) != tuple(int(v) for v in g["counts"][k]) or np.float32(ov).view(np.uint32) != g["overlap"][k].view(np.uint32):
            bad.append((k, g["case"][k], cnt, g["counts"][k], ov, g["overlap"][k]))
    assert not bad, bad[:5]
    case = np.array([c.decode() for c in g["case"]])
    assert (g["overlap"][case == "a"] == 1.0).all() and (g["overlap"][case == "b"] == 0.0).all()
    assert (g["counts"][case == "c", 0] > 0).all()                   # touching boxes intersect (>=): a grid exists


@pytest.mark.parametrize("name", SHAPES)
def test_restatement_reproduces_every_list(name):
    g = load_golden(f"nms_{name}.npz")
    shape = (g["boundary"], g["extent"])
    alone = 0
    for li in (0, 1):
        marks, keep, rounds, by_overlap = R.nms(shape, g["centroid"], g[f"list{li}_poses"], g[f"list{li}_scores"], float(g["dist_threshold"]))
        assert (marks == g[f"list{li}_marks"]).all(), (name, li)
        assert (keep == np.flatnonzero(g[f"list{li}_marks"] == 1)).all() and rounds == len(keep)
        alone += len(by_overlap)
    if name != "chair":
        assert alone > 0          # some discard is decided by the overlap alone (distance >= threshold, score >= 0.01)


def test_division_is_not_the_multiply_by_the_inverse():
    """Some boundary point of the fixtures sits so close to a voxel face that floorf( o / voxel ) and floorf( o * ( 1 / voxel ) )
    name different cells: the fixtures can tell the two apart."""
    differ = 0
    for name in SHAPES:
        g = load_golden(f"nms_{name}.npz")
        for k in np.flatnonzero((g["counts"][:, 0] > 0))[:120]:
            origin, _ = R.grid_of(R.box(g["pose_a"][k], g["extent"]), R.box(g["pose_b"][k], g["extent"]), g["voxel"][k])
            for pose in (g["pose_a"][k], g["pose_b"][k]):
                o = R.xform(pose, g["boundary"]) - origin[None, :]
                differ += int((np.floor(o / g["voxel"][k]) != np.floor(o * (np.float32(1.0) / g["voxel"][k]))).sum())
    assert differ > 0


def test_restatement_refusals():
    g = load_golden("nms_crate.npz")
    shape = (g["boundary"], g["extent"])
    I = np.eye(4, dtype=np.float32).T.ravel().copy()
    with pytest.raises(R.OutsideGrid):
        small = (g["boundary"], g["extent"][:4] * np.float32(0.01))       # an extent cloud far smaller than the boundary cloud
        R.overlap(small, I, small, I, 0.1, 1, 0)
    wide = I.copy(); wide[0] = 1000.0
    with pytest.raises(R.LineTooLong):
        R.overlap(shape, wide, shape, I, 0.1, 1, 0)


def test_new_symbols_exist(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    for s in ("rs_hip_overlap_factors", "rs_hip_nms", "rs_hip_isect_lds_budget", "rs_hip_isect_pairs"):
        assert re.search(r" T %s\b" % s, out), s
    out = subprocess.check_output(["nm", "-D", "--defined-only", DROPIN], text=True)
    for s in ("rsd_overlap_factor", "rsd_non_maxima_suppression"):
        assert re.search(r" T %s\b" % s, out), s
    from rescan_amd import capi
    assert callable(capi.overlap_factors) and callable(capi.nms)


def test_arguments_are_checked_before_a_device_is_touched(built):
    """In a child process (a regression would read through a null pointer): RS_HIP_E_ARG (-2) for NULL arrays, n < 0, a NaN
    score, a shape index out of range — with or without a device; with valid arguments and no device RS_HIP_E_NODEVICE (-1)."""
    code = r"""
import ctypes as C, sys
lib = C.CDLL(sys.argv[1]); no_gpu = sys.argv[2] == "1"
vp, i32, f = C.c_void_p, C.c_int32, C.c_float
class Shape(C.Structure): _fields_ = [("boundary", vp), ("extent", vp)]
sh = (Shape * 2)(); sh[0].boundary = sh[0].extent = sh[1].boundary = sh[1].extent = 1      # never dereferenced by the checks
poses = (C.c_float * 64)(); idx = (i32 * 4)(0, 1, 0, 1); out = (C.c_float * 4)(); cnt = (i32 * 12)()
ov = lib.rs_hip_overlap_factors; ov.restype = C.c_int
ov.argtypes = [vp, i32, vp, vp, vp, vp, i32, f, C.c_int, C.c_int, vp, vp]
S = C.addressof(sh)
assert ov(None, 2, idx, poses, idx, poses, 4, 0.1, 1, 0, out, cnt) == -2
assert ov(S, 2, None, poses, idx, poses, 4, 0.1, 1, 0, out, cnt) == -2
assert ov(S, 2, idx, poses, idx, None, 4, 0.1, 1, 0, out, cnt) == -2
assert ov(S, 2, idx, poses, idx, poses, 4, 0.1, 1, 0, None, cnt) == -2
assert ov(S, 2, idx, poses, idx, poses, -1, 0.1, 1, 0, out, cnt) == -2
assert ov(S, 2, idx, poses, idx, poses, 4, 0.0, 1, 0, out, cnt) == -2
bad = (i32 * 4)(0, 1, 2, 0)
lib.rs_hip_last_error.restype = C.c_char_p
assert ov(S, 2, bad, poses, idx, poses, 4, 0.1, 1, 0, out, cnt) == -2 and b"pair 2" in lib.rs_hip_last_error()
neg = (i32 * 4)(0, -1, 0, 0)
assert ov(S, 2, idx, poses, neg, poses, 4, 0.1, 1, 0, out, cnt) == -2
nms = lib.rs_hip_nms; nms.restype = C.c_int
nms.argtypes = [vp, vp, vp, vp, i32, f, vp, vp, vp, vp]
cen = (C.c_float * 3)(); sc = (C.c_float * 4)(0.5, 0.4, 0.3, 0.2); marks = (i32 * 4)(7, 7, 7, 7); keep = (i32 * 4)(); nk = i32(-5); nr = i32(-5)
assert nms(None, cen, poses, sc, 4, 0.2, marks, keep, C.addressof(nk), C.addressof(nr)) == -2
assert nms(S, None, poses, sc, 4, 0.2, marks, keep, C.addressof(nk), C.addressof(nr)) == -2
assert nms(S, cen, None, sc, 4, 0.2, marks, keep, C.addressof(nk), C.addressof(nr)) == -2
assert nms(S, cen, poses, None, 4, 0.2, marks, keep, C.addressof(nk), C.addressof(nr)) == -2
assert nms(S, cen, poses, sc, 4, 0.2, None, keep, C.addressof(nk), C.addressof(nr)) == -2
assert nms(S, cen, poses, sc, 4, 0.2, marks, keep, None, C.addressof(nr)) == -2
assert nms(S, cen, poses, sc, -2, 0.2, marks, keep, C.addressof(nk), C.addressof(nr)) == -2
sc[2] = float("nan")
assert nms(S, cen, poses, sc, 4, 0.2, marks, keep, C.addressof(nk), C.addressof(nr)) == -2 and b"score 2" in lib.rs_hip_last_error()
sc[2] = -2e9
assert nms(S, cen, poses, sc, 4, 0.2, marks, keep, C.addressof(nk), C.addressof(nr)) == -2
assert list(marks) == [7, 7, 7, 7] and nk.value == -5 and nr.value == -5
if no_gpu:
    sc[2] = 0.3
    assert nms(S, cen, poses, sc, 4, 0.2, marks, keep, C.addressof(nk), C.addressof(nr)) == -1
    assert ov(S, 2, idx, poses, idx, poses, 4, 0.1, 1, 0, out, cnt) == -1
    assert list(marks) == [7, 7, 7, 7] and nk.value == -5
print("ok")
"""
    import torch
    no_gpu = "0" if torch.cuda.is_available() else "1"
    out = subprocess.run([sys.executable, "-c", code, LIB, no_gpu], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


def test_shim_fails_loudly_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    code = r"""
import ctypes as C, sys
lib = C.CDLL(sys.argv[1])
vp, i32, f = C.c_void_p, C.c_int32, C.c_float
pts = (C.c_float * 30)(); poses = (C.c_float * 32)(); cen = (C.c_float * 3)(); sc = (C.c_float * 2)(0.5, 0.4); marks = (i32 * 2)(); keep = (i32 * 2)(); nk = i32()
fn = lib.rsd_non_maxima_suppression; fn.restype = C.c_int
fn.argtypes = [vp, i32, vp, i32, vp, vp, vp, i32, f, vp, vp, vp]
assert fn(pts, 10, pts, 10, cen, poses, sc, 2, 0.2, marks, keep, C.addressof(nk)) < 0
ov = lib.rsd_overlap_factor; ov.restype = C.c_int
ov.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, i32, vp, f, C.c_int, C.c_int, vp]
o = C.c_float(-7.0)
assert ov(pts, 10, pts, 10, poses, pts, 10, pts, 10, poses, 0.1, 1, 0, C.addressof(o)) < 0 and o.value == -7.0
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code, DROPIN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
