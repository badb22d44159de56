"""CPU: the arrangement fixture (tests/golden/fuse_arrangement.npz, the reference's own loop over five placements: tools/fuse_fixture)
is reproduced bit for bit by chaining the NumPy restatement (tests/fuse_restate.py) with the recorded xforms, the dependent
placement's model being what its model_from left; the entry points of the one-call form exist and are bound; every refusal that can
be judged without a cloud is decided before a device is touched, with nothing written."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
import fuse_restate as R

LIB = os.path.join(ROOT, "rescan_amd", "librescan_hip.so")
DROPIN = os.path.join(ROOT, "rescan_amd", "librescan_dropin.so")
KEYS = ("pos", "nor", "col", "radii", "qual", "cls", "inst")
E_ARG, E_CAPACITY = -2, -4
SYMBOLS = ("rs_hip_cloud_fuse_arrangement", "rs_hip_shuffle_permutations", "rs_hip_merge_shuffled_multi")


@pytest.fixture(scope="module")
def lib():
    from rescan_amd import build
    build.build()
    lib = C.CDLL(LIB)
    lib.rs_hip_last_error.restype = C.c_char_p
    return lib


def test_fixture_holds_the_cases():
    g = load_golden("fuse_arrangement.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "fuse_arrangement.npz")) < 757075
    assert g["model_from"].tolist() == [-1, -1, -1, -1, 0] and g["is_static"].tolist() == [0, 1, 0, 0, 0]
    n_ext = g["n_extracted"].tolist()
    assert n_ext[2] == 0 and "p2_merged_pos" not in g and not (g["scan_inst"] == g["uidx"][2]).any()
    assert all(0 < n_ext[p] <= 16384 for p in (0, 3, 4)) and n_ext[1] > 0
    assert g["uidx"][4] == g["uidx"][0] and len(np.unique(g["scan_inst"])) == 5 and 2000 <= len(g["scan_pos"]) <= 9000
    start = np.linalg.inv(g["poses"][0].astype(np.float64).reshape(4, 4).T).T.ravel()
    assert np.linalg.norm(g["p0_xform"].astype(np.float64) - start) > 1e-3
    assert len(g["p4_merged_pos"]) == n_ext[4] + len(g["p0_merged_pos"])             # the dependent placement's model is the chair's merged cloud


def test_restatement_chain_reproduces_every_merged_array():
    g = load_golden("fuse_arrangement.npz")
    shapes = []
    for p in range(len(g["uidx"])):
        uidx, frm = int(g["uidx"][p]), int(g["model_from"][p])
        model = shapes[frm] if frm >= 0 else {k: g[f"p{p}_model_{k}"] for k in KEYS}
        idx = R.select(g["scan_inst"], [uidx])
        assert len(idx) == int(g["n_extracted"][p])
        for k in KEYS:
            assert R.same_bits(g["scan_" + k][idx], g[f"p{p}_extracted_{k}"]), (p, k)
        if len(idx) == 0:
            shapes.append(model)                                                     # database_update.cpp:58
            continue
        pos, nor, source = R.merge(g["scan_pos"][idx], g["scan_nor"][idx], g[f"p{p}_xform"], model["pos"], model["nor"])
        merged = dict(pos=pos, nor=nor, inst=np.full(len(pos), uidx, np.int32))
        for k in ("col", "radii", "qual", "cls"):
            merged[k] = np.concatenate([g["scan_" + k][idx], model[k]])[source]
        for k in KEYS:
            assert R.same_bits(merged[k], g[f"p{p}_merged_{k}"]), (p, k)
        shapes.append(merged)
    # the dependent placement is reproduced only through the chair's merged cloud: the chair's own model has another size
    assert len(shapes[0]["pos"]) != len(g["p0_model_pos"])


def test_new_symbols_exist_and_are_bound(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    for s in SYMBOLS:
        assert re.search(r" T %s\b" % s, out), s
    out = subprocess.check_output(["nm", "-D", "--defined-only", DROPIN], text=True)
    assert re.search(r" T rsd_augment_models\b", out)
    from rescan_amd import capi
    for s in SYMBOLS:
        assert s in capi.SIGNATURES, s
    for f in (capi.Cloud.fuse_arrangement, capi.shuffle_permutations, capi.merge_shuffled_multi):
        assert callable(f)
    assert C.sizeof(capi.FusePlacement) == 88 and C.sizeof(capi.FuseResult) == 104     # the records of include/rescan_hip.h


def test_permutation_refusals_need_no_device(lib):
    f = lib.rs_hip_shuffle_permutations
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p]
    perm = np.full(16, -7, np.int32)
    sizes = lambda *v: np.array(v, np.int64)                                         # noqa: E731
    n = sizes(3, 4)
    assert f(n.ctypes.data, -1, 12346, perm.ctypes.data) == E_ARG and b"negative" in lib.rs_hip_last_error()
    assert f(None, 2, 12346, perm.ctypes.data) == E_ARG
    assert f(n.ctypes.data, 2, 12346, None) == E_ARG
    n = sizes(3, -1)
    assert f(n.ctypes.data, 2, 12346, perm.ctypes.data) == E_ARG
    n = sizes(3, (1 << 24) + 1)
    assert f(n.ctypes.data, 2, 12346, perm.ctypes.data) == E_CAPACITY and b"2^24" in lib.rs_hip_last_error()
    n = np.full(129, 1 << 24, np.int64)                                              # each within 2^24, the sum beyond int32
    assert f(n.ctypes.data, 129, 12346, perm.ctypes.data) == E_CAPACITY and b"int32" in lib.rs_hip_last_error()
    assert f(n.ctypes.data, 0, 12346, None) == 0 and f(None, 0, 12346, None) == 0    # no placements: nothing to do
    n = sizes(0, 0, 0)
    assert f(n.ctypes.data, 3, 12346, None) == 0                                     # nothing to write
    assert (perm == -7).all()


def test_merge_refusals_need_no_device(lib):
    f = lib.rs_hip_merge_shuffled_multi
    f.restype = C.c_int
    f.argtypes = [C.c_int32] + [C.c_void_p] * 7 + [C.c_uint32] + [C.c_void_p] * 3
    pts = np.zeros((4, 3), np.float32); x = np.tile(np.eye(4, dtype=np.float32).ravel(), 2); out = np.full((16, 3), -7, np.float32)
    src = np.full(16, -7, np.int32)
    ptrs = (C.c_void_p * 2)(pts.ctypes.data, pts.ctypes.data); null_one = (C.c_void_p * 2)(pts.ctypes.data, None)
    a = C.addressof(ptrs); n = np.array([4, 4], np.int64); o = (out.ctypes.data, out.ctypes.data, src.ctypes.data)

    def call(P=2, a_pos=a, a_nor=a, n_a=n, xf=x, b_pos=a, b_nor=a, n_b=n, outs=o):
        return f(P, a_pos, a_nor, None if n_a is None else n_a.ctypes.data, None if xf is None else xf.ctypes.data, b_pos, b_nor,
                 None if n_b is None else n_b.ctypes.data, 12346, *outs)
    assert call(P=-1) == E_ARG and b"negative" in lib.rs_hip_last_error()
    assert call(a_pos=None) == E_ARG and call(n_a=None) == E_ARG and call(xf=None) == E_ARG and call(b_nor=None) == E_ARG
    assert call(a_nor=C.addressof(null_one)) == E_ARG                                # a placement's A without normals
    assert call(n_a=np.array([4, -1], np.int64)) == E_ARG
    assert call(outs=(None, out.ctypes.data, None)) == E_ARG
    assert call(n_a=np.array([4, (1 << 24) + 1], np.int64)) == E_CAPACITY
    assert call(n_a=np.array([4, 1 << 24], np.int64), n_b=np.array([4, 1], np.int64)) == E_CAPACITY and b"2^24" in lib.rs_hip_last_error()
    assert call(P=0, outs=(None, None, None)) == 0
    zero = np.zeros(2, np.int64); nulls = (C.c_void_p * 2)(None, None)
    assert call(a_pos=C.addressof(nulls), a_nor=C.addressof(nulls), n_a=zero, b_pos=C.addressof(nulls), b_nor=C.addressof(nulls), n_b=zero,
                outs=(None, None, None)) == 0                                        # empty merges
    assert (out == -7).all() and (src == -7).all()


def test_arrangement_refusals_need_no_device(lib):
    from rescan_amd import capi
    f = lib.rs_hip_cloud_fuse_arrangement
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_void_p]
    recs = (capi.FusePlacement * 3)(); outs = (capi.FuseResult * 3)()
    C.memset(C.addressof(outs), 0x5A, C.sizeof(outs))
    before = bytes(outs)
    ids = np.zeros(8, np.int32)
    fake = C.c_void_p(0x1000)                 # never dereferenced: every call below is refused before a cloud is read
    args = (0.05, 0.17, -1.0)
    assert f(fake, ids.ctypes.data, C.addressof(recs), -1, *args, C.addressof(outs)) == E_ARG and b"negative" in lib.rs_hip_last_error()
    assert f(None, None, None, 0, *args, None) == 0                                   # no placements
    assert f(None, ids.ctypes.data, C.addressof(recs), 3, *args, C.addressof(outs)) == E_ARG
    assert f(fake, ids.ctypes.data, None, 3, *args, C.addressof(outs)) == E_ARG
    assert f(fake, ids.ctypes.data, C.addressof(recs), 3, *args, None) == E_ARG
    for p in range(3):
        recs[p].model_from = -1; recs[p].model = 0x2000
    for p, bad in ((0, 0), (1, 1), (2, 3), (1, -2)):                                  # model_from outside [-1, p)
        recs[p].model_from = bad
        assert f(fake, ids.ctypes.data, C.addressof(recs), 3, *args, C.addressof(outs)) == E_ARG and b"model_from" in lib.rs_hip_last_error(), (p, bad)
        recs[p].model_from = -1
    recs[1].model = None                                                              # model_from == -1 with no model
    assert f(fake, ids.ctypes.data, C.addressof(recs), 3, *args, C.addressof(outs)) == E_ARG and b"no model" in lib.rs_hip_last_error()
    assert bytes(outs) == before
    with pytest.raises(capi.RescanHipError, match="model_from"):
        class Stub:
            handle, n = 0x1000, 8
        capi.Cloud.fuse_arrangement(Stub(), ids, [dict(uidx=1, pose=np.eye(4), model_from=0)])


def test_shim_refusals_need_no_device(lib):
    d = C.CDLL(DROPIN)
    f = d.rsd_augment_models
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p] * 7 + [C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_void_p] * 2 + [C.c_void_p] * 3 + [C.c_void_p] * 7 + [C.c_void_p, C.c_void_p]
    g = load_golden("fuse_arrangement.npz")
    scan = [g["scan_" + k].ctypes.data for k in KEYS]
    P = 2
    models = [(C.c_void_p * P)(*[g[f"p{p}_model_{k}"].ctypes.data for p in (0, 1)]) for k in KEYS[:6]]
    n_model = np.array([len(g["p0_model_pos"]), len(g["p1_model_pos"])], np.int32)
    poses = np.ascontiguousarray(g["poses"][:2]); uidx = np.ascontiguousarray(g["uidx"][:2]); static = np.ascontiguousarray(g["is_static"][:2])
    outs = [(C.c_void_p * P)() for _ in range(7)]; out_n = np.full(P, -7, np.int64)

    def call(n_pl=P, frm=(-1, -1), scan0=scan[0]):
        frm = np.array(frm, np.int32)
        return f(scan0, *scan[1:], len(g["scan_pos"]), n_pl, *[C.addressof(m) for m in models], n_model.ctypes.data, frm.ctypes.data,
                 poses.ctypes.data, uidx.ctypes.data, static.ctypes.data, *[C.addressof(o) for o in outs], out_n.ctypes.data, None)
    assert call(n_pl=-1) == E_ARG and call(scan0=None) == E_ARG and call(frm=(0, -1)) == E_ARG and call(frm=(-1, 1)) == E_ARG and call(frm=(-1, -2)) == E_ARG
    assert call(n_pl=0) == 0
    assert all(not o[k] for o in outs for k in range(P)) and (out_n == -7).all()
