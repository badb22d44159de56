"""CPU: the scan-to-objects fixtures (tests/golden/split_*.npz, written by the reference's own pointcloud_to_rsdb: tools/split_fixture)
are reproduced bit for bit by the NumPy restatement (tests/split_restate.py) and by the host plan behind rs_hip_split_plan through
the C ABI; every refusal is decided before a device is touched; the new entry points exist and fail loudly without a GPU.

The comparison rule (split_restate.same_bits): everything as integers, except that where the reference's value is a NaN, and only
there, any NaN will do."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
import split_restate as R

LIB = os.path.join(ROOT, "rescan_amd", "librescan_hip.so")
DROPIN = os.path.join(ROOT, "rescan_amd", "librescan_dropin.so")
KEYS = R.KEYS
E_NODEVICE, E_ARG, E_CAPACITY = -1, -2, -4
SYMBOLS = ("rs_hip_split_plan", "rs_hip_instance_table", "rs_hip_split_by_instance", "rs_hip_segment_centroids", "rs_hip_scan_to_objects",
           "rs_hip_cloud_split_objects", "rs_hip_split_layout", "rs_hip_split_lds_ranks", "rs_hip_split_chains_form", "rs_hip_split_chains_sequential",
           "rs_hip_split_seconds")
QUIRKS = ("mixed_static", "mixed_dynamic", "extreme_ids", "single", "seventy", "last_first", "abab")


@pytest.fixture(scope="module")
def capi():
    from rescan_amd import build, capi
    build.build()
    return capi


def cases():
    """(name, fixture dict with the prefix stripped) of every table-bearing case of the room and quirks fixtures."""
    out = [("room", load_golden("split_room.npz"))]
    q = load_golden("split_quirks.npz")
    for name in q["names"].tolist():
        p = f"case_{name}_"
        d = {k[len(p):]: v for k, v in q.items() if k.startswith(p)}
        d["static_classes"] = q["static_classes"]
        out.append((name, d))
    return out


CASES = cases()


def check_against_fixture(got, g, what):
    """A plan (restatement, host plan or device) against a fixture case: the table, the seven cut arrays, centroids, xforms, poses."""
    scan = {k: g["scan_" + k] for k in KEYS}
    assert got["n_instances"] == len(g["inst_ids"]), what
    for k in ("inst_ids", "class_of", "counts", "offsets"):
        assert (got[k] == g[k]).all(), (what, k)
    assert (got["first"] == [int(np.flatnonzero(scan["inst"] == v)[0]) for v in g["inst_ids"]]).all(), what
    cen = g["centroids"].copy(); cen[:, 1] = 0                  # main.cpp:119
    assert R.same_bits(got["centroids"], cen), what
    assert R.same_bits(got["xforms"], g["xforms"]) and R.same_bits(got["poses"], g["poses"]), what
    assert (got["is_static"] == np.isin(g["class_of"], g["static_classes"])).all(), what
    assert R.same_bits(got["out_pos"], g["out_pos"]) and R.same_bits(got["out_nor"], g["out_nor"]), what
    for k in ("col", "radii", "qual", "cls", "inst"):
        assert R.same_bits(scan[k][got["order"]], g["out_" + k]), (what, k)
    # segment k of order is a plain selection of the id
    for k, v in enumerate(got["inst_ids"]):
        assert (got["order"][got["offsets"][k]:got["offsets"][k + 1]] == np.flatnonzero(scan["inst"] == v)).all(), (what, k)
    # the doubles before the division give the reference's centroid
    with np.errstate(all="ignore"):
        assert R.same_bits((got["sums"] / got["counts"][:, None].astype(np.float64)).astype(np.float32), g["centroids"]), what


def test_fixtures_are_small_and_hold_the_cases():
    for name in ("room", "quirks", "hostile"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"split_{name}.npz")) < 757075
    g = load_golden("split_room.npz")
    assert len(g["scan_pos"]) == 6122 and g["inst_ids"].tolist() == [3, 2, 0, 1] and g["counts"].tolist() == [1002, 960, 3200, 960]
    assert [int(np.flatnonzero(g["scan_inst"] == v)[0]) for v in (0, 1, 2, 3)] == [3, 5, 1, 0]
    assert sorted(set(g["class_of"].tolist())) == [1, 2, 5] and g["static_classes"].tolist() == [1, 2, 0]
    eye = np.eye(4, dtype=np.float32).ravel()
    assert [bool((x == eye).all()) for x in g["xforms"]] == [False, True, True, True]          # the chair moves, floor and walls stay
    q = dict(CASES)
    assert tuple(load_golden("split_quirks.npz")["names"].tolist()) == QUIRKS
    assert len(set(q["mixed_static"]["scan_cls"].tolist())) == 2 and (q["mixed_static"]["xforms"][0] == eye).all()
    assert len(set(q["mixed_dynamic"]["scan_cls"].tolist())) == 2 and not (q["mixed_dynamic"]["xforms"][0] == eye).all()
    assert q["extreme_ids"]["inst_ids"].tolist() == [2 ** 31 - 1, -1, -(2 ** 31), 1024]
    assert len(q["single"]["scan_pos"]) == 1
    assert len(q["seventy"]["scan_pos"]) == 70 and len(q["seventy"]["inst_ids"]) == 70
    assert int(np.flatnonzero(q["last_first"]["scan_inst"] == 6)[0]) == len(q["last_first"]["scan_inst"]) - 1
    assert (q["abab"]["scan_inst"][:64:2] == 11).all() and (q["abab"]["scan_inst"][1:64:2] == 12).all()


@pytest.mark.parametrize("name,g", CASES, ids=[c[0] for c in CASES])
def test_restatement_reproduces_every_array(capi, name, g):
    got = R.plan(g["scan_pos"], g["scan_nor"], g["scan_cls"], g["scan_inst"], g["static_classes"].tolist())
    check_against_fixture(got, g, name)


@pytest.mark.parametrize("name,g", CASES, ids=[c[0] for c in CASES])
def test_plan_reproduces_every_array(capi, name, g):
    """Fails on a library without rs_hip_split_plan."""
    got = capi.split_plan(g["scan_pos"], g["scan_nor"], g["scan_cls"], g["scan_inst"], g["static_classes"])
    check_against_fixture(got, g, name)


def test_a_static_object_keeps_the_scan_bits(capi):
    """Points with -0.0 components: a static object's arrays are the scan's bits, a dynamic object's -0.0 normal comes out +0.0."""
    q = dict(CASES)
    g = q["mixed_static"]
    got = capi.split_plan(g["scan_pos"], g["scan_nor"], g["scan_cls"], g["scan_inst"], g["static_classes"])
    assert got["is_static"].tolist() == [1]
    assert got["out_pos"].tobytes() == g["scan_pos"][got["order"]].tobytes() and got["out_nor"].tobytes() == g["scan_nor"][got["order"]].tobytes()
    zero = g["scan_nor"] == 0
    assert np.signbit(g["scan_nor"][zero]).any() and np.signbit(got["out_nor"][got["out_nor"] == 0]).any()
    g = q["mixed_dynamic"]
    got = capi.split_plan(g["scan_pos"], g["scan_nor"], g["scan_cls"], g["scan_inst"], g["static_classes"])
    assert got["is_static"].tolist() == [0]
    assert np.signbit(g["scan_nor"][g["scan_nor"] == 0]).any() and not np.signbit(got["out_nor"][got["out_nor"] == 0]).any()
    # the same scan with no static list at all: NULL with a count of 0 is allowed, and everything moves
    got = capi.split_plan(q["mixed_static"]["scan_pos"], q["mixed_static"]["scan_nor"], q["mixed_static"]["scan_cls"], q["mixed_static"]["scan_inst"], ())
    assert got["is_static"].tolist() == [0]


def test_the_chains_of_the_room_need_no_order(capi):
    """The block walk of rs_split.hip restated (split_restate.chain_by_blocks): on the room every step is order-free and the sums are
    the reference's; math.fsum and the sequential sum agree in all 64 bits there."""
    import math
    g = load_golden("split_room.npz")
    got = capi.split_plan(g["scan_pos"], g["scan_nor"], g["scan_cls"], g["scan_inst"], g["static_classes"])
    for k in range(got["n_instances"]):
        seg = g["scan_pos"][got["order"][got["offsets"][k]:got["offsets"][k + 1]]]
        for a in range(3):
            s, one_by_one = R.chain_by_blocks(seg[:, a])
            assert one_by_one == 0 and s.view(np.uint64) == got["sums"][k, a].view(np.uint64), (k, a)
            assert np.float64(math.fsum(seg[:, a].astype(np.float64).tolist())).view(np.uint64) == got["sums"][k, a].view(np.uint64), (k, a)


def out_record(capi, n, room):
    k = C.c_int32(-7)
    a = dict(inst_ids=np.full(room, -7, np.int32), counts=np.full(room, -7, np.int64), first=np.full(room, -7, np.int64), offsets=np.full(room + 1, -7, np.int64),
             order=np.full(max(n, 1), -7, np.int32), class_of=np.full(room, -7, np.int32), is_static=np.full(room, -7, np.int32),
             sums=np.full((room, 3), -7.0), centroids=np.full((room, 3), -7, np.float32), xforms=np.full((room, 16), -7, np.float32),
             poses=np.full((room, 16), -7, np.float32), out_pos=np.full((max(n, 1), 3), -7, np.float32), out_nor=np.full((max(n, 1), 3), -7, np.float32))
    return k, a, capi.SplitOut(n_instances=C.addressof(k), **{key: v.ctypes.data for key, v in a.items()})


def untouched(k, a):
    return k.value == -7 and all((v == -7).all() for v in a.values())


def test_refusals_need_no_device(capi):
    lib = capi.load()
    lay = capi.split_layout()
    assert lay["max_instances"] == 4096 and lay["tile"] > 0 and lay["tile"] % 64 == 0 and 0 < lay["lds_ranks"] < lay["max_instances"] and lay["chain_block"] % 64 == 0
    n = lay["max_instances"] + 1
    pos = np.zeros((n, 3), np.float32); cls = np.zeros(n, np.int32); ids = np.arange(n, dtype=np.int32); static = np.array([1], np.int32)
    k, a, out = out_record(capi, n, n)
    args = (pos.ctypes.data, pos.ctypes.data, cls.ctypes.data, ids.ctypes.data)
    # max_instances + 1 distinct ids: refused with nothing written; max_instances pass
    assert lib.rs_hip_split_plan(*args, n, static.ctypes.data, 1, C.addressof(out)) == E_CAPACITY and b"distinct" in lib.rs_hip_last_error()
    assert untouched(k, a)
    assert lib.rs_hip_split_plan(*args, n - 1, static.ctypes.data, 1, C.addressof(out)) == 0 and k.value == n - 1
    with pytest.raises(R.Refused):
        R.table(ids)
    for call in (lib.rs_hip_split_plan, lib.rs_hip_scan_to_objects):
        k, a, out = out_record(capi, 8, 8)
        assert call(*args, -1, static.ctypes.data, 1, C.addressof(out)) == E_ARG
        assert call(None, *args[1:], 8, static.ctypes.data, 1, C.addressof(out)) == E_ARG
        assert call(*args[:2], None, args[3], 8, static.ctypes.data, 1, C.addressof(out)) == E_ARG
        assert call(*args[:3], None, 8, static.ctypes.data, 1, C.addressof(out)) == E_ARG
        assert call(args[0], None, *args[2:], 8, static.ctypes.data, 1, C.addressof(out)) == E_ARG         # normals asked for, none given
        assert call(*args, 8, None, 1, C.addressof(out)) == E_ARG                                             # a static list without its array
        assert call(*args, 8, static.ctypes.data, -1, C.addressof(out)) == E_ARG
        assert untouched(k, a)
        # n = 0 succeeds with no instances
        assert call(None, None, None, None, 0, None, 0, C.addressof(out)) == 0 and k.value == 0 and a["offsets"][0] == 0
    assert lib.rs_hip_scan_to_objects(*args, 8, static.ctypes.data, 1, None) == E_ARG
    cnt = C.c_int32(-7)
    assert lib.rs_hip_instance_table(ids.ctypes.data, -1, None, None, None, C.byref(cnt)) == E_ARG
    assert lib.rs_hip_instance_table(None, 8, None, None, None, C.byref(cnt)) == E_ARG
    assert lib.rs_hip_instance_table(ids.ctypes.data, 8, None, None, None, None) == E_ARG and cnt.value == -7
    assert lib.rs_hip_instance_table(None, 0, None, None, None, C.byref(cnt)) == 0 and cnt.value == 0
    cnt = C.c_int32(-7); order = np.full(8, -7, np.int32)
    assert lib.rs_hip_split_by_instance(ids.ctypes.data, -1, None, None, order.ctypes.data, C.byref(cnt)) == E_ARG
    assert lib.rs_hip_split_by_instance(ids.ctypes.data, 8, None, None, None, C.byref(cnt)) == E_ARG and cnt.value == -7 and (order == -7).all()
    assert lib.rs_hip_split_by_instance(None, 0, None, None, None, C.byref(cnt)) == 0 and cnt.value == 0
    sums = np.full((2, 3), -7.0); off = np.array([0, 4, 8], np.int64); o8 = np.arange(8, dtype=np.int32)
    seg = lib.rs_hip_segment_centroids
    assert seg(pos.ctypes.data, -1, o8.ctypes.data, off.ctypes.data, 2, sums.ctypes.data, None) == E_ARG
    assert seg(pos.ctypes.data, 8, o8.ctypes.data, None, 2, sums.ctypes.data, None) == E_ARG
    assert seg(pos.ctypes.data, 8, o8.ctypes.data, off.ctypes.data, 2, None, None) == E_ARG
    assert seg(pos.ctypes.data, 8, o8.ctypes.data, off.ctypes.data, -1, sums.ctypes.data, None) == E_ARG
    assert seg(pos.ctypes.data, 7, o8.ctypes.data, off.ctypes.data, 2, sums.ctypes.data, None) == E_ARG and b"names no point" in lib.rs_hip_last_error()
    bad = np.array([0, 5, 4], np.int64)
    assert seg(pos.ctypes.data, 8, o8.ctypes.data, bad.ctypes.data, 2, sums.ctypes.data, None) == E_ARG
    bad = np.array([1, 4, 8], np.int64)
    assert seg(pos.ctypes.data, 8, o8.ctypes.data, bad.ctypes.data, 2, sums.ctypes.data, None) == E_ARG
    assert seg(None, 0, None, None, 0, None, None) == 0 and (sums == -7).all()
    objs = (C.c_void_p * 4)()
    k, a, out = out_record(capi, 8, 8)
    assert lib.rs_hip_cloud_split_objects(None, cls.ctypes.data, ids.ctypes.data, None, 0, -1.0, C.addressof(objs), C.addressof(out)) == E_ARG
    assert untouched(k, a) and not any(objs)


def test_the_setters_return_the_previous_value(capi):
    before = capi.split_lds_ranks(-1)
    try:
        assert capi.split_lds_ranks(0) == before and capi.split_lds_ranks(-1) == 0 and capi.split_layout()["lds_ranks"] == 0
        assert capi.split_lds_ranks(7) == 0 and capi.split_lds_ranks(-5) == 7
    finally:
        capi.split_lds_ranks(before)
    assert capi.split_lds_ranks(-1) == before
    assert capi.split_chains_form(-1) == 0
    try:
        assert capi.split_chains_form(1) == 0 and capi.split_chains_form(-1) == 1
    finally:
        capi.split_chains_form(0)


def test_new_symbols_exist(capi):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    for s in SYMBOLS:
        assert re.search(r" T %s\b" % s, out), s
        assert s in capi.SIGNATURES, s
    out = subprocess.check_output(["nm", "-D", "--defined-only", DROPIN], text=True)
    assert re.search(r" T rsd_scan_to_objects\b", out)
    for f in (capi.instance_table, capi.split_by_instance, capi.segment_centroids, capi.split_plan, capi.scan_to_objects, capi.Cloud.split_objects):
        assert callable(f)


def test_new_entry_points_fail_loudly_without_gpu(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    g = load_golden("split_room.npz")
    with pytest.raises(capi.RescanHipError, match="no HIP device"):
        capi.instance_table(g["scan_inst"])
    with pytest.raises(capi.RescanHipError, match="no HIP device"):
        capi.split_by_instance(g["scan_inst"])
    with pytest.raises(capi.RescanHipError, match="no HIP device"):
        capi.segment_centroids(g["scan_pos"], np.arange(8), [0, 8])
    with pytest.raises(capi.RescanHipError, match="no HIP device"):
        capi.scan_to_objects(g["scan_pos"], g["scan_nor"], g["scan_cls"], g["scan_inst"], g["static_classes"])


def test_the_shim_answers_from_the_host_plan_without_a_device(capi):
    """rsd_scan_to_objects: the fixture's arrays on any machine — from the device where there is one, from the host plan otherwise."""
    d = C.CDLL(DROPIN)
    f = d.rsd_scan_to_objects
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 8
    g = load_golden("split_room.npz")
    n = len(g["scan_pos"])
    static = np.ascontiguousarray(g["static_classes"])
    inst = np.full(8, -7, np.int32); cls = np.full(8, -7, np.int32); off = np.full(9, -7, np.int64); order = np.full(n, -7, np.int32)
    pos = np.full((n, 3), -7, np.float32); nor = np.full((n, 3), -7, np.float32); x = np.full((8, 16), -7, np.float32); p = np.full((8, 16), -7, np.float32)
    ins = [g["scan_" + k].ctypes.data for k in ("pos", "nor", "cls", "inst")]
    outs = [a.ctypes.data for a in (inst, cls, off, order, pos, nor, x, p)]
    assert f(None, *ins[1:], n, static.ctypes.data, len(static), 8, *outs) == E_ARG
    assert f(*ins, n, static.ctypes.data, len(static), 3, *outs) == E_CAPACITY                 # four instances, room for three
    assert all((a == -7).all() for a in (inst, cls, off, order, pos, nor, x, p))
    assert f(*ins, n, static.ctypes.data, len(static), 8, *outs) == 4
    assert (inst[:4] == g["inst_ids"]).all() and (cls[:4] == g["class_of"]).all() and (off[:5] == g["offsets"]).all()
    assert R.same_bits(pos, g["out_pos"]) and R.same_bits(nor, g["out_nor"]) and R.same_bits(x[:4], g["xforms"]) and R.same_bits(p[:4], g["poses"])
    assert (g["scan_inst"][order] == g["out_inst"]).all() and (inst[4:] == -7).all()
