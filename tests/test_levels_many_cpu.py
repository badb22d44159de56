"""CPU: the batched level builder's host side.  The plan of rescan_amd/csrc/rs_levels.h -- level order, global ids, tile table,
refusals, groups, lane classes -- printed by tests/host/levelplan_check.cpp, a plain host program built and run under the address and
undefined-behaviour sanitizers, and recomputed here in numpy line by line; and the entry points' ABI surface and the refusals they
decide without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("rs_hip_level_samples_many", "rs_hip_cloud_create_levels_many")
E_ARG, E_CAPACITY = -2, -4


@pytest.fixture(scope="module")
def lib():
    from rescan_amd import build, capi
    build.build()
    return capi.load()


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("levelplan") / "levelplan_check")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-Wall", "-Werror", "-Wno-unknown-pragmas",     # (the runtimes inside the executable: it needs nothing preloaded)
           "-I", os.path.join(ROOT, "rescan_amd", "csrc"), os.path.join(HERE, "host", "levelplan_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, (b.stdout[-2000:], b.stderr[-2000:])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("levelplan_check ok"), (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout.splitlines()


def _ints(s):
    return [int(x) for x in s.split(",")] if s else []


def _fields(text):
    return {k: v for k, v in re.findall(r"(\w+)=(\"[^\"]*\"|\S*)", text)}


def _consts(lines):
    return {k: int(v) for k, v in _fields([ln for ln in lines if ln.startswith("consts")][0]).items()}


def _plan(sizes, tiles, radii_bits, caps, K):
    """The plan restated: (rc, fields)."""
    nc, nl = len(sizes), len(radii_bits)
    radii = np.array(radii_bits, np.uint32).view(np.float32)
    if nl > K["MAX_LEVELS"] or nc * nl > K["MAX_PROBLEMS"]:
        return E_ARG, None
    if nc == 0 or nl == 0:
        return 0, None
    if not all(r > 0 for r in radii) or any(c <= 0 for c in caps) or any(s < 0 for s in sizes):
        return E_ARG, None
    if sum(sizes) * nl > K["MAX_IDS"]:
        return E_CAPACITY, None
    order = np.argsort(radii, kind="stable")
    rank = np.empty(nl, np.int64); rank[order] = np.arange(nl)
    rs = radii[order]
    rsq = (rs.astype(np.float64) * rs.astype(np.float64)).astype(np.float32)
    pfirst = np.concatenate([[0], np.cumsum(sizes)]); tfirst = np.concatenate([[0], np.cumsum(tiles)])
    gfirst = [int(rank[l]) * int(pfirst[-1]) + int(pfirst[c]) for c in range(nc) for l in range(nl)]
    return 0, dict(order=list(order), rank=list(rank), cap=[caps[i] for i in order], radius=list(rs.view(np.uint32)), rsq=list(rsq.view(np.uint32)),
                   pfirst=list(pfirst), tile_first=list(tfirst), gfirst=gfirst, n_points=int(pfirst[-1]), n_ids=int(pfirst[-1]) * nl, n_tiles=int(tfirst[-1]))


def test_plan_lines_equal_the_numpy_restatement(lines):
    K = _consts(lines)
    assert K == dict(MAX_LEVELS=8, MAX_PROBLEMS=32768, MAX_IDS=1 << 30, ENTRY_BUDGET=1 << 28, ENTRY_MAX=(1 << 32) - 1, SINGLE_ABOVE=1000000)
    plans = [ln for ln in lines if ln.startswith("plan ")]
    assert len(plans) >= 28
    seen = {0: 0, E_ARG: 0, E_CAPACITY: 0}
    for ln in plans:
        left, right = ln.split(" -> ")
        i, o = _fields(left), _fields(right)
        sizes, tiles, rb, caps = _ints(i["sizes"]), _ints(i["tiles"]), _ints(i["radii"]), _ints(i["caps"])
        rc, want = _plan(sizes, tiles, rb, caps, K)
        assert int(o["rc"]) == rc, ln[:300]
        seen[rc] += 1
        if rc:
            assert len(o["err"]) > 12 and "levels_many" in o["err"], ln[:300]
        if want:
            for k, v in want.items():
                got = _ints(o[k]) if isinstance(v, list) else int(o[k])
                assert got == ([int(x) for x in v] if isinstance(v, list) else v), (k, ln[:300])
            # ids: problem (c, l) owns gfirst + [0, size): disjoint, below n_ids, a level's ids together
            nl = len(rb)
            spans = sorted((want["gfirst"][c * nl + l], want["gfirst"][c * nl + l] + sizes[c]) for c in range(len(sizes)) for l in range(nl))
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and (not spans or spans[-1][1] <= want["n_ids"])
    assert seen[0] >= 12 and seen[E_ARG] >= 9 and seen[E_CAPACITY] >= 3
    # the named cases are there: equal radii keep the caller's order, the sizes around a tile and a block, the bounds themselves
    text = "\n".join(plans)
    assert " order=1,3,0,2 " in text and " order=0,1,2 " in text and "sizes=0,1,63,64,65,255,256,257 " in text
    assert "tile_first=0,0,1,2,3,5,9,13,18 " in text
    assert f"sizes={1 << 29},{1 << 29} " in text and f"sizes={1 << 29},{(1 << 29) + 1} " in text


def _groups(totals, budget):
    gend, s, first = [], 0, 0
    for k, t in enumerate(totals):
        if k > first and s + t > budget:
            gend.append(k); first = k; s = 0
        s += t
    if totals:
        gend.append(len(totals))
    return gend


def test_groups_fit_the_entry_budget(lines):
    B = _consts(lines)["ENTRY_BUDGET"]
    rows = [ln for ln in lines if ln.startswith("groups")]
    assert len(rows) >= 10
    shapes = set()
    for ln in rows:
        left, right = ln.split(" -> ")
        i, o = _fields(left), _fields(right)
        totals, budget, gend = _ints(i["totals"]), int(i["budget"]), _ints(o["gend"])
        assert gend == _groups(totals, budget) and int(o["n"]) == len(gend), ln
        # what the rule promises: consecutive, complete, within the budget unless a group is one unit, and no two neighbours could merge
        assert gend == sorted(set(gend)) and (gend[-1] == len(totals) if totals else not gend)
        sums = [sum(totals[a:b]) for a, b in zip([0] + gend[:-1], gend)]
        sizes = [b - a for a, b in zip([0] + gend[:-1], gend)]
        assert all(s <= budget or n == 1 for s, n in zip(sums, sizes)), ln
        for g in range(len(gend) - 1):
            assert sums[g] + totals[gend[g]] > budget, ln
        if budget == B:
            shapes.add((tuple(totals), tuple(gend)))
    assert ((B // 2, B // 2 - 1), (2,)) in shapes and ((B // 2, B // 2), (2,)) in shapes and ((B // 2, B // 2 + 1), (1, 2)) in shapes
    assert ((1, B + 7, 1, 1), (1, 2, 4)) in shapes and ((B + 7,), (1,)) in shapes


def test_lane_classes_on_both_sides_of_each_cut(lines):
    row = [ln for ln in lines if ln.startswith("lanes")][0].split()[1:]
    got = [(float.fromhex(a), int(g)) for a, g in (x.rsplit(":", 1) for x in row)]
    assert [g for _, g in got] == [64 if a >= 24.0 else (8 if a >= 3.0 else 1) for a, _ in got]
    avgs = [a for a, _ in got]
    assert np.nextafter(3.0, 0.0) in avgs and 3.0 in avgs and np.nextafter(24.0, 0.0) in avgs and 24.0 in avgs
    assert [g for _, g in got] == [1, 1, 1, 8, 8, 8, 64, 64]


def test_symbols_are_declared_exported_and_bound(lib):
    from rescan_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rescan_hip.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    assert callable(capi.Cloud.levels_many) and callable(capi.level_samples_many)
    shim_hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rescan_dropin.h")).read(), flags=re.S)
    shim = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "rescan_amd", "librescan_dropin.so")], text=True)
    assert re.search(r"\brsd_levels_poisson\s*\(", shim_hdr) and re.search(r" T rsd_levels_poisson$", shim, flags=re.M)


def test_refusals_need_no_device(lib):
    """A NULL base and the other host refusals come back with their code and text before anything touches a device (there is none
    where this test runs); the outputs stay as they were; a batch of no clouds or no levels is RS_HIP_OK."""
    radii = (C.c_float * 2)(0.02, 0.01); caps = (C.c_int32 * 2)(512, 256)
    bases = (C.c_void_p * 2)(None, None)
    out = (C.c_void_p * 4)(0x11, 0x22, 0x33, 0x44)
    counts = (C.c_int32 * 4)(-7, -7, -7, -7)
    idx = (C.c_void_p * 4)(None, None, None, None)
    rounds = C.c_int32(-9)

    def samples(b, nc, r, k, nl):
        return lib.rs_hip_level_samples_many(C.addressof(b) if b is not None else None, nc, C.addressof(r) if r is not None else None,
                                             C.addressof(k) if k is not None else None, nl, C.addressof(idx), C.addressof(counts), C.byref(rounds))

    def clouds(b, nc, r, k, nl):
        return lib.rs_hip_cloud_create_levels_many(C.addressof(b) if b is not None else None, nc, C.addressof(r) if r is not None else None,
                                                   C.addressof(k) if k is not None else None, None, nl, C.addressof(out), None, C.addressof(counts))
    for fn in (samples, clouds):
        assert fn(bases, 2, radii, caps, 2) == E_ARG
        assert b"cloud 0 is NULL" in lib.rs_hip_last_error(), lib.rs_hip_last_error()
        assert fn(bases, 1, (C.c_float * 2)(0.02, 0.0), caps, 2) == E_ARG and b"radius" in lib.rs_hip_last_error()
        assert fn(bases, 1, radii, (C.c_int32 * 2)(512, 0), 2) == E_ARG and b"max_n_neigh" in lib.rs_hip_last_error()
        assert fn(bases, 1, (C.c_float * 9)(*([0.5] * 9)), (C.c_int32 * 9)(*([9] * 9)), 9) == E_ARG and b"at most 8" in lib.rs_hip_last_error()
        assert fn(bases, -1, radii, caps, 2) == E_ARG and fn(bases, 2, radii, caps, -1) == E_ARG
        assert fn(None, 2, radii, caps, 2) == E_ARG and fn(bases, 2, None, caps, 2) == E_ARG and fn(bases, 2, radii, None, 2) == E_ARG
        assert fn(bases, 0, radii, caps, 2) == 0 and fn(None, 0, None, None, 2) == 0 and fn(bases, 2, radii, caps, 0) == 0
    assert list(out) == [0x11, 0x22, 0x33, 0x44] and list(counts) == [-7] * 4
    assert lib.rs_hip_cloud_create_levels_many(C.addressof(bases), 2, C.addressof(radii), C.addressof(caps), None, 2, None, None, None) == E_ARG
