"""CPU: the batched cloud build's two entry points (rs_hip_cloud_create_many, rs_hip_cloud_many_single_above) are declared, exported
and bound; they answer without a device where they can; and the grouping rule of the batch (rs_buildplan.h: bp_many_groups) holds on
the batches of tests/host/buildmany_check.cpp, a plain host program run under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("rs_hip_cloud_create_many", "rs_hip_cloud_many_single_above")


@pytest.fixture(scope="module")
def lib():
    from rescan_amd import build, capi
    build.build()
    return capi.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from rescan_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rescan_hip.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    assert callable(capi.Cloud.many) and callable(capi.cloud_many_single_above)


def test_setter_reads_and_returns_the_previous_value(lib):
    from rescan_amd import capi
    before = capi.cloud_many_single_above()
    try:
        assert capi.cloud_many_single_above(-5) == before
        assert capi.cloud_many_single_above(100) == before
        assert capi.cloud_many_single_above(-1) == 100
        assert capi.cloud_many_single_above(0) == 100 and capi.cloud_many_single_above() == 0
    finally:
        capi.cloud_many_single_above(before)
    assert capi.cloud_many_single_above() == before


def test_refusals_and_the_empty_batch_need_no_device(lib):
    """Bad arguments are refused with RS_HIP_E_ARG before anything else happens, `out` stays as it was, and a batch of no clouds is
    RS_HIP_OK: all without touching a device (there is none where this test runs)."""
    fn = lib.rs_hip_cloud_create_many
    pts = (C.c_float * 6)(0, 0, 0, 1, 1, 1)
    pos = (C.c_void_p * 2)(C.addressof(pts), C.addressof(pts))
    out = (C.c_void_p * 2)(0x1234, 0x5678)
    n = (C.c_int32 * 2)(2, 2)

    def call(pos_, n_, k, out_):
        return fn(C.addressof(pos_) if pos_ is not None else None, None, C.addressof(n_) if n_ is not None else None, None, k,
                  C.addressof(out_) if out_ is not None else None)
    assert call(pos, n, -1, out) == -2 and b"create_many" in lib.rs_hip_last_error()
    assert call(pos, n, 2, None) == -2
    assert call(pos, (C.c_int32 * 2)(2, -3), 2, out) == -2 and b"cloud 1" in lib.rs_hip_last_error()
    assert call((C.c_void_p * 2)(C.addressof(pts), None), n, 2, out) == -2 and b"cloud 1" in lib.rs_hip_last_error()
    assert call(None, n, 2, out) == -2 and call(pos, None, 2, out) == -2
    assert call(pos, n, 0, out) == 0 and call(None, None, 0, out) == 0
    assert out[0] == 0x1234 and out[1] == 0x5678


def test_grouping_rule_in_a_sanitized_host_program(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "buildmany_check")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-Wall", "-Werror", "-Wno-unknown-pragmas",     # (the runtimes inside the executable: it needs nothing preloaded)
           "-I", os.path.join(ROOT, "rescan_amd", "csrc"), os.path.join(HERE, "host", "buildmany_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, (b.stdout[-2000:], b.stderr[-2000:])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().startswith("buildmany_check ok"), (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
