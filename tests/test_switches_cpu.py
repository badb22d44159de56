"""CPU: rescan_amd/csrc/rs_switches.h is the one place that reads the environment; its table is the parent's switches (names, kinds,
defaults, the moment each is read, setters: tests/switch_table_parent.py); rs_hip_switch_get reports them; the eleven setters keep
their contracts; and the documents and tools/switch_matrix.sh name only switches that exist."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from switch_table_parent import AT_LEAST, PARENT, STORED

CSRC = os.path.join(ROOT, "rescan_amd", "csrc")
ROW = re.compile(r'X\(\s*(\w+),\s*"(RS_\w+)",\s*(\w+),\s*([^,]+?),\s*(\w+),\s*"(\w*)",\s*(\w+),\s*([^,]+?),\s*"([^"]+)"\s*\)')
NAME = re.compile(r"\bRS_(?:HIP|DROPIN)_[A-Z0-9_]+")


def header_rows():
    """name -> (kind, default, class, setter, stored, at_least, meaning) as rs_switches.h's table has them."""
    txt = open(os.path.join(CSRC, "rs_switches.h")).read()
    rows = {}
    for _id, name, kind, default, cls, setter, stored, lo, meaning in ROW.findall(txt):
        assert name not in rows, name
        rows[name] = (kind.lower(), float(default), cls.lower(), setter or None, stored, None if lo == "SW_NO_MIN" else float(lo), meaning)
    assert len(rows) == txt.count("  X( "), "a row of the table does not parse"
    return rows


def child(code, env=None, *args):
    """`code` in a fresh Python process whose environment has none of the library's names but those of `env`."""
    e = {k: v for k, v in os.environ.items() if not NAME.match(k)}
    e.update(env or {})
    e["PYTHONPATH"] = ROOT
    out = subprocess.run([sys.executable, "-c", code, *args], env=e, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    return json.loads(out.stdout.strip().splitlines()[-1])


GET_ALL = "import json, sys; from rescan_amd import capi; print(json.dumps({n: capi.switch_get(n) for n in json.loads(sys.argv[1])}))"


@pytest.fixture(scope="module")
def built():
    from rescan_amd import build
    build.build()


def test_nothing_else_reads_the_environment():
    for f in sorted(os.listdir(CSRC)):
        if f != "rs_switches.h" and f.endswith((".h", ".hip", ".cpp")):
            assert "getenv" not in open(os.path.join(CSRC, f)).read(), f


def test_table_is_the_parents():
    rows = header_rows()
    assert set(rows) == set(PARENT), (sorted(set(rows) - set(PARENT)), sorted(set(PARENT) - set(rows)))
    for name, (kind, default, cls, setter) in PARENT.items():
        h = rows[name]
        want = float(np.float32(default)) if kind == "float" else float(default)
        have = float(np.float32(h[1])) if kind == "float" else h[1]
        assert (h[0], have, h[2], h[3]) == (kind, want, cls, setter), (name, h)
        assert h[5] == AT_LEAST.get(name), name
        assert h[4] == {"rs_hip_icp_exact_centroids": "MODE"}.get(setter, "ONOFF" if setter in STORED else "ASIS"), name
        assert h[6].strip(), name


def test_defaults_in_a_clean_process(built):
    got = child(GET_ALL, None, json.dumps(sorted(PARENT)))
    for name, (kind, default, _cls, _setter) in PARENT.items():
        assert got[name] == (float(np.float32(default)) if kind == "float" else float(default)), name


def distinctive(k, kind):
    """(text, value): a non-default setting of the k-th name — beyond 32 bits for i64, an exact float, `0` for a flag (set at all)."""
    if kind == "flag":
        return "0", 1.0
    if kind == "word":
        return "spin", 1.0
    if kind == "int":
        return str(1000 + k), 1000.0 + k
    if kind == "i64":
        return str(5_000_000_000 + k), 5e9 + k
    if kind == "float":
        return repr(0.625 + k / 64.0), 0.625 + k / 64.0
    return repr(1234.5 + k), 1234.5 + k


def test_every_name_set_in_a_fresh_process(built):
    names = sorted(PARENT)
    env, want = {}, {}
    for k, n in enumerate(names):
        env[n], want[n] = distinctive(k, PARENT[n][0])
    got = child(GET_ALL, env, json.dumps(names))
    assert got == want
    # ... and below their clamps
    low = child(GET_ALL, {n: "-5" for n in AT_LEAST}, json.dumps(sorted(AT_LEAST)))
    assert low == {n: float(v) for n, v in AT_LEAST.items()}


def test_switch_get_refuses_unknown_names(built):
    from rescan_amd import capi
    for bad in ("RS_HIP_NO_SUCH_SWITCH", "RS_HIP_LIB", "", "RS_HIP_NO_WAR"):
        with pytest.raises(capi.RescanHipError):
            capi.switch_get(bad)
    assert capi.load().rs_hip_switch_get(b"RS_HIP_NO_WARM", None) == -2


def test_setters_return_the_previous_value_and_store(built):
    from rescan_amd import capi
    setters = {s: n for n, (_k, _d, _c, s) in PARENT.items() if s}
    assert len(setters) == 11
    for k, (setter, name) in enumerate(sorted(setters.items())):
        fn = getattr(capi, setter[len("rs_hip_"):])
        kind = PARENT[name][0]
        new = 0.25 + k / 1024.0 if kind == "float" else (1 << 40) + k if kind == "i64" else 2 if setter in STORED else 100 + k
        stored = STORED.get(setter, lambda v: v)(new)
        before = fn(-1)
        try:
            assert before == capi.switch_get(name)
            assert fn(new) == before, setter                      # the previous value comes back
            assert fn(-1) == stored and fn(-7) == stored          # a negative argument leaves the value alone
            assert capi.switch_get(name) == stored, setter
            assert fn(0) == stored and fn(-1) == 0 and capi.switch_get(name) == 0.0
        finally:
            fn(before)
        assert fn(-1) == before
    for fn, arg in ((capi.icp_exact_centroids, 3), (capi.icp_early_plain, 7)):
        before = fn(-1)
        try:
            fn(arg)
            assert fn(-1) == 1
        finally:
            fn(before)
    before = capi.icp_exact_centroids(2)
    assert capi.icp_exact_centroids(before) == 2               # (2 is a mode of its own)


def test_live_is_seen_and_first_is_latched(built):
    code = """
import json, os
from rescan_amd import capi
out = [capi.switch_get("RS_HIP_NO_WARM"), capi.switch_get("RS_HIP_ROWS_TILED_FROM"), capi.switch_get("RS_HIP_ICP_CHUNK"), capi.switch_get("RS_HIP_REF_ORDER_BELOW")]
os.environ.update(RS_HIP_NO_WARM="1", RS_HIP_ROWS_TILED_FROM="0", RS_HIP_ICP_CHUNK="9", RS_HIP_REF_ORDER_BELOW="5")
out += [capi.switch_get("RS_HIP_NO_WARM"), capi.switch_get("RS_HIP_ROWS_TILED_FROM"), capi.switch_get("RS_HIP_ICP_CHUNK"), capi.switch_get("RS_HIP_REF_ORDER_BELOW")]
del os.environ["RS_HIP_NO_WARM"]
out += [capi.switch_get("RS_HIP_NO_WARM")]
print(json.dumps(out))
"""
    #                      clean                       live: seen   first, boot: not   live again
    assert child(code) == [0.0, 4096.0, 4.0, 16384.0,  1.0, 0.0,    4.0, 16384.0,      0.0]


def test_the_shim_reads_its_switches_through_the_table(built):
    """RS_DROPIN_STATS is read when librescan_dropin.so is loaded — after the table it reads it from is there."""
    code = """
import ctypes, json, os, sys
lib = ctypes.CDLL(os.path.join(sys.argv[1], "rescan_amd", "librescan_dropin.so"))
grid = (ctypes.c_char * 120)(); pts = (ctypes.c_float * 30)(*range(30))
lib.msh_hash_grid_init_3d.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_float]
lib.msh_hash_grid_init_3d(grid, pts, 10, 0.5)
lib.msh_hash_grid_term.argtypes = [ctypes.c_void_p]
lib.msh_hash_grid_term(grid)
print(json.dumps("ok"))
"""
    e = {k: v for k, v in os.environ.items() if not NAME.match(k)}
    e.update(RS_DROPIN_STATS="1", RS_DROPIN_INIT_WITHOUT_DEVICE="1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], env=e, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "[rescan_hip stats] grid init (host index)" in out.stderr, out.stderr


def public_macros():
    hdr = open(os.path.join(ROOT, "include", "rescan_hip.h")).read()
    return set(re.findall(r"^#define\s+(RS_HIP_[A-Z0-9_]+)", hdr, flags=re.M))


def is_exception(name):
    """Names with the switches' prefix that are no switches: RS_HIP_LIB (the Python binding's: which build to load) and the
    constants include/rescan_hip.h defines (error codes, RS_HIP_KNN_MAX_K, the step kinds), also written as a family: RS_HIP_E_*.
    (RS_X, a name nothing reads, and bench.py's RS_BENCH_* do not carry the prefix.)"""
    macros = public_macros()
    return name == "RS_HIP_LIB" or name in macros or (name.endswith("_") and any(m.startswith(name) for m in macros))


def test_documents_and_matrix_name_only_switches_that_exist():
    rows = header_rows()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec6 = design[design.index("\n## 6. "):design.index("\n## 7. ")]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    matrix = open(os.path.join(ROOT, "tools", "switch_matrix.sh")).read()
    for where, txt in (("DESIGN.md §6", sec6), ("INTEGRATION.md", integration), ("tools/switch_matrix.sh", matrix)):
        for name in set(NAME.findall(txt)):
            assert name in rows or is_exception(name), (where, name)
    assert "rs_switches.h" in sec6 and "rs_switches.h" in integration
    documented = set(NAME.findall(sec6)) | set(NAME.findall(integration))
    assert not set(rows) - documented, sorted(set(rows) - documented)


def test_matrix_stops_at_the_first_failure():
    matrix = open(os.path.join(ROOT, "tools", "switch_matrix.sh")).read()
    assert "set -o pipefail" in matrix and "timeout -k 10 " in matrix and re.search(r"if \[ \$rc -ne 0 \]; then .*exit \$rc", matrix)
