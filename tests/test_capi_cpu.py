"""CPU: the C-ABI library builds, loads, exports every symbol include/rescan_hip.h declares, its
host-side helpers match the golden vectors, and compute entry points FAIL LOUDLY without a GPU
(no CPU fallback anywhere in the product path)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

LIB = os.path.join(ROOT, "rescan_amd", "librescan_hip.so")


@pytest.fixture(scope="module")
def lib():
    from rescan_amd import build, capi
    build.build()
    return capi.load()


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "rescan_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(rs_hip_[a-z0-9_]+)\s*\(", hdr)))


def test_every_declared_symbol_is_exported(lib):
    from rescan_amd import capi
    names = declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/rescan_hip.h but not exported"
        assert n in capi.SIGNATURES, f"{n} has no ctypes signature in rescan_amd/capi.py"
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = set(re.findall(r" T (rs_hip_[a-z0-9_]+)", out))
    assert set(names) <= exported


def test_code_object_is_gfx950_only():
    """Every device code object bundled in the library targets gfx950 (the .hip_fatbin entries are named
    `hipv4-amdgcn-amd-amdhsa--<arch>`; rocPRIM's host-side tuning tables mention other arch names as plain
    strings, which is not code)."""
    from rescan_amd import capi
    blob = open(capi.LIB_PATH, "rb").read()
    targets = set(re.findall(rb"hipv4-amdgcn-amd-amdhsa--([a-z0-9:+-]+)", blob))
    assert targets == {b"gfx950"}, targets


def test_product_does_not_touch_the_oracle():
    """rescan_amd/, include/, shadow/ and tools/ never import, link or name anything under oracle/ (only tests/,
    __graft_entry__.smoke() and bench.py's CPU-baseline leg do)."""
    for base in ("rescan_amd", "include", "shadow", "tools"):
        for dp, _, fs in os.walk(os.path.join(ROOT, base)):
            for f in fs:
                if f.endswith((".py", ".h", ".hip", ".cpp", ".sh")):
                    txt = open(os.path.join(dp, f), errors="ignore").read()
                    assert "pyoracle" not in txt and "rs_oracle" not in txt and "libref" not in txt, os.path.join(dp, f)
    from rescan_amd import capi
    needed = subprocess.check_output(["readelf", "-d", capi.LIB_PATH], text=True)
    assert "oracle" not in needed


def test_host_math_vs_golden(lib):
    from rescan_amd import capi
    g = load_golden("mat4.npz")
    for k in range(len(g["m"])):
        assert (capi.mat4_inverse(g["m"][k]) == g["inverse"][k]).all()
        assert (capi.mat4_mul(g["m"][k], g["b"][k]) == g["mul"][k]).all()


def test_device_sincosf_model_is_the_host_libm(lib):
    """The reference composes its poses with libm's sinf/cosf (msh_vec_math.h:2091-2092), which are not correctly
    rounded (0.85 % of the arguments differ from the rounded double result); the ICP loop runs on the device, so the
    device carries a restatement of glibc's algorithm.  It must return libm's bits: ICP-step-sized angles, the whole
    polynomial range, the range-reduced one, the large-argument one (|x| >= 120, which a one-normal segment's step reaches:
    tests/hard_systems.py) log-uniformly up to FLT_MAX and uniformly up to 1e4, and the edges of each: 120 itself, both sides of
    every power of two above it, FLT_MAX.  Inf and NaN give NaN.  (A stand-alone host build of the model had zero mismatches on
    3.7e7 arguments of that range, every 37th float from 120 to FLT_MAX among them.)"""
    import ctypes as C
    from rescan_amd import capi
    libm = C.CDLL("libm.so.6")
    libm.sinf.restype = C.c_float; libm.sinf.argtypes = [C.c_float]
    libm.cosf.restype = C.c_float; libm.cosf.argtypes = [C.c_float]
    rng = np.random.default_rng(1)
    x = np.concatenate([
        rng.uniform(-0.2, 0.2, 60000), rng.uniform(-0.75, 0.75, 40000), rng.uniform(-120, 120, 40000),
        10.0 ** rng.uniform(-7, -2, 20000) * rng.choice([-1, 1], 20000),
        np.array([0.0, -0.0, 2.0 ** -12, np.nextafter(np.float32(2.0 ** -12), np.float32(0)), 0.75, np.nextafter(np.float32(0.75), np.float32(0)),
                  np.pi / 4, np.pi / 2, np.pi, 119.99999, 120.0, 1e5, -1e5]),
        np.exp(rng.uniform(np.log(120.0), np.log(3.4e38), 60000)) * rng.choice([-1, 1], 60000), rng.uniform(120, 1e4, 20000),
    ]).astype(np.float32)
    edges = np.ldexp(np.float32(1), np.arange(7, 128)).astype(np.float32).view(np.uint32)[:, None].astype(np.int64) + np.arange(-2, 3)
    edges = edges[edges < 0x7f800000].astype(np.uint32)
    fmax = np.finfo(np.float32).max
    x = np.concatenate([x, edges.ravel().view(np.float32), -edges.ravel().view(np.float32),
                        np.array([120.0, -120.0, np.nextafter(np.float32(120), np.float32(121)), fmax, -fmax], np.float32)])
    s, c = capi.sincosf_model(x)
    want_s = np.array([libm.sinf(float(v)) for v in x], np.float32)
    want_c = np.array([libm.cosf(float(v)) for v in x], np.float32)
    assert (s.view(np.uint32) == want_s.view(np.uint32)).all(), x[s.view(np.uint32) != want_s.view(np.uint32)][:8]
    assert (c.view(np.uint32) == want_c.view(np.uint32)).all(), x[c.view(np.uint32) != want_c.view(np.uint32)][:8]
    assert (np.abs(x) >= 120).sum() > 80000
    s, c = capi.sincosf_model(np.array([np.inf, -np.inf, np.nan], np.float32))
    assert np.isnan(s).all() and np.isnan(c).all()
    # the point of the exercise: libm is NOT the correctly rounded function
    assert (want_s != np.sin(x.astype(np.float64)).astype(np.float32)).sum() > 100


def test_two_over_pi_words_are_what_integer_arithmetic_gives():
    """The 24 words of 2/pi that rs_sincosf_model's large-argument reduction reads (rescan_amd/csrc/rs_math.h), computed again:
    pi from Machin's formula in integers with 64 guard bits, 2/pi by one integer division to 400 bits, word i =
    floor(2/pi * 2^(8 (i + 1))) mod 2^32.  The computation is itself checked: its leading 53 bits are the double 2 / math.pi."""
    import math

    def atan_inv(q, bits):                       # atan(1 / q) * 2^bits
        t = (1 << bits) // q
        s, k = t, 1
        while t:
            t //= q * q
            k += 2
            s += -(t // k) if (k // 2) % 2 else t // k
        return s
    B = 400
    pi = (16 * atan_inv(5, B + 64) - 4 * atan_inv(239, B + 64)) >> 64
    two_over_pi = (2 << (2 * B)) // pi
    assert abs((two_over_pi >> (B - 60)) / 2.0 ** 60 - 2 / math.pi) < 2.0 ** -52
    assert abs(pi / 2.0 ** B - math.pi) < 2.0 ** -50
    words = [(two_over_pi >> (B - 8 * (i + 1))) & 0xffffffff for i in range(24)]
    src = open(os.path.join(ROOT, "rescan_amd", "csrc", "rs_math.h")).read()
    body = re.search(r"const uint32_t W\[24\] = \{(.*?)\};", src, flags=re.S).group(1)
    assert [int(w.rstrip("u"), 16) for w in re.findall(r"0x[0-9a-f]+u", body)] == words


def test_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from rescan_amd import capi
    with pytest.raises(capi.RescanHipError):
        capi.init(0)
    with pytest.raises(capi.RescanHipError):
        capi.Cloud(np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32))
    rc = lib.rs_hip_synchronize()
    assert rc == -1 and b"no HIP device" in lib.rs_hip_last_error()


def test_cloud_layout_refuses_without_a_cloud(lib):
    """rs_hip_cloud_layout needs a cloud, and a cloud needs a device: without either it answers RS_HIP_E_ARG, names itself in the
    error text and leaves the caller's struct alone — before it touches the HIP runtime."""
    from rescan_amd import capi
    L = capi.Layout()
    L.n_tiles = 77
    assert lib.rs_hip_cloud_layout(None, ctypes.addressof(L)) == -2 and b"cloud_layout" in lib.rs_hip_last_error()
    assert L.n_tiles == 77 and not L.cell_start
    assert lib.rs_hip_cloud_layout(None, None) == -2
    assert [k for k, _ in capi.Layout._fields_][-len(capi.Layout.ARRAYS):] == list(capi.Layout.ARRAYS)
    assert ctypes.sizeof(capi.Layout) == 5 * 4 + 3 * 4 + 3 * 8 + 3 * 4 + 4 + 9 * 8      # (one word of padding before the pointers)


def test_spin_flags_hand_work_between_threads():
    """tools/benchaux (the harness's own helper library, NOT the product ABI): a worker thread and the caller ping-pong through two
    int32 flags without ever sleeping in a queue; a wait that cannot succeed times out; and none of these helpers is exported by
    librescan_hip.so any more (round-2 verdict: bench plumbing out of the product ABI)."""
    import threading
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import benchaux
    flags = np.zeros(4, np.int32)
    addr = lambda k: flags.ctypes.data + 4 * k          # noqa: E731
    seen = []

    def worker():
        for k in range(1, 201):
            benchaux.spin_wait(addr(0), k, 30.0)
            seen.append(k)
            benchaux.spin_post(addr(1), k)

    t = threading.Thread(target=worker)
    t.start()
    for k in range(1, 201):
        (benchaux.spin_post if k % 2 else benchaux.spin_post_holding_gil)(addr(0), k)
        benchaux.spin_wait(addr(1), k, 30.0)
        assert seen[-1] == k
    t.join()
    with pytest.raises(RuntimeError):
        benchaux.spin_wait(addr(0), 10 ** 6, 0.05)
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    assert not re.search(r"rs_hip_(spin_|post_|probe_placement)", out)


def test_missing_extension_is_an_error(monkeypatch, tmp_path):
    from rescan_amd import capi
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(capi.RescanHipError):
        capi.load()


def test_graft_entry_build():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(os.path.join(ROOT, "rescan_amd", "librescan_hip.so"))
    assert os.path.exists(os.path.join(ROOT, "oracle", "librs_oracle.so"))


def test_icp_batch_entry_points_validate_arguments_first(lib):
    """rs_hip_icp_align_batch / _multi and rs_hip_icp_trace_begin reject null arrays and negative counts with RS_HIP_E_ARG
    before they read anything (the batch used to copy its start poses through T1s first) — and without a device.  In a
    child process: a regression would read through a null pointer."""
    code = r"""
import ctypes as C, sys
lib = C.CDLL(sys.argv[1])
vp, i32, f = C.c_void_p, C.c_int32, C.c_float
buf = (C.c_float * 64)(); ibuf = (C.c_int32 * 16)(); src = (C.c_void_p * 1)(1)
for name in ("rs_hip_icp_align_batch", "rs_hip_icp_align_multi"):
    fn = getattr(lib, name); fn.restype = C.c_int
    fn.argtypes = [vp, vp, vp, i32, vp, f, f, i32, i32, vp, vp]
    first = C.addressof(src) if name.endswith("multi") else None
    assert fn(first, None, None, 1, buf, 0.1, 1.0, 10, 0, buf, ibuf) == -2, name                   # null T1s (and clouds)
    assert fn(first, None, buf, -1, buf, 0.1, 1.0, 10, 0, buf, ibuf) == -2, name                   # n < 0
    assert fn(None, None, buf, 1, None, 0.1, 1.0, 10, 0, None, ibuf) == -2, name                   # null T2 / errs
tb = lib.rs_hip_icp_trace_begin; tb.restype = C.c_int; tb.argtypes = [vp, vp, vp, vp, i32, i32]
assert tb(None, buf, ibuf, ibuf, 2, 1) == -2 and tb(buf, buf, ibuf, ibuf, 0, 1) == -2 and tb(buf, buf, ibuf, ibuf, 2, -3) == -2
lib.rs_hip_icp_trace_end.restype = C.c_int
assert lib.rs_hip_icp_trace_end() == 0
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code, LIB], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
