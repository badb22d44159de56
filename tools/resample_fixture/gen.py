"""Writes tests/golden/resample_<name>.npz from the REFERENCE's own rs_pointcloud_uniform_resample and
msh_discrete_distribution_init.

    python tools/resample_fixture/gen.py [--ref /path/to/reference] [--out tests/golden]

Run once, by hand, where the reference tree is available; no test runs it.  driver.cpp is compiled into a temporary directory
outside the tree (-O2 -std=c++11, no -march, as oracle/Makefile compiles the reference: no FMA contraction).

Fixtures (tests/test_resample_cpu.py, tests/test_gpu_resample.py compare every array bit for bit), meshes from tests/hard_meshes.py:
  resample_patch  a bumpy 9 x 9 grid, one large triangle, two zero-area faces; about 6 000 samples.  The mesh, the six output arrays,
                  the sampled face per sample, prob, alias, n_samples, total_area.
  resample_skew   200 faces whose areas span six decades, one of them with more than 99 % of the area; about 3 000 samples.  The same.
  resample_long   two triangles, more than 65 536 samples.  The mesh, n_samples, total_area, prob, alias, the SHA-256 of each output
                  array's bytes, and the first and last 256 samples in full.
An alias entry the reference leaves unwritten (its prob is 1.0; driver.cpp finds them) is stored as the column's own index.

    python tools/resample_fixture/gen.py --time

prints the reference's own time for the mesh of tools/resample_timing.py (this machine, one thread; context only)."""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hard_meshes as H  # noqa: E402

F = np.float32
KEYS = ("pos", "nor", "col", "radii", "cls", "inst")
ENDS = 256


def fp(a):
    return a.ctypes.data_as(C.c_void_p)


def reference(lib, m, faces_too=True):
    L = C.CDLL(lib)
    L.fx_resample.restype = C.c_void_p
    L.fx_resample.argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.fx_get.argtypes = [C.c_void_p] * 7
    L.fx_free.argtypes = [C.c_void_p]
    L.fx_alias.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    n, sec = C.c_int64(), C.c_double()
    h = L.fx_resample(*[fp(m[k]) for k in KEYS], len(m["pos"]), fp(m["faces"]), len(m["faces"]), C.addressof(n), C.addressof(sec))
    n = n.value
    out = dict(pos=np.zeros((n, 3), F), nor=np.zeros((n, 3), F), col=np.zeros((n, 3), F), radii=np.zeros(n, F),
               cls=np.zeros(n, np.int32), inst=np.zeros(n, np.int32))
    L.fx_get(h, *[fp(out[k]) for k in KEYS])
    L.fx_free(h)
    out["n_samples"], out["seconds"] = n, sec.value
    if faces_too:
        nf = len(m["faces"])
        prob, alias, written = np.zeros(nf, np.float64), np.zeros(nf, np.int32), np.zeros(nf, np.uint8)
        total, face = C.c_double(), np.zeros(n, np.int32)
        L.fx_alias(fp(m["pos"]), fp(m["faces"]), nf, fp(prob), fp(alias), fp(written), C.addressof(total), fp(face), n)
        assert (prob[written == 0] == 1.0).all(), "an alias entry that differs between two runs belongs to a column with prob < 1"
        out["prob"], out["alias"] = prob, np.where(written == 1, alias, np.arange(nf, dtype=np.int32)).astype(np.int32)
        out["total_area"], out["face"] = np.float64(total.value), face
    return out


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def write(lib, out_dir, name):
    m = getattr(H, name)()
    r = reference(lib, m)
    n = r["n_samples"]
    out = {"mesh_" + k: m[k] for k in KEYS + ("faces",)}
    out.update(n_samples=np.int64(n), total_area=r["total_area"], prob=r["prob"], alias=r["alias"])
    if name == "long":
        assert n > 65536 + ENDS
        for k in KEYS + ("face",):
            out["sha256_" + k], out["head_" + k], out["tail_" + k] = digest(r[k]), r[k][:ENDS], r[k][n - ENDS:]
    else:
        for k in KEYS + ("face",):
            out[k] = r[k]
    # the cases the tests rely on
    used = np.bincount(r["face"], minlength=len(m["faces"]))
    if name == "patch":
        assert 5000 <= n <= 7000 and len(m["faces"]) == 131 and (used[-2:] == 0).all() and used[-3] > n // 3, (n, used[-3:])
    if name == "skew":
        big = int(np.argmax(used))
        assert 2500 <= n <= 3500 and used[big] > 0.99 * n and (r["alias"] == big).sum() >= 190 and (r["prob"] < 1e-4).any(), (n, used[big])
    path = os.path.join(out_dir, f"resample_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 757075, f"{path}: {size} bytes, larger than the largest fixture there is"
    print(f"{name}: {len(m['pos'])} vertices, {len(m['faces'])} faces, {n} samples, total area {float(r['total_area'])!r}, "
          f"{int((r['prob'] == 1.0).sum())} columns with prob 1, {int(np.isnan(r['nor']).sum())} NaN normal entries, {size} bytes -> {path}")


def time_reference(lib):
    m = H.big()
    ts = []
    for _ in range(3):
        r = reference(lib, m, faces_too=False)
        ts.append(r["seconds"])
    print(f"reference CPU (this machine, one thread): rs_pointcloud_uniform_resample, {len(m['pos'])} vertices, {len(m['faces'])} faces, "
          f"{r['n_samples']} samples: median {1e3 * np.median(ts):.1f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="only print the reference's CPU time for the mesh of tools/resample_timing.py")
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as tmp:
        lib = os.path.join(tmp, "librsfx.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++11", "-fPIC", "-w", "-shared", f"-I{a.ref}/lib", f"-I{a.ref}/lib/rs",
                               "-o", lib, os.path.join(here, "driver.cpp"), "-lm"])
        if a.time:
            return time_reference(lib)
        for name in ("patch", "skew", "long"):
            write(lib, a.out, name)


if __name__ == "__main__":
    main()
