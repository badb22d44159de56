"""Writes tests/golden/normals_<name>.npz from the REFERENCE's own rs_pointcloud__compute_normals.

    python tools/normals_fixture/gen.py --ref /path/to/reference [--out tests/golden]

Run once, by hand, where the reference tree is available; no test runs it.  driver.cpp is compiled into a temporary directory
outside the tree (-O2 -std=c++11, no -march, as oracle/Makefile compiles the reference: no FMA contraction).

Fixtures (tests/test_normals_cpu.py, tests/test_gpu_normals.py compare them bit for bit where the value is not NaN), meshes from
tests/normal_meshes.py:
  normals_patch   hard_meshes.patch(): the 9 x 9 grid, one large triangle, two zero-area faces.
  normals_fan     one hub vertex named by 3 000 faces, in two face orders (faces, faces_shuffled) with the reference's output for each:
                  the hub's normal differs between them in its last bits.
  normals_quirks  cancellation, doubled and tripled vertices, an isolated vertex, overflow, NaN, underflow, denormals.
Each holds pos, faces, nor (the function alone), nor_loader (with rs_pointcloud__load_ply's pass, :743-751) and counts (the corners
that name each vertex: the reference frees its own array, so these are counted here).

    python tools/normals_fixture/gen.py --ref /path/to/reference --time

prints the reference's own time for the mesh of tools/normals_timing.py (this machine, one thread; context only)."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hard_meshes as H  # noqa: E402
import normal_meshes as M  # noqa: E402

F = np.float32
LARGEST = 757075


def reference(lib, pos, faces, loader_pass):
    L = C.CDLL(lib)
    L.fx_normals.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    out = np.zeros((len(pos), 3), F); sec = C.c_double()
    L.fx_normals(pos.ctypes.data, len(pos), faces.ctypes.data, len(faces), int(loader_pass), out.ctypes.data, C.addressof(sec))
    return out, sec.value


def both(lib, pos, faces, suffix=""):
    return {"nor" + suffix: reference(lib, pos, faces, 0)[0], "nor_loader" + suffix: reference(lib, pos, faces, 1)[0]}


def counts(pos, faces):
    return np.bincount(faces.ravel(), minlength=len(pos)).astype(np.int32)


def write(lib, out_dir, name):
    pos, faces = getattr(M, name)()
    out = dict(pos=pos, faces=faces, counts=counts(pos, faces), **both(lib, pos, faces))
    note = ""
    if name == "patch":
        assert len(faces) == 131 and not np.isnan(out["nor"]).any()
    if name == "fan":
        _, shuffled = M.fan_shuffled()
        out["faces_shuffled"] = shuffled
        out.update(both(lib, pos, shuffled, "_shuffled"))
        a, b = out["nor"][0], out["nor_shuffled"][0]
        assert out["counts"][0] == M.FAN_FACES and (a.view(np.uint32) != b.view(np.uint32)).any() and np.abs(a - b).max() < 1e-4, (a, b)
        rest = slice(1, None)                              # a rim vertex has two faces: their order can matter too, the hub's must
        note = f", hub {a!r} / shuffled {b!r}, {int((out['nor'][rest].view(np.uint32) != out['nor_shuffled'][rest].view(np.uint32)).any(1).sum())} rim normals differ"
    if name == "quirks":
        n, nl = out["nor"], out["nor_loader"]
        y = np.array([0.0, 1.0, 0.0], F)
        assert (n[[0, 1, 2, 3, 4, 9]] == y).all(), "cancellation, zero cross products and the isolated vertex give +y"
        assert np.isnan(n[[10, 11, 12], 2]).all() and (nl[[10, 11, 12]] == 0).all(), "overflow: NaN after the finish, zeros after the loader's pass"
        assert (n[[13, 14, 15]] == y).all(), "a NaN fails the compare"
        assert (n[16:22] == y).all() and not (n[22:25] == y).all(1).any() and not np.isnan(n[22:25]).any(), "underflow gives +y, a denormal sum a normal"
        assert (out["counts"][[3, 4, 5, 8, 9]] == [7, 2, 5, 4, 0]).all()
        assert not np.isnan(nl).any()
    path = os.path.join(out_dir, f"normals_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= LARGEST, f"{path}: {size} bytes, larger than the largest fixture there is"
    print(f"{name}: {len(pos)} vertices, {len(faces)} faces, {int(np.isnan(out['nor']).sum())} NaN entries{note}, {size} bytes -> {path}")


def time_reference(lib):
    m = H.big()
    ts = [reference(lib, m["pos"], m["faces"], 0)[1] for _ in range(5)]
    print(f"reference CPU (this machine, one thread): rs_pointcloud__compute_normals, {len(m['pos'])} vertices, {len(m['faces'])} faces: "
          f"median {1e3 * np.median(ts):.1f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="only print the reference's CPU time for the mesh of tools/normals_timing.py")
    ap.add_argument("--ref", default=os.environ.get("REF"), required="REF" not in os.environ)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as tmp:
        lib = os.path.join(tmp, "librsfx.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++11", "-fPIC", "-w", "-shared", f"-I{a.ref}/lib", f"-I{a.ref}/lib/rs",
                               "-o", lib, os.path.join(here, "driver.cpp"), "-lm"])
        if a.time:
            return time_reference(lib)
        for name in ("patch", "fan", "quirks"):
            write(lib, a.out, name)


if __name__ == "__main__":
    main()
