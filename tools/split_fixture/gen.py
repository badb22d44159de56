"""Writes tests/golden/split_<name>.npz from the REFERENCE's own pointcloud_to_rsdb (apps/seg2rsdb/main.cpp:45-159): driver.cpp includes
apps/seg2rsdb/main.cpp itself, its main renamed on the command line, and calls pointcloud_to_rsdb on a level 0 assembled from arrays,
with the class table synth.write_class_table writes and rsdb_load reads.  The two values that function does not keep — the centroid
rs_pointcloud_centroid returns and the transform — are read out by its statements :113-126 in order, on the same arrays (fx_centroid),
and checked against what pointcloud_to_rsdb stored: the pose and the transformed points.

    python tools/split_fixture/gen.py [--ref /path/to/reference] [--out tests/golden]

Run once, by hand, where the reference tree is available; no test runs it.  driver.cpp is compiled into a temporary directory
outside the tree (-O2 -std=c++11, no -march, as oracle/Makefile compiles the reference: no FMA contraction).

Fixtures (tests/test_split_cpu.py, tests/test_gpu_split.py compare every array bit for bit):
  split_room     synth.make_scene( seed=21, width=2.0, depth=2.0, height=0.6, density=800.0, objects=("chair",) ) with the attribute
                 arrays drawn as tools/fuse_fixture/gen.py draws them: 6 122 points, four instances, floor and walls static, the chair
                 dynamic.  The scan's seven arrays; the table; the seven cut arrays of all objects, concatenated in table order;
                 centroids (as rs_pointcloud_centroid returns them, before y = 0), xforms and poses.
  split_quirks   case_<name>_*: an instance whose points carry two classes, the first point's class deciding both ways (mixed_static,
                 mixed_dynamic); ids INT32_MIN, -1, 1024, INT32_MAX (extreme_ids); n = 1 (single); 70 points with 70 ids (seventy);
                 an id whose first point is the last of the scan (last_first); ids interleaved ABAB across a wave (abab).
  split_hostile  stream_<name>_*: the streams of tests/hard_split.py, each as a one-instance dynamic scan: the scan, the centroid, the
                 transform, the pose and the transformed arrays.

    python tools/split_fixture/gen.py --time

prints the reference's own time for the room of tools/split_timing.py (this machine, one thread; context only)."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rescan_amd import synth  # noqa: E402

F = np.float32
KEYS = ("pos", "nor", "col", "radii", "qual", "cls", "inst")
LARGEST = 757075          # the largest fixture there is (scene.npz)
STATIC = [synth.CLASS_IDX[k] for k in synth.STATIC_CLASSES]
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1


class Arrays(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in KEYS]


def empty(n):
    return dict(pos=np.zeros((n, 3), F), nor=np.zeros((n, 3), F), col=np.zeros((n, 3), F), radii=np.zeros(n, F), qual=np.zeros(n, F),
                cls=np.zeros(n, np.int32), inst=np.zeros(n, np.int32))


def handle(a):
    for k in KEYS:
        assert a[k].flags["C_CONTIGUOUS"] and a[k].dtype in (F, np.int32), k
    return Arrays(*[a[k].ctypes.data for k in KEYS])


def attributes(rng, pos, nor, cls, inst):
    n = len(pos)
    return dict(pos=np.ascontiguousarray(pos, F), nor=np.ascontiguousarray(nor, F), col=rng.uniform(0, 1, (n, 3)).astype(F),
                radii=rng.uniform(0.004, 0.012, n).astype(F), qual=rng.uniform(0, 1, n).astype(F),
                cls=np.ascontiguousarray(cls, np.int32), inst=np.ascontiguousarray(inst, np.int32))


def load(lib):
    L = C.CDLL(lib)
    L.fx_split.restype = C.c_int32
    L.fx_split.argtypes = [C.c_char_p, C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 6
    L.fx_centroid.restype = C.c_int64
    L.fx_centroid.argtypes = [C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 5
    return L


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.itemsize]
    nan = np.isnan(b) if b.dtype.kind == "f" else np.zeros(b.shape, bool)
    an = np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.shape, bool)
    return a.shape == b.shape and bool((an == nan).all() and (a.view(u)[~nan] == b.view(u)[~nan]).all())


def split(L, table, scan):
    """pointcloud_to_rsdb on the scan, and per instance what fx_centroid reads out.  Everything the fixtures hold."""
    n = len(scan["pos"])
    cap = n
    inst = np.zeros(cap, np.int32); cls = np.zeros(cap, np.int32); counts = np.zeros(cap, np.int64); poses = np.zeros((cap, 16), F)
    out = empty(n); seconds = C.c_double()
    hs, ho = handle(scan), handle(out)
    sys.stdout.flush()
    k = L.fx_split(table.encode(), C.addressof(hs), n, cap, inst.ctypes.data, cls.ctypes.data, counts.ctypes.data, poses.ctypes.data,
                   C.addressof(ho), C.addressof(seconds))
    assert k >= 0, k
    inst, cls, counts, poses = inst[:k].copy(), cls[:k].copy(), counts[:k].copy(), poses[:k].copy()
    assert counts.sum() == n
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    centroids = np.zeros((k, 3), F); xforms = np.zeros((k, 16), F)
    eye = np.eye(4, dtype=F).ravel()
    for j in range(k):
        m = int(counts[j])
        c = np.zeros(3, F); x = np.zeros(16, F); q = np.zeros(16, F); p = np.zeros((m, 3), F); nr = np.zeros((m, 3), F)
        got = L.fx_centroid(C.addressof(hs), n, int(inst[j]), c.ctypes.data, x.ctypes.data, q.ctypes.data, p.ctypes.data, nr.ctypes.data)
        assert got == m
        centroids[j] = c
        seg = slice(int(offsets[j]), int(offsets[j + 1]))
        if cls[j] in STATIC:
            xforms[j] = eye
            first = int(np.flatnonzero(scan["inst"] == inst[j])[0])
            assert scan["cls"][first] == cls[j]
        else:
            # the statements :113-126 and pointcloud_to_rsdb itself agree on the pose and on every transformed value
            xforms[j] = x
            assert same_bits(q, poses[j]) and same_bits(p, out["pos"][seg]) and same_bits(nr, out["nor"][seg]), j
    return dict(inst_ids=inst, class_of=cls, counts=counts, offsets=offsets, poses=poses, centroids=centroids, xforms=xforms, out=out,
                seconds=seconds.value)


def save(out_dir, name, out):
    path = os.path.join(out_dir, f"split_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < LARGEST, f"{path}: {size} bytes, not below the largest fixture there is"
    return path, size


def pack(prefix, scan, r):
    out = {f"{prefix}scan_{k}": scan[k] for k in KEYS}
    out.update({f"{prefix}out_{k}": r["out"][k] for k in KEYS})
    out.update({f"{prefix}{k}": r[k] for k in ("inst_ids", "class_of", "counts", "offsets", "poses", "centroids", "xforms")})
    return out


def room_scan():
    rng = np.random.default_rng(402)
    s = synth.make_scene(seed=21, width=2.0, depth=2.0, height=0.6, density=800.0, objects=("chair",))
    return attributes(rng, s["points"], s["normals"], s["class_idx"], s["instance_idx"])


def write_room(L, table, out_dir):
    scan = room_scan()
    r = split(L, table, scan)
    assert len(scan["pos"]) == 6122 and r["inst_ids"].tolist() == [3, 2, 0, 1] and r["counts"].tolist() == [1002, 960, 3200, 960]
    assert r["class_of"].tolist() == [5, 1, 2, 1]
    out = pack("", scan, r)
    out["static_classes"] = np.array(STATIC, np.int32)
    path, size = save(out_dir, "room", out)
    print(f"room: {len(scan['pos'])} points, instances {r['inst_ids'].tolist()} with {r['counts'].tolist()} points, classes {r['class_of'].tolist()}, {size} bytes -> {path}")


def quirk_cases():
    """name -> (class ids, instance ids); positions are drawn."""
    W, F_, CH, TB = synth.CLASS_IDX["wall"], synth.CLASS_IDX["floor"], synth.CLASS_IDX["chair"], synth.CLASS_IDX["table"]
    c = {}
    # one instance whose points carry two classes: the first point's decides (main.cpp:114)
    c["mixed_static"] = (np.array([W] + [CH] * 40 + [W] * 9), np.full(50, 4))
    c["mixed_dynamic"] = (np.array([CH] + [W] * 40 + [CH] * 9), np.full(50, 4))
    ids = np.array([I32_MAX, -1, I32_MIN, 1024, -1, I32_MIN, I32_MAX, 1024, 1024, -1] * 7)
    c["extreme_ids"] = (np.where(ids < 0, F_, TB), ids)
    c["single"] = (np.array([CH]), np.array([77]))
    c["seventy"] = (np.tile([CH, W, TB, F_, CH, TB, W], 10), (np.arange(70) * 37) % 70 - 20)
    c["last_first"] = (np.array([CH] * 99 + [TB]), np.array([5] * 99 + [6]))
    c["abab"] = (np.tile([CH, TB], 100), np.tile([11, 12], 100))
    return c


def write_quirks(L, table, out_dir):
    rng = np.random.default_rng(403)
    out = {}
    names = []
    for name, (cls, inst) in quirk_cases().items():
        n = len(inst)
        pos = rng.uniform(-1.5, 1.5, (n, 3)); nor = rng.normal(0, 1, (n, 3)); nor /= np.linalg.norm(nor, axis=1)[:, None]
        nor[::5, 0] = -0.0; pos[::7, 2] = -0.0                      # a static object's -0.0 must stay -0.0
        scan = attributes(rng, pos, nor, cls, inst)
        r = split(L, table, scan)
        out.update(pack(f"case_{name}_", scan, r)); names.append(name)
    r = lambda name: {k: out[f"case_{name}_{k}"] for k in ("inst_ids", "class_of", "counts", "xforms")}        # noqa: E731
    eye = np.eye(4, dtype=F).ravel()
    assert r("mixed_static")["class_of"].tolist() == [synth.CLASS_IDX["wall"]] and (r("mixed_static")["xforms"][0] == eye).all()
    assert r("mixed_dynamic")["class_of"].tolist() == [synth.CLASS_IDX["chair"]] and not (r("mixed_dynamic")["xforms"][0] == eye).all()
    assert r("extreme_ids")["inst_ids"].tolist() == [I32_MAX, -1, I32_MIN, 1024]
    assert len(r("seventy")["inst_ids"]) == 70 and (r("seventy")["counts"] == 1).all()
    assert r("last_first")["inst_ids"].tolist() == [5, 6] and r("last_first")["counts"].tolist() == [99, 1]
    z = out["case_mixed_static_out_nor"]
    assert np.signbit(z[z == 0]).any(), "no -0.0 survives in the static object"
    out["names"] = np.array(names); out["static_classes"] = np.array(STATIC, np.int32)
    path, size = save(out_dir, "quirks", out)
    print(f"quirks: {names}, {size} bytes -> {path}")


def write_hostile(L, table, out_dir):
    import hard_split as H
    out = {}
    finite = []
    for name in H.STREAMS:
        pos, nor, cls, inst = H.scan(name)
        rng = np.random.default_rng(404)
        scan = attributes(rng, pos, nor, cls, inst)
        r = split(L, table, scan)
        assert r["inst_ids"].tolist() == [H.INSTANCE] and r["class_of"].tolist() == [H.DYNAMIC_CLASS]
        # the reference's chain is the sequential sum hard_split.py restates
        want = H.centroid_of(H.seq_sum(pos[:, 0]), len(pos))
        assert same_bits(r["centroids"][0, :1], np.array([want], F)), (name, r["centroids"][0], want)
        out.update({f"stream_{name}_{k}": v for k, v in (("pos", scan["pos"]), ("nor", scan["nor"]), ("centroid", r["centroids"][0]), ("xform", r["xforms"][0]),
                                                         ("pose", r["poses"][0]), ("out_pos", r["out"]["pos"]), ("out_nor", r["out"]["nor"]))})
        if all(np.isfinite(out[f"stream_{name}_{k}"]).all() for k in ("centroid", "xform", "pose", "out_pos", "out_nor")):
            finite.append(name)
    # the NaN allowance of the comparison must not be able to hide a failure: these outputs hold no NaN at all
    assert set(finite) == set(H.FINITE), finite
    m = H.measure("cancel")
    assert m["seq_centroid"] != m["exact_centroid"]
    out["names"] = np.array(H.STREAMS); out["finite"] = np.array(finite); out["static_classes"] = np.array(STATIC, np.int32)
    path, size = save(out_dir, "hostile", out)
    print(f"hostile: {len(H.STREAMS)} streams, entirely finite outputs for {finite}, {size} bytes -> {path}")


def time_reference(L, table):
    import split_timing as T
    scan = T.room()
    rng = np.random.default_rng(405)
    a = attributes(rng, scan["pos"], scan["nor"], scan["cls"], scan["inst"])
    r = split(L, table, a)
    print(f"reference CPU (this machine, one thread): pointcloud_to_rsdb on {len(a['pos'])} points, {len(r['inst_ids'])} instances: {1e3 * r['seconds']:.1f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="only print the reference's CPU time for the room of tools/split_timing.py")
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default="", help="write this fixture alone (room, quirks, hostile)")
    a = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as tmp:
        lib = os.path.join(tmp, "librsfx.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++11", "-fPIC", "-w", "-shared", "-Dmain=seg2rsdb_main", f"-I{a.ref}", f"-I{a.ref}/lib",
                               f"-I{a.ref}/lib/rs", "-o", lib, os.path.join(here, "driver.cpp"), "-lm"])
        table = os.path.join(tmp, "classes.txt")
        synth.write_class_table(table)
        L = load(lib)
        if a.time:
            return time_reference(L, table)
        for name, write in (("room", write_room), ("quirks", write_quirks), ("hostile", write_hostile)):
            if a.only in ("", name):
                write(L, table, a.out)


if __name__ == "__main__":
    main()
