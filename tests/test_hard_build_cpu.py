"""CPU: the restatement of the index build (tests/build_restate.py) holds its own invariants on the clouds of tests/hard_builds.py, is
tied to the expressions the kernels compile (rescan_amd/csrc/rs_buildplan.h, run by tests/host/buildplan_check.cpp under the
sanitizers), and shows what the build did before that header: trial cells outside their bit table when a coordinate is +Inf."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import build_restate as R  # noqa: E402
import hard_builds as H  # noqa: E402

F = np.float32
SCALE, EXTENT_MAX = F(1.0), F(0.3)          # the switches' defaults: nothing here depends on the environment


def test_restated_hilbert_index_is_a_unit_step_bijection():
    for bits in (3, 4, 5):
        side = 1 << bits
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3).astype(np.uint32)
        h = R.hilbert3(g[:, 0], g[:, 1], g[:, 2], bits)
        assert sorted(h.tolist()) == list(range(side ** 3))
        along = g[np.argsort(h)].astype(np.int64)
        assert (np.abs(np.diff(along, axis=0)).sum(axis=1) == 1).all(), "consecutive indices are unit steps"


def assert_tiling(q, tiles, limit):
    n = len(q)
    assert tiles[0] == 0 or n == 0
    assert tiles[-1] == n and (np.diff(tiles.astype(np.int64)) > 0).all(), "tiles partition [0, n)"
    with np.errstate(all="ignore"):
        for a, b in zip(tiles[:-1], tiles[1:]):
            a, b = int(a), int(b)
            assert b - a <= 64

            def box(pts):
                lo, hi = pts[0].copy(), pts[0].copy()
                for p in pts[1:]:
                    lo, hi = np.fmin(lo, p), np.fmax(hi, p)
                return hi - lo
            assert not (box(q[a:b]) > limit).any(), (a, b)
            if b - a < 64 and b < n:
                assert (box(q[a:b + 1]) > limit).any(), ("a short tile that its next point would not stretch beyond the limit", a, b)


def families():
    return H.all_families()


@pytest.fixture(scope="module")
def plans():
    """name -> (family, {layout name: plan}), computed once"""
    out = {}
    for name, maker in families():
        f = maker()
        out[name] = (f, {ln: R.plan(f["points"], c, f["normals"], SCALE, EXTENT_MAX) for ln, c in f["cells"]})
    return out


def test_restated_tiling_keeps_its_invariants(plans):
    for name, (f, by_layout) in plans.items():
        for ln, P in by_layout.items():
            assert_tiling(f["points"][P["qorder"]], P["tiles"], P["extent_limit"])
            n = len(f["points"])
            assert sorted(P["order"].tolist()) == list(range(n)) and sorted(P["qorder"].tolist()) == list(range(n))
            assert (P["qorder"][P["by_orig"]] == np.arange(n)).all()
            assert int(P["cell_start"][-1]) == n and P["occupied"] <= max(n, 1)
    for n in H.SIZES:
        assert plans[f"stones_{n}"][1]["auto"]["n_tiles"] == n
        if n >= 64:
            assert (np.diff(plans[f"blob_{n}"][1]["auto"]["tiles"].astype(np.int64))[:-1] == 64).all(), "a dense cloud's tiles are full"
    lens = np.diff(plans["clusters_4097"][1]["auto"]["tiles"].astype(np.int64))
    assert len(set(lens.tolist())) > 40 and lens.max() == 64, "tile lengths follow the cluster sizes, cut at 64"


def test_cell_edge_families_test_something():
    """fp32 rounding decides the cell of some point: its cell in float, as the kernel computes it, is not its cell in exact
    arithmetic.  Points on k * cell, a step either side and on the box maximum are all there."""
    for name in H.CELL_EDGES:
        f = H.make(name)
        (_, c), = f["cells"]
        P = R.plan(f["points"], c, None, SCALE, EXTENT_MAX)
        got = R.cell_coords(f["points"], P["min"], P["inv_cell"], P["dims"])
        exact = H.float64_cells(f["points"], P["min"], P["cell"], P["dims"].astype(np.int64))
        differ = (got != exact).any(axis=1).sum()
        assert differ > 0, name
        assert (np.abs(got - exact) <= 1).all()
        assert (got.max(axis=0) == P["dims"] - 1).all() and (got.min(axis=0) == 0).all()
    f = H.make("cell_edges")
    on, = np.nonzero((np.fmod(f["points"], F(0.25)) == 0).all(axis=1))
    assert len(on) > 10


def outside_table(trials):
    """(points whose word is outside the bit table, points) over the counted trial grids"""
    out = total = 0
    for _, _, g, ids in trials:
        out += sum(1 for i in ids if (i >> 5) >= g["words"])
        total += len(ids)
    return out, total


def test_trial_cells_stay_inside_their_bit_table():
    """The witness: as the build stood, one +Inf coordinate reset its axis to [0, 0] and left every other point of that axis to mark
    a bit by its unclamped cell — most of them beyond the table.  With the clamp no family writes outside its table."""
    f = H.make("one_pinf")
    mn, mx = R.bounds(f["points"], finite_only=False)
    assert mn[0] == 0 and mx[0] == 0 and mx[1] > 4
    trials = []
    R.auto_cell(f["points"], mn, mx, SCALE, clamped=False, trace=trials)
    out, total = outside_table(trials)
    print("one_pinf, unclamped:", out, "of", total, "marks outside", [g["words"] for _, _, g, _ in trials], "words")
    assert out > 0
    for name, maker in families():
        f = maker()
        if not len(f["points"]):
            continue
        mn, mx = R.bounds(f["points"])
        trials = []
        R.auto_cell(f["points"], mn, mx, SCALE, clamped=True, trace=trials)
        out, total = outside_table(trials)
        assert out == 0, (name, out, total)
        for _, _, g, ids in trials:
            assert max(ids) < g["cells"] and min(ids) >= 0


def host_report(P):
    """what tests/host/buildplan_check.cpp prints for the cloud of plan P"""
    b = lambda v: "%08x" % int(F(v).view(np.uint32))      # noqa: E731
    lines = ["mn " + " ".join(b(v) for v in P["min"]), "mx " + " ".join(b(v) for v in P["max"])]
    for attempt, c0, g, ids in P["trials"]:
        lines.append("trial %d c0 %s td %d %d %d top %s words %d occupied %d idsum %d" % (
            attempt, b(c0), g["td"][0], g["td"][1], g["td"][2], " ".join(b(v) for v in g["top"]), g["words"], len(set(ids)), sum(ids) % (1 << 64)))
    lines.append("cell_size " + b(P["cell_size"]))
    lines.append("cell %s inv_cell %s dims %d %d %d" % (b(P["cell"]), b(P["inv_cell"]), *P["dims"]))
    lines.append("occupied %d limit %s" % (P["occupied"], b(P["restated_limit"])))
    lines.append("hilbert_scale " + b(P["hilbert_scale"]))
    lines.append("buildplan_check ok")
    return lines


def test_build_arithmetic_in_a_sanitized_host_program(tmp_path, plans):
    """tests/host/buildplan_check.cpp: the header the kernels and the host's decisions are compiled from, on every family under every
    layout, under the address, undefined-behaviour and float-cast sanitizers, every index inside a table of the library's size; its
    output equals the restatement's field for field.  A plain executable: nothing of it is loaded into this process."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "buildplan_check")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-Wall", "-Werror", "-Wno-unknown-pragmas",     # (the runtimes inside the executable: it needs nothing preloaded)
           "-I", os.path.join(ROOT, "rescan_amd", "csrc"), os.path.join(HERE, "host", "buildplan_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, (b.stdout[-2000:], b.stderr[-2000:])
    src, dst = str(tmp_path / "cloud.bin"), str(tmp_path / "plan.bin")
    ran = 0
    for name, (f, by_layout) in plans.items():
        for ln, c in f["cells"]:
            P = by_layout[ln]
            with open(src, "wb") as fh:
                fh.write(struct.pack("<ifff", len(f["points"]), c, SCALE, EXTENT_MAX)); fh.write(f["points"].tobytes())
            p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, (name, ln, p.returncode, p.stdout[-2000:], p.stderr[-2000:])
            got, want = p.stdout.split("\n")[:-1], host_report(P)
            if len(f["points"]) and P["inv_cell"] == 0:       # (the brute layout: its occupied cells are an estimate that goes through pow, the limit is held to its range)
                lim = np.array([int(got[-3].split()[-1], 16)], np.uint32).view(F)[0]
                assert F(0.25) <= lim <= EXTENT_MAX, (name, lim)
                got, want = got[:-3] + got[-2:], want[:-3] + want[-2:]
            assert got == want, (name, ln, [(g, w) for g, w in zip(got, want) if g != w][:3], len(got), len(want))
            arr = np.fromfile(dst, np.uint32)
            n = len(f["points"])
            assert (arr[:n] == P["cell_ids"]).all() and (arr[n:] == P["keys"]).all(), (name, ln)
            ran += 1
    assert ran > 200
