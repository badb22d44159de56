"""CPU side of tests/test_gpu_coop_stream.py: its yardstick is not the code under test, its inputs are what their names say, and the
row table's index arithmetic (rescan_amd/csrc/rs_rowtable.h) agrees with a linear walk in a stand-alone, sanitized host program."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_coop_stream as cs  # noqa: E402


def test_brute_force_agrees_with_the_oracle(oracle):
    """brute_find_corrs against oracle.icp_find_corrs on every case (no case holds two candidates at one d² from a query that matter:
    the oracle's order among exact ties is its heap's, DESIGN.md §4 — the comparison would show one)."""
    for name, c in cs.cases().items():
        want = oracle.icp_find_corrs(c["src"], c["src_nor"], c["tgt"], c["tgt_nor"], cs.I4, cs.I4, cs.R, cs.MA)
        cs.assert_brute(name, want, name)


def _cell_index(v, gmin, cell):
    f = np.float32
    return np.floor((v.astype(f) - f(gmin)) * (f(1.0) / f(cell))).astype(np.int64)


def test_cases_are_what_their_names_say():
    """Rows and stream length of every grid case from the grid arithmetic: the sweep of any tile — whatever queries the library's
    Hilbert order puts into it — covers all h x d rows, leaves the pins out and takes every placed point in."""
    cases = cs.cases()
    for name, c in cases.items():
        if c["rows"] is None:
            continue
        mn, dims = cs.grid_of(c)
        h, d, cell = c["h"], c["d"], c["cell"]
        assert dims[1] == h and dims[2] == d and mn[0] == np.float32(cs.PIN_X) and mn[1] == 0.0 and mn[2] == 0.0, (name, dims, mn)
        x0s, x1s = [], []
        for q in c["src"]:
            assert cs.axis_cells(q[1], q[1], cs.R, mn[1], cell, h) == (0, h - 1), (name, "y", q)
            assert cs.axis_cells(q[2], q[2], cs.R, mn[2], cell, d) == (0, d - 1), (name, "z", q)
            x0, x1 = cs.axis_cells(q[0], q[0], cs.R, mn[0], cell, dims[0])
            x0s.append(x0); x1s.append(x1)
        placed = c["tgt"][2:]
        cx = np.minimum(_cell_index(placed[:, 0], mn[0], cell), dims[0] - 1) if len(placed) else np.zeros(0, np.int64)
        assert min(x0s) > 0, (name, "the pins' cell column is outside every query's reach")
        if name != "rank_15_16_17":        # (its three queries are 1 m apart: each reaches its own group only; the tile's box reaches all)
            assert len(cx) == 0 or (cx.min() >= max(x0s) and cx.max() <= min(x1s)), (name, "every placed point inside every query's x range")
        else:
            assert cx.min() >= min(x0s) and cx.max() <= max(x1s), name
        assert c["rows"] == h * d and c["stream"] == len(placed), name
    for rows in cs.ROW_SHAPES:
        assert cases[f"rows_{rows}"]["rows"] == rows
    assert {nw * 64 + e for nw in (2, 4, 8) for e in (-1, 0, 1)} == set(cs.ROW_SHAPES), "one row short of, exactly, and one row past a table for 2, 4 and 8 waves"
    for n in cs.STREAMS:
        assert cases[f"stream_{n}"]["stream"] == n and cases[f"stream_{n}"]["rows"] == 128
    assert {0, 1, 63, 64, 65} <= set(cs.STREAMS) and all(nw * 64 * dd + e in cs.STREAMS for nw in (2, 4, 8) for dd in cs.PREFETCH for e in (-1, 0, 1))
    # the rows a case's points lie in, from the binning itself
    def rows_of(c):
        mn, _ = cs.grid_of(c)
        p = c["tgt"][2:]
        return _cell_index(p[:, 2], mn[2], c["cell"]) * c["h"] + _cell_index(p[:, 1], mn[1], c["cell"])
    for row in (511, 64, 128, 448):
        c = cases[f"only_row_{row}"]
        assert c["rows"] == 512 and set(rows_of(c).tolist()) == {row}, row
    assert 511 == 8 * 64 - 1 and 64 % 64 == 0 and 128 % 64 == 0 and 448 == 7 * 64, "the table's last row at 8 waves; first rows of the blocks of waves 1, 2 (0 at 2 waves) and 7"
    for rows in cs.ROW_SHAPES:
        occ = np.unique(rows_of(cases[f"rows_{rows}"]))
        gaps = np.diff(occ)
        assert occ[-1] == rows - 1 and gaps.max() >= 10, (rows, "runs of empty rows between occupied ones, and the last row occupied")
    c = cases["rank_15_16_17"]
    near_edges = set(rows_of(c).tolist())
    assert {127, 128, 255, 256, 511, 512, 1023, 1024} <= near_edges, "closer candidates on both sides of every table edge"
    assert cs.brute("rank_15_16_17")[0].tolist() == [0], "15 closer: accepted; 16, 17: rejected"
    # outside the grid, within reach of it
    c = cases["outside_within_reach"]
    mn, dims = cs.grid_of(c)
    assert (_cell_index(c["src"][:, 1], mn[1], c["cell"]) < 0).all() and len(cs.brute("outside_within_reach")[0]) > 0
    # more than two tables' worth of rows for any query, at any NW
    c = cases["cells_r16"]
    mn, dims = cs.grid_of(c)
    for q in c["src"]:
        (y0, y1), (z0, z1) = cs.axis_cells(q[1], q[1], cs.R, mn[1], c["cell"], dims[1]), cs.axis_cells(q[2], q[2], cs.R, mn[2], c["cell"], dims[2])
        assert (y1 - y0 + 1) * (z1 - z0 + 1) > 2 * 8 * 64, q
    n = len(cs.brute("cells_r16")[0])
    assert 0 < n < len(c["src"]), "some queries are rejected by their rank, some accepted"


def test_row_table_arithmetic_in_a_sanitized_host_program(tmp_path):
    """tests/host/rowtable_check.cpp: the header the kernels use, against a linear walk, under the address and undefined-behaviour
    sanitizers.  A plain executable: nothing of it is loaded into this process."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rowtable_check")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",      # (the runtimes inside the executable: it needs nothing preloaded)
           "-I", os.path.join(ROOT, "rescan_amd", "csrc"), os.path.join(HERE, "host", "rowtable_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, (b.stdout[-2000:], b.stderr[-2000:])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "rowtable_check ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
