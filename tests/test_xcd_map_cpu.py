"""Phase A's tile map (rescan_amd/csrc/rs_xcdmap.h: which natural block a workgroup of k_icp_corr takes, the grid's natural part, a
tile's XCD class) holds its contract in a stand-alone, sanitized host program."""
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_xcd_map as xm  # noqa: E402


def test_the_gpu_tests_yardstick_agrees_with_the_oracle(oracle):
    """tests/test_gpu_xcd_map.py's expectation — the brute-force rows of tests/hard_clouds.py, the gate and the rank on top — is what
    oracle.icp_find_corrs returns on its clouds under both poses (every size: the clouds are prefixes of the largest), and its
    assert_corrs passes the oracle's arrays and fails a stale tile: one cluster's rows of the other pose."""
    w = xm.world()
    assert len(set(xm.TILE_COUNTS)) == 7 and xm.n_points(max(xm.TILE_COUNTS)) == len(w["src"]) and xm.n_points(1) == 2
    # two clusters never share a tile and a cluster's points share one position
    first = np.searchsorted(w["cl"], np.arange(max(xm.TILE_COUNTS)))
    c = w["src"][first]
    assert (w["src"] == c[w["cl"]]).all() and np.bincount(w["cl"]).max() <= 3 and np.bincount(w["cl"]).min() >= 2
    gaps = np.abs(c[:, None, :] - c[None, :, :]).max(axis=2)
    np.fill_diagonal(gaps, 1.0)
    assert gaps.min() > 0.3 + 0.04, "every pair of clusters is further apart on some axis than the largest tile extent"
    for which in (0, 1):
        want = oracle.icp_find_corrs(w["src"], w["src_nor"], w["tgt"], w["tgt_nor"], xm.pose(xm.POSES[which]), xm.I4, xm.R, xm.MA)
        _, slot, _, _ = xm.expected(which)
        assert 0.3 * len(slot) < (slot >= 0).sum() < 0.95 * len(slot), "matched and unmatched points"
        xm.assert_corrs(want, max(xm.TILE_COUNTS), which, ("oracle", which))
    # a source of fewer tiles: the oracle's weights are cut by ITS correspondences' statistics
    nt = xm.ALIGN_TILES
    n = xm.n_points(nt)
    want = oracle.icp_find_corrs(w["src"][:n], w["src_nor"][:n], w["tgt"], w["tgt_nor"], xm.pose(xm.POSES[1]), xm.I4, xm.R, xm.MA)
    xm.assert_corrs(want, nt, 1, ("oracle", nt))
    # the two poses differ in most rows: a tile left with the other pose's rows shows
    s0, s1 = xm.expected(0)[1], xm.expected(1)[1]
    per_cluster = np.bincount(w["cl"], weights=(s0 != s1))
    assert (per_cluster > 0).mean() > 0.95, "in nineteen clusters of twenty some point's match differs between the poses"
    stale = oracle.icp_find_corrs(w["src"][:n], w["src_nor"][:n], w["tgt"], w["tgt_nor"], xm.pose(xm.POSES[0]), xm.I4, xm.R, xm.MA)
    try:
        xm.assert_corrs(stale, nt, 1, "stale")
    except AssertionError:
        pass
    else:
        raise AssertionError("the other pose's rows pass")


def test_tile_map_arithmetic_in_a_sanitized_host_program(tmp_path):
    """tests/host/xcdmap_check.cpp: the header the kernel, its launch and the census use — every tile once, every workgroup in its own
    class, ascending within a class, a grid that is a multiple of 8, the contiguous eighths restated literally, two problems under one
    grid — under the address and undefined-behaviour sanitizers.  A plain executable: nothing of it is loaded into this process."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "xcdmap_check")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",      # (the runtimes inside the executable: it needs nothing preloaded)
           "-I", os.path.join(ROOT, "rescan_amd", "csrc"), os.path.join(HERE, "host", "xcdmap_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, (b.stdout[-2000:], b.stderr[-2000:])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "xcdmap_check ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
