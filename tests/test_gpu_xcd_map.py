"""Phase A's tile map (rescan_amd/csrc/rs_xcdmap.h; k_icp_corr: natural_tile): the Hilbert order cut into chunks of C natural blocks
dealt round-robin to the eight XCD classes.  A workgroup that takes the wrong block leaves a tile unsearched or searches one twice;
neither changes a single bit of a tile that IS searched, so the tests look for the tile that is not: source clouds whose tile counts
sit on the edges of a chunk and of a round of eight chunks, searched under two poses back to back (an unsearched tile keeps the
first pose's rows), every point's match against the brute-force rows of tests/hard_clouds.py.

The clouds.  A tile is a run of at most 64 points of the Hilbert order whose box stays within the tile extent (0.3 m at most) on
every axis.  The sources are CLUSTERS on a lattice of 0.35 m: the 2 or 3 points of a cluster share one position (and so one Hilbert
key: they are neighbours in the order) and differ in their normals, two clusters never share a tile — a cloud of n clusters has
exactly n tiles (asserted through Cloud.n_tiles), and the clouds are prefixes of one list of clusters, so one set of brute-force
rows serves them all.  The target holds a few dozen points around every cluster.  Normals are axis directions: a dot product is
-1, 0 or 1, nowhere near the 60 degree gate.  The poses are translations, so a query is fl( p + t ) whatever the order of the
transform's additions.

Launches of this size go straight to the cooperative kernel by default, and the switches that decide it are latched at the library's
first use: everything runs in child processes (a new python running this file as a script, each under its own time limit) with
RS_HIP_COOP_ALL_BELOW=0 — phase A first — and with the slow-tile thresholds lowered to these clouds' few candidates per tile, so
that the front slots, flag 1 and flag 2 take part.  The children run one after the other, and after one that failed none is started."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import hard_clouds as hc  # noqa: E402

I4 = np.eye(4, dtype=np.float32).ravel()
R = np.float32(0.1)
MA = np.float32(np.deg2rad(60.0))
K = 16
WHAT = ("c_pts1", "c_nor1", "c_pts2", "c_nor2", "weights")
N_ITER = 10


def shipped_chunk():
    """C of the library as built by default: 2^RS_XCD_CHUNK_LOG2 of rs_xcdmap.h (the cold launch's, the one every first search takes)."""
    text = open(os.path.join(ROOT, "rescan_amd", "csrc", "rs_xcdmap.h")).read()
    k = int(re.search(r"^#define RS_XCD_CHUNK_LOG2 (-?\d+)", text, re.M).group(1))
    assert 0 <= k <= 10, "the tests are written for a chunked map"
    return 1 << k


C_ = shipped_chunk()
TILE_COUNTS = (1, C_, C_ + 1, 8 * C_ - 1, 8 * C_, 8 * C_ + 1, 17 * C_ + 3)
ALIGN_TILES = 8 * C_ + 1
MULTI_TILES = (1, 2 * C_, 8 * C_ + 1)
SPACING = np.float32(0.35)                   # more than the largest tile extent (RS_HIP_TILE_EXTENT_MAX, 0.3 m): two clusters never share a tile
AXES = np.float32([[0, 0, 1], [1, 0, 0], [0, 0, -1], [0, 1, 0], [-1, 0, 0], [0, -1, 0]])
POSES = (np.float32([0.0625, 0.0, 0.0]), np.float32([-0.0625, 0.03125, 0.015625]))      # further apart than the radius: a point keeps no match from one to the other
ALIGN_T0 = np.float32([0.01, -0.0075, 0.005])

# child -> its environment.  Thresholds in candidates streamed by a tile's lone wave: a tile here streams a few dozen.
BASE_ENV = {"RS_HIP_COOP_ALL_BELOW": "0", "RS_HIP_HEAVY_STREAMED": "24", "RS_HIP_HEAVY_HANDOFF": "48"}
CHILDREN = {"chunks": dict(BASE_ENV), "no_lpt": dict(BASE_ENV, RS_HIP_NO_LPT="1")}


def pose(t):
    T = I4.copy()
    T[12:15] = t
    return T


_WORLD = {}


def world():
    """(cluster of every source point, source positions, source normals, target positions, target normals) of the largest cloud;
    the cloud of n tiles is the points of the first n clusters."""
    if not _WORLD:
        n_cl = max(TILE_COUNTS)
        g = int(np.ceil(n_cl ** (1.0 / 3.0)))
        i = np.arange(n_cl)
        centre = (np.stack([i % g, (i // g) % g, i // (g * g)], axis=1).astype(np.float32) * SPACING).astype(np.float32)
        mult = 2 + (i % 2)
        cl = np.repeat(i, mult)
        within = np.concatenate([np.arange(m) for m in mult])
        src = centre[cl]
        src_nor = AXES[(cl + 2 * within) % 3]                       # a cluster's points: +z, +x, -z in turn, from a start that moves on
        rng = np.random.default_rng(20)
        per = np.where(i % 5 == 0, 96, 40)                          # every fifth cluster: more than 16 points within reach of most queries
        tcl = np.repeat(i, per)
        tgt = (centre[tcl] + rng.uniform(-0.16, 0.16, (len(tcl), 3)).astype(np.float32)).astype(np.float32)
        tgt_nor = AXES[rng.integers(0, 6, len(tcl))]
        _WORLD.update(cl=cl, src=np.ascontiguousarray(src), src_nor=np.ascontiguousarray(src_nor), tgt=np.ascontiguousarray(tgt), tgt_nor=np.ascontiguousarray(tgt_nor))
    return _WORLD


def n_points(n_tiles):
    return int(np.searchsorted(world()["cl"], n_tiles))


_EXPECT = {}


def expected(which):
    """Per source point of the largest cloud under POSES[which]: (query, slot or -1, d², dot) — the reference's rule on the brute-force
    rows: the nearest candidate within the radius whose normal passes the gate, if fewer than 16 candidates precede it in (d², index)."""
    if which not in _EXPECT:
        w = world()
        q = (w["src"] + POSES[which][None, :]).astype(np.float32)
        D, I, n, _, _ = hc.brute_rows(w["tgt"], q, R, K)
        tn, qn = w["tgt_nor"][I], w["src_nor"][:, None, :]
        dot = (tn[..., 0] * qn[..., 0] + tn[..., 1] * qn[..., 1]) + tn[..., 2] * qn[..., 2]
        dc = np.maximum(dot, np.float32(0.0))
        ok = (np.arange(K)[None, :] < n[:, None]) & (dc >= np.float32(np.cos(np.float64(MA))))
        first = np.argmax(ok, axis=1)
        rows = np.arange(len(q))
        has = ok.any(axis=1)
        _EXPECT[which] = q, np.where(has, I[rows, first], -1), D[rows, first], dc[rows, first]
    return _EXPECT[which]


def assert_corrs(got, n_tiles, which, what):
    """slot (through the matched point and normal), d² and dot (through the weight) of every point of the cloud of n_tiles tiles"""
    w = world()
    n = n_points(n_tiles)
    q, slot, d2, dot = (a[:n] for a in expected(which))
    rows = np.nonzero(slot >= 0)[0]
    assert len(got[0]) == len(rows), (what, "correspondences", len(got[0]), len(rows))
    s = slot[rows]
    for a, b, field in zip((q[rows], w["src_nor"][:n][rows], w["tgt"][s], w["tgt_nor"][s]), got[:4], WHAT):
        bad = np.nonzero((a.view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=1))[0]
        assert len(bad) == 0, (what, field, "first differing source points (clusters = tiles)", rows[bad[:5]].tolist(), w["cl"][rows[bad[:5]]].tolist())
    # icp.h:387: w = ( 1 - d² / max_dist ) * dot, then zero where d² > 2.5 stddev( d² ): every weight is the uncut one or zero, and
    # the zeroed ones are the far ones
    uncut = ((np.float32(1.0) - d2[rows] / R) * dot[rows]).astype(np.float32)
    wt = np.ascontiguousarray(got[4])
    zero = wt == 0.0
    assert (uncut > 0.0).all() and (wt.view(np.uint32)[~zero] == uncut.view(np.uint32)[~zero]).all(), (what, "weights: d² or dot of a match")
    if zero.any() and (~zero).any():
        assert d2[rows][zero].min() > d2[rows][~zero].max(), (what, "weights: the cut")


# ---- the children ----------------------------------------------------------------------------------------------------------------

def result_bytes(err, T, it):
    return np.frombuffer(np.float32(err).tobytes() + np.asarray(T, np.float32).tobytes() + np.int32(it).tobytes(), np.uint8)


def compute(capi):
    """Everything a child is asked for, as a flat dict of arrays."""
    w = world()
    out = {}
    tgt = capi.Cloud(w["tgt"], w["tgt_nor"], cell_size=0.1)
    clouds = {}
    for nt in sorted(set(TILE_COUNTS) | set(MULTI_TILES) | {ALIGN_TILES}):
        n = n_points(nt)
        clouds[nt] = capi.Cloud(w["src"][:n], w["src_nor"][:n], cell_size=0.1)
        out[f"tiles/{nt}"] = np.int64([clouds[nt].n_tiles, n])
    for nt in TILE_COUNTS:
        for which in (0, 1):
            for a, what in zip(capi.icp_find_corrs(clouds[nt], tgt, pose(POSES[which]), I4, R, MA), WHAT):
                out[f"corrs/{nt}/{which}/{what}"] = a
    out["align"] = result_bytes(*capi.icp_align(clouds[ALIGN_TILES], tgt, pose(ALIGN_T0), I4, 0.1, MA, max_iter=N_ITER, fixed_iters=True))
    T0s = np.stack([pose(ALIGN_T0 * np.float32(s)) for s in (1.0, -1.0, 0.5)])
    errs, Ts, its = capi.icp_align_multi([clouds[nt] for nt in MULTI_TILES], tgt, T0s, I4, 0.1, MA, max_iter=N_ITER, fixed_iters=True)
    for p, nt in enumerate(MULTI_TILES):
        out[f"multi/{p}"] = result_bytes(errs[p], Ts[p], its[p])
        out[f"single/{p}"] = result_bytes(*capi.icp_align(clouds[nt], tgt, T0s[p], I4, 0.1, MA, max_iter=N_ITER, fixed_iters=True))
    for c in clouds.values():
        c.close()
    tgt.close()
    return out


def child_main(path):
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()                  # (torch's copy of the HIP runtime first: tests/conftest.py)
    except ImportError:
        pass
    from rescan_amd import capi
    capi.init(0)
    np.savez(path, **compute(capi))


_CHILD = {}
_FAILED = []


def child(name, tmp_path_factory):
    """The results of child `name`: it runs once per session, under its own time limit; a failed child fails the test, and after a
    child that failed (a fault, an abort, a time limit) no further child is started."""
    if name not in _CHILD:
        assert not _FAILED, f"not started: the child {_FAILED[0]} failed"
        path = str(tmp_path_factory.mktemp("xcd_map") / (name + ".npz"))
        env = {k: v for k, v in os.environ.items() if not k.startswith("RS_HIP_") or k == "RS_HIP_LIB"}
        env.update(CHILDREN[name])
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), path]
        try:
            p = subprocess.run(cmd, env=env, timeout=60, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            _FAILED.append(name)
            raise
        if p.returncode != 0:
            _FAILED.append(name)
        assert p.returncode == 0, (name, p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        _CHILD[name] = dict(np.load(path))
    return _CHILD[name]


@pytest.mark.gpu
def test_clouds_have_the_tile_counts_their_names_say(tmp_path_factory):
    got = child("chunks", tmp_path_factory)
    for nt in sorted(set(TILE_COUNTS) | set(MULTI_TILES) | {ALIGN_TILES}):
        assert got[f"tiles/{nt}"].tolist() == [nt, n_points(nt)], nt
    assert {1, C_, C_ + 1, 8 * C_ - 1, 8 * C_, 8 * C_ + 1, 17 * C_ + 3} == set(TILE_COUNTS)


@pytest.mark.gpu
@pytest.mark.parametrize("n_tiles", TILE_COUNTS)
def test_every_tile_is_searched_under_both_poses(tmp_path_factory, n_tiles):
    got = child("chunks", tmp_path_factory)
    for which in (0, 1):
        assert_corrs([got[f"corrs/{n_tiles}/{which}/{w}"] for w in WHAT], n_tiles, which, (n_tiles, "pose", which))


@pytest.mark.gpu
def test_ten_iterations_carry_the_same_bits_without_the_slow_tile_lists(tmp_path_factory):
    """pose, error and iteration count of a ten-iteration icp_align at 8 C + 1 tiles: front slots, flags 1 and 2 and the warm
    launches against RS_HIP_NO_LPT, where every tile is taken by the natural part in every launch"""
    a, b = child("chunks", tmp_path_factory), child("no_lpt", tmp_path_factory)
    assert int(np.frombuffer(a["align"].tobytes()[-4:], np.int32)[0]) == N_ITER
    assert np.isfinite(np.frombuffer(a["align"].tobytes()[:-4], np.float32)).all()
    assert a["align"].tobytes() == b["align"].tobytes()
    for nt in TILE_COUNTS:
        for which in (0, 1):
            for w in WHAT:
                assert a[f"corrs/{nt}/{which}/{w}"].tobytes() == b[f"corrs/{nt}/{which}/{w}"].tobytes(), (nt, which, w)


@pytest.mark.gpu
def test_three_sources_in_one_call_equal_three_calls(tmp_path_factory):
    """icp_align_multi of sources of 1, 2 C and 8 C + 1 tiles — the grid is the largest problem's — bit for bit the single calls"""
    for name in CHILDREN:
        got = child(name, tmp_path_factory)
        for p in range(len(MULTI_TILES)):
            assert got[f"multi/{p}"].tobytes() == got[f"single/{p}"].tobytes(), (name, MULTI_TILES[p])
        # (a source of two or three points stops when its step degenerates; the largest runs all ten)
        assert int(np.frombuffer(got[f"multi/{len(MULTI_TILES) - 1}"].tobytes()[-4:], np.int32)[0]) == N_ITER


if __name__ == "__main__":
    child_main(sys.argv[1])
