"""The numpy restatements of tests/rows_restate.py (level builder, neighbourhood graph, label transfer) against the CPU oracle on
the hard families of tests/hard_clouds.py and the inputs rows_restate adds to them.  tests/test_gpu_hard_rows.py holds the device
to the restatements, so the restatements must themselves be the reference's answer.  No GPU needed.

Where the reference's answer is an accident of its heap (a tie across the K-th slot of a full row; equidistant nearest object
points whose normals gate differently) the inputs are shown here to be free of it, or -- offset_1e4 and collinear under the
graph's K = 8 -- shown to have it, which is why the GPU test holds those two to bounds instead of to an edge list."""
import numpy as np
import pytest

import hard_clouds as hc
import rows_restate as R
from oracle.pyoracle import LEVEL_VOXEL, level_max_n_neigh

LEVEL_CASES = [(name, lv) for name in R.LEVEL_FAMILIES for lv in (1, 2, 3, 4)] + \
              [(name, lv) for name in ("collinear_sorted", "planar_raster", "repeated") for lv in (1, 2, 4)]


def level_points(name):
    return R.level_extra_inputs()[name][0] if name in ("collinear_sorted", "planar_raster", "repeated") else R.family(name)["points"]


# ---- level builder ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,level", LEVEL_CASES)
def test_level_restatement_equals_the_oracle(oracle, name, level):
    p = level_points(name)
    r, cap = LEVEL_VOXEL[level], level_max_n_neigh(level)
    got, within = R.level_samples(p, r)
    assert within <= cap                                      # the reference's own search is not truncated
    want = oracle.level_poisson(p, r, cap)
    assert len(got) == len(want) and (got == want).all()


@pytest.mark.parametrize("shuffled", [False, True])
def test_level_restatement_on_the_lattice(oracle, shuffled):
    p = R.lattice(shuffled=shuffled)
    got, within = R.level_samples(p, 0.125)
    assert within == 27
    want = oracle.level_poisson(p, 0.125, 512)
    assert len(got) == len(want) and (got == want).all()


@pytest.mark.parametrize("m", [256, 257])
def test_level_restatement_on_the_clusters(oracle, m):
    """The max_n_neigh boundary of the GPU file: every point of the cluster has all m within the radius, one sample."""
    c = R.cluster(m, 0.01)
    got, within = R.level_samples(c, 0.01)
    want = oracle.level_poisson(c, 0.01, m)
    assert within == m and list(got) == [0] and list(want) == [0]


# ---- neighbourhood graph ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.EDGE_TIE_FREE)
def test_edge_restatement_equals_the_oracle(oracle, name):
    """Pairs and orientation, self-edges included; the input has no tie across the K-th slot, so the answer is defined."""
    p, nor = R.edge_input(name)
    n = len(p)
    r = R.graph_radius(R.EDGE_R2)
    assert len(R.edge_bounds(p, r, R.EDGE_K)[2]) == 0
    D, I, nn, _, _ = hc.brute_rows(p, p, r, R.EDGE_K)
    a, b = R.edges(D, I, nn, n)
    wa, wb, ww = oracle.compute_neighborhood(p, nor, R.EDGE_K, R.EDGE_R2)
    o = np.argsort(R.edge_key(wa, wb, n), kind="stable")
    assert len(a) == len(wa) and (wa[o] == a).all() and (wb[o] == b).all()
    assert (a == b).sum() == n                                # every self-edge
    # and the weight is the reference's cost of the edge's own d² and dot
    d2, dot = R.edge_inputs(p, nor, wa, wb)
    assert (R.edge_costs(oracle, d2, dot, R.EDGE_R2).view(np.uint32) == ww.view(np.uint32)).all()


def assert_edges(oracle, p, nor, K, r2, rows=None, cache=None):
    """The restatement equals the oracle's edge list on an input without a tie across the K-th slot.  rows: brute-force rows of a
    larger K to cut down; cache: edge_bounds' sorted pairs."""
    n, r = len(p), R.graph_radius(r2)
    assert len(R.edge_bounds(p, r, K, cache)[2]) == 0
    D, I, nn = hc.truncate(rows, K)[:3] if rows is not None else hc.brute_rows(p, p, r, K)[:3]
    a, b = R.edges(D, I, nn, n)
    wa, wb, ww = oracle.compute_neighborhood(p, nor, K, r2)
    o = np.argsort(R.edge_key(wa, wb, n), kind="stable")
    assert len(a) == len(wa) and (wa[o] == a).all() and (wb[o] == b).all()
    d2, dot = R.edge_inputs(p, nor, wa, wb)
    assert (R.edge_costs(oracle, d2, dot, r2).view(np.uint32) == ww.view(np.uint32)).all()
    return len(a)


def test_edge_restatement_at_other_k(oracle):
    """K on both sides of 16 on the whole of offset_1e3: no row ties across the K-th slot at any of them, so the GPU file's
    comparison there is exact, and the restatement is the oracle's answer."""
    p, nor = R.edge_input("offset_1e3")
    rows = hc.brute_rows(p, p, R.graph_radius(R.EDGE_R2), 17)
    cache = {}
    counts = [assert_edges(oracle, p, nor, K, R.EDGE_R2, rows, cache) for K in (1, 2, 16, 17)]
    assert counts[0] == len(p) and counts[3] > counts[2] > counts[1] > counts[0]


def test_edge_restatement_at_the_scan_seams_and_on_the_lattice(oracle):
    """The prefixes of offset_1e3 around the seams of the edge scan, and the 0.0625 lattice at r² = 0.015625, K = 32 (27 within
    the radius: the set is defined despite the ties)."""
    P, N = R.edge_input("offset_1e3")
    for n in (1, 2, 1023, 1024, 1025, 2049):
        assert_edges(oracle, np.ascontiguousarray(P[:n]), np.ascontiguousarray(N[:n]), R.EDGE_K, R.EDGE_R2)
    lat = R.lattice()
    m = assert_edges(oracle, lat, np.tile(np.float32([0.0, 0.0, 1.0]), (len(lat), 1)), 32, 0.015625)
    assert m > 10 * len(lat)


@pytest.mark.parametrize("name,rows", [("offset_1e4", 18), ("collinear", 6)])
def test_tied_edge_families_have_ties(name, rows):
    """Rows with an exact tie across the 8th slot: which of the tied points the reference keeps is its heap's accident."""
    p, _ = R.edge_input(name)
    must, may, tied = R.edge_bounds(p, R.graph_radius(R.EDGE_R2), R.EDGE_K)
    assert len(tied) == rows and len(may) > len(must)


# ---- label transfer --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tmin(oracle):
    t = R.gate_tmin(oracle.label_gate)
    assert abs(float(t) - 0.3420201) < 1e-7
    return t


def assert_labels(oracle, tmin, scene_pos, scene_nor, objects, placements, radius, modes=(0, 1)):
    cache, out = {}, []
    for prio in modes:
        want = oracle.arrangement_to_labels(scene_pos, scene_nor, objects, placements, radius, prio, 37)
        got = R.arrangement(scene_pos, scene_nor, objects, placements, radius, prio, 37, tmin, oracle.mat4_inverse, cache)
        for k in ("labels", "order", "class_ids", "instance_ids"):
            assert (want[k] == got[k]).all(), (prio, k)
        assert (want["min_dists"].view(np.uint32) == got["min_dists"].view(np.uint32)).all(), prio
        assert got["tie_dependent"] == 0                      # a condition on the inputs: no decision hung on the heap's choice
        out.append(got)
    return out


@pytest.mark.parametrize("name", hc.FAMILIES)
def test_label_restatement_equals_the_oracle(oracle, tmin, name):
    f = R.family(name)
    objects, placements = R.six_placements(f)
    a, b = assert_labels(oracle, tmin, f["points"], f["normals"], objects, placements, 0.05)
    assert list(a["order"]) == [4, 0, 1, 2, 3, 5]
    assert (a["labels"] != 0).sum() >= 2 and (b["labels"] == 6).sum() >= 2 and (a["labels"] == 5).sum() == 0


@pytest.mark.parametrize("shifted", [False, True])
def test_label_restatement_on_the_shell(oracle, tmin, shifted):
    sp, sn, obj, pose = R.shell(shifted)
    plc = [dict(pose=pose, object_idx=0, uidx=5)]
    a, b = assert_labels(oracle, tmin, sp, sn, [obj], plc, R.SHELL_RADIUS)
    # prioritised: radius r.  The six axis points at d = r are out (d² == r²), the six just inside are in, 1.5 r and the blocks out.
    r2 = hc.radius_sq(R.SHELL_RADIUS)
    d2 = hc.d2_rows(R.xform(oracle.mat4_inverse(pose), sp, 1.0), np.zeros((1, 3), np.float32))[0]
    assert (d2[:6] == r2).all() and (b["labels"][:6] == 0).all() and (b["labels"][14:20] == 1).all() and (b["labels"][28:] == 0).all()
    assert ((d2[:28] < r2) == (b["labels"][:28] == 1)).all()
    assert (a["labels"][:28] == 1).all()                      # without a static placement every placement runs at 1.5 r


def test_label_restatement_on_exact_ties(oracle, tmin):
    sp, sn, obj, pose, r = R.lattice_ties()
    a, b = assert_labels(oracle, tmin, sp, sn, [obj], [dict(pose=pose, object_idx=0, uidx=5)], r)
    assert b["tied"] > 500 and (b["labels"] == 1).all()


def test_label_restatement_with_zero_normals(oracle, tmin):
    """Zeroed scene points are never labelled, a label won on a zeroed object normal is lost, and the rest is unchanged."""
    f = R.family("offset_1e3")
    objects, placements = R.six_placements(f)
    caches = {prio: {} for prio in (0, 1)}
    base = [R.arrangement(f["points"], f["normals"], objects, placements, 0.05, prio, 37, tmin, oracle.mat4_inverse, caches[prio]) for prio in (0, 1)]
    sn, zobjects = R.zero_normals(f["normals"], objects)
    got = assert_labels(oracle, tmin, f["points"], sn, zobjects, placements, 0.05)
    zero = ~sn.any(axis=1)
    assert zero.sum() > 500 and (base[0]["labels"][zero] != 0).any()
    for prio in (0, 1):
        b, g = base[prio], got[prio]
        keep = R.zero_normal_survivors(b, caches[prio], sn)
        assert (g["labels"][zero] == 0).all() and (g["labels"] != 0).sum() > 100
        assert (g["labels"][keep] == b["labels"][keep]).all() and (g["min_dists"].view(np.uint32)[keep] == b["min_dists"].view(np.uint32)[keep]).all()
        lost = ~keep & (b["labels"] != 0)
        assert lost.sum() > 20 and (g["labels"][lost] != b["labels"][lost]).all() and (keep & (b["labels"] != 0)).sum() > 100


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_label_restatement_on_tiny_scenes(oracle, tmin, n):
    """The scene sizes the GPU file runs: prefixes of `outside`, and its points nearest the cut (most of those are labelled)."""
    f = R.family("outside")
    objects, placements = R.six_placements(f)
    labelled = 0
    for sel in R.tiny_scenes(f, n):
        a, _ = assert_labels(oracle, tmin, f["points"][sel], f["normals"][sel], objects, placements, 0.05)
        labelled += int((a["labels"] != 0).sum())
    assert labelled > 0.5 * n


def test_label_restatement_at_the_cap(oracle, tmin):
    sp, sn, objects, placements = R.cap_arrangement(127)
    got, = assert_labels(oracle, tmin, sp, sn, objects, placements, 0.05, modes=(0,))
    assert (got["labels"] == 127).sum() >= 8 and got["labels"].min() >= 0


# ---- the inputs reach what they are for ------------------------------------------------------------------------------------

def test_families_reach_what_they_are_for():
    def stats(p, level):
        s = {}
        R.level_samples(p, LEVEL_VOXEL[level], s)
        return s
    # all three instantiations of the frontier kernel: the host picks 1, 8 or 64 lanes per item below 3, below 24, from 24
    room = R.family("offset_1e4")["points"]
    assert stats(room, 1)["avg_later"] < 3 and stats(room, 2)["avg_later"] < 3
    assert 3 <= stats(room, 3)["avg_later"] < 24 and 3 <= stats(room, 4)["avg_later"] < 24
    assert stats(R.family("planar")["points"], 4)["avg_later"] >= 24 and stats(R.family("collinear")["points"], 4)["avg_later"] >= 24
    # dependence chains of hundreds of rounds: several 16-launch batches of the host loop
    assert stats(R.sorted_collinear(), 2)["depth"] > 100 and stats(R.sorted_collinear(), 1)["depth"] > 100
    assert stats(R.raster_planar(), 4)["depth"] > 100
    # the lattice has exact d² == r² pairs, which the strict comparison excludes
    p = R.lattice()
    d2 = hc.d2_rows(p, p[:64])
    assert (d2 == hc.radius_sq(0.125)).sum() > 200 and ((d2 < hc.radius_sq(0.125)).sum(axis=1) <= 27).all()
    # contrast is the refusal case at every level; the cluster sits exactly on the boundary
    dense = R.family("contrast")["points"]
    i = int(np.argmin(np.linalg.norm(dense.astype(np.float64) - np.array([1.31, 0.71, 2.11]), axis=1)))
    for level in (1, 2, 3, 4):
        assert R.within_count(dense, dense[i], LEVEL_VOXEL[level]) > level_max_n_neigh(level)
    for m in (256, 257):
        c = R.cluster(m, 0.01)
        got, within = R.level_samples(c, 0.01)
        assert within == m and list(got) == [0]
    # coincident triples make K = 1 itself a tie
    p, _ = R.edge_input("repeated")
    assert len(R.edge_bounds(p, R.graph_radius(R.EDGE_R2), 1)[2]) == len(p)
