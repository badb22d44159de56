"""The cases of tests/hard_grids.py are what they claim to be, by the restated cascade (tests/propose_restate.py) over the oracle's
alignment score: the planner's counts, which object dies at which level, lists on both sides of a scan block, thresholds that tie,
a grid past 65 535 poses -- and, for the cases on which tests/test_gpu_hard_grids.py holds the device to the oracle, how far the
oracle's own scores stay from every decision.  No GPU needed.

The margins (cases hg.MARGIN), all conditions on the inputs that the seeds were chosen to meet:
- no oracle score of any level within 2 * SCORE_TOL of the level's threshold;
- no oracle score within 2 * SCORE_TOL of 0 other than an exact 0.  (An exact 0 is a pose under which no object point has a
  compatible scene point at all; it is decided by the searches, not by rounding.  The smallest score that is not 0 is one point's
  term over n: at least ( 0.05 exp( -(35 deg)^2 / 0.5 ) + 0.95 exp( -0.5 ) ) / n > 0.6 / n, 2e-4 for the largest level here, so a
  device score that differs from an exact 0 differs by a hundred times SCORE_TOL and fails the comparison, not the margin.)
- at most 2 % of the proposing cells have a runner-up rotation within 2 * SCORE_TOL of the best."""
import numpy as np
import pytest

import hard_grids as hg
import propose_restate as R

F = np.float32
TOL2 = 2 * hg.SCORE_TOL
PLANS = dict(base=(18, 14, 10), offset=(19, 14, 10), overhang=(29, 24, 10), inside=(5, 5, 10), tall_clear=(18, 14, 10), tall_low=(18, 14, 10),
             brute_object=(18, 14, 10), smallest=(2, 2, 10), cells_255=(15, 17, 10), cells_256=(16, 16, 10), cells_258=(6, 43, 10),
             cells_510=(17, 30, 10), cells_512=(16, 32, 10), cells_513=(19, 27, 10), yaw_1=(18, 14, 1), yaw_2=(18, 14, 2),
             inside_out=(0, 14, 10), chunk=(100, 66, 10), ties=(18, 14, 10), negative=(23, 19, 10), zero=(23, 19, 10),
             four_levels=(18, 14, 10), repeated=(18, 14, 10), batch=(22, 18, 2))

_RUNS = {}


def run(oracle, name, o=0, thresholds=None):
    """The oracle's cascade of object o of a case, once per module: final lists, trace, storage and every level's scores."""
    key = (name, o, None if thresholds is None else np.asarray(thresholds, F).tobytes())
    if key not in _RUNS:
        c, log = hg.make(name), []
        fp, fs, trace, (sp, ss) = hg.cascade(c, hg.oracle_scorer(oracle, c, o, log), o, thresholds)
        _RUNS[key] = dict(final_poses=fp, final_scores=fs, trace=trace, poses=sp, scores=ss, log=log)
    return _RUNS[key]


@pytest.mark.parametrize("name", hg.CASES)
def test_planner_counts_and_sizes(name):
    c = hg.make(name)
    assert c["plan"] == PLANS[name]
    n_cells, n_grid = c["plan"][0] * c["plan"][1], c["plan"][0] * c["plan"][1] * c["plan"][2]
    if name.startswith("cells_"):
        assert n_cells == int(name[6:])
    if name == "inside_out":
        assert n_grid == 0
    elif name == "chunk":
        assert 65535 < n_grid < 80000 and len(c["objects"][0][0][0]) == 9
    else:
        assert 40 <= n_grid <= 8000
    assert len(c["scene_pos"]) <= 6500 and c["radius"] == 0.1 and c["max_n_neigh"] == 64
    assert all(len(lv) == len(c["thresholds"]) for lv in c["objects"])
    sizes = [len(p) for lv in c["objects"] for p, _ in lv]
    assert all(n == 0 or 9 <= n <= 3000 for n in sizes)
    for lv in c["objects"]:
        for p, n in lv:
            assert p.dtype == F and n.dtype == F and p.shape == n.shape and (len(p) == 0 or np.allclose(np.linalg.norm(n, axis=1), 1.0))


def test_the_object_has_no_rotation_onto_itself():
    """A rotation about the pose's axis that mapped the L onto itself would keep its centroid; the cut-out quarter puts the
    centroid 5 cm off that axis, so each of the grid's other rotations moves it by centimetres: yaw maxima are not tied by symmetry."""
    pos, nor = hg.l_solid(1, 3000)
    centre = pos.astype(np.float64).mean(axis=0)
    assert np.hypot(centre[0], centre[2]) > 0.04
    yaw = R.grid_plan((0, 0, 0), (1, 1, 1), 0.1, hg.DELTA10)[2]
    for k in range(1, len(yaw)):
        M = yaw[k].astype(np.float64).reshape(4, 4).T[:3, :3]
        assert np.linalg.norm(M @ centre - centre) > 0.02, k


def test_placements_do_what_they_are_for(oracle):
    c = hg.make("offset")
    assert np.abs(c["scene_pos"]).min(axis=0).min() > 4e3 and np.abs(c["bbox_min"][0]) > 9e3            # the pad 1e-5 |q| is 0.1 m
    r = run(oracle, "offset")
    assert r["trace"][0][1] > 50 and r["trace"][2][1] > 20
    # overhang: rows of cells on every side whose poses all score an exact 0, and cells next to them that do not
    c, r = hg.make("overhang"), run(oracle, "overhang")
    n_x, n_z, n_yaw = c["plan"]
    best = r["log"][0][2].reshape(n_x, n_z, n_yaw).max(axis=2)
    assert (best[:2] == 0).all() and (best[-2:] == 0).all() and (best[:, :2] == 0).all() and (best[:, -2:] == 0).all()
    assert (best[4:-4, 4:-4] > 0).all() and r["trace"][0][1] > 50
    # inside: the object's box under the rotations is many times the box of the grid
    c, r = hg.make("inside"), run(oracle, "inside")
    assert (c["bbox_max"] - c["bbox_min"])[[0, 2]].max() < 0.07 and r["trace"][0][1] == c["plan"][0] * c["plan"][1]
    # tall: clear of the scene nothing scores and no level after the first has anything to do; just above the wall little does
    r = run(oracle, "tall_clear")
    assert (r["log"][0][2] == 0).all() and r["trace"] == [(2520, 0), (0, 0), (0, 0)] and len(r["final_scores"]) == 0
    c, r = hg.make("tall_low"), run(oracle, "tall_low")
    lifted = c["objects"][0][0][0][:, 1] + F(c["height"])
    outside = lifted > c["scene_pos"][:, 1].max() + c["radius"]
    assert 0.6 < outside.mean() < 0.8, "most of the object is above the scene's box grown by the radius, its lowest slice is not"
    s0 = r["log"][0][2]
    assert 0 < (s0 > 0).sum() < 0.1 * len(s0) and s0.max() < 0.02 and r["trace"][0][1] > 10 and r["trace"][2][1] > 5
    b, c = hg.make("base"), hg.make("brute_object")              # the same search; only the object clouds' layout differs
    assert c["object_cell"] == 0.0 and b["object_cell"] < 0 and all(x[0].tobytes() == y[0].tobytes() for x, y in zip(b["objects"][0], c["objects"][0]))
    for name in ("yaw_1", "yaw_2", "smallest", "four_levels", "repeated", "chunk"):
        t = run(oracle, name)["trace"]
        assert t[-1][1] > 0 and (name == "smallest" or t[0][1] > t[-1][1]), (name, t)
    assert hg.make("repeated")["objects"][0][1] is hg.make("repeated")["objects"][0][2]
    # chunk: the second launch's poses (from pose 65 535 on) all score, most of the first launch's head do, and not alike
    s0 = run(oracle, "chunk")["log"][0][2]
    tail = s0[65535:]
    assert len(tail) > 400 and (tail > 0).all() and (s0[:len(tail)] > 0).mean() > 0.8 and (tail != s0[:len(tail)]).mean() > 0.9
    assert len(np.unique(tail.reshape(-1, 5)[:, 0])) > 20


def test_ties_really_tie(oracle):
    """Every level's threshold is a score the level meets; strict > drops exactly those entries and the ones below."""
    c = hg.make("ties")
    thr = hg.tie_thresholds(c, hg.oracle_scorer(oracle, c))
    r = run(oracle, "ties", thresholds=thr)
    n_yaw = c["plan"][2]
    best = R.cell_best(r["log"][0][2].reshape(-1, n_yaw), thr[0])
    assert (best[1] == thr[0]).sum() >= 1 and (best[2][best[1] == thr[0]] == -1).all() and (best[2][best[1] > thr[0]] >= 0).all()
    for l, P, s in r["log"][1:]:
        assert (s == thr[l]).sum() >= 1, l
    # an entry that equals its level's threshold ends as -1
    live = r["poses"][r["scores"] > 0]
    for l, P, s in r["log"][1:]:
        for p in P[s == thr[l]]:
            assert not (live == p).all(axis=1).any()
    assert 0 < r["trace"][2][1] < r["trace"][1][1] < r["trace"][0][1]


def test_odd_thresholds(oracle):
    c, r = hg.make("negative"), run(oracle, "negative")
    n_cells = c["plan"][0] * c["plan"][1]
    zero_matrix = (r["poses"] == 0).all(axis=1)
    assert len(r["scores"]) == n_cells and zero_matrix.sum() > 50 and (r["scores"][zero_matrix] == 0).all()
    assert len(r["final_scores"]) == n_cells - zero_matrix.sum() == r["trace"][0][1], "score 0 drops out of the final list"
    c, r = hg.make("zero"), run(oracle, "zero")
    assert len(r["scores"]) == r["trace"][0][1] < n_cells and (r["log"][2][2] == 0).sum() >= 1
    assert (r["final_scores"] == -1).sum() == sum(int((s == 0).sum()) for _, _, s in r["log"][1:])


def test_batch_deaths_and_list_lengths(oracle):
    c = hg.make("batch")
    assert c["names"] == ("tiny", "floating", "mid", "big", "hollow")
    assert [len(lv[0][0]) for lv in c["objects"]] == [9, 40, 600, 3000, 200] and len(c["objects"][4][1][0]) == 0
    runs = [run(oracle, "batch", o) for o in range(5)]
    n_grid = c["plan"][0] * c["plan"][1] * c["plan"][2]
    proposed = [len(r["scores"]) for r in runs]
    print("batch: proposals per object", proposed, "traces", [r["trace"] for r in runs])
    assert runs[1]["trace"] == [(n_grid, 0), (0, 0), (0, 0)] and proposed[1] == 0                      # floating: nothing at level 0
    assert runs[4]["trace"] == [(n_grid, proposed[4]), (proposed[4], 0), (0, 0)] and proposed[4] > 0  # hollow: everything at level 1
    assert (runs[4]["final_scores"] == -1).all()
    for o in (0, 2, 3):
        assert runs[o]["trace"][2][1] > 20, o
    # lists on both sides of a scan block (256), at level 0 and among the survivors
    assert min(proposed[o] for o in (0, 2, 3, 4)) < 256 < max(proposed)
    kept1 = [runs[o]["trace"][1][1] for o in (0, 2, 3)]
    assert min(kept1) < 256 < max(kept1)


@pytest.mark.parametrize("name", hg.MARGIN)
def test_margins_of_the_oracle_comparison(oracle, name):
    c, r = hg.make(name), run(oracle, name)
    assert c["margin"]
    for l, P, s in r["log"]:
        gap = np.abs(s.astype(np.float64) - np.float64(c["thresholds"][l]))
        assert gap.min() > TOL2, (l, gap.min())
        assert ((s == 0) | (np.abs(s) > TOL2)).all(), l
        n = len(c["objects"][0][l][0])
        assert 0.6 / n > 50 * hg.SCORE_TOL
    und, proposing = hg.undecided_cells(c, r["log"][0][2].reshape(-1, c["plan"][2]), c["thresholds"][0])
    print(f"{name}: {proposing} proposing cells, {len(und)} undecided")
    assert proposing == len(r["scores"]) and len(und) <= 0.02 * proposing
