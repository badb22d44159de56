"""GPU: rs_hip_propose_poses on the hostile grids of tests/hard_grids.py, on both score routes.  The search is the only caller that
hands the score kernels poses living on the device; there the scene-space route (rs_score.hip: k_score_scene) cuts its lattice to
the box the search derives from the grid's four extreme cells (rs_propose.hip: propose_query_box) instead of from the poses.

- route matrix: every case under score_scene_space_from(0) (always scene space, no density test), (1 << 60) (never) and the
  default; lists and traces byte-equal among the three, and each equal to the restated cascade (tests/propose_restate.py) composed
  over capi.alignment_scores under the same setting.  Two messages, as in tests/test_gpu_propose.py: the search differing from the
  composed cascade is the search's fault, the routes differing from each other the scorer's.  offset, overhang and chunk once more
  in scene space with the radix sort and without the normal bin (read-once switches: the child's environment).
- independent reference: the cases hg.MARGIN against the cascade over the oracle scorer, computed here on the CPU; proposing
  cells, counts and winning poses identical, scores within SCORE_TOL, outside the cells tests/test_hard_grids_cpu.py bounds.
- thresholds that tie, a negative one, 0, four levels, a repeated level: what the restatement says must happen.
- batches: alone == in the batch, permuted, dead objects' trace rows, repeats, after a release, a small call after chunk.
- capacity: the largest need, one less (-4, counts hold the needs, arrays untouched), 0 on an empty grid.

Not tested: a batch crossing chunk_poses = 2^30 / object->n on the scene-space route (more than 2^30 queries, tens of GB of keys).
The zero matrix k_keep writes for a proposal without a winning rotation (negative threshold) cannot be seen through this call: such a
proposal's score is 0, no later level scores it and the final copy drops it; the tests pin the counts around it.

Every GPU body runs in a child process under its own time limit and ends with `ok`; nothing here provokes a fault."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
import hard_grids as hg

pytestmark = pytest.mark.gpu

PRELUDE = r"""
import ctypes as C, os, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from rescan_amd import capi
import propose_restate as R
import hard_grids as hg
capi.init(0)
F = np.float32
SEARCH = "the search differs from the cascade composed over alignment_scores under the same setting: the search's fault"
SCORER = "the search equals the composed cascade under each setting, but the settings differ: the scorer's routes disagree"
def clouds_of(c):
    scene = capi.Cloud(c["scene_pos"], c["scene_nor"])
    return scene, [[capi.Cloud(p, n, cell_size=c["object_cell"]) for p, n in lv] for lv in c["objects"]]
def native(c, scene, objs, thresholds=None, **kw):
    return capi.propose_poses(objs, scene, *hg.args_of(c, thresholds), **kw)
def scorer(c, scene, levels, log=None):
    # (batches of at most 40 000 poses: the composed cascade does not lean on the chunk loop the search is checked for)
    def fn(l, P):
        s = np.concatenate([capi.alignment_scores(levels[l], scene, P[k:k + 40000], c["radius"], c["max_n_neigh"]) for k in range(0, len(P), 40000)] + [np.zeros(0, F)])
        if log is not None: log.append((l, np.array(P, F), s.copy()))
        return s
    return fn
def composed(c, scene, objs, thresholds=None):
    return [hg.cascade(c, scorer(c, scene, lv), o, thresholds) for o, lv in enumerate(objs)]
def same(a, b): return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
def same_trace(a, b): return all((a[k] == b[k]).all() for k in ("n_scored", "n_kept", "n_proposed"))
def equals_composed(got, tr, comp):
    for k, (cp, cs, ctrace, (sp, ss)) in enumerate(comp):
        if not same(got[k], (cp, cs)): return False
        if [tuple(x) for x in ctrace] != list(zip(tr["n_scored"][k].tolist(), tr["n_kept"][k].tolist())): return False
        if tr["n_proposed"][k] != len(ss): return False
    return True
def under(frm, f):
    # f() with the scene-space route starting at frm queries (None: as it is), the previous value restored
    if frm is None: return f()
    prev = capi.score_scene_space_from(frm)
    try: return f()
    finally: capi.score_scene_space_from(prev)
def refused(code, f, *a, **k):
    try:
        f(*a, **k)
    except capi.RescanHipError as e:
        assert f"error {code}:" in str(e), str(e)
        return True
    return False
"""


def run_child(body, limit=120, env=None):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True,
                         env=dict(os.environ, **(env or {})))
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


@pytest.mark.parametrize("name", hg.CASES)
def test_route_matrix(name):
    run_child(r"""
c = hg.make(NAME); scene, objs = clouds_of(c)
thr = hg.tie_thresholds(c, scorer(c, scene, objs[0])) if NAME == "ties" else None
runs = {}
for label, frm in (("scene space", 0), ("object tiles", 1 << 60), ("default", None)):
    t0 = time.perf_counter()
    got, tr = under(frm, lambda: native(c, scene, objs, thr, trace=True))
    t1 = time.perf_counter()
    comp = under(frm, lambda: composed(c, scene, objs, thr))
    ok = equals_composed(got, tr, comp)
    print(f"{NAME} / {label}: plan {c['plan']}, proposals {tr['n_proposed'].tolist()}, kept {tr['n_kept'].tolist()}, final {[len(s) for _, s in got]}; "
          f"equals composed cascade {ok}; call {(t1 - t0) * 1e3:.1f} ms, composed {(time.perf_counter() - t1) * 1e3:.1f} ms")
    assert ok, SEARCH
    runs[label] = (got, tr)
for label in ("object tiles", "default"):
    a, b = runs["scene space"], runs[label]
    assert all(same(x, y) for x, y in zip(a[0], b[0])) and same_trace(a[1], b[1]), SCORER
print("ok")
""".replace("NAME", repr(name)))


@pytest.mark.parametrize("name", ("offset", "overhang", "chunk"))
def test_scene_space_with_the_radix_sort_and_without_the_normal_bin(name):
    """The object-tile route does not read the two switches: its lists are the yardstick inside the child."""
    run_child(r"""
assert capi.switch_get("RS_HIP_SCORE_COUNTING") == 0 and capi.switch_get("RS_HIP_SCORE_NBIN") == 0
c = hg.make(NAME); scene, objs = clouds_of(c)
got, tr = under(0, lambda: native(c, scene, objs, trace=True))
assert equals_composed(got, tr, under(0, lambda: composed(c, scene, objs))), SEARCH
tiles, ttr = under(1 << 60, lambda: native(c, scene, objs, trace=True))
assert all(same(x, y) for x, y in zip(got, tiles)) and same_trace(tr, ttr), SCORER
assert tr["n_kept"][0][-1] > 0
print("ok")
""".replace("NAME", repr(name)), env=dict(RS_HIP_SCORE_COUNTING="0", RS_HIP_SCORE_NBIN="0"))


@pytest.mark.parametrize("name", hg.MARGIN)
def test_against_the_oracle_scorer(name):
    """Forced scene space, forced object tiles and the default against the cascade over the oracle (CPU).  The cells whose two best
    rotations the oracle cannot tell apart (tests/test_hard_grids_cpu.py: at most 2 % of the proposing ones) may differ in pose and
    in what becomes of it; everything else may not."""
    run_child(r"""
from oracle.pyoracle import Oracle
c = hg.make(NAME); scene, objs = clouds_of(c)
log = []
t0 = time.perf_counter()
wp, ws, wtrace, (sp, ss) = hg.cascade(c, hg.oracle_scorer(Oracle(), c, 0, log))
und, proposing = hg.undecided_cells(c, log[0][2].reshape(-1, c["plan"][2]), c["thresholds"][0])
print(f"{NAME}: oracle cascade {time.perf_counter() - t0:.1f} s; {proposing} proposing cells, {len(und)} undecided, trace {wtrace}")
assert proposing == len(ss) and len(und) <= 0.02 * proposing
wc = hg.cells_of(c, wp)
for label, frm in (("scene space", 0), ("object tiles", 1 << 60), ("default", None)):
    got, tr = under(frm, lambda: native(c, scene, objs, trace=True))
    gp, gs = got[0]
    assert tr["n_proposed"][0] == proposing and len(gs) == len(ws), (label, tr["n_proposed"], len(gs), len(ws))
    assert (hg.cells_of(c, gp) == wc).all(), label + ": other cells propose"
    decided = ~np.isin(wc, und)
    assert (gp[decided] == wp[decided]).all(), label + ": another rotation wins a decided cell"
    assert ((gs == -1) == (ws == -1))[decided].all(), label + ": a decided proposal fails a level it passes under the oracle, or the reverse"
    err = np.abs(gs.astype(np.float64) - ws)[decided]
    print(f"{NAME} / {label}: {len(gs)} proposals, {int((gs == -1).sum())} marked -1, max |score - oracle| {err.max() if len(err) else 0.0:.3e}")
    assert (err < hg.SCORE_TOL).all(), label
    for l, (n_scored, n_kept) in enumerate(wtrace):
        assert abs(int(tr["n_scored"][0][l]) - n_scored) <= len(und) and abs(int(tr["n_kept"][0][l]) - n_kept) <= len(und), (label, l)
print("ok")
""".replace("NAME", repr(name)))


@pytest.mark.parametrize("name", hg.THRESHOLDS)
def test_ties_and_odd_thresholds(name):
    run_child(r"""
c = hg.make(NAME); scene, objs = clouds_of(c)
n_cells, n_yaw = c["plan"][0] * c["plan"][1], c["plan"][2]
thr = hg.tie_thresholds(c, scorer(c, scene, objs[0])) if NAME == "ties" else c["thresholds"]
log = []
cp, cs, ctrace, (sp, ss) = hg.cascade(c, scorer(c, scene, objs[0], log), 0, thr)
got, tr = native(c, scene, objs, thr, trace=True)
gp, gs = got[0]
print(f"{NAME}: thresholds {thr.tolist()}, trace {ctrace}, {len(gs)} in the final list, {int((gs == -1).sum())} of them -1")
assert equals_composed(got, tr, [(cp, cs, ctrace, (sp, ss))]), SEARCH
best = R.cell_best(log[0][2].reshape(n_cells, n_yaw), thr[0])[1]
if NAME == "ties":
    tied = np.flatnonzero(best == thr[0])
    assert len(tied) >= 1 and tr["n_proposed"][0] == (best > thr[0]).sum() and not np.isin(tied, hg.cells_of(c, gp)).any()   # best == threshold: not proposed
    for l, P, s in log[1:]:
        hit = np.flatnonzero(s == thr[l])
        assert len(hit) >= 1, l
        for p in P[hit]:                                                          # score == threshold: -1
            at = np.flatnonzero((gp == p).all(axis=1))
            assert len(at) == 1 and gs[at[0]] == -1, l
        assert tr["n_kept"][0][l] == (s > thr[l]).sum()
elif NAME == "negative":
    zeros = int((best == 0).sum())
    assert zeros > 50 and tr["n_proposed"][0] == n_cells and (sp[ss == 0] == 0).all() and (ss == 0).sum() == zeros   # proposals without a rotation: the zero matrix
    assert tr["n_kept"][0][0] == n_cells - zeros == tr["n_scored"][0][1] and len(gs) == n_cells - zeros               # never scored again, dropped by the final copy
    assert (np.abs(gs) > 1e-6).all() and (gp[:, 15] == 1).all()
elif NAME == "zero":
    assert tr["n_proposed"][0] == (best > 0).sum() < n_cells                      # best == 0 == threshold: not proposed
    dropped = sum(int((s == 0).sum()) for _, _, s in log[1:])
    assert dropped >= 1 and (gs == -1).sum() == dropped                           # a later score of 0 is not > 0: -1
    assert len(gs) == tr["n_proposed"][0]
elif NAME == "four_levels":
    assert tr["n_kept"].shape == (1, 4) and (np.diff(tr["n_kept"][0]) < 0).all() and tr["n_kept"][0][3] > 0
    assert len(log) == 4 and (gs > thr[3]).sum() == tr["n_kept"][0][3]
elif NAME == "repeated":
    s1, s2 = log[1][2], log[2][2]
    assert s2.tobytes() == s1[s1 > thr[1]].tobytes()                              # the same cloud under the same poses: the same bits
    alive = gs[gs != -1]
    assert alive.tobytes() == s1[s1 > thr[2]].tobytes() and thr[2] > thr[1] and 0 < len(alive) < (s1 > thr[1]).sum()
print("ok")
""".replace("NAME", repr(name)))


def test_batches():
    run_child(r"""
c = hg.make("batch"); scene, objs = clouds_of(c)
n_grid = c["plan"][0] * c["plan"][1] * c["plan"][2]
batch, tr = native(c, scene, objs, trace=True)
need = [len(s) for _, s in batch]
print("batch:", dict(zip(c["names"], need)), "proposed", tr["n_proposed"].tolist(), "kept", tr["n_kept"].tolist())
assert equals_composed(batch, tr, composed(c, scene, objs)), SEARCH
for k in range(len(objs)):                                                       # alone == its slot in the batch
    alone, atr = native(c, scene, [objs[k]], trace=True)
    assert same(alone[0], batch[k]), k
    assert all((atr[x][0] == tr[x][k]).all() for x in atr), k
order = [3, 0, 4, 2, 1]                                                          # a permuted batch: permuted lists
perm, ptr = native(c, scene, [objs[k] for k in order], trace=True)
assert all(same(perm[i], batch[k]) for i, k in enumerate(order)) and all((ptr[x] == tr[x][order]).all() for x in ptr)
# the dead: floating proposes nothing, hollow loses everything at its empty level; zero rows from there on
assert tr["n_scored"][1].tolist() == [n_grid, 0, 0] and tr["n_kept"][1].tolist() == [0, 0, 0] and need[1] == 0
assert tr["n_scored"][4].tolist() == [n_grid, need[4], 0] and tr["n_kept"][4].tolist() == [need[4], 0, 0] and (batch[4][1] == -1).all()
assert all(tr["n_kept"][k][2] > 20 for k in (0, 2, 3))
assert min(need[k] for k in (0, 2, 3, 4)) < 256 < max(need)
again, atr = native(c, scene, objs, trace=True)                                  # a second identical call: the same bytes
assert all(same(x, y) for x, y in zip(again, batch)) and same_trace(atr, tr)
capi.propose_release()
fresh, ftr = native(c, scene, objs, trace=True)                                  # after a release
assert all(same(x, y) for x, y in zip(fresh, batch)) and same_trace(ftr, tr)
print("ok")
""")


def test_a_small_call_after_the_chunked_one():
    run_child(r"""
small = hg.make("cells_258"); sscene, sobjs = clouds_of(small)
big = hg.make("chunk"); bscene, bobjs = clouds_of(big)
for frm in (0, None):
    fresh = under(frm, lambda: native(small, sscene, sobjs, trace=True))
    first = under(frm, lambda: native(big, bscene, bobjs, trace=True))
    assert first[1]["n_scored"][0][0] > 65535
    after = under(frm, lambda: native(small, sscene, sobjs, trace=True))
    assert same(after[0][0], fresh[0][0]) and same_trace(after[1], fresh[1]), frm
    second = under(frm, lambda: native(big, bscene, bobjs, trace=True))
    assert same(second[0][0], first[0][0]) and same_trace(second[1], first[1]), frm
    capi.propose_release()
print("ok")
""")


def test_capacity():
    run_child(r"""
c = hg.make("batch"); scene, objs = clouds_of(c)
full = native(c, scene, objs)
need = [len(s) for _, s in full]
assert len(set(need)) == len(need) and min(need) == 0, need                       # ragged
exact = native(c, scene, objs, capacity=max(need))
assert all(same(x, y) for x, y in zip(exact, full))
lib = capi.load()
a = hg.args_of(c)
lo, hi, thr = np.ascontiguousarray(a[0], F), np.ascontiguousarray(a[1], F), np.ascontiguousarray(a[5], F)
handles = (C.c_void_p * 15)(*[x.handle for o in objs for x in o])
cap = max(need) - 1
counts = np.full(5, -7, np.int32); poses = np.full((5, cap, 16), -7, F); scores = np.full((5, cap), -7, F)
rc = lib.rs_hip_propose_poses(handles, 5, 3, scene.handle, lo.ctypes.data, hi.ctypes.data, float(a[2]), float(a[3]), float(a[4]), thr.ctypes.data,
                              float(a[6]), a[7], cap, counts.ctypes.data, poses.ctypes.data, scores.ctypes.data, None)
assert rc == -4 and counts.tolist() == need and (poses == -7).all() and (scores == -7).all(), (rc, counts)
assert refused(-4, native, c, scene, objs, capacity=cap)
e = hg.make("inside_out"); escene, eobjs = clouds_of(e)
got, tr = native(e, escene, eobjs, capacity=0, trace=True)
assert len(got[0][1]) == 0 and got[0][0].shape == (0, 16) and not tr["n_scored"].any() and not tr["n_kept"].any() and tr["n_proposed"][0] == 0
print("ok")
""")
