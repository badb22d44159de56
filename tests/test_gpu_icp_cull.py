"""The ball-culled, middle-out shells of the ICP's cold launch (rs_search.h: cull_tile; k_icp_corr<false>) return the bits of the
unculled search, whether a tile ends in phase A or is handed to the cooperative kernels (k_icp_corr_coop<2|4|8>, which sweep unculled).

Which kernel a launch takes is latched at the library's first use, so every ROUTE below runs in a fresh child process (a new python
running this file as a script, under its own time limit) that writes what it computed to an .npz; the tests compare.  One child per
route does all the work of that route, and the tests of a route share it.

1. every family of tests/hard_clouds.py: icp_find_corrs against the oracle bit for bit, scene cells auto, 2 r and 0.25 r;
2. the culling's own edges (CASES) against the numpy brute force below, which the CPU test of this file holds to the oracle:
   the nearest gated candidate, accepted iff fewer than 16 candidates precede it in (d², index).  For the rank cases (15, 16 and 17
   candidates closer than the only gated one) the test sees the decision, not whether a rank pass ran: the count that triggers it is
   an upper bound of the rank in any order, 15 never triggers a rejection and 16 / 17 must be rejected;
3. six warm iterations of tests/test_gpu_switches.py's pair, and the nine icp_* golden calls: pose, error and iteration count
   bit-identical to the default route of this process, to RS_HIP_NO_CERT=1 and to the fixtures."""
import os
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
EPS = np.float32(1e-5)           # inside the culling's own margin (1e-4 cell + 2e-5 m), far above the rounding of the coordinates used
N_ITER = 6
WHAT = ("c_pts1", "c_nor1", "c_pts2", "c_nor2", "weights")

# route -> environment of its child.  RS_HIP_COOP_ALL_BELOW=0: phase A (k_icp_corr<false>) and the hand-off, whatever the launch's size.
ROUTES = {
    "phase_a":        {"RS_HIP_COOP_ALL_BELOW": "0"},
    "phase_a_ladder": {"RS_HIP_COOP_ALL_BELOW": "0", "RS_HIP_SOLO_STAGES": "65535", "RS_HIP_HANDOFF_K": "0"},     # the lone wave climbs its whole ladder
    "phase_a_noseed": {"RS_HIP_COOP_ALL_BELOW": "0", "RS_HIP_NO_SEED": "1"},                                     # every lane starts from nothing
    "coop2":          {"RS_HIP_COOP_WAVES": "2"},
    "coop4":          {"RS_HIP_COOP_WAVES": "4"},
    "coop8":          {"RS_HIP_COOP_WAVES": "8"},
}


def cells(r):
    return {"auto": -1.0, "2r": 2.0 * float(r), "r4": 0.25 * float(r)}


# ---- the edge cases --------------------------------------------------------------------------------------------------------

UP = np.float32([0.0, 0.0, 1.0])
DOWN = np.float32([0.0, 0.0, -1.0])          # dot = -1 with UP: never passes the gate


def _case(src, tgt, tgt_nor=None):
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    if tgt_nor is None:
        tgt_nor = np.tile(UP, (len(tgt), 1))
    return dict(src=src, src_nor=np.tile(UP, (len(src), 1)), tgt=tgt, tgt_nor=np.ascontiguousarray(tgt_nor, np.float32))


def _tile(rng, lo, size, n=64):
    """n points of one tile: the corners of the box [lo, lo + size]³ among them, the rest uniform inside."""
    lo = np.asarray(lo, np.float64)
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64) * size + lo
    return np.concatenate([corners, rng.uniform(lo, lo + size, (n - 8, 3))]).astype(np.float32)


def _plane(rng, origin, normal, n=900, half=0.16):
    """n points of the plane through `origin` with unit `normal`, a lattice and a jittered copy, out to `half` around the origin."""
    normal = np.asarray(normal, np.float64)
    a = np.cross(normal, [1.0, 0.0, 0.0]); a = a / np.linalg.norm(a) if np.linalg.norm(a) > 1e-6 else np.array([0.0, 1.0, 0.0])
    b = np.cross(normal, a)
    s = int(np.sqrt(n // 2))
    u, v = np.meshgrid(np.linspace(-half, half, s), np.linspace(-half, half, s), indexing="ij")
    uv = np.concatenate([np.stack([u.ravel(), v.ravel()], 1), rng.uniform(-half, half, (n - s * s, 2))])
    return np.asarray(origin, np.float64) + uv[:, :1] * a + uv[:, 1:] * b


def make_cases():
    """name -> dict(src, src_nor, tgt, tgt_nor): identity poses, normals along +z (gate value exactly 1) or -z (exactly 0)."""
    rng = np.random.default_rng(1507)
    cases = {}
    # a plane parallel to a face (or an edge) of the tile's box, R - eps, R and R + eps from it.  The box is [0, 0.03]³, so that a plane
    # at y = 0.03 + d faces the corner lanes at exactly d; for d = R the lanes at y = 0 see it from y = -R: d² == r², strictly outside.
    size = 0.03
    for axis, normal, origin in (("x", (1, 0, 0), (size, 0.015, 0.015)), ("y", (0, 1, 0), (0.015, size, 0.015)), ("z", (0, 0, 1), (0.015, 0.015, size)),
                                 ("yz", (0, np.sqrt(0.5), np.sqrt(0.5)), (0.015, size, size)), ("-y", (0, -1, 0), (0.015, 0.0, 0.015))):
        for tag, d in (("in", R - EPS), ("at", R), ("out", R + EPS)):
            src = _tile(rng, (0, 0, 0), size)
            o, nrm = np.asarray(origin, np.float64) + np.asarray(normal, np.float64) * float(d), np.asarray(normal, np.float64)
            feet = src.astype(np.float64) - ((src.astype(np.float64) - o) @ nrm)[:, None] * nrm       # every lane's nearest point of the plane
            pl = np.concatenate([_plane(rng, o, normal), feet])
            if axis == "-y" and tag == "at":
                pl[:, 1] = -float(R)          # exactly R below the face y = 0: v = -R, d² == r² for the lanes on the face
            cases[f"plane_{axis}_{tag}"] = _case(src, pl)
    # 63 lanes with matches a millimetre away, one lane 0.25 m from them with none; clutter between the two groups that neither reaches,
    # and points just outside the radius of the lone lane
    src = np.concatenate([rng.uniform(0.0, 0.03, (63, 3)), [[0.27, 0.01, 0.02]]]).astype(np.float32)
    near = src[:63] + rng.normal(0.0, 0.001 / np.sqrt(3.0), (63, 3))
    clutter = rng.uniform((0.08, -0.1, -0.1), (0.15, 0.12, 0.12), (800, 3))
    ring = src[63].astype(np.float64) + hc._unit(rng, 300).astype(np.float64) * (float(R) + 1e-4)
    cases["lone_lane"] = _case(src, np.concatenate([near, clutter, ring]))
    ring_in = src[63].astype(np.float64) + hc._unit(rng, 40).astype(np.float64) * rng.uniform(float(R) - 2e-3, float(R) - 1e-4, (40, 1))     # (no two at one d²)
    cases["lone_lane_matched"] = _case(src, np.concatenate([near, clutter, ring, ring_in]))
    # tiles outside the grid on each of its six sides, within reach of it (0.05) and beyond (0.15), and well inside
    box = rng.uniform(0.0, 0.4, (3000, 3))
    groups = [rng.uniform(0.1, 0.3, (64, 3))]
    for a in range(3):
        for side in (-1, 1):
            for dist in (0.05, 0.15):
                c = rng.uniform(0.1, 0.3, (32, 3))
                c[:, a] = (-dist if side < 0 else 0.4 + dist) + rng.uniform(-0.01, 0.01, 32)
                groups.append(c)
    cases["outside_six"] = _case(np.concatenate(groups), box)
    # a grid one cell thick in each axis
    for a, ax in enumerate("xyz"):
        sheet = rng.uniform(-0.3, 0.3, (2500, 3)); sheet[:, a] = 0.125
        src = rng.uniform(-0.2, 0.2, (256, 3)); src[:, a] = 0.125 + rng.uniform(-0.12, 0.12, 256)
        cases[f"thin_{ax}"] = _case(src, sheet)
    # exactly 15, 16 and 17 candidates closer than the only gated one; queries 1 m apart (a tile each), the ungated ones arrive from
    # all directions.  The same with the gated candidate tied in d² with an ungated one of lower / higher index (mirror images about
    # the query on a binary-exact offset), 15 others closer: rank 16 (rejected) / 15 (accepted).
    src, tgt, nor = [], [], []
    for qi, n_closer in enumerate((15, 16, 17)):
        q = np.array([float(qi), 0.25, 0.5])
        src.append(q)
        tgt.extend(q + hc._unit(rng, n_closer).astype(np.float64) * rng.uniform(0.01, 0.06, (n_closer, 1))); nor.extend([DOWN] * n_closer)
        tgt.append(q + np.array([0.0, 0.08, 0.0])); nor.append(UP)
    cases["rank_15_16_17"] = _case(np.array(src), np.array(tgt), np.array(nor))
    src, tgt, nor = [], [], []
    for qi, gated_first in enumerate((False, True)):
        q = np.array([float(qi), 0.25, 0.5])
        src.append(q)
        tgt.extend(q + hc._unit(rng, 15).astype(np.float64) * rng.uniform(0.01, 0.05, (15, 1))); nor.extend([DOWN] * 15)
        pair = [(q + np.array([0.0625, 0.0, 0.0]), UP), (q - np.array([0.0625, 0.0, 0.0]), DOWN)]
        for p, n in (pair if gated_first else pair[::-1]):
            tgt.append(p); nor.append(n)
    cases["ties"] = _case(np.array(src), np.array(tgt), np.array(nor))
    return cases


def brute_find_corrs(c, radius=R, k=K):
    """The reference's rule restated on all pairs (identity poses): rows of the sources that have a correspondence, and the target's index."""
    r2 = np.float32(np.float64(radius) * np.float64(radius))
    rows, idx = [], []
    tgt, tn = c["tgt"], c["tgt_nor"]
    for i, (q, n) in enumerate(zip(c["src"], c["src_nor"])):
        v = tgt - q
        d2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        dot = (tn[:, 0] * n[0] + tn[:, 1] * n[1]) + tn[:, 2] * n[2]
        dc = np.maximum(dot, np.float32(0.0))
        ok = (d2 < r2) & (dc >= np.float32(np.cos(np.float64(MA)))) & (dc <= np.float32(1.0))
        if not ok.any():
            continue
        cand = np.nonzero(ok)[0]
        w = cand[np.lexsort((cand, d2[cand]))[0]]
        before = (d2 < r2) & ((d2 < d2[w]) | ((d2 == d2[w]) & (np.arange(len(tgt)) < w)))
        if before.sum() < k:
            rows.append(i); idx.append(w)
    return np.asarray(rows, np.int64), np.asarray(idx, np.int64)


def assert_brute(c, got, what):
    rows, idx = brute_find_corrs(c)
    assert len(got[0]) == len(rows), (what, len(got[0]), len(rows))
    for a, b, name in zip((c["src"][rows], c["src_nor"][rows], c["tgt"][idx], c["tgt_nor"][idx]), got, WHAT):
        assert a.astype(np.float32).tobytes() == np.ascontiguousarray(b).tobytes(), (what, name)


def assert_same(want, got, what):
    for a, b, name in zip(want, got, WHAT):
        assert a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b).tobytes(), (what, name)


# Among candidates at exactly one d² the reference's order is an accident of its heap, which the oracle repeats and the library does not
# (the library's order is (d², index)): the tie case is held to the brute force alone.
TIES = ("ties",)
_CASES = {}


def cases():
    if not _CASES:
        _CASES.update(make_cases())
    return _CASES


# ---- CPU: the yardstick of the GPU tests is not the code under test ----------------------------------------------------------

def test_brute_force_agrees_with_the_oracle(oracle):
    """brute_find_corrs against oracle.icp_find_corrs on every edge case; the cases are what their names say."""
    cs = cases()
    for name, c in cs.items():
        if name in TIES:
            continue
        want = oracle.icp_find_corrs(c["src"], c["src_nor"], c["tgt"], c["tgt_nor"], I4, I4, R, MA)
        assert_brute(c, want, name)
    n = {name: len(brute_find_corrs(c)[0]) for name, c in cs.items()}
    for axis in ("x", "y", "z", "yz", "-y"):
        assert n[f"plane_{axis}_in"] > 0 and n[f"plane_{axis}_out"] == 0, (axis, n)
    assert n["plane_-y_at"] == 0, "d² == r² is outside (the other planes' coordinates do not subtract to exactly R)"
    assert n["lone_lane"] == 63 and n["lone_lane_matched"] == 64, n
    assert n["outside_six"] == 64 + 6 * 32, "the tile inside and the six within reach of the grid find matches, the six beyond none"
    assert brute_find_corrs(cs["rank_15_16_17"])[0].tolist() == [0], "15 closer: accepted; 16, 17: rejected"
    assert brute_find_corrs(cs["ties"])[0].tolist() == [1], "gated candidate tied behind a lower index: rank 16, rejected; before a higher one: rank 15, accepted"


# ---- the children ----------------------------------------------------------------------------------------------------------

def switches_pair(capi):
    """tests/test_gpu_switches.py's pair: (source cloud, target cloud, start pose)."""
    from rescan_amd import synth
    s = synth.make_scene(seed=3, density=860.0, timestep=1)
    pos, nor = synth.make_object("table", 3 * 7919, 1125.0, 1.0, 0.0)
    src = capi.Cloud(np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(nor, np.float32), cell_size=0.1)
    tgt = capi.Cloud(s["points"], s["normals"], cell_size=0.1)
    return src, tgt, synth.perturbed_pose(s["objects"][0]["pose"], np.random.default_rng(5))


def golden_names():
    return sorted(f for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("icp_"))


def compute(capi):
    """Everything a route is asked for, as a flat dict of arrays."""
    out = {}
    for name in hc.FAMILIES:
        f = hc.make(name)
        oc = capi.Cloud(f["obj"]["pos"], f["obj"]["nor"])
        for tag, cell in cells(R).items():
            scn = capi.Cloud(f["points"], f["normals"], cell_size=cell)
            for a, what in zip(capi.icp_find_corrs(oc, scn, f["T0"], I4, R, MA), WHAT):
                out[f"fam/{name}/{tag}/{what}"] = a
            scn.close()
        oc.close()
    for name, c in cases().items():
        oc = capi.Cloud(c["src"], c["src_nor"])
        for tag, cell in cells(R).items():
            scn = capi.Cloud(c["tgt"], c["tgt_nor"], cell_size=cell)
            for a, what in zip(capi.icp_find_corrs(oc, scn, I4, I4, R, MA), WHAT):
                out[f"case/{name}/{tag}/{what}"] = a
            scn.close()
        oc.close()
    src, tgt, T0 = switches_pair(capi)
    err, T, it = capi.icp_align(src, tgt, T0, I4, 0.1, MA, max_iter=N_ITER, fixed_iters=True)
    out["warm"] = np.frombuffer(np.float32(err).tobytes() + np.asarray(T, np.float32).tobytes() + np.int32(it).tobytes(), np.uint8)
    src.close(); tgt.close()
    sc = dict(np.load(os.path.join(HERE, "golden", "scene.npz")))
    clouds = {r: capi.Cloud(sc["points"], sc["normals"], cell_size=2 * r) for r in (0.05, 0.1)}
    clouds[0.075] = capi.Cloud(sc["points"], sc["normals"])
    objs = [capi.Cloud(sc[f"obj{i}_pos"], sc[f"obj{i}_nor"], cell_size=0.1) for i in range(int(sc["n_obj"]))]
    for fname in golden_names():
        g = dict(np.load(os.path.join(HERE, "golden", fname)))
        md = float(g["max_dist"])
        err, T, it = capi.icp_align(objs[int(g["obj"])], clouds[round(md, 3)], g["T1"], g["T2"], md, g["max_angle"])
        out[f"golden/{fname}"] = np.frombuffer(np.float32(err).tobytes() + np.asarray(T, np.float32).tobytes() + np.int32(it).tobytes(), np.uint8)
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


_ROUTE = {}


def route(name, tmp_path_factory):
    """The results of route `name`: its child runs once per session, under its own time limit; a failed child fails the test."""
    if name not in _ROUTE:
        path = str(tmp_path_factory.mktemp("icp_cull") / (name + ".npz"))
        env = {k: v for k, v in os.environ.items() if not k.startswith("RS_HIP_") or k == "RS_HIP_LIB"}
        env.update(ROUTES[name])
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), path]
        p = subprocess.run(cmd, env=env, timeout=120, capture_output=True, text=True)
        assert p.returncode == 0, (name, p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        _ROUTE[name] = dict(np.load(path))
    return _ROUTE[name]


@pytest.fixture(scope="module")
def capi():
    from rescan_amd import capi as c
    c.init(0)
    return c


_WANT = {}


def family_want(oracle, name):
    if name not in _WANT:
        f = hc.make(name)
        _WANT[name] = oracle.icp_find_corrs(f["obj"]["pos"], f["obj"]["nor"], f["points"], f["normals"], f["T0"], I4, R, MA)
    return _WANT[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROUTES))
def test_hostile_families(oracle, tmp_path_factory, name):
    got = route(name, tmp_path_factory)
    for fam in hc.FAMILIES:
        want = family_want(oracle, fam)
        for tag in cells(R):
            assert_same(want, [got[f"fam/{fam}/{tag}/{w}"] for w in WHAT], (name, fam, tag))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROUTES))
def test_edges_of_the_culling(oracle, tmp_path_factory, name):
    got = route(name, tmp_path_factory)
    for cname, c in cases().items():
        want = oracle.icp_find_corrs(c["src"], c["src_nor"], c["tgt"], c["tgt_nor"], I4, I4, R, MA)
        for tag in cells(R):
            g = [got[f"case/{cname}/{tag}/{w}"] for w in WHAT]
            assert_brute(c, g, (name, cname, tag))
            if cname not in TIES:
                assert_same(want, g, (name, cname, tag))


@pytest.mark.gpu
def test_default_route_in_process(capi, oracle, tmp_path_factory):
    """The route this process takes by itself (launches of this size: cooperative only, waves by queue length, unless an earlier test of
    the session latched something else), and RS_HIP_NO_CERT=1 (a live flag), against the oracle, the brute force and every child: the
    warm iterations and the golden calls carry the same bits everywhere.  None of the library's names is in the environment meanwhile."""
    saved = {k: v for k, v in os.environ.items() if k.startswith("RS_HIP_") and k != "RS_HIP_LIB"}
    for k in saved:
        del os.environ[k]
    try:
        base = compute(capi)
        os.environ["RS_HIP_NO_CERT"] = "1"
        src, tgt, T0 = switches_pair(capi)
        err, T, it = capi.icp_align(src, tgt, T0, I4, 0.1, MA, max_iter=N_ITER, fixed_iters=True)
        src.close(); tgt.close()
    finally:
        os.environ.pop("RS_HIP_NO_CERT", None)
        os.environ.update(saved)
    assert it == N_ITER
    assert base["warm"].tobytes() == np.float32(err).tobytes() + np.asarray(T, np.float32).tobytes() + np.int32(it).tobytes(), "RS_HIP_NO_CERT=1"
    for fname in golden_names():
        g = dict(np.load(os.path.join(HERE, "golden", fname)))
        want = np.float32(g["err"]).tobytes() + np.asarray(g["T_out"], np.float32).ravel().tobytes() + np.int32(g["iters"]).tobytes()
        assert base[f"golden/{fname}"].tobytes() == want, fname
    for fam in hc.FAMILIES:
        for tag in cells(R):
            assert_same(family_want(oracle, fam), [base[f"fam/{fam}/{tag}/{w}"] for w in WHAT], ("default", fam, tag))
    for cname, c in cases().items():
        for tag in cells(R):
            assert_brute(c, [base[f"case/{cname}/{tag}/{w}"] for w in WHAT], ("default", cname, tag))
    for name in ROUTES:
        got = route(name, tmp_path_factory)
        assert got["warm"].tobytes() == base["warm"].tobytes(), name
        for fname in golden_names():
            assert got[f"golden/{fname}"].tobytes() == base[f"golden/{fname}"].tobytes(), (name, fname)


if __name__ == "__main__":
    child_main(sys.argv[1])
