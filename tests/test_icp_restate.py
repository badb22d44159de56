"""CPU: tests/icp_restate.py, the fp64 restatement of one ICP estimator step that tests/test_gpu_icp_steps.py holds every
traced device iteration to — checked here against exact solutions, the oracle's own variants and the reference's centroid
chains, so that a GPU failure there points at the device and not at the restatement."""
import ctypes as C

import numpy as np
import pytest

import icp_restate as R
from conftest import golden_files, load_golden

I4 = np.eye(4, dtype=np.float32).ravel()


def test_recovers_a_known_rigid_motion():
    """Noise-free point-to-plane correspondences built so that (r, t') solves the centred system with zero residual (the
    target offsets along the normals are the linear model's own, with their mean normal component taken out so that both
    centroids coincide): the fp64 solve returns x to 1e-9, and the error (of the pose before the step) is the offsets' RMS."""
    rng = np.random.default_rng(3)
    n_pts = 5000
    p = rng.uniform(-1.0, 2.0, (n_pts, 3)).astype(np.float32)
    nrm = rng.normal(0, 1, (n_pts, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    w = rng.uniform(0.2, 1.0, n_pts).astype(np.float32)
    r = np.array([0.004, -0.007, 0.002]); t = np.array([0.01, -0.003, 0.006])
    c1 = R.fp64_centroids(p, p, w)[0]
    pc = p.astype(np.float64) - c1.astype(np.float64)
    W = w.astype(np.float64)
    delta = np.sum(np.cross(pc, nrm) * r, axis=1) + nrm @ t
    m = np.linalg.solve((nrm * W[:, None]).T @ nrm, (nrm * (W * delta)[:, None]).sum(axis=0))
    delta -= nrm @ m
    q = p.astype(np.float64) + nrm * delta[:, None]
    x, err = R.solve_x(p, q, nrm, w, c1, c1)
    want = np.concatenate([r, t - m])
    assert np.abs(x - want).max() < 1e-9, (x, want)
    assert err == np.float32(np.sqrt(np.sum(W * delta * delta) / np.sum(W)))
    # and the LDLᵀ is the plain fp64 solve on a well-posed system
    C6, b, _, _ = R.centred_system(p, q, nrm, w, c1, c1)
    assert np.abs(R.ldlt6_solve(C6, b) - np.linalg.solve(C6, b)).max() < 1e-12


def test_ldlt_zero_pivot_solves_with_what_it_has():
    """A singular system (all normals equal): the factorisation stops at the zero pivot like trimesh's, no exception."""
    A = np.zeros((6, 6)); A[3, 3] = 2.0
    assert (R.ldlt6_solve(A, np.ones(6)) == 0).all()      # (the first pivot is 0: every rdiag stays 0)
    assert (R.ldlt6_solve(np.eye(6) * 2.0, np.arange(6.0)) == np.arange(6.0) / 2.0).all()


def test_seq_centroids_are_the_reference_chain(oracle):
    """The fp32 centroid chains of the restatement give orc_weighted_centroid's bits (which tests/test_oracle_vs_ref.py pins
    to the reference's icp__compute_weighted_centroid) — sums that cross many binades, zero weights, far offsets."""
    rng = np.random.default_rng(11)
    for n, off in ((1, 0.0), (63, 1.0), (1025, -4.0), (40_000, 0.0), (200_000, 6.0)):
        p1 = (rng.normal(0, 2.0, (n, 3)) + off).astype(np.float32)
        p2 = (p1 + rng.normal(0, 0.01, (n, 3))).astype(np.float32)
        w = rng.uniform(0, 1, n).astype(np.float32)
        w[rng.uniform(0, 1, n) < 0.2] = 0.0
        if n == 1:
            w[:] = 0.75
        c1, c2, _ = R.seq_centroids(p1, p2, w)
        assert c1.tobytes() == oracle.weighted_centroid(p1, w).tobytes()
        assert c2.tobytes() == oracle.weighted_centroid(p2, w).tobytes()


def test_device_cut_is_the_variant_cut(oracle, gscene):
    """The modelled cut on fp64 sums keeps exactly the weights the oracle's own variant search (find_corrs_variant, mode 2)
    would, and the uncut weights the new oracle export returns are the reference's wherever its cut left them."""
    pts, nor = gscene["points"], gscene["normals"]
    for fname in golden_files("icp_"):
        g = load_golden(fname)
        o = gscene["objects"][int(g["obj"])]
        md = float(g["max_dist"])
        grid = oracle.grid_create(pts, md)
        try:
            c = R.Corrs(oracle, grid, o["pos"], o["nor"], pts, nor, g["T1"], g["T2"], md, g["max_angle"])
        finally:
            oracle.grid_destroy(grid)
        a = oracle.icp_find_corrs(o["pos"], o["nor"], pts, nor, g["T1"], g["T2"], md, g["max_angle"])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, [c.p1, c.n1, c.p2, c.n2, c.w_ref]))
        kept = c.w_ref != 0
        assert (c.w_uncut[kept] == c.w_ref[kept]).all() and len(c) > 100
        w, amb = R.device_weights(c.d2, c.w_uncut, md)
        assert amb == 0
        assert ((w != 0) | (c.w_uncut == 0)).sum() >= kept.sum() * 0.9


def _iterate_variant(oracle, o, pts, nor, g, mode):
    f = oracle.lib.orc_icp_iterate_variant
    f.restype = C.c_float
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    f.argtypes = [f32p, f32p, C.c_int32, f32p, f32p, C.c_int32, f32p, f32p, C.c_float, C.c_float, C.c_int32, C.c_int32,
                  C.c_int32, C.POINTER(C.c_int32), C.c_void_p]
    T = np.asarray(g["T1"], np.float32).ravel().copy()
    it = C.c_int32()
    P, N = np.ascontiguousarray(o["pos"], np.float32), np.ascontiguousarray(o["nor"], np.float32)
    err = f(P, N, len(P), pts, nor, len(pts), T, np.asarray(g["T2"], np.float32).ravel().copy(), float(g["max_dist"]),
            float(g["max_angle"]), 1, 0, mode, C.byref(it), None)
    return np.float32(err), T


@pytest.mark.parametrize("fname", golden_files("icp_"))
def test_first_step_vs_oracle_variants(oracle, gscene, fname):
    """The first iteration of each icp_* fixture: the chains restatement against orc_icp_iterate_variant mode 2 (reference
    chains + fp64 moments whose products and normal matrix it rounds to fp32), the plain one against mode 3 (fp64 centroids
    of fp32 products).  They differ only by that model's roundings: <= 1e-6 per pose entry; the error within 2e-6 relative on
    the same centroids (mode 2: the variant rounds each residual s to fp32), 5e-5 against mode 3, whose centroids are sums of
    fp32 products divided in fp32 — a centroid a few ulp away moves every residual, and the error at first order."""
    g = load_golden(fname)
    o = gscene["objects"][int(g["obj"])]
    pts = np.ascontiguousarray(gscene["points"], np.float32); nor = np.ascontiguousarray(gscene["normals"], np.float32)
    md = float(g["max_dist"])
    grid = oracle.grid_create(pts, md)
    try:
        c = R.Corrs(oracle, grid, o["pos"], o["nor"], pts, nor, g["T1"], g["T2"], md, g["max_angle"])
    finally:
        oracle.grid_destroy(grid)
    for kind, mode, err_tol in ((R.STEP_GRID_CHAINS, 2, 2e-6), (R.STEP_PLAIN, 3, 5e-5)):
        T, err, info = R.restate_step(oracle, kind, c, g["T1"])
        e_v, T_v = _iterate_variant(oracle, o, pts, nor, g, mode)
        d = np.abs(T.astype(np.float64) - T_v).max()
        print(f"{fname} kind {kind} vs mode {mode}: pose {d:.2e}, err {err} vs {e_v}")
        assert info["ambiguous"] == 0
        assert d <= 1e-6 and abs(float(err) - float(e_v)) <= err_tol * float(e_v), (d, err, e_v)
    # the reference-order kinds are the oracle's own step
    T, err, _ = R.restate_step(oracle, R.STEP_REF_ORDER, c, g["T1"])
    e0, T0 = oracle.icp_estimate_pt2pl(c.p1, c.p2, c.n2, c.w_ref, g["T1"])
    assert T.tobytes() == T0.tobytes() and err == np.float32(e0)
