"""TEST INFRASTRUCTURE — an fp64 restatement of ONE step of the device's ICP estimators (lib/rs/icp.h:210-298,393-402 as
rescan_amd/csrc/rs_icp_update.hip, rs_icp_faithful.hip, rs_icp_chain.hip and rs_math.h:icp_solve compute it), for the per-iteration checks of
tests/test_gpu_icp_steps.py and their CPU tests.  A plain helper module: no fixtures, no pytest hooks.

Given the pose T_i a traced call reports before iteration i and that iteration's max_dist, `restate_step` returns the
pose after it and its error, by the estimator kind the device says it ran (rescan_amd.capi.ICP_STEP_*):

* reference order / replay: the oracle's own icp_estimate_pt2pl on the oracle's correspondences (bit-identical expected);
* lane / grid chains, the chains' sums from records: the reference's SEQUENTIAL fp32 centroid chains (icp.h:136-148,
  `1.0f / s` multiplied in, msh_vec_math.h:754) — the device's 2.5 sigma cut is taken from the searches' dist² statistics
  (rs_icp_estimate.h: chain_stats), modelled here from the same fp64 sums (`device_cut`);
* plain / k_icp_moments: fp64 centroids rounded to float as icp_solve rounds them, with the same cut;

and for all four the centred normal equations  Σw c cᵀ, Σw c nᵀ, Σw n nᵀ, Σw c s, Σw n s, Σw s²  in fp64 straight from the fp32
inputs (not by the device's uncentred route), an fp64 LDLᵀ solve (trimesh's ldltdc/ldltsl, as rs_math.h:ldlt6_solve), and the
pose composed in fp32 by the oracle's translate / rotate / mat4_mul in the order of icp.h:280-295.
"""
import numpy as np

STEP_REF_ORDER, STEP_REPLAY, STEP_LANE_CHAINS, STEP_GRID_CHAINS, STEP_PLAIN, STEP_RECORDS, STEP_MOMENTS = range(7)
CHAIN_KINDS = (STEP_LANE_CHAINS, STEP_GRID_CHAINS, STEP_RECORDS)
FP64_CENTROID_KINDS = (STEP_PLAIN, STEP_MOMENTS)
REF_KINDS = (STEP_REF_ORDER, STEP_REPLAY)

f32 = np.float32


def next_max_dist(md):
    """icp.h:493 as the device shrinks it: max(max_dist * 0.95 in double, 0.05), rounded to float."""
    nd = float(f32(md)) * 0.95
    return f32(nd if nd > 0.05 else 0.05)


def _stat_scales(max_dist):
    """rs_icp_api.hip: icp_set_radius — the fixed-point scales of the searches' Σd², Σd⁴ (r² of the float radius)."""
    r2 = float(f32(max_dist) * f32(max_dist))
    e1 = 35 - (np.frexp(r2)[1] - 1)
    e2 = 35 - (np.frexp(r2 * r2)[1] - 1)
    return 2.0 ** e1, 2.0 ** e2


def _cut_from_sums(n, s1, s2, fused):
    """chain_stats / k_icp_moments: mean, sqm in float from the fp64 sums; var = sqm - mean² in float (fused: as one
    rounding of the exact value, what a contracted multiply-add gives); sd = (float)sqrt((double)var)."""
    mean = f32(s1 / n)
    sqm = f32(s2 / n)
    if fused:
        var = f32(float(sqm) - float(mean) * float(mean))       # mean² is exact in fp64 (24 x 24 bits)
    else:
        var = f32(sqm - f32(mean * mean))
    sd = f32(np.sqrt(np.float64(var))) if var >= 0 else f32(np.nan)
    use = bool(np.float64(sd) > 0.000001)
    return use, f32(f32(2.5) * sd)


def device_cut(d2, max_dist):
    """The device's 2.5 sigma cut for these correspondences' dist² (float32 array): (use_sd, cut, ambiguous).

    The searches add Σ1, Σd², Σd⁴ (d⁴ = d2*d2 in fp32) per wave in fp64 and as integers truncated to the fixed-point quantum
    2^-e of icp_set_radius; the fp64 sums here are the exact ones, and the device's lie at most one quantum per wave below
    them (fewer waves than correspondences: bounded by n quanta).  The mean and stddev then round to float, and whether
    var = sqm - mean·mean is contracted into one rounding is the compiler's choice.  Every corner of that box and both
    roundings are evaluated: `ambiguous` counts the correspondences whose weight depends on which one holds (0 almost
    always; the tests report it)."""
    d2 = np.asarray(d2, np.float32)
    n = len(d2)
    if n == 0:
        return False, f32(0), 0
    s1 = float(np.sum(d2.astype(np.float64)))
    s2 = float(np.sum((d2 * d2).astype(np.float64)))
    q1, q2 = _stat_scales(max_dist)
    cuts = set()
    for a in (s1, s1 - n / q1):
        for b in (s2, s2 - n / q2):
            for fused in (False, True):
                cuts.add(_cut_from_sums(n, a, b, fused))
    use0, cut0 = _cut_from_sums(n, s1, s2, False)
    if len(cuts) == 1:
        return use0, cut0, 0
    # correspondences whose fate differs between two candidate cuts
    keep = np.stack([(~u) | (d2 <= c) for u, c in cuts])
    ambiguous = int(np.sum(keep.any(axis=0) & ~keep.all(axis=0)))
    return use0, cut0, ambiguous


def device_weights(d2, w_uncut, max_dist):
    """The weights the chains / plain / k_icp_moments estimators use: the uncut weight, zero beyond the device's cut."""
    use, cut, amb = device_cut(d2, max_dist)
    w = np.asarray(w_uncut, np.float32).copy()
    if use:
        w[np.asarray(d2, np.float32) > cut] = f32(0)
    return w, amb


def seq_centroids(p1, p2, w):
    """icp__compute_weighted_centroid (icp.h:136-148) for both point sets: sequential fp32 chains Σw, Σw·p (fp32 products),
    then msh_vec3_scalar_div = multiply by 1.0f / Σw.  Returns (c1, c2, Σw) as float32."""
    w = np.asarray(w, np.float32)
    if len(w) == 0:
        z = np.zeros(3, np.float32)
        return z, z, f32(0)
    zero = np.zeros(1, np.float32)                                      # (the chains start at +0: 0 + -0 = +0, where accumulate alone would keep x[0])
    tw = np.add.accumulate(np.concatenate([zero, w]), dtype=np.float32)[-1]
    inv = f32(1.0) / tw
    c = []
    for P in (p1, p2):
        P = np.asarray(P, np.float32)
        s = np.array([np.add.accumulate(np.concatenate([zero, P[:, k] * w]), dtype=np.float32)[-1] for k in range(3)], np.float32)
        c.append((s * inv).astype(np.float32))
    return c[0], c[1], f32(tw)


def fp64_centroids(p1, p2, w):
    """icp_solve's own centroids: fp64 Σw·p / Σw rounded to float (rs_math.h:230-231)."""
    W = float(np.sum(np.asarray(w, np.float64)))
    wd = np.asarray(w, np.float64)[:, None]
    c1 = (np.sum(wd * np.asarray(p1, np.float64), axis=0) / W).astype(np.float32)
    c2 = (np.sum(wd * np.asarray(p2, np.float64), axis=0) / W).astype(np.float32)
    return c1, c2


def ldlt6_solve(A, b):
    """trimesh ldltdc / ldltsl <double, 6> (lib/rs/lineqn.h:153-218) as rs_math.h:ldlt6_solve: unpivoted, the upper triangle
    read, a zero pivot stops the factorisation and the solve goes on with what was produced."""
    A = [list(map(float, r)) for r in np.asarray(A, np.float64)]
    rd = [0.0] * 6
    ok = True
    for i in range(6):
        v = [A[i][k] * rd[k] if k < i else 0.0 for k in range(6)]
        for j in range(i, 6):
            if not ok:
                break
            s = A[i][j]
            for k in range(i):
                s -= v[k] * A[j][k]
            if i == j:
                if s == 0:
                    ok = False
                else:
                    rd[i] = 1 / s
            else:
                A[j][i] = s
    x = [0.0] * 6
    for i in range(6):
        s = float(b[i])
        for k in range(i):
            s -= A[i][k] * x[k]
        x[i] = s * rd[i]
    for i in range(5, -1, -1):
        s = 0.0
        for k in range(i + 1, 6):
            s += A[k][i] * x[k]
        x[i] -= s * rd[i]
    return np.array(x, np.float64)


def centred_system(p1, p2, n2, w, c1, c2):
    """The normal equations of icp.h:226-277 centred on (c1, c2), in fp64 from the fp32 inputs with no intermediate
    rounding: returns (C 6x6, b 6, Σw·s², Σw)."""
    W = np.asarray(w, np.float64)
    p = np.asarray(p1, np.float64) - np.asarray(c1, np.float32).astype(np.float64)
    q = np.asarray(p2, np.float64) - np.asarray(c2, np.float32).astype(np.float64)
    n = np.asarray(n2, np.float64)
    c = np.cross(p, n)
    s = np.sum((p - q) * n, axis=1)
    TL = (c * W[:, None]).T @ c
    TR = (c * W[:, None]).T @ n
    BR = (n * W[:, None]).T @ n
    bc = (c * (W * s)[:, None]).sum(axis=0)
    bn = (n * (W * s)[:, None]).sum(axis=0)
    C = np.block([[TL, TR], [TR.T, BR]])
    b = -np.concatenate([bc, bn])
    return C, b, float(np.sum(W * s * s)), float(np.sum(W))


def solve_x(p1, p2, n2, w, c1, c2):
    """The fp64 step x = (rx, ry, rz, tx, ty, tz) and the error sqrt(Σw s² / Σw) rounded to float."""
    C, b, sum_s2, W = centred_system(p1, p2, n2, w, c1, c2)
    err = f32(np.sqrt(max(sum_s2, 0.0) / W))
    return ldlt6_solve(C, b), err


def compose(oracle, x, c1, T1):
    """icp.h:280-295 in fp32 with the oracle's own matrix helpers."""
    c1 = np.asarray(c1, np.float32)
    T = np.eye(4, dtype=np.float32).ravel()
    T = oracle.translate(T, c1)
    T = oracle.translate(T, np.asarray(x[3:6], np.float64).astype(np.float32))
    for k in range(3):
        ax = np.zeros(3, np.float32); ax[k] = 1.0
        T = oracle.rotate(T, f32(x[k]), ax)
    T = oracle.translate(T, -c1)
    return oracle.mat4_mul(T, T1)


class Corrs:
    """One iteration's correspondences from the oracle (pinned bit for bit to the device's searches)."""

    def __init__(self, oracle, grid2, src_pos, src_nor, tgt_pos, tgt_nor, T1, T2, max_dist, max_angle):
        self.p1, self.n1, self.p2, self.n2, self.w_ref, self.d2, self.w_uncut = oracle.icp_find_corrs_uncut(
            grid2, src_pos, src_nor, tgt_pos, tgt_nor, T1, T2, max_dist, max_angle)
        self.max_dist = f32(max_dist)

    def __len__(self):
        return len(self.w_ref)


def restate_step(oracle, kind, corrs, T1):
    """One estimator step of `kind` from pose T1 (16 floats) on `corrs`: (T_next float32[16], err float32 or None, info).
    err None: the iteration produced no error (no correspondences, Σw <= 1e-7: icp.h:455-466) and the pose stays.
    info: dict(ambiguous = correspondences on the uncertain side of the modelled cut, n = correspondences)."""
    T1 = np.asarray(T1, np.float32).ravel()
    info = dict(ambiguous=0, n=len(corrs))
    if len(corrs) == 0:
        return T1.copy(), None, info
    if kind in REF_KINDS:
        tw = np.add.accumulate(corrs.w_ref, dtype=np.float32)[-1]
        if float(tw) <= 1e-7:                                      # icp.h:466: the float against the DOUBLE 1e-7; f32(1e-7) lies above it
            return T1.copy(), None, info
        err, T = oracle.icp_estimate_pt2pl(corrs.p1, corrs.p2, corrs.n2, corrs.w_ref, T1)
        return T, f32(err), info
    w, info["ambiguous"] = device_weights(corrs.d2, corrs.w_uncut, corrs.max_dist)
    if float(f32(np.sum(w.astype(np.float64)))) <= 1e-7:       # icp_solve: (float)W <= 1e-7, compared in double
        return T1.copy(), None, info
    if kind in CHAIN_KINDS:
        c1, c2, _ = seq_centroids(corrs.p1, corrs.p2, w)
    elif kind in FP64_CENTROID_KINDS:
        c1, c2 = fp64_centroids(corrs.p1, corrs.p2, w)
    else:
        raise ValueError(f"no restatement for estimator kind {kind}")
    x, err = solve_x(corrs.p1, corrs.p2, corrs.n2, w, c1, c2)
    return compose(oracle, x, c1, T1), err, info
