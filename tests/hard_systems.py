"""Seeded 6x6 systems on which the end of an ICP iteration — the Σw test, the unpivoted LDLᵀ, the pose composed through sinf / cosf,
the n_corr == 0 break and the `i > 5 && delta < 1e-5` stop — does something else than on a well-conditioned room, and the measures to
hold each family to its claim (tests/test_hard_systems_cpu.py).  A plain helper module like hard_sums.py: no fixtures, no pytest hooks.

The clouds match themselves as hard_sums.cloud does: the target's points lie on a 0.125 lattice (3-D, so that Σw c cᵀ has rank 3
wherever the normals allow it), above the 0.1 m search radius; the source is the target moved by per-point offsets that are multiples of
2^-10 within 2^-7, so every source point finds its own twin and the right-hand side is not zero.  Source and target normals are equal.

  axis_x, axis_y, axis_z     every normal is one axis.  With n = e_k the k-th component of c = p x n is p_i * 0 - p_j * 0: row and column k
                             of the 6x6 are zero in any arithmetic, centred (icp.h:226-277) or uncentred (rs_math.h:icp_solve).  Pivot k is
                             exactly 0, the factorisation stops there (lineqn.h:153-196), rd[k..5] stay 0 and x[k..5] = 0: axis_x never
                             moves the pose, axis_y turns about x only, axis_z about x and y — and tz stays 0 although the target is
                             shifted in z: the reference's quirk, kept.
  axes_yz, axes_xz, axes_xy  normals drawn from two axes: the missing translation's row (3, 4, 5) is zero; pivots 0..2 are not.  The stop at
                             pivot 3 also zeroes ty and tz.
  tilted_jitter              one generic unit normal plus multiples of 2^-22 per component: no exact zeros, the system has rank 3 up to
                             rounding noise, pivots 2, 4 and 5 are tiny (1e-15 ... 1e-11 in fp64) and of either sign, and the fp64 step
                             runs to hundreds or thousands of radians (rs_sincosf_model's large-argument branch): the fp64 kinds' next
                             search finds nothing, n_corr == 0 in iteration 1.  The reference's own fp32 accumulators carry noise of
                             2^-24 of their values, ten thousand times the jitter's share: ITS pivots are larger, its steps stay
                             below a few radians (no pose entry above 2), and its loop runs on for 2 to 10 iterations.
  big_step                   free systems (big_step) that are WELL conditioned and whose twins lie thousands of metres away: steps of
                             1e2 ... 2e5 radians in the reference's own arithmetic — sinf / cosf beyond 120 with a defined value.
  vanish                     one to three points whose source normals are nearly perpendicular to the target's: dots of 2^-24, 2^-23 or 0
                             under max_angle = 1.6 (every dot passes the gate): Σw on either side of the double 1e-7.

and free systems for rs_hip_icp_estimate_pt2pl alone (free_system): single weights at f32(1e-7) and its neighbours, negative weights,
n = 1, 2, 3.
"""
import numpy as np

import hard_sums as H
import icp_restate as R

F = np.float32
I4 = np.eye(4, dtype=F).ravel()
MA = F(np.deg2rad(60.0))
RADIUS = H.RADIUS
SPACING = H.SPACING
BASE = np.array([0.5, -0.75, 1.25])                       # the lattice's corner: exact in binary
NORMAL_AXES = {"axis_x": (0,), "axis_y": (1,), "axis_z": (2,), "axes_yz": (1, 2), "axes_xz": (0, 2), "axes_xy": (0, 1)}
DEAD_PIVOT = {"axis_x": 0, "axis_y": 1, "axis_z": 2, "axes_yz": 3, "axes_xz": 4, "axes_xy": 5}
AXIS_FAMILIES = tuple(NORMAL_AXES)
CLOUDS = AXIS_FAMILIES + ("tilted_jitter",)
TILT = np.array([0.36, -0.48, 0.8])                       # a unit vector with no zero component
# the whole target is this far from where the offsets alone would put it: every family has a step to take
BIAS = np.array([3, -2, 5]) * 2.0 ** -10
F32_1E7 = F(1e-7)                                         # 1.0000000116860974e-07: ABOVE the double 1e-7 the reference compares with
VANISH_MAX_ANGLE = F(1.6)

REF_SIZES = (3, 7, 64, 129, 1025)                         # reference order and replay
LANE_SIZES = (64, 1025)
GRID_SIZES = (65, 4097)                                   # grid chains and RECORDS
MOMENTS_SIZE = 257
PLAIN_SIZE = 65537


JITTERED = 16
# tilted_jitter holds its claim (all three step angles in [120, 1e6)) at these sizes; at 3 points the step is zero, and at 65 537 the
# angles stay below 25 rad however few points are jittered (tests/test_hard_systems_cpu.py prints what it meets)
TILTED_SIZES = (7, 64, 65, 129, 257, 1025, 4097)
# the offsets are chosen so that the oracle's own stop test is decided by a margin (every |err_i - err_{i-1}|, i > 5, outside
# [0.5e-5, 2e-5]): the seed per (family, size) where seed 0 does not give that
SEEDS = {("axes_yz", 257): 1, ("axes_xz", 64): 1, ("axes_xz", 129): 2, ("axes_xy", 64): 1, ("axes_xy", 1025): 6, ("axes_xy", 4097): 1,
         ("tilted_jitter", 1025): 1, ("tilted_jitter", 4097): 1}
# ... which no seed gives at 65 537 points: every weight is (1 - d² / max_dist) * dot, max_dist shrinks by 5 % per iteration, and with
# 65 537 addends that alone moves the error by ~1e-5 per iteration.  That size runs a fixed number of iterations (the plain step's
# only use below 262 144 points anyway); the stop test is met at the sizes up to 4 097.
STOP_TEST_UP_TO = 4097
PLAIN_ITERS = 5                                           # three plain iterations and two of the grid chains


def sizes_of(name):
    every = sorted(set(REF_SIZES + LANE_SIZES + GRID_SIZES + (MOMENTS_SIZE, PLAIN_SIZE)))
    return [n for n in every if name != "tilted_jitter" or n in TILTED_SIZES]


def cloud(name, n, seed=None):
    """(src_pos, tgt_pos, nor) float32 of family `name` with n points; source and target share the normals."""
    seed = SEEDS.get((name, n), 0) if seed is None else seed
    rng = np.random.default_rng([seed, 300 + CLOUDS.index(name), n])
    g = H._lattice3(n)
    g = g[rng.permutation(len(g))[:n]]
    tgt = g * SPACING + BASE
    k = rng.integers(-8, 9, (n, 3))
    k = np.clip(k + np.array([3, -2, 5]), -8, 8)                      # multiples of 2^-10 within 2^-7, not centred on zero
    src = tgt + k * 2.0 ** -10
    if name in NORMAL_AXES:
        ax = np.array(NORMAL_AXES[name])
        nor = np.zeros((n, 3), F)
        nor[np.arange(n), ax[rng.integers(0, len(ax), n)]] = rng.choice(np.array([1.0, -1.0], F), n)
        for j, a in enumerate(ax[:min(n, len(ax))]):
            nor[j] = 0; nor[j, a] = 1.0                                 # every axis of the family is met, whatever n
    elif name == "tilted_jitter":
        # (shortened by 2^-18: no dot product of two of these exceeds 1, where acosf is NaN and the gate closes.  JITTERED points carry
        #  the jitter whatever n: the tiny pivots stay of one size while the right-hand side grows with n)
        j = rng.integers(-3, 4, (n, 3)) * 2.0 ** -22
        j[rng.permutation(n)[JITTERED:]] = 0
        nor = ((TILT * (1 - 2.0 ** -18)).astype(F)[None, :] + j.astype(F)).astype(F)
    else:
        raise KeyError(name)
    return src.astype(F), tgt.astype(F), nor


VANISH_CASES = {"one_2^-24": (2.0 ** -24,), "one_2^-23": (2.0 ** -23,), "two_2^-24": (2.0 ** -24, 2.0 ** -24),
                "2^-24_and_0": (2.0 ** -24, -1.0), "three_2^-24": (2.0 ** -24,) * 3, "2^-24_2^-23_0": (2.0 ** -24, 2.0 ** -23, -0.5)}


def vanish(case):
    """(src_pos, src_nor, tgt_pos, tgt_nor): the target's normals are +z, source normal i is (1, 0, d_i) with d_i of VANISH_CASES (a
    negative d_i: the clamped dot is 0), so that the dot product is d_i exactly; positions as in cloud()."""
    d = np.array(VANISH_CASES[case])
    n = len(d)
    tgt = np.arange(n)[:, None] * np.array([SPACING, 0, 0]) + BASE
    src = tgt + np.array([[1, 0, -2], [0, -2, 1], [-2, 1, 0]])[:n] * 2.0 ** -10      # one dist² for all: sd = 0, no 2.5 sigma cut
    src_nor = np.stack([np.ones(n), np.zeros(n), d], axis=1)
    tgt_nor = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    return src.astype(F), src_nor.astype(F), tgt.astype(F), tgt_nor.astype(F)


def vanish_weights(case, max_dist=RADIUS):
    """The weights the search gives a vanish case at the identity, from the design alone: (1 - d² / max_dist) * max(dot, 0) in fp32,
    d² in the reference's expression order (icp.h:387)."""
    src, sn, tgt, tn = vanish(case)
    v = tgt - src
    d2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).astype(F)
    dot = np.maximum(sn[:, 2], F(0))
    return ((F(1.0) - d2 / F(max_dist)) * dot).astype(F)


def vanished(total):
    """icp.h:466 and all four sites of the library: the FLOAT total against the DOUBLE 1e-7."""
    return bool(float(F(total)) <= 1e-7)


FREE_WEIGHTS = {"f32(1e-7)": (F32_1E7,), "below": (np.nextafter(F32_1E7, F(0)),), "above": (np.nextafter(F32_1E7, F(1)),),
                "2^-24": (F(2.0 ** -24),), "2^-23": (F(2.0 ** -23),),
                "negative_3": (F(1.0), F(-0.25), F(-0.5)), "negative_2": (F(-0.5), F(1.0)),
                "n1": (F(0.75),), "n2": (F(0.75), F(1.0)), "n3": (F(0.75), F(1.0), F(0.5))}
NEGATIVE = ("negative_3", "negative_2")


def free_system(case, seed=0):
    """(p1, p2, n2, w) float32 for rs_hip_icp_estimate_pt2pl: len(w) lattice points, their twins 2^-10 offsets away, generic unit normals
    and the weights of FREE_WEIGHTS[case]."""
    w = np.array(FREE_WEIGHTS[case], F)
    n = len(w)
    rng = np.random.default_rng([seed, 400 + list(FREE_WEIGHTS).index(case)])
    p2 = H._lattice3(8)[rng.permutation(8)[:n]] * SPACING + BASE
    p1 = p2 + rng.integers(-8, 9, (n, 3)) * 2.0 ** -10 + BIAS
    return p1.astype(F), p2.astype(F), H._unit(rng, n), w


BIG_STEP_SIZES = (7, 64, 129, 1025)                      # (three points: singular)
BIG_STEP_SEEDS = range(48)


def big_step(n, seed=0):
    """(p1, p2, n2, w) float32, WELL conditioned, with a step of hundreds to thousands of radians in the reference's own arithmetic:
    the source on the lattice, every twin thousands of metres from it in a direction of its own, generic unit normals, weights from
    CLOUD_WEIGHTS.  Residuals of ~2^12 (2^15 above 129 points) over lever arms of ~1/2 are angles of ~2^13 / sqrt(n); nothing is near singular, so the fp64
    restatement's angles (icp_restate.solve_x) are the reference's to a few ulp — and every one of them goes through the
    large-argument branch of sinf / cosf."""
    rng = np.random.default_rng([seed, 500, n])
    g = H._lattice3(max(n, 8))
    p1 = g[rng.permutation(len(g))[:n]] * SPACING + BASE
    far = 2.0 ** 15 if n > 129 else 2.0 ** 12                      # (the angles fall as 1 / sqrt(n))
    p2 = p1 + np.round(rng.normal(0, 1.0, (n, 3)) * far * 16) / 16
    w = rng.choice(np.array(H.CLOUD_WEIGHTS), n)
    return p1.astype(F), p2.astype(F), H._unit(rng, n), w.astype(F)


# ---- the reference's loop, row by row ---------------------------------------------------------------------------------------------

def oracle_rows(O, src, src_nor, tgt, tgt_nor, T0, max_dist=RADIUS, max_angle=MA, max_iter=100, fixed_iters=False):
    """icp_align (icp.h:416-500) driven from here through the oracle's own search and estimator, so that every iteration is seen:
    (poses (iters, 16), errs (iters,), n_corr (iters,)).  A row of an iteration that broke off (no correspondence, Σw <= 1e-7)
    holds the pose and the error it met.  tests/test_hard_systems_cpu.py holds the last row to O.icp_align's own bits."""
    T = np.asarray(T0, F).ravel().copy()
    md = F(max_dist)
    err = F(1e6)
    poses, errs, ncs = [], [], []
    g = O.grid_create(tgt, max_dist)
    try:
        for i in range(max_iter):
            prev = err
            p1, n1, p2, n2, w = O.icp_find_corrs_uncut(g, src, src_nor, tgt, tgt_nor, T, I4, md, max_angle)[:5]
            ncs.append(len(w))
            stop = len(w) == 0 or vanished(H.seq(w)[-1])
            if not stop:
                with np.errstate(all="ignore"):
                    e, T = O.icp_estimate_pt2pl(p1, p2, n2, w, T)
                err = F(e)
            poses.append(T.copy()); errs.append(err)
            if stop:
                break
            with np.errstate(all="ignore"):
                delta = np.abs(F(prev - err))
            if not fixed_iters and i > 5 and delta < 1e-5:
                break
            md = R.next_max_dist(md)
    finally:
        O.grid_destroy(g)
    return np.array(poses, F).reshape(-1, 16), np.array(errs, F), np.array(ncs)


def stop_deltas(errs):
    """|err_i - err_{i-1}| in fp32 for i > 5 (err_-1 = 1e6): what the stop test of icp.h:489 compares with 1e-5."""
    e = np.concatenate([[F(1e6)], np.asarray(errs, F)])
    with np.errstate(all="ignore"):
        d = np.abs((e[:-1] - e[1:]).astype(F))
    return d[6:]


# ---- the two systems: centred (the reference, icp_restate) and uncentred (rs_math.h: icp_solve, op for op) ---------------------------

def moments(p1, p2, n2, w):
    """The 35 uncentred fp64 moments of rs_icp_estimate.h:moments_add, summed in index order."""
    M = np.zeros(35)
    for i in range(len(w)):
        W = float(w[i]); p = [float(v) for v in p1[i]]; q = [float(v) for v in p2[i]]; n = [float(v) for v in n2[i]]
        a = [p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0]]
        e = (p[0] - q[0]) * n[0] + (p[1] - q[1]) * n[1] + (p[2] - q[2]) * n[2]
        M[0] += W
        for k in range(3):
            M[1 + k] += W * p[k]; M[4 + k] += W * q[k]
        M[7] += W * a[0] * a[0]; M[8] += W * a[0] * a[1]; M[9] += W * a[0] * a[2]
        M[10] += W * a[1] * a[1]; M[11] += W * a[1] * a[2]; M[12] += W * a[2] * a[2]
        for r in range(3):
            for c in range(3):
                M[13 + 3 * r + c] += W * a[r] * n[c]
        M[22] += W * n[0] * n[0]; M[23] += W * n[0] * n[1]; M[24] += W * n[0] * n[2]
        M[25] += W * n[1] * n[1]; M[26] += W * n[1] * n[2]; M[27] += W * n[2] * n[2]
        for k in range(3):
            M[28 + k] += W * a[k] * e; M[31 + k] += W * n[k] * e
        M[34] += W * e * e
    return M


def uncentred_system(M, cen=None):
    """rs_math.h:icp_solve from the moments to the 6x6, the right-hand side and the error, operation for operation in Python floats
    (fp64): returns (C 6x6, b 6, err float32, c1 float32[3])."""
    W = float(M[0])
    c1f = [F(M[1 + k] / W) if cen is None else F(cen[k]) for k in range(3)]
    c2f = [F(M[4 + k] / W) if cen is None else F(cen[3 + k]) for k in range(3)]
    c1 = [float(v) for v in c1f]
    dl = [float(c1f[k]) - float(c2f[k]) for k in range(3)]
    Maa = [[M[7], M[8], M[9]], [M[8], M[10], M[11]], [M[9], M[11], M[12]]]
    Man = [[M[13 + 3 * r + c] for c in range(3)] for r in range(3)]
    Mnn = [[M[22], M[23], M[24]], [M[23], M[25], M[26]], [M[24], M[26], M[27]]]
    vae, vne, see = [M[28], M[29], M[30]], [M[31], M[32], M[33]], M[34]
    X = [[0.0, -c1[2], c1[1]], [c1[2], 0.0, -c1[0]], [-c1[1], c1[0], 0.0]]

    def acc(terms):
        s = 0.0
        for t in terms:
            s += t
        return s
    XMnn = [[acc(X[r][k] * Mnn[k][c] for k in range(3)) for c in range(3)] for r in range(3)]
    ManXt = [[acc(Man[r][k] * X[c][k] for k in range(3)) for c in range(3)] for r in range(3)]
    XMnnXt = [[acc(XMnn[r][k] * X[c][k] for k in range(3)) for c in range(3)] for r in range(3)]
    TL = [[Maa[r][c] - ManXt[r][c] - ManXt[c][r] + XMnnXt[r][c] for c in range(3)] for r in range(3)]
    TR = [[Man[r][c] - XMnn[r][c] for c in range(3)] for r in range(3)]
    Mnn_d = [acc(Mnn[r][k] * dl[k] for k in range(3)) for r in range(3)]
    Man_d = [acc(Man[r][k] * dl[k] for k in range(3)) for r in range(3)]
    bc, bn = [0.0] * 3, [0.0] * 3
    for r in range(3):
        xv = acc(X[r][k] * vne[k] for k in range(3)); xm = acc(X[r][k] * Mnn_d[k] for k in range(3))
        bc[r] = vae[r] - Man_d[r] - xv + xm
        bn[r] = vne[r] - Mnn_d[r]
    s = see - 2.0 * (dl[0] * vne[0] + dl[1] * vne[1] + dl[2] * vne[2]) + (dl[0] * Mnn_d[0] + dl[1] * Mnn_d[1] + dl[2] * Mnn_d[2])
    clamped = s < 0.0
    if clamped:
        s = 0.0
    with np.errstate(all="ignore"):
        err = F(np.sqrt(np.float64(s) / np.float64(W)))
    C = np.zeros((6, 6)); b = np.zeros(6)
    for r in range(3):
        for c in range(3):
            C[r][c] = TL[r][c]; C[r][3 + c] = TR[r][c]; C[3 + r][c] = TR[c][r]; C[3 + r][3 + c] = Mnn[r][c]
        b[r] = -bc[r]; b[3 + r] = -bn[r]
    return C, b, err, np.array(c1f, F), clamped


def pivots(A):
    """The pivots R.ldlt6_solve meets (the factorisation of lineqn.h:153-196, upper triangle read), up to and including the first that
    is exactly zero: a list of at most six floats."""
    A = [list(map(float, r)) for r in np.asarray(A, np.float64)]
    rd, out = [0.0] * 6, []
    for i in range(6):
        v = [A[i][k] * rd[k] if k < i else 0.0 for k in range(6)]
        for j in range(i, 6):
            s = A[i][j]
            for k in range(i):
                s -= v[k] * A[j][k]
            if i == j:
                out.append(s)
                if s == 0:
                    return out
                rd[i] = 1 / s
            else:
                A[j][i] = s
    return out


def first_step(O, name, n, seed=0):
    """The first iteration of family `name` at the identity: the oracle's correspondences (with its cut) and, from them, the centred
    system (C, b), the uncentred one (C, b) and the step x of the centred one."""
    src, tgt, nor = cloud(name, n, seed)
    g = O.grid_create(tgt, RADIUS)
    try:
        p1, n1, p2, n2, w = O.icp_find_corrs_uncut(g, src, nor, tgt, nor, I4, I4, RADIUS, MA)[:5]
    finally:
        O.grid_destroy(g)
    c1, c2, _ = R.seq_centroids(p1, p2, w)
    C, b, _, _ = R.centred_system(p1, p2, n2, w, c1, c2)
    Cu, bu, _, _, _ = uncentred_system(moments(p1, p2, n2, w))
    return dict(n_corr=len(w), C=C, b=b, Cu=Cu, bu=bu, x=R.ldlt6_solve(C, b), xu=R.ldlt6_solve(Cu, bu))
