"""Hostile inputs for the plane detector, the inlier gather and the relabel, and NumPy emulations of the arithmetic the kernels must
NOT take.  Plain NumPy, importable without a GPU; every generator is deterministic from its seed.

fp32 operations are emulated in float64: the product of two floats is exact there, a sum or difference of two floats rounds once
to 53 bits and then to 24, which is the correctly rounded fp32 result (53 >= 2 * 24 + 2), and a fused multiply-add is the exact
product plus the addend, rounded to odd in float64 and then to fp32.  A *witness* for a variant is a point whose decision
(|offset| < dist_threshold, |dot| > dot_threshold, val < 0) under that variant differs from the decision under `plain`, the
reference's order: a kernel that took the variant's arithmetic gives another count there, so a test that holds witnesses can fail.

tests/test_hard_planes_cpu.py asserts that `plain` is the restatement bit for bit, that every family holds the witnesses it is
meant to hold, and that the restatement reproduces the reference's recordings of trimmed subsets (tests/golden/planes_hostile.npz,
written by tools/plane_fixture/gen.py); tests/test_gpu_hard_planes.py runs the kernels on the families."""
import numpy as np

import planes_restate as R

F, D = np.float32, np.float64
PLANE_TILE = 1024                                        # rs_planes.hip
N_CAND, N_HYP = 2 * PLANE_TILE + 1, 257                  # across a tile, a block of hypotheses and a wave
FLT_MAX, FLT_MIN = np.finfo(F).max, np.finfo(F).tiny
T08 = F(0.8)
INT32_MAX, INT32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


# ---- fp32 arithmetic in float64 ----------------------------------------------------------------------------------------------

def r32(x):
    with np.errstate(all="ignore"):
        return np.asarray(x, D).astype(F).astype(D)


def mul(a, b):
    with np.errstate(all="ignore"):
        return r32(np.asarray(a, D) * np.asarray(b, D))


def add(a, b):
    with np.errstate(all="ignore"):
        return r32(np.asarray(a, D) + np.asarray(b, D))


def sub(a, b):
    with np.errstate(all="ignore"):
        return r32(np.asarray(a, D) - np.asarray(b, D))


def fma(a, b, c):
    """round32( a * b + c ) with one rounding: the float64 sum is rounded to odd before it is rounded to fp32"""
    a, b, c = np.broadcast_arrays(np.asarray(a, D), np.asarray(b, D), np.asarray(c, D))
    shape = a.shape
    a, b, c = a.reshape(-1), b.reshape(-1), c.reshape(-1)
    with np.errstate(all="ignore"):
        p = a * b                                        # exact
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                    # TwoSum: p + c = s + e exactly
        bits = s.copy().view(np.int64)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((bits & 1) == 0)
        away = (e > 0) == (s > 0)
        bits = np.where(fix, np.where(away, bits + 1, bits - 1), bits)
        return r32(bits.view(D)).reshape(shape)


def _dot3_variants(x, y):
    """x, y: three float64 arrays each (fp32 values).  The fp32 dot under each order."""
    t = [mul(x[i], y[i]) for i in range(3)]
    return dict(plain=add(add(t[0], t[1]), t[2]), fma=fma(x[2], y[2], fma(x[1], y[1], t[0])), other=add(t[0], add(t[1], t[2])))


def offset_variants(pos, center, normal):
    """The fp32 offset n . (p - c) of every point under four orders of evaluation: plain (the reference's and the restatement's),
    fma (fma( n2, d2, fma( n1, d1, n0 * d0 ) )), pre (n . p - n . c) and other (x + (y + z)).  center, normal: (3,) gives (N,)
    arrays, (H, 3) gives (H, N)."""
    p = np.ascontiguousarray(pos, F).reshape(-1, 3).astype(D)
    c, n = np.asarray(center, F).astype(D), np.asarray(normal, F).astype(D)
    if c.ndim == 2:
        c, n, p = c[:, None, :], n[:, None, :], p[None, :, :]
    P, C, N = [p[..., i] for i in range(3)], [c[..., i] for i in range(3)], [n[..., i] for i in range(3)]
    d = [sub(P[i], C[i]) for i in range(3)]
    out = _dot3_variants(N, d)
    n_p, n_c = _dot3_variants(N, P)["plain"], _dot3_variants(N, C)["plain"]
    out["pre"] = sub(n_p, n_c)
    with np.errstate(all="ignore"):
        return {k: np.broadcast_to(v, np.broadcast(P[0], C[0]).shape).astype(F) for k, v in out.items()}


def dot_variants(nor, normal):
    """The gather's nrm . n per point: plain, fma, other (before msh_abs)."""
    q, n = np.ascontiguousarray(nor, F).reshape(-1, 3).astype(D), np.asarray(normal, F).astype(D)
    out = _dot3_variants([q[:, i] for i in range(3)], [n[i] for i in range(3)])
    with np.errstate(all="ignore"):
        return {k: v.astype(F) for k, v in out.items() if k != "pre"}


def val_variants(pos, poly):
    """The quad test's val = n1 . n2 for the three tested corners: (3, N) fp32 arrays, plain and with the last dot contracted
    (the cross products as the reference rounds them)."""
    pos, poly = np.ascontiguousarray(pos, F).reshape(-1, 3), np.asarray(poly, F)
    out = dict(plain=[], fma=[])
    with np.errstate(all="ignore"):
        for i in range(3):
            a, b, c = poly[i], poly[i + 1], poly[(i + 2) % 4]
            v1, v2 = (b - a)[None, :], (c - b)[None, :]
            v3 = pos - b[None, :]
            n1, n2 = R.cross(v1, v2).astype(D), R.cross(np.broadcast_to(v1, v3.shape), v3).astype(D)
            v = _dot3_variants([n1[:, k] for k in range(3)], [n2[:, k] for k in range(3)])
            for k in out:
                out[k].append(np.broadcast_to(v[k], (len(pos),)).astype(F))
    return {k: np.stack(v) for k, v in out.items()}


def inlier(off, dist_threshold):
    with np.errstate(invalid="ignore"):
        return R.absf(off) < F(dist_threshold)


def variant_votes(case, mask=None):
    """{variant: (H,) int32 counts} the votes kernel would give had it taken that arithmetic; `plain` is the restatement's."""
    m = np.ones(len(case["pos"]), bool) if mask is None else np.asarray(mask).astype(bool)
    off = offset_variants(case["pos"][m], case["center"], case["normal"])
    return {k: inlier(v, case["dist_threshold"]).sum(axis=1).astype(np.int32) for k, v in off.items()}


def vote_witnesses(case):
    """{variant: number of (hypothesis, point) pairs whose decision differs from plain}"""
    off = offset_variants(case["pos"], case["center"], case["normal"])
    plain = inlier(off["plain"], case["dist_threshold"])
    return {k: int((inlier(v, case["dist_threshold"]) != plain).sum()) for k, v in off.items() if k != "plain"}


def flushed_votes(case):
    """The counts with every subnormal product, sum and the threshold flushed to zero."""
    def ftz(x):
        return np.where(np.abs(x) < FLT_MIN, D(0), x)
    p = case["pos"].astype(D)[None]; c = case["center"].astype(D)[:, None]; n = case["normal"].astype(D)[:, None]
    t = [ftz(mul(n[..., i], ftz(sub(p[..., i], c[..., i])))) for i in range(3)]
    off = ftz(add(ftz(add(t[0], t[1])), t[2]))
    with np.errstate(invalid="ignore"):
        return (np.abs(off) < ftz(D(F(case["dist_threshold"])))).sum(axis=1).astype(np.int32)


# ---- vote families -----------------------------------------------------------------------------------------------------------

def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _oblique(rng, k):
    """k unit normals with no component below 0.25 in magnitude (float64)"""
    v = rng.uniform(0.25, 1.0, (k, 3)) * rng.choice([-1.0, 1.0], (k, 3))
    return _unit(v)


def _frame(n):
    """(a, b): orthonormal float64 directions in the planes of the normals n (k, 3)"""
    n = _unit(np.asarray(n, D))
    helper = np.where(np.abs(n[:, :1]) < 0.7, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    a = _unit(np.cross(n, helper))
    return a, np.cross(n, a)


def _band_points(rng, center, normal, thr, span=1.0, u0=0.0):
    """One point per row of (center, normal), fp32 models: c + u a + v b +- (thr + e) n / (n . n), e within 2 ulp of the largest
    coordinate, in float64 and then rounded.  Returns (pos, side)."""
    c, n = np.asarray(center, F).astype(D), np.asarray(normal, F).astype(D)
    a, b = _frame(n)
    k = len(c)
    u, v = u0 + rng.uniform(-span, span, (k, 1)), rng.uniform(-span, span, (k, 1))
    base = c + u * a + v * b
    side = rng.choice([-1.0, 1.0], (k, 1))
    e = rng.uniform(-2, 2, (k, 1)) * np.spacing(np.abs(base).max(axis=1, keepdims=True).astype(F)).astype(D)
    p = base + side * (D(F(thr)) + e) * n / (n * n).sum(axis=1, keepdims=True)
    return p.astype(F), side[:, 0]


def _case(name, pos, center, normal, thr, special):
    h = len(center)
    return dict(name=name, pos=np.ascontiguousarray(pos, F), mask=np.ones(len(pos), np.uint8), center=np.ascontiguousarray(center, F),
                normal=np.ascontiguousarray(normal, F), valid=(np.arange(h) % 5 != 3).astype(np.uint8), dist_threshold=F(thr),
                special=np.asarray(special).astype(np.uint8))


def _band_case(name, seed, thr, centres, n=N_CAND, h=N_HYP):
    rng = np.random.default_rng(seed)
    normal = _oblique(rng, h).astype(F)
    center = np.asarray(centres(rng, h), D).astype(F)
    owner = np.arange(n) % h
    pos, side = _band_points(rng, center[owner], normal[owner], thr)
    out = _case(name, pos, center, normal, thr, side > 0)
    out["owner"] = owner
    return out


def _near(rng, h):
    return rng.uniform(-0.55, 0.55, (h, 3))              # within 1 m of the origin


def _three_metres(rng, h):
    return 3.0 * _unit(rng.normal(0, 1, (h, 3))) + rng.uniform(-0.2, 0.2, (h, 3))


FAR_CENTRES = np.array([[1e3, -1e3, -5e2], [1e4, -1e4, 1e4], [-1e3, -1e3, -5e2]])          # the last: an all-negative copy


def _far(rng, h):
    return FAR_CENTRES[np.arange(h) % 3] + rng.uniform(-0.5, 0.5, (h, 3))


def band(n=N_CAND, h=N_HYP):
    return [_band_case("band_0.01", 11, 0.01, _near, n, h), _band_case("band_0.033", 12, 0.033, _near, n, h)]


def band_3m(n=N_CAND, h=N_HYP):
    return [_band_case("band_3m_0.01", 21, 0.01, _three_metres, n, h), _band_case("band_3m_0.033", 22, 0.033, _three_metres, n, h)]


def far(n=N_CAND, h=N_HYP):
    return [_band_case("far", 31, 0.033, _far, n, h)]


def exact(n=N_CAND, h=N_HYP):
    """Axis-aligned normals, centre components 0 and 1.0: the offset is one subtraction.  Each point sits on its own axis at the
    centre component +- t, t in (thr, the float below, the float above), rounded once where the centre component is 1.0; its other
    two coordinates come from OTHER, whose distances to 0 and 1 are 0 or at least 0.25.  out["inlier"] (H, N) is the decision in
    exact arithmetic, |p_k - c_k| < thr: every difference is either exactly representable or further than 0.2 from the threshold
    (asserted below), so no rounding of the kernel's can matter.  The counts are its row sums."""
    thr = F(0.033)
    T = np.array([thr, np.nextafter(thr, F(0)), np.nextafter(thr, F(np.inf))], F)
    OTHER = np.array([0.0, -0.0, 1.0, 0.25, -3.0, 7.5], F)
    k = np.arange(n)
    axis, cc, kind, sign = k % 3, (k // 3) % 2, (k // 6) % 3, np.where((k // 18) % 2 == 0, F(1), F(-1))
    pos = np.stack([OTHER[(k // 36 + 1 + 2 * j) % 6] for j in range(3)], axis=1)
    pos[k, axis] = cc.astype(F) + sign * T[kind]         # an fp32 sum
    j = np.arange(h)
    h_axis, h_sign = j % 3, np.where((j // 3) % 2 == 0, F(1), F(-1))
    center = np.stack([((j // 6) >> b & 1).astype(F) for b in range(3)], axis=1)
    center[::7] = np.where(center[::7] == 0, F(-0.0), center[::7])
    normal = np.zeros((h, 3), F); normal[j, h_axis] = h_sign
    normal[1::2] = np.where(normal[1::2] == 0, F(-0.0), normal[1::2])
    diff = pos.astype(D)[None, :, :] - center.astype(D)[:, None, :]
    diff = np.take_along_axis(diff, np.broadcast_to(h_axis[:, None, None], (h, n, 1)), axis=2)[..., 0]
    assert ((r32(diff) == diff) | (np.abs(np.abs(diff) - D(thr)) > 0.2)).all()
    out = _case("exact", pos, center, normal, thr, np.signbit(pos).any(axis=1) & (pos == 0).any(axis=1))
    out.update(inlier=np.abs(diff) < D(thr), design=dict(axis=axis, cc=cc, kind=kind, h_axis=h_axis))
    return [out]


SPECIAL_POINTS = np.array([
    [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [1e-45, -1e-45, 1e-40],
    [FLT_MAX, 0.0, 0.0], [-FLT_MAX, FLT_MAX, FLT_MAX], [np.inf, np.inf, np.inf], [np.nan, np.nan, np.nan], [1.2e-38, 1.2e-38, -1.2e-38],
    [0.25, -0.0, 1e-41], [-np.inf, 0.0, np.inf], [0.5, 0.5, FLT_MAX], [5e-39, 0.5, 0.25], [0.5, np.nan, -0.0]], F)


def special(n=N_CAND, h=N_HYP):
    """(a) ordinary points of a unit cube with 64 special ones (out["special"]) at both ends and across the first tile boundary;
    hypotheses of triples of the ordinary points, some replaced: a NaN normal, a zero normal (every finite point votes, an Inf
    point does not: 0 * Inf is NaN), a -0 normal, an Inf centre, a FLT_MAX centre (the sum overflows to Inf - Inf).
    (b) normals of magnitude 1e-20, coordinates of 1e-19, a threshold of 1e-39: every product and the threshold are subnormal."""
    rng = np.random.default_rng(41)
    pos = rng.uniform(0, 1, (n, 3)).astype(F)
    pos[np.arange(n) % 4 == 0, 1] *= F(0.02)
    at = np.unique(np.r_[0:8, PLANE_TILE - 4:PLANE_TILE + 4, n - 48:n] % n)
    spec = np.zeros(n, bool); spec[at] = True
    pos[at] = SPECIAL_POINTS[np.arange(len(at)) % len(SPECIAL_POINTS)]
    ordinary = np.flatnonzero(~spec)
    idx = ordinary[rng.integers(0, len(ordinary), (h, 3))].astype(np.int32)
    center, normal = R.hypotheses(pos, idx)
    swaps = ((0, "nan_normal"), (1, "zero_normal"), (2, "inf_centre"), (3, "max_centre"), (5, "neg_zero_normal"), (64, "zero_normal"), (255, "nan_normal"),
             (256, "zero_normal"))
    for j, what in swaps:
        if j >= h:
            continue
        if what == "nan_normal": normal[j] = (np.nan, 0.5, 0.5)
        if what == "zero_normal": normal[j] = 0.0
        if what == "neg_zero_normal": normal[j] = -0.0
        if what == "inf_centre": center[j] = (np.inf, 0.25, 0.25)
        if what == "max_centre": center[j] = (FLT_MAX, -FLT_MAX, FLT_MAX)
    a = _case("special", pos, center, normal, 0.033, spec)
    a["swaps"] = {what + "@" + str(j): j for j, what in swaps if j < h}
    rng = np.random.default_rng(42)
    normal = (_oblique(rng, h) * 1e-20).astype(F)
    center = np.where(rng.uniform(0, 1, (h, 3)) < 0.5, 0.0, rng.uniform(-1e-19, 1e-19, (h, 3))).astype(F)
    pos = rng.uniform(-3e-19, 3e-19, (n, 3)).astype(F)
    b = _case("special_subnormal", pos, center, normal, 1e-39, np.arange(n) % 3 == 0)
    return [a, b]


VOTE_FAMILIES = dict(band=band, band_3m=band_3m, far=far, exact=exact, special=special)


def vote_cases(n=N_CAND, h=N_HYP):
    return [c for f in VOTE_FAMILIES.values() for c in f(n, h)]


def vote_masks(case):
    n = len(case["pos"])
    return dict(all=np.ones(n, np.uint8), alternating=(np.arange(n) % 2).astype(np.uint8), special=case["special"].copy())


def trimmed(case, n=512, h=64):
    """A subset for the fixture: the first h - 8 and the last 8 hypotheses; the points made for them where the family assigns
    points to hypotheses, otherwise the first n - 64 and the last 64 points."""
    H, N = len(case["center"]), len(case["pos"])
    hyp = np.r_[0:h - 8, H - 8:H]
    pts = np.flatnonzero(np.isin(case["owner"], hyp))[:n] if "owner" in case else np.r_[0:n - 64, N - 64:N]
    out = dict(case)
    for k in ("pos", "mask", "special"):
        out[k] = np.ascontiguousarray(case[k][pts])
    for k in ("center", "normal", "valid"):
        out[k] = np.ascontiguousarray(case[k][hyp])
    return out


# ---- gather and relabel families ---------------------------------------------------------------------------------------------

GATHER_SIZES = (1, 64, 65, 257, 2049)
GATHER_PARAMS = ((0.8, 0.05, False, False), (0.8, 0.033, False, True), (0.0, 0.05, True, True))
CLASSES = np.array([0, 0, 1, 2, 5, -1, INT32_MAX], np.int32)
INSTANCES = np.array([0, 3, 1023, 1024, 1025, INT32_MAX, -1, -1024, INT32_MIN], np.int32)
IDS = (2, 1, 0)                                          # floor_idx, wall_idx, unlabelled_idx


def _axes(a, b, n):
    return np.concatenate([a, b, n], axis=-1)            # column-major: x axis, y axis, normal


def _finish(rng, name, pos, nor, M, order):
    n = len(pos)
    pos, nor = np.ascontiguousarray(pos, F), np.ascontiguousarray(nor, F)
    if order == "reverse":                               # reverse spatial order: the cloud handle reorders points internally
        o = np.lexsort((pos[:, 2], pos[:, 1], pos[:, 0]))[::-1]
        pos, nor = np.ascontiguousarray(pos[o]), np.ascontiguousarray(nor[o])
    M = {k: np.ascontiguousarray(v, np.int8 if k == "valid" else F) for k, v in M.items()}
    return dict(name=name, pos=pos, nor=nor, models=M, cls=rng.choice(CLASSES, n).astype(np.int32), inst=rng.choice(INSTANCES, n).astype(np.int32),
                ids=IDS)


EXACT_NORMALS = np.array([[0.5, 0, 0.5], [-0.5, 0, -0.5], [0, 1, 0], [0, 0, 0], [-0.0, -0.0, -0.0], [1e-38, 0, 0], [0, 0, 1e-38], [1e-45, 0, 0],
                          [0.5, 0, 0.25], [0.25, 0, 0.5], [-0.0, -0.0, 0.0]], F)


def dot_band(n, seed=0, order=None):
    """Points within 4 mm of their model's plane and well inside its quad, so that the normals decide.  Models 0-2: oblique unit
    normals; a point's normal has |nrm . n| within 2 ulp of 0.8f, or (every third) within 1e-8 of 0 for the relabel's > 0.0f.
    Model 3: the normal (0.5, 0, -0.5); its points' normals come from EXACT_NORMALS: a dot of exactly 0 from exact binary
    components, +0 and -0 (three products of -0), a subnormal product, and a product that rounds to 0."""
    rng = np.random.default_rng([51, seed, n])
    normal = np.concatenate([_oblique(rng, 3), [[0.5, 0, -0.5]]]).astype(F)
    a, b = _frame(normal)
    center = rng.uniform(-0.5, 0.5, (4, 3)).astype(F)
    M = dict(center=center, normal=normal, axes=_axes(a, b, _unit(normal.astype(D))), extends=np.tile([2.0, 2.0, -2.0, -2.0], (4, 1)), valid=np.ones(4),
             up_dot=np.array([1.0, 0.0, 0.5, 0.9]))
    k = np.arange(n)
    own = k % 4
    nn = normal[own].astype(D); nsq = (nn * nn).sum(axis=1, keepdims=True)
    pos = center[own].astype(D) + rng.uniform(-1, 1, (n, 1)) * a[own] + rng.uniform(-1, 1, (n, 1)) * b[own] + rng.uniform(-0.004, 0.004, (n, 1)) * nn / nsq
    kind = (k // 4) % 3
    ang = rng.uniform(0, 2 * np.pi, (n, 1))
    t = np.cos(ang) * a[own] + np.sin(ang) * b[own]
    e8 = rng.uniform(-2, 2, (n, 1)) * D(np.spacing(T08))
    near08 = (D(T08) + e8) * nn / nsq + 0.6 * t
    near0 = t + rng.uniform(-1e-8, 1e-8, (n, 1)) * nn / nsq
    nor = np.where((kind == 2)[:, None], near0, near08) * rng.choice([-1.0, 1.0], (n, 1))
    nor = nor.astype(F)
    ex = own == 3
    nor[ex] = EXACT_NORMALS[(k[ex] // 4) % len(EXACT_NORMALS)]
    out = _finish(rng, "dot_band", pos, nor, M, order)
    return out


def _quad_models(rng):
    obl = _oblique(rng, 1).astype(F)
    a, b = _frame(obl)
    ax_obl = _axes(a, b, _unit(obl.astype(D)))[0]
    c_obl = rng.uniform(-0.5, 0.5, 3)
    c_small = rng.uniform(-0.02, 0.02, 3)
    return dict(center=np.array([[1.0, 0, 1.0], c_small, c_obl + 0.01, c_obl, [0, 0.3, 1.0]]),
                normal=np.array([[0, 1, 0], obl[0], obl[0], obl[0], [1, 0, 0]]),
                axes=np.array([[1, 0, 0, 0, 0, 1, 0, 1, 0], ax_obl, ax_obl, ax_obl, [-0.0, 0, 1, -0.0, 1, 0, 1, 0, -0.0]]),
                extends=np.array([[0.75, 0.5, -0.875, -0.625], [0.06, 0.04, -0.07, -0.03], [0, 0, 0, 0], [-0.6, -0.4, 0.7, 0.3], [0.8, 0.25, -0.9, -0.2]]),
                valid=np.ones(5), up_dot=np.array([1.0, 0.0, 0.0, 0.9, 0.0]))


def quad_edges(n, seed=0, order=None):
    """Five quads: 0 axis-aligned, 1 oblique and small, at the origin (coordinates as small as the 3 cm a point may lie off the plane:
    that is where val's rounding decides), 2 degenerate (every extend 0: n1 = 0, val = +-0, nobody is outside), 3 negative
    extends, 4 axes with -0.0 components.  Point k belongs to quad k % 5 and sits, by (k // 5) % 12: on one of the four edges
    (0-3), at one of the four corners (4-7) — each exactly, one ulp inside or one ulp outside, most of them up to 3 cm off the plane
    — or 0.3 m beyond one of the four edges (8-11).  Edge 3, corner 3 to corner 0, is the one the reference never tests: out["place"] and out["owner"] let the tests
    show that points beyond it are kept."""
    rng = np.random.default_rng([52, seed, n])
    M = _quad_models(rng)
    M32 = {k: np.ascontiguousarray(v, F) for k, v in M.items()}
    k = np.arange(n)
    own, place, step = k % 5, (k // 5) % 12, (k // 60) % 3 - 1
    pos = np.zeros((n, 3), D); nor = np.zeros((n, 3), D)
    for i in range(n):
        m = own[i]
        poly = R.quad(M32["center"][m], M32["axes"][m], M32["extends"][m]).astype(D)
        mid = poly.mean(axis=0)
        j = place[i] % 4
        p0, p1 = poly[j], poly[(j + 1) % 4]
        edge = p1 - p0
        length = np.linalg.norm(edge)
        nn = _unit(M32["normal"][m].astype(D)[None])[0]
        if length == 0:                                  # the degenerate quad: around its centre, in its plane
            fa, fb = _frame(nn[None])
            q = p0 + rng.uniform(-0.1, 0.1) * fa[0] + rng.uniform(-0.1, 0.1) * fb[0]
        else:
            outward = np.cross(edge / length, nn)
            if np.dot(outward, p0 - mid) < 0:
                outward = -outward
            q = p0 + (rng.uniform(0.05, 0.95) * edge if place[i] < 4 or place[i] >= 8 else 0.0)
            ulp = D(np.spacing(np.abs(q).max().astype(F)))
            q = q + (0.3 if place[i] >= 8 else step[i] * rng.uniform(1, 2) * ulp) * outward
        if step[i] == 0 or rng.uniform() < 0.5:          # above or below the edge: v1 x v3 lies in the plane and val is all rounding
            q = q + rng.uniform(-0.03, 0.03) * nn
        pos[i] = q
        nor[i] = nn * rng.choice([-1.0, 1.0])
    out = _finish(rng, "quad_edges", pos, nor, M, None)
    out.update(owner=own, place=place)
    if order == "reverse":
        o = np.lexsort((out["pos"][:, 2], out["pos"][:, 1], out["pos"][:, 0]))[::-1]
        for key in ("pos", "nor", "owner", "place"):
            out[key] = np.ascontiguousarray(out[key][o])
    return out


def labels(n, seed=0, order=None):
    """Four models in the plane y = 0.  0: x, z in [0, 2], up_dot exactly 0.8f (not > 0.8f: a wall).  1: the quad of 2, NOT valid,
    up_dot 0 (a wall: applied, it would take the points of 2 that 0 does not hold).  2: [0.5, 2.5]^2, up_dot the float above 0.8f
    (a floor): it overlaps 0, and each field of a point in both is decided by 0.  3: x in [3, 4], up_dot NaN (a wall).  Ids: CLASSES and INSTANCES."""
    rng = np.random.default_rng([53, seed, n])
    floor_axes = [1, 0, 0, 0, 0, 1, 0, 1, 0]
    M = dict(center=np.array([[1.0, 0, 1.0], [1.5, 0.004, 1.5], [1.5, 0.004, 1.5], [3.5, 0, 1.0]]), normal=np.tile([0.0, 1.0, 0.0], (4, 1)),
             axes=np.tile(floor_axes, (4, 1)), extends=np.array([[1, 1, -1, -1], [1, 1, -1, -1], [1, 1, -1, -1], [0.5, 1, -0.5, -1]], D),
             valid=np.array([1, 0, 1, 1]), up_dot=np.array([T08, F(0.0), np.nextafter(T08, F(1)), F(np.nan)], F))
    pos = np.stack([rng.uniform(-0.2, 4.2, n), rng.uniform(-0.06, 0.06, n), rng.uniform(-0.2, 2.7, n)], axis=1)
    nor = np.tile([0.0, 1.0, 0.0], (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
    nor[np.arange(n) % 11 == 10] = (1.0, 0.0, 0.0)
    return _finish(rng, "labels", pos, nor, M, order)


GATHER_FAMILIES = dict(dot_band=dot_band, quad_edges=quad_edges, labels=labels)


def gather_witnesses(case, dot_threshold):
    """{variant: points whose |nrm . n| > dot_threshold decision for their own model differs from plain} over the case's models"""
    out = dict(fma=0, other=0)
    for m in range(len(case["models"]["normal"])):
        v = dot_variants(case["nor"], case["models"]["normal"][m])
        with np.errstate(invalid="ignore"):
            plain = R.absf(v["plain"]) > F(dot_threshold)
            for k in out:
                out[k] += int(((R.absf(v[k]) > F(dot_threshold)) != plain).sum())
    return out


def quad_witnesses(case):
    """points whose val < 0 decision differs between plain and fma at one of the three tested corners, over the case's quads"""
    M, count = case["models"], 0
    for m in range(len(M["center"])):
        v = val_variants(case["pos"], R.quad(M["center"][m], M["axes"][m], M["extends"][m]))
        with np.errstate(invalid="ignore"):
            count += int(((v["plain"] < 0) != (v["fma"] < 0)).any(axis=0).sum())
    return count


# ---- masks and best ----------------------------------------------------------------------------------------------------------

def probe_normals():
    """64 normals for the candidate masks' edges: dot = x * 0 + y * 1 + z * 0, floor where dot > 0.8f, wall where |dot| < 1 - 0.8f"""
    lim = F(1) - T08
    up, dn = lambda x: np.nextafter(F(x), F(np.inf)), lambda x: np.nextafter(F(x), F(-np.inf))
    ys = [T08, up(T08), dn(T08), -T08, lim, up(lim), dn(lim), -lim, up(-lim), dn(-lim), F(0.0), F(-0.0), F(np.nan), F(1e-45), F(-1e-45), F(1.0)]
    rows = [(F(0.6), y, F(0.0)) for y in ys]
    for x, y, z in ((np.inf, 0.9, 0), (0, 0.9, np.nan), (-np.inf, 0.1, 0), (np.nan, 0.0, 0), (0, 0.1, np.inf), (0, -0.9, -np.inf), (np.nan, 0.9, np.nan),
                    (np.inf, 0.0, -np.inf), (FLT_MAX, 0.9, FLT_MAX), (-0.0, 0.1, -0.0), (FLT_MAX, 0.1, -FLT_MAX), (0, np.inf, 0), (0, -np.inf, 0),
                    (1e-45, 0.9, 0), (0, 0.19999999, 0), (0, 0.20000002, 0)):
        rows.append((F(x), F(y), F(z)))
    rows = np.array(rows, F)
    return np.concatenate([rows, rows[::-1]])            # 64


N_BAND, N_BOOST = 192, 160


def _first_wall(pos, wall_mask, idx, dist_threshold):
    c, nn = R.hypotheses(pos, idx)
    with np.errstate(invalid="ignore"):
        valid = (R.absf(R.up_dot(nn)) < (F(1) - T08)).astype(np.uint8)
    counts = R.votes(pos, wall_mask, c, nn, dist_threshold, valid)
    return c, nn, counts, R.best_of(counts)


def room_with_probes(seed=0):
    """A floor slab and two walls (2 900 points, 8 mm thick), N_BAND band points, N_BOOST boosters and 64 probes several metres away
    whose normals are probe_normals().  Band points and boosters carry wall normals.  The triples of a round depend on the
    candidate mask alone, so the round-1 hypotheses are known before those points are placed: with them scattered far away the
    best wall hypothesis is found, the band points go onto its threshold (2.5 - 4 m along the wall) and the boosters into its plane
    10 - 20 m out, where a hypothesis tilted against it loses them, so that it stays the best (checked; otherwise the next
    attempt).  k_plane_remove then decides the band points with the model they were made for.
    Returns dict(pos, nor, band (indices), probes (indices), model (centre, normal of the round-1 best), best, dist_threshold)."""
    thr = F(0.033)
    for attempt in range(16):
        rng = np.random.default_rng([61, seed, attempt])

        def slab(n, origin, eu, ev, normal):
            P = np.asarray(origin, D) + rng.uniform(0, 1, (n, 1)) * np.asarray(eu, D) + rng.uniform(0, 1, (n, 1)) * np.asarray(ev, D)
            P = P + rng.normal(0, 0.004, (n, 1)) * np.asarray(normal, D)
            N = _unit(np.asarray(normal, D) + rng.normal(0, 0.02, (n, 3)))
            return P, N
        parts = [slab(1200, (0, 0, 0), (2, 0, 0), (0, 0, 2), (0, 1, 0)), slab(900, (0, 0, 0), (0, 1.2, 0), (0, 0, 2), (1, 0, 0)),
                 slab(800, (0, 0, 0), (2, 0, 0), (0, 1.2, 0), (0, 0, 1))]
        ang = np.deg2rad(35.0)                            # about +y: the walls stay vertical and become oblique
        rot = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        parts = [(p @ rot.T + [1.5, 0.0, -0.7], q @ rot.T) for p, q in parts]
        k = N_BAND + N_BOOST
        extra_pos = rng.uniform(30, 90, (k, 3)) * [1, 0.2, -1]                   # placeholders, scattered
        extra_nor = _unit(rot @ np.array([1.0, 0, 0]) + rng.normal(0, 0.02, (k, 3)))
        probe_pos = np.stack([6 + 0.11 * np.arange(64), np.full(64, 3.0), 6 + 0.07 * (np.arange(64) % 9)], axis=1)
        P = np.concatenate([p[0] for p in parts] + [extra_pos, probe_pos]); N = np.concatenate([p[1] for p in parts] + [extra_nor, probe_normals().astype(D)])
        n_room = sum(len(p[0]) for p in parts)
        o = rng.permutation(len(P))
        pos, nor = np.ascontiguousarray(P[o], F), np.ascontiguousarray(N.astype(F)[o])
        where = np.empty(len(o), np.int64); where[o] = np.arange(len(o))
        band_at, boost_at, probes_at = where[n_room:n_room + N_BAND], where[n_room + N_BAND:n_room + k], where[n_room + k:]
        wall_mask = R.candidate_masks(nor, T08)[1]
        idx = R.triples(wall_mask, R.WALL_ITERS, 1)
        c, nn, counts, best = _first_wall(pos, wall_mask, idx, thr)
        if best < 0 or np.isin(idx[best], where[n_room:n_room + k]).any():
            continue
        pos[band_at] = _band_points(rng, np.tile(c[best], (N_BAND, 1)), np.tile(nn[best], (N_BAND, 1)), thr, span=0.75, u0=3.25)[0]
        n64 = nn[best].astype(D)
        a, b = _frame(n64[None])
        u = rng.uniform(10, 20, (N_BOOST, 1)) * rng.choice([-1.0, 1.0], (N_BOOST, 1))
        pos[boost_at] = (c[best].astype(D) + u * a + rng.uniform(-0.5, 0.5, (N_BOOST, 1)) * b + rng.uniform(-0.2, 0.2, (N_BOOST, 1)) * D(thr) * n64).astype(F)
        if _first_wall(pos, wall_mask, idx, thr)[3] == best:
            return dict(pos=pos, nor=nor, band=band_at, probes=probes_at, model=(c[best].copy(), nn[best].copy()), best=int(best), dist_threshold=thr)
    raise AssertionError("room_with_probes: the planted wall did not stay the best")


def _plant(rng, idx, wall_ids, t, exclusive):
    """(line, off): wall candidates to put on one vertical plane — `line` collinear, `off` beside the line — so that triple t is the
    first (exclusive: the only) drawn triple that spans the plane: no other drawn triple before t (or at all) has three distinct
    members in line + off that are not all on the line."""
    a, b, c = (int(x) for x in idx[t])
    if len({a, b, c}) < 3:
        return None
    sets = [frozenset(int(x) for x in row) for row in idx]
    others = np.array([w for w in wall_ids if w not in (a, b, c)])
    for trial in range(400):
        extra = [int(x) for x in rng.choice(others, 6, replace=False)]
        line, off = {a, b, *extra[:3]}, {c, *extra[3:]}
        planted = line | off
        if all(not (len(s) == 3 and s <= planted and not s <= line) for k, s in enumerate(sets) if k < t or (exclusive and k > t)):
            return sorted(line), sorted(off)
    return None


def _tie_cloud(name, n_floor, seed, planted):
    """planted None: n_floor floor candidates and ten wall candidates (four on x = 0, four on z = 0, two elsewhere), every
    hypothesis one of a few planes.  planted "late" / "last": 200 wall candidates in a 40 m box (with a handful, 5 000 draws would hold every triple many times),
    nine of them on one vertical plane chosen after the triples are known (see _plant)."""
    for attempt in range(200):
        rng = np.random.default_rng([71, seed, attempt])
        n_wall = 10 if planted is None else 200
        n_fill = 5 + attempt % 7                         # points that are no candidate: they move every candidate's index
        kinds = rng.permutation(np.r_[np.zeros(n_floor), np.ones(n_wall), np.full(n_fill, 2)]).astype(int)
        n = len(kinds)
        nor = np.array([[0, 1, 0], [1, 0, 0], [0.7, 0.5, 0.5]], F)[kinds]
        pos = rng.uniform(-20, 20, (n, 3))
        floor_ids, wall_ids = np.flatnonzero(kinds == 0), np.flatnonzero(kinds == 1)
        pos[floor_ids] = np.stack([rng.uniform(0, 2, n_floor), rng.uniform(-0.002, 0.002, n_floor), rng.uniform(0, 2, n_floor)], axis=1)
        out = dict(name=name, nor=nor, count_threshold=2, first=None)
        if planted is None:
            w = wall_ids
            pos[w[:4], 0] = 0.0; pos[w[:4], 1:] = rng.uniform(0, 2, (4, 2))
            pos[w[4:8], 2] = 0.0; pos[w[4:8], :2] = rng.uniform(0, 2, (4, 2))
            out["pos"] = np.ascontiguousarray(pos, F)
            try:                                         # the reference must be defined on it: no round with fewer than two candidates
                if len(R.detect(out["pos"], nor, T08, F(0.033), 2)["rounds"]) >= 4:
                    return out
            except R.Refused:
                pass
            continue
        wall_mask = R.candidate_masks(nor, T08)[1]
        idx = R.triples(wall_mask, R.WALL_ITERS, 1)
        t = R.WALL_ITERS - 1 if planted == "last" else 256 + attempt
        got = _plant(rng, idx, wall_ids.tolist(), t, planted == "last")
        if got is None:
            continue
        line, off = got
        origin, ang = rng.uniform(-1, 1, 3), rng.uniform(0, np.pi)
        hdir, vdir = np.array([np.cos(ang), 0, np.sin(ang)]), np.array([0, 1.0, 0])
        ldir, mdir = _unit(hdir + 0.5 * vdir), _unit(vdir - 0.5 * hdir)
        for k, i in enumerate(line):
            pos[i] = origin + (k - 2) * 0.7 * ldir
        for k, i in enumerate(off):
            pos[i] = origin + rng.uniform(-1.5, 1.5) * ldir + (0.5 + 0.4 * k) * mdir * rng.choice([-1, 1])
        out["pos"] = np.ascontiguousarray(pos, F)
        c, nn, counts, best = _first_wall(out["pos"], wall_mask, idx, F(0.033))
        top = np.flatnonzero(counts == counts.max())
        if best == t and (planted == "late" or len(top) == 1) and counts.max() >= len(line) + len(off):
            out.update(count_threshold=5, first=dict(index=int(t), tied=top))
            return out
    raise AssertionError(f"tie cloud {name}: no seed gave the property")


TIE_CLOUDS = dict(t3=(3, 0, None), t4=(4, 1, None), t5_late=(5, 2, "late"), t5_last=(5, 3, "last"))


def tie_clouds(names=tuple(TIE_CLOUDS)):
    """t3, t4: three and four floor candidates and a handful of wall candidates: almost every hypothesis is a duplicate, the maximal
    count is shared by indices in every lane and stride.  t5_late: the first maximal wall hypothesis has index >= 256.  t5_last:
    the only maximal wall hypothesis is the last.  out["first"] holds what the construction found for round 1."""
    return [_tie_cloud(k, *TIE_CLOUDS[k]) for k in names]
