"""Seeded addend streams on which a parallel restatement of a sequential fp32 sum is easy to get subtly wrong, and the sequential
reference to hold the ICP estimators' sums to.  A plain helper module like hard_clouds.py: no fixtures, no pytest hooks.

The estimators of rescan_amd/csrc/rs_icp_faithful.hip and rs_icp_chain.hip reproduce the reference's seven centroid chains Σw, Σw·p, Σw·q (icp.h:136-148)
— and the replay also the 33 fp32 + 2 fp64 accumulators of the normal equations — by parallel code that leans on what an fp32
addition does inside one binade.  The cases that decide whether such code is right:

  a tie            an addend exactly half a grid step of the running sum: rounds to even, i.e. by the parity of the sum it meets
  a binade change  the grid doubles or halves under the chain
  a sign change    or a sum of exactly zero: no binade at all
  a tiny sum       below 2^-63 (the lane chains' one-by-one range) or denormal
  a wide range     a value that rises more than 7 binades inside one segment (the replay's records give such a segment up)

Two kinds of input:

  stream(name, n, seed) -> (p1, p2, n2, w)      free arrays for rs_hip_icp_estimate_pt2pl (STREAMS)
  cloud(name, n, seed)  -> (pos, src_nor, tgt_nor)   a cloud that matches ITSELF (CLOUDS): the points lie more than the 0.1 m search
       radius apart (a 0.125 lattice, at most 7 * 2^-10 of jitter: >= 0.111), source and target share the positions
       (target_positions: `shifted` moves the target by (2^-9, 0, -2^-9)), so at the identity pose every source point matches its
       own copy with d² = 0, the 2.5 sigma cut never applies (sd = 0), the weight is the dot of the two normals, the right-hand
       side is zero and the pose never moves: every iteration of icp_align adds exactly the designed addends, in source order.
       A source normal turned round (`gated_*`) fails the normal gate: that point adds nothing.

The reference: seq_sums (np.add.accumulate in float32 is the sequential sum), and tie_count / binade_changes / sign_changes, which
measure each family's defining property (tests/test_hard_sums_cpu.py holds every family to its own).
"""
import numpy as np

F = np.float32
STREAMS = ("dyadic", "pow2_steps", "alternating", "range", "zeros_first", "zeros_middle", "zeros_all_but_first", "zeros_all_but_last",
           "tiny", "offset_1e3", "offset_1e4", "negative")
MOMENT_STREAMS = ("dyadic", "offset_1e3", "offset_1e4", "negative")
CLOUDS = ("dyadic_lattice", "pow2_plane", "straddle", "gated_first", "gated_middle", "gated_all_but_one", "gated_alternate",
          "tiny_axis", "range_plane", "offset_1e3", "shifted")
DYADIC_OFFSET = np.array([64.5, -96.25, 1000.25])
SPACING = 0.125                     # the clouds' lattice: exact in binary, above the 0.1 m search radius
RADIUS = 0.1
SHIFT = np.array([2.0 ** -9, 0.0, -(2.0 ** -9)])
# weights whose products with a coordinate on the 2^-10 grid are exact in fp32, and which move the addend's lowest set bit by 0-3 places
CLOUD_WEIGHTS = (1.0, 0.75, 0.875, 0.625)


# ---- the sequential reference and the measures ---------------------------------------------------------------------------------

def seq(x):
    """The prefix sums of x as the reference forms them: one fp32 addition after the other, from +0."""
    x = np.asarray(x, F)
    if len(x) == 0:
        return np.zeros(0, F)
    with np.errstate(all="ignore"):
        return np.add.accumulate(np.concatenate([np.zeros(1, F), x]), dtype=F)[1:]      # (from +0: 0 + -0 = +0, not x[0] itself)


def seq_sums(p1, p2, w):
    """The seven centroid sums Σw, Σw·p1 (x, y, z), Σw·p2 (x, y, z): fp32 products, sequential fp32 chains (icp.h:136-148, as
    icp_restate.seq_centroids).  float32[7]."""
    w = np.asarray(w, F)
    out = np.zeros(7, F)
    if len(w) == 0:
        return out
    out[0] = seq(w)[-1]
    with np.errstate(all="ignore"):
        for j, P in enumerate((p1, p2)):
            P = np.asarray(P, F)
            for k in range(3):
                out[1 + 3 * j + k] = seq(P[:, k] * w)[-1]
    return out


def addend_rows(p1, p2, w):
    """The seven chains' addends, (7, n) float32, in seq_sums' order."""
    w = np.asarray(w, F); p1 = np.asarray(p1, F); p2 = np.asarray(p2, F)
    with np.errstate(all="ignore"):
        return np.stack([w] + [p1[:, k] * w for k in range(3)] + [p2[:, k] * w for k in range(3)]).astype(F)


def tie_mask(x):
    """True where the addition S + x[i] of the sequential chain is a TIE: the exact sum lies half way between two neighbouring floats
    (decided by the parity of a mantissa).  Exact where fp64 holds S + x exactly (every finite case here but `range`'s 2^30 steps,
    which are no ties: counted as none)."""
    x = np.asarray(x, F)
    S = seq(x)
    prev = np.concatenate([np.zeros(1, F), S[:-1]]).astype(np.float64)
    with np.errstate(all="ignore"):
        e = prev + x.astype(np.float64)
        exact = (e - prev == x.astype(np.float64)) & np.isfinite(e) & np.isfinite(S)
        r = S.astype(np.float64)
        toward = np.where(e > r, np.inf, -np.inf).astype(F)
        nb = np.nextafter(S, toward).astype(np.float64)
        return exact & (e != r) & (e - r == nb - e)


def tie_count(x):
    return int(tie_mask(x).sum())


def _binade(v):
    """The exponent field's role: frexp's exponent for finite non-zero values, a value of its own for zero."""
    v = np.asarray(v, F)
    e = np.frexp(v)[1].astype(np.int64)
    return np.where(v == 0, np.int64(-(1 << 20)), e)


def binade_changes(x):
    """The indices i at which addend i meets a running sum (the sum of addends [0, i)) in another binade than addend i - 1 met; the
    step from the initial zero counts.  With w = 1 throughout, Σw changes binade exactly at every i = 2^k."""
    S = np.concatenate([np.zeros(1, F), seq(x)[:-1]])
    b = _binade(S)
    return np.nonzero(b[1:] != b[:-1])[0] + 1


def sign_changes(x):
    """How often the running sum changes between negative, exactly zero and positive."""
    s = np.sign(seq(x))
    return int((s[1:] != s[:-1]).sum())


def binade_rise_in_segment(x, seg=64):
    """The largest rise of the running sum's exponent inside one segment of `seg` addends: highest exponent reached in the segment
    minus the exponent of the non-zero sum that entered it (zero entering sums, which have no binade, are skipped)."""
    S = seq(x)
    n = len(S)
    best = 0
    for g0 in range(seg, n, seg):
        s_in = S[g0 - 1]
        if s_in == 0 or not np.isfinite(s_in):
            continue
        inside = S[g0:g0 + seg]
        inside = inside[(inside != 0) & np.isfinite(inside)]
        if len(inside):
            best = max(best, int(np.frexp(inside)[1].max() - np.frexp(s_in)[1]))
    return best


# ---- building blocks -----------------------------------------------------------------------------------------------------------

def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def _axis_normals(rng, n):
    nor = np.zeros((n, 3), F)
    nor[np.arange(n), rng.integers(0, 3, n)] = rng.choice(np.array([1.0, -1.0], F), n)
    return nor


def _dyadic_coords(rng, shape):
    """Multiples of 2^-10 in (0, 4) whose LOWEST SET BIT is spread evenly over 2^1 ... 2^-10: as a sum grows through its binades,
    about one addend in twelve sits exactly half a grid step off, whatever the grid has become."""
    j = rng.integers(-1, 11, shape)                                  # lowest set bit 2^-j
    m = 2 * np.floor(rng.random(shape) * np.exp2(j + 1)).astype(np.int64) + 1      # odd, m * 2^-j < 4
    return m * np.exp2(-j.astype(np.float64))


def _rigid_copy(rng, p, noise):
    """p moved by a small rigid motion about its middle plus noise: what a target looks like a step away from convergence."""
    c = p.mean(axis=0)
    a = rng.normal(0, 0.004, 3)
    R = np.array([[1, -a[2], a[1]], [a[2], 1, -a[0]], [-a[1], a[0], 1]])
    return (p - c) @ R.T + c + rng.normal(0, 0.004, 3) + rng.normal(0, noise, p.shape)


def _room_stream(rng, n, offset):
    p = rng.uniform(0, 1, (n, 3)) * np.array([4.0, 3.0, 2.5])
    if offset is None:                                                # `negative`: as hard_clouds — wholly below zero on every axis
        offset = -(np.array([4.0, 3.0, 2.5]) + np.array([0.37, 0.011, 2.5]))
    p1 = p + offset
    p2 = _rigid_copy(rng, p1, 0.002)
    w = rng.uniform(0, 1, n)
    w[rng.random(n) < 0.1] = 0.0
    return p1.astype(F), p2.astype(F), _unit(rng, n), w.astype(F)


def stream(name, n, seed=0):
    """(p1, p2, n2, w) float32 of family `name` with n correspondences."""
    rng = np.random.default_rng([seed, STREAMS.index(name), n])
    i = np.arange(n)
    if name == "dyadic":
        p1 = _dyadic_coords(rng, (n, 3)) + DYADIC_OFFSET
        p2 = p1 + rng.integers(-8, 9, (n, 3)) * 2.0 ** -10           # multiples of 2^-10 within 2^-7
        w = rng.choice(np.array([1.0, 0.75, 0.5, 0.25, 0.0]), n, p=[0.3, 0.25, 0.2, 0.15, 0.1])
        return p1.astype(F), p2.astype(F), _axis_normals(rng, n), w.astype(F)
    if name == "pow2_steps":
        # Σw = i and Σw·x = i enter addend i = 2^k in a new binade: on segment (64, 128), stretch (1 024) and block (4 096) boundaries;
        # Σw·y the same below zero; Σw·z = 0.75 i changes binade between them.  The target's x = 1 + 2^-13 is a tie at EVERY addend
        # while its sum lies in [2^11, 2^12) (grid 2^-12: 2 047 ties in a row), and its sum crosses each power of two a little BEFORE
        # index 2^k.
        p1 = np.tile(np.array([1.0, -1.0, 0.75]), (n, 1))
        p2 = p1 + np.array([2.0 ** -13, 3 * 2.0 ** -13, -(2.0 ** -13)])
        return p1.astype(F), p2.astype(F), _unit(rng, n), np.ones(n, F)
    if name == "alternating":
        x = (-1.0) ** i * (1.0 + (i // 2) * 2.0 ** -12)              # exactly zero after every second addend
        # y hovers across 2^10: 1024.25 + r'_k after every even addend, half a unit lower after every odd one (r' bounded: no drift)
        r, rp = 0.1 * rng.random(n // 2 + 1), rng.uniform(-0.1, 0.1, n // 2 + 2)
        rp[0] = 0.0
        y = np.where(i % 2 == 1, -(0.5 + r[i // 2]), 0.5 + r[np.maximum(i // 2 - 1, 0)] + rp[i // 2] - rp[np.maximum(i // 2 - 1, 0)])
        y[0] = 1024.25
        walk = np.zeros(n + 1)                                       # z: a walk that keeps coming back through zero (S = 0.9 S + noise)
        for k, e in enumerate(rng.normal(0, 1, n)):
            walk[k + 1] = 0.9 * walk[k] + e
        z = np.diff(walk)
        p1 = np.stack([x, y, z], axis=1)
        p2 = p1 + rng.integers(-8, 9, (n, 3)) * 2.0 ** -10
        return p1.astype(F), p2.astype(F), _unit(rng, n), np.ones(n, F)
    if name == "range":
        # addends near 2^-20, absorbed whenever the sum stands at 2^30.  x and y: +-2^30 alternating at 0, 63, 64, 127, 128 (those below
        # n - 1), an open one closed at n - 1 — the sum is 2^30 or exactly zero.  z: the same at 0, 63, 64, 127 only, then +2^30 / -2^30
        # alternating every 97 addends from 200 on: between them the small addends add up from zero to ~2^-13, so a segment entered
        # there rises 43 binades and falls back to exactly zero.
        p1 = 2.0 ** -20 * (1.0 + rng.random((n, 3)))
        for axis, (sgn, at) in enumerate(((1.0, (0, 63, 64, 127, 128)), (-1.0, (0, 63, 64, 127, 128)), (1.0, (0, 63, 64, 127)))):
            ks = [k for k in at if k < n - 1]
            if axis == 2:
                inner = list(range(200, n - 1, 97))
                ks += inner[:len(inner) - len(inner) % 2]
                ks = ks[:len(ks) - len(ks) % 2]
            elif len(ks) % 2:
                ks.append(n - 1)
            for t, k in enumerate(ks):
                p1[k, axis] = sgn * (1.0 if t % 2 == 0 else -1.0) * 2.0 ** 30
        p2 = p1 * (1.0 + 2.0 ** -12)
        return p1.astype(F), p2.astype(F), _unit(rng, n), np.ones(n, F)
    if name.startswith("zeros_"):
        p1, p2, n2, w = stream("dyadic", n, seed + 1)
        keep = {"zeros_first": i >= 640, "zeros_middle": (i < n // 3) | (i >= 2 * n // 3), "zeros_all_but_first": i == 0,
                "zeros_all_but_last": i == n - 1}[name]
        w = np.where(keep, np.maximum(w, F(0.25)), F(0.0)).astype(F)
        neg = rng.random(n) < 0.25                                   # some of the zero weights are -0.0, and some coordinates
        w[~keep & neg] = F(-0.0)
        p1 = p1.copy(); p1[rng.random(n) < 0.05, 1] = F(-0.0)
        return p1, p2, n2, w
    if name == "tiny":
        # x: multiples of 2^-75 whose sum stays below 2^-63; y: multiples of 2^-140 — denormal addends, a denormal sum; z: ordinary
        kx = rng.integers(0, 4, n) * (rng.random(n) < min(1.0, 1500.0 / max(n, 1)))
        ky = rng.integers(1, 4, n) * (rng.random(n) < min(1.0, 3000.0 / max(n, 1)))      # Σ k w < 2^14: the sum stays denormal
        ky[0] = 1
        p1 = np.stack([kx * 2.0 ** -75, ky * 2.0 ** -140, rng.uniform(0, 1, n)], axis=1)
        p2 = p1 * np.array([1.5, 1.5, 1.0]) + np.array([0, 0, 2.0 ** -9])
        w = rng.choice(np.array([1.0, 0.5]), n)
        return p1.astype(F), p2.astype(F), _unit(rng, n), w.astype(F)
    if name == "offset_1e3":
        return _room_stream(rng, n, np.array([1000.3, -1000.7, -500.1]))
    if name == "offset_1e4":
        return _room_stream(rng, n, np.array([10000.3, -10000.7, -5000.1]))
    if name == "negative":
        return _room_stream(rng, n, None)
    raise KeyError(name)


def nonfinite_stream(kind, n, seed=0):
    """`dyadic` with one NaN coordinate at index 130 (kind "nan"), or with two 3e38 addends of one sign in the x chain (kind "inf":
    the chain overflows to +inf and stays there)."""
    p1, p2, n2, w = stream("dyadic", n, seed)
    p1 = p1.copy(); w = w.copy()
    if kind == "nan":
        p1[130, 1] = np.nan; w[130] = F(1.0)
    elif kind == "inf":
        p1[40, 0] = F(3e38); p1[200, 0] = F(3e38); w[40] = w[200] = F(1.0)
    else:
        raise KeyError(kind)
    return p1, p2, n2, w


# ---- self-matching clouds --------------------------------------------------------------------------------------------------------

def _lattice3(n):
    s = 1
    while s ** 3 < n:
        s += 1
    return np.stack(np.meshgrid(np.arange(s), np.arange(s), np.arange(s), indexing="ij"), -1).reshape(-1, 3)


def _lattice2(n):
    s = 1
    while s * s < n:
        s += 1
    return np.stack(np.meshgrid(np.arange(s), np.arange(s), indexing="ij"), -1).reshape(-1, 2)


def _dyadic_jitter(rng, shape):
    """Multiples of 2^-10 within +-7 * 2^-10; half of them zero, so that the lattice's own coarser bits (2^-3 and up) are the lowest
    set bit of every second coordinate: ties on every grid from 2^-13 to 2^1."""
    k = rng.integers(-7, 8, shape) * (rng.random(shape) < 0.5)
    return k * 2.0 ** -10


def _weighted_normals(rng, n):
    """Source normals +z; target normals (sqrt(1 - c²), 0, c) with c from CLOUD_WEIGHTS: the dot, c exactly, is the weight."""
    c = rng.choice(np.array(CLOUD_WEIGHTS), n)
    src = np.tile(np.array([0.0, 0.0, 1.0], F), (n, 1))
    tgt = np.stack([np.sqrt(1.0 - c * c), np.zeros(n), c], axis=1).astype(F)
    return src, tgt


def gated_mask(name, n):
    """The points of a `gated_*` cloud whose source normal is turned round (they fail the normal gate and add nothing)."""
    i = np.arange(n)
    if name == "gated_first":
        return i < 5 * 64
    if name == "gated_middle":
        return (i >= n // 3) & (i < 2 * n // 3)
    if name == "gated_all_but_one":
        return i != min(n - 1, 70)
    if name == "gated_alternate":
        return (i // 64) % 2 == 0
    return np.zeros(n, bool)


def cloud(name, n, seed=0):
    """(pos, src_nor, tgt_nor) float32 of family `name` with n points; the target's positions are target_positions(name, pos)."""
    rng = np.random.default_rng([seed, 100 + CLOUDS.index(name), n])
    if name in ("dyadic_lattice", "shifted", "offset_1e3") or name.startswith("gated_"):
        g = _lattice3(n)
        g = g[rng.permutation(len(g))[:n]]
        if name == "offset_1e3":
            pos = g * SPACING + rng.uniform(-0.0068, 0.0068, (n, 3)) + np.array([1000.3, -1000.7, -500.1])
        else:
            pos = g * SPACING + _dyadic_jitter(rng, (n, 3)) + DYADIC_OFFSET
        src, tgt = _weighted_normals(rng, n)
        src[gated_mask(name, n)] *= F(-1.0)
        return pos.astype(F), src, tgt
    if name == "pow2_plane":
        g = _lattice2(n)
        g = g[rng.permutation(len(g))[:n]]
        pos = np.concatenate([np.ones((n, 1)), g * SPACING + _dyadic_jitter(rng, (n, 2)) + DYADIC_OFFSET[1:]], axis=1)
        nor = np.tile(np.array([1.0, 0.0, 0.0], F), (n, 1))             # w = 1: Σw and Σw·x enter addend 2^k in a new binade
        return pos.astype(F), nor, nor.copy()
    if name == "straddle":
        # half a lattice of cell centres around the origin and its mirror image, ordered p, -p, p', -p', ...: all three coordinate sums
        # are exactly zero after every second addend
        m = (n + 1) // 2
        s = 2
        while s ** 3 < 2 * m:
            s += 2                                                       # an even side: no coordinate of a cell centre is zero
        g = np.stack(np.meshgrid(np.arange(s), np.arange(s), np.arange(s), indexing="ij"), -1).reshape(-1, 3)
        c = (g - (s - 1) / 2.0) * SPACING                                # symmetric about the origin
        first = c[:, 0] + 1e-3 * c[:, 1] + 1e-6 * c[:, 2] > 0            # one of every pair {p, -p}
        h = c[first]
        h = h[rng.permutation(len(h))[:m]]
        h = h + _dyadic_jitter(rng, h.shape)
        pos = np.empty((2 * m, 3)); pos[0::2] = h; pos[1::2] = -h
        pos = pos[:n]
        nor = np.tile(np.array([0.0, 0.0, 1.0], F), (n, 1))
        return pos.astype(F), nor, nor.copy()
    if name == "tiny_axis":
        g = _lattice2(n)
        g = g[rng.permutation(len(g))[:n]]
        k = rng.integers(1, 4, n) * (rng.random(n) < min(1.0, 1500.0 / n))      # Σ k stays below 2^12: the sum below 2^-63
        pos = np.concatenate([g * SPACING + _dyadic_jitter(rng, (n, 2)) + DYADIC_OFFSET[:2], (k * 2.0 ** -75)[:, None]], axis=1)
        src, tgt = _weighted_normals(rng, n)
        return pos.astype(F), src, tgt
    if name == "range_plane":
        g = _lattice2(n)
        g = g[rng.permutation(len(g))[:n]]
        x = rng.integers(1, 1 << 10, n) * 2.0 ** -30
        x[60::61] = 30.0
        pos = np.concatenate([x[:, None], g * SPACING + _dyadic_jitter(rng, (n, 2)) + np.array([-3.0, 0.25])], axis=1)
        src, tgt = _weighted_normals(rng, n)
        return pos.astype(F), src, tgt
    raise KeyError(name)


def target_positions(name, pos):
    return (pos.astype(np.float64) + SHIFT).astype(F) if name == "shifted" else pos


def cloud_max_iter(name):
    return 1 if name == "shifted" else 3


def expected_corrs(name, pos, src_nor, tgt_nor, max_dist=RADIUS):
    """What the search must find at the identity pose, from the design alone: (p1, p2, w_uncut, d2) — the points whose normals pass
    the gate, in source order; d² = |shift|² in the reference's expression order; w = (1 - d² / max_dist) * dot (icp.h:387)."""
    keep = np.einsum("ij,ij->i", src_nor, tgt_nor) > 0
    p1 = pos[keep]; p2 = target_positions(name, pos)[keep]
    v = p2 - p1
    d2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).astype(F)
    a, b = src_nor[keep], tgt_nor[keep]
    dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]).astype(F)
    w = ((F(1.0) - d2 / F(max_dist)) * dot).astype(F)
    return p1, p2, w, d2


def min_distance(pos, cell=0.11):
    """The smallest distance between two points of the cloud (fp64): every point against the points of its own and the 26 neighbouring
    cells of a hash grid (a pair nearer than `cell` shares a cell or sits in adjacent ones; inf if there is none)."""
    p = np.asarray(pos, np.float64)
    n = len(p)
    c = np.floor((p - p.min(axis=0)) / cell).astype(np.int64) + 1
    dims = c.max(axis=0) + 2
    key = (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
    order = np.argsort(key, kind="stable")
    ks, ps = key[order], p[order]
    best = np.inf
    me = np.empty(n, np.int64); me[order] = np.arange(n)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                nk = ((c[:, 0] + dx) * dims[1] + c[:, 1] + dy) * dims[2] + c[:, 2] + dz
                lo, hi = np.searchsorted(ks, nk, "left"), np.searchsorted(ks, nk, "right")
                for t in range(int((hi - lo).max()) if n else 0):
                    j = lo + t
                    ok = (j < hi) & (j != me)
                    if ok.any():
                        best = min(best, float(np.linalg.norm(p[ok] - ps[j[ok]], axis=1).min()))
    return best


# ---- perturbed references: what a subtly wrong implementation would give ----------------------------------------------------------

def pairwise_sum(x):
    """The same addends summed as a balanced tree in fp32: another association."""
    x = np.asarray(x, F).copy()
    with np.errstate(all="ignore"):
        while len(x) > 1:
            if len(x) % 2:
                x = np.concatenate([x, np.zeros(1, F)])
            x = (x[0::2] + x[1::2]).astype(F)
    return x[0] if len(x) else F(0)


def seq_half_away(x):
    """The sequential chain with ties rounded AWAY from zero instead of to even: parts from seq at the first tie whose even neighbour is
    the one nearer to zero."""
    x = np.asarray(x, F)
    s = np.float64(0.0)
    for v in x.astype(np.float64):
        e = s + v                                                       # exact for the streams this is used on
        r = np.float64(F(e))
        if r != e:
            nb = np.float64(np.nextafter(F(r), F(np.inf) if e > r else F(-np.inf)))
            if e - r == nb - e and abs(nb) > abs(r):
                r = nb
        s = r
    return F(s)


# ---- the comparisons the device tests make (tests/test_hard_sums_cpu.py shows that each can fail) ------------------------------------

def totals_words(sums):
    """The seven sums as RS_HIP_DEBUG_TOTALS prints them: eight hex digits each."""
    return ["%08x" % int(u) for u in np.asarray(sums, F).view(np.uint32)]


def parse_totals(stderr):
    """{problem: [seven hex words]} of the LAST `[rs_hip totals]` line per problem in a child's stderr (a call the grid chains gave up
    prints once for the attempt and once for the run that replaced it)."""
    out = {}
    for line in stderr.splitlines():
        if line.startswith("[rs_hip totals]"):
            head, words = line.split(":", 1)
            out[int(head.split()[-1])] = words.split()
    return out


def bits_or_class_differ(got, want):
    """Indices where `got` is not `want`: a finite entry of `want` must be matched bit for bit, a NaN by a NaN, an infinity by the
    infinity of the same sign."""
    got = np.atleast_1d(np.asarray(got, F)).ravel(); want = np.atleast_1d(np.asarray(want, F)).ravel()
    same = np.where(np.isnan(want), np.isnan(got), np.where(np.isinf(want), got == want, got.view(np.uint32) == want.view(np.uint32)))
    return np.nonzero(~same)[0]
