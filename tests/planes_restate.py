"""fp32 NumPy restatement of the plane detector, the inlier gather and the wall / floor relabel (lib/rs/rs_pointcloud_filters.cpp:
96-323, 617-671; the sampler of lib/msh/msh_std.h:1863-1941).  NumPy does not contract a * b + c, so every product and sum rounds
as the reference's scalar code does.  tests/test_planes_cpu.py pins it to the reference's recordings (tests/golden/planes_*.npz); the
GPU tests use it for shapes that no recording covers."""
import numpy as np

from resample_restate import M64, PCG_MUL, Refused, pcg_seed, same_bits  # noqa: F401

F = np.float32
E_ARG, E_CAPACITY = -2, -4
MAX_POINTS = 1 << 24
SEED = 12346
FLOOR_ITERS, WALL_ITERS = 2500, 5000


def absf(x):                                             # msh_abs: x < 0 ? -x : x
    x = np.asarray(x, F)
    return np.where(x < 0, -x, x)


def up_dot(v):                                           # msh_vec3_dot( v, posy ): the zero products stay
    v = np.asarray(v, F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return v[:, 0] * F(0) + v[:, 1] * F(1) + v[:, 2] * F(0)


def candidate_masks(nor, dot_threshold):
    """(floor, wall) uint8 masks (:141-146, :209-214)."""
    d = up_dot(nor)
    with np.errstate(invalid="ignore"):
        return (d > F(dot_threshold)).astype(np.uint8), (absf(d) < (F(1) - F(dot_threshold))).astype(np.uint8)


class Sampler:
    """msh_discrete_distribution_init over weights 1.0 / 0.0, and _sample."""

    def __init__(self, active, seed=SEED):
        active = np.asarray(active).astype(bool)
        n = len(active)
        if n > MAX_POINTS:
            raise Refused(E_CAPACITY, "more than 2^24 points")
        total = float(active.sum())                      # a sequential double sum of ones and zeros is exact
        norm = float(F(total))
        if norm <= 0.00000001:
            raise Refused(E_ARG, "no candidate")
        inv = 1.0 / norm
        pdf = [(1.0 if a else 0.0) * inv for a in active]
        avg = 1.0 / n
        self.prob, self.alias = [0.0] * n, list(range(n))
        small = [i for i in range(n) if not pdf[i] >= avg]
        large = [i for i in range(n) if pdf[i] >= avg]
        while small and large:                           # msh_std.h:1884-1897
            l, g = small.pop(), large.pop()
            self.prob[l] = pdf[l] * n
            self.alias[l] = g
            pdf[g] = (pdf[g] + pdf[l]) - avg
            (large if pdf[g] >= avg else small).append(g)
        for i in small + large:
            self.prob[i] = 1.0
        self.n, self.n_active = n, int(total)
        self.state, self.inc = pcg_seed(seed)

    def _nextf(self):
        s = self.state
        self.state = (s * PCG_MUL + self.inc) & M64
        xs = (((s >> 18) ^ s) >> 27) & 0xffffffff
        rot = s >> 59
        u = ((xs >> rot) | (xs << ((-rot) & 31))) & 0xffffffff
        return np.array([(u >> 9) | 0x3F800000], np.uint32).view(F)[0] - F(1.0)

    def sample(self):
        column = int(self._nextf() * F(self.n))          # msh_rand_range: an fp32 product, truncated
        coin = float(self._nextf()) < self.prob[column]
        return column if coin else self.alias[column]


def triples(active, n_iter, distinct, seed=SEED):
    s = Sampler(active, seed)
    if distinct and s.n_active < 2:
        raise Refused(E_ARG, "fewer than 2 wall candidates")
    idx = np.zeros((n_iter, 3), np.int32)
    for h in range(n_iter):
        a = s.sample()
        if distinct:
            b = s.sample()
            while b == a:
                b = s.sample()
            c = s.sample()
            while c == b:
                c = s.sample()
        else:
            b, c = s.sample(), s.sample()
        idx[h] = (a, b, c)
    return idx


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def hypotheses(pos, idx):
    """(center, normal) of the triples: p_a and normalize( cross( p_b - p_a, p_c - p_a ) ), NaN for a degenerate triple."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    a, b, c = pos[idx[:, 0]], pos[idx[:, 1]], pos[idx[:, 2]]
    with np.errstate(all="ignore"):
        v = cross(b - a, c - a)
        denom = F(1.0) / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        return a.copy(), v * denom[:, None]


def offsets(pos, center, normal):
    """n.x * (p.x - c.x) + n.y * (p.y - c.y) + n.z * (p.z - c.z) for one plane and every point"""
    with np.errstate(all="ignore"):
        return (normal[0] * (pos[:, 0] - center[0]) + normal[1] * (pos[:, 1] - center[1])) + normal[2] * (pos[:, 2] - center[2])


def votes(pos, active, center, normal, dist_threshold, valid=None):
    """evaluate_plane_model for every hypothesis; 0 where valid[h] == 0."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)[np.asarray(active).astype(bool)]
    center, normal = np.asarray(center, F).reshape(-1, 3), np.asarray(normal, F).reshape(-1, 3)
    out = np.zeros(len(center), np.int32)
    chunk = max(1, 2000000 // max(len(pos), 1))
    with np.errstate(all="ignore"):
        for h0 in range(0, len(center), chunk):
            c, nn = center[h0:h0 + chunk, None, :], normal[h0:h0 + chunk, None, :]
            d = (nn[..., 0] * (pos[None, :, 0] - c[..., 0]) + nn[..., 1] * (pos[None, :, 1] - c[..., 1])) + nn[..., 2] * (pos[None, :, 2] - c[..., 2])
            out[h0:h0 + chunk] = (absf(d) < F(dist_threshold)).sum(axis=1)
    if valid is not None:
        out[np.asarray(valid) == 0] = 0
    return out


def best_of(counts):
    """The lowest index among the maximal counts, -1 if that count is 0."""
    return int(np.argmax(counts)) if len(counts) and counts.max() > 0 else -1


def remove(pos, mask, center, normal, dist_threshold):
    with np.errstate(invalid="ignore"):
        hit = absf(offsets(np.ascontiguousarray(pos, F).reshape(-1, 3), center, normal)) < F(dist_threshold)
    return (mask.astype(bool) & ~hit).astype(np.uint8)


def detect(pos, nor, dot_threshold=0.8, dist_threshold=0.033, count_threshold=250, floor_iters=FLOOR_ITERS, wall_iters=WALL_ITERS):
    """rspf__detect_floor then rspf__detect_walls: dict(centers, normals, n_inliers, n_floors, n_walls, rounds), rounds[r] =
    dict(idx, center, normal, valid, counts (0 where not valid), best, mask_before, mask_after)."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    floor_mask, wall_mask = candidate_masks(nor, dot_threshold)
    limit = F(1) - F(dot_threshold)

    def one_round(mask, n_iter, distinct):
        idx = triples(mask, n_iter, distinct)
        c, nn = hypotheses(pos, idx)
        with np.errstate(invalid="ignore"):
            valid = (absf(up_dot(nn)) < limit).astype(np.uint8) if distinct else np.ones(n_iter, np.uint8)
        counts = votes(pos, mask, c, nn, dist_threshold, valid)
        return dict(idx=idx, center=c, normal=nn, valid=valid, counts=counts, best=best_of(counts), mask_before=mask.copy())

    rounds, models = [], []
    r = one_round(floor_mask, floor_iters, 0)
    r["mask_after"] = floor_mask.copy()
    rounds.append(r)
    n_floors = 0
    if r["best"] >= 0:
        models.append((r["center"][r["best"]], r["normal"][r["best"]], int(r["counts"][r["best"]]))); n_floors = 1
    mask = wall_mask
    best = (np.zeros(3, F), np.zeros(3, F), 0)
    n_walls = 0
    while True:
        r = one_round(mask, wall_iters, 1)
        best = (best[0], best[1], 0)
        if r["best"] >= 0:
            best = (r["center"][r["best"]], r["normal"][r["best"]], int(r["counts"][r["best"]]))
            models.append(best)
        mask = remove(pos, mask, best[0], best[1], dist_threshold)        # the stale model where nothing was detected
        r["mask_after"] = mask.copy()
        rounds.append(r)
        n_walls += 1
        if not best[2] > count_threshold:
            break
    if not models:
        raise Refused(E_ARG, "the reference would pop an empty model array")
    models.pop(); n_walls -= 1
    m = len(models)
    return dict(centers=np.array([x[0] for x in models], F).reshape(m, 3), normals=np.array([x[1] for x in models], F).reshape(m, 3),
                n_inliers=np.array([x[2] for x in models], np.int64), n_floors=n_floors, n_walls=n_walls, rounds=rounds)


def quad(center, axes, extends):
    """The four corners of :288-296; axes (9,) column-major."""
    center, axes, extends = np.asarray(center, F), np.asarray(axes, F), np.asarray(extends, F)
    px, py, nx, ny = axes[0:3] * extends[0], axes[3:6] * extends[1], axes[0:3] * extends[2], axes[3:6] * extends[3]
    return np.stack([(center + px) + py, (center + px) + ny, (center + nx) + ny, (center + nx) + py])


def within(pos, poly):
    """rspf__is_point_within_convex_poly as written: three of the four corners"""
    ok = np.ones(len(pos), bool)
    with np.errstate(all="ignore"):
        for i in range(3):
            a, b, c = poly[i], poly[i + 1], poly[(i + 2) % 4]
            v1, v2 = (b - a)[None, :], (c - b)[None, :]
            v3 = pos - b[None, :]
            n1, n2 = cross(v1, v2), cross(np.broadcast_to(v1, v3.shape), v3)
            val = (n1[:, 0] * n2[:, 0] + n1[:, 1] * n2[:, 1]) + n1[:, 2] * n2[:, 2]
            ok &= ~(val < 0)
    return ok


def inlier_flags(pos, nor, center, normal, axes, extends, dot_threshold, dist_threshold, check_extends):
    pos, nor = np.ascontiguousarray(pos, F).reshape(-1, 3), np.ascontiguousarray(nor, F).reshape(-1, 3)
    center, normal = np.asarray(center, F), np.asarray(normal, F)
    with np.errstate(all="ignore"):
        dist = absf(offsets(pos, center, normal))
        dot = absf((nor[:, 0] * normal[0] + nor[:, 1] * normal[1]) + nor[:, 2] * normal[2])
        ok = (dot > F(dot_threshold)) & (dist < F(dist_threshold))
    if check_extends:
        ok &= within(pos, quad(center, axes, extends))
    return ok


def gather(pos, nor, centers, normals, axes=None, extends=None, valid=None, dot_threshold=0.8, dist_threshold=0.05, check_validity=False,
           check_extends=False):
    """rspf__gather_model_inliers: one increasing int32 index array per model (empty for a skipped one)."""
    out = []
    for m in range(len(centers)):
        if check_validity and not valid[m]:
            out.append(np.zeros(0, np.int32)); continue
        ok = inlier_flags(pos, nor, centers[m], normals[m], None if axes is None else axes[m], None if extends is None else extends[m],
                          dot_threshold, dist_threshold, check_extends)
        out.append(np.flatnonzero(ok).astype(np.int32))
    return out


def relabel(pos, nor, centers, normals, axes, extends, valid, normal_up_dot, floor_idx, wall_idx, unlabelled_idx, class_ids, instance_ids):
    """rspf_relabel_walls_and_floors: the rewritten (class_ids, instance_ids)."""
    cls, inst = np.array(class_ids, np.int32), np.array(instance_ids, np.int32)
    lists = gather(pos, nor, centers, normals, axes, extends, valid, 0.0, 0.05, True, True)
    for m, index in enumerate(lists):
        if not valid[m]:
            continue
        is_floor = F(normal_up_dot[m]) > F(0.8)
        i = index[inst[index] >= 1024]; inst[i] = 0 if is_floor else 1
        i = index[cls[index] == unlabelled_idx]; cls[i] = floor_idx if is_floor else wall_idx
    return cls, inst
