"""A vectorised NumPy restatement of rs_pointcloud_uniform_resample (lib/rs/rs_pointcloud.h:1132-1227): every sample computed on
its own from the two PCG32 states 2 i steps after the seeding (msh_std.h:1413-1470), uint64 arrays with wrap-around.

Not the product's code and not the reference's: a third statement of the same semantics, checked bit for bit against the
reference's recorded output (tests/test_resample_cpu.py) and then used where no recording exists (small counts, hostile meshes,
windows near 2^31)."""
import numpy as np

F = np.float32
D = np.float64
U64 = np.uint64
M64 = (1 << 64) - 1
PCG_MUL = 0x5851f42d4c957f2d
SEED_BARYCENTRIC, SEED_ALIAS = 12346, 64321           # rs_pointcloud.h:1135
MAX_FACES = 1 << 24
INT32_MAX = (1 << 31) - 1


# ---- PCG32 -------------------------------------------------------------------------------------------------------------------

def _murmur(h):                                          # msh_std.h:1423-1432
    h ^= h >> 33; h = (h * 0xff51afd7ed558ccd) & M64
    h ^= h >> 33; h = (h * 0xc4ceb9fe1a85ec53) & M64
    h ^= h >> 33
    return h


def pcg_seed(seed):
    """(state, increment) after msh_rand_init (msh_std.h:1434-1444), as Python ints."""
    value = _murmur((((seed & 0xffffffff) << 1) | 1) & M64)
    inc = ((value << 1) | 1) & M64
    state = (0 * PCG_MUL + inc) & M64
    state = (state + _murmur(value)) & M64
    state = (state * PCG_MUL + inc) & M64
    return state, inc


def advance(state, inc, steps):
    """The states `steps` (uint64 array) steps after `state`: s -> A^n s + c (A^n - 1) / (A - 1), by squaring over the bits of n."""
    steps = np.asarray(steps, U64)
    s = np.full(steps.shape, state, U64)
    mul, add = PCG_MUL, inc
    for k in range(64):
        if not (steps >> U64(k)).any():
            break
        bit = ((steps >> U64(k)) & U64(1)).astype(bool)
        s = np.where(bit, s * U64(mul) + U64(add), s)
        add = (add * (mul + 1)) & M64
        mul = (mul * mul) & M64
    return s


def pcg_draw(s, inc):
    """(output uint32 array, next states) of msh_rand_next (msh_std.h:1447-1455)."""
    nxt = s * U64(PCG_MUL) + U64(inc)
    xs = (((s >> U64(18)) ^ s) >> U64(27)).astype(np.uint32)
    rot = (s >> U64(59)).astype(np.uint32)
    out = (xs >> rot) | (xs << ((np.uint32(0) - rot) & np.uint32(31)))
    return out, nxt


def unit_float(u):                                       # msh_std.h:1412-1421
    return ((u >> np.uint32(9)) | np.uint32(0x3F800000)).view(F) - F(1.0)


# ---- the plan ----------------------------------------------------------------------------------------------------------------

class Refused(Exception):
    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


E_ARG, E_CAPACITY = -2, -4


def face_areas(pos, faces):
    """Twice the triangle areas, as :1143-1154 has them: fp32 cross product, (float)sqrt of the fp32 sum, widened to double."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3); faces = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = pos[faces[:, 0]], pos[faces[:, 1]], pos[faces[:, 2]]
    with np.errstate(invalid="ignore", over="ignore"):          # (non-finite meshes are refused by plan, from the sum)
        v1, v2 = b - a, c - a
        x = v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1]
        y = v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2]
        z = v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]
        sq = x * x + y * y + z * z
        return np.sqrt(sq.astype(D)).astype(F).astype(D)


def plan(pos, faces):
    """(n_samples, total_area, prob, alias).  An alias entry the reference never writes holds its own index."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3); faces = np.asarray(faces).reshape(-1, 3)
    n = len(faces)
    if n <= 0:
        raise Refused(E_ARG, "no faces")
    if n > MAX_FACES:
        raise Refused(E_CAPACITY, "more than 2^24 faces")
    faces = faces.astype(np.int64)
    if (faces < 0).any() or (faces >= len(pos)).any():
        raise Refused(E_ARG, "vertex index out of range")
    areas = face_areas(pos, faces)
    with np.errstate(over="ignore", invalid="ignore"):
        total = np.cumsum(areas)[-1]                      # sequential, in face order (np.sum is pairwise)
    if not np.isfinite(total):
        raise Refused(E_ARG, "total area not finite")
    norm = D(F(total))                                   # msh_accumulated returns float (msh_std.h:1788-1797,1845)
    if norm <= 0.00000001:
        raise Refused(E_ARG, "area sum at or below 1e-8")
    want = D(0.5) * total * D(12800.0)
    if want >= 2147483648.0:
        raise Refused(E_CAPACITY, "more than INT32_MAX samples")
    n_samples = int(want)
    inv = D(1.0) / norm
    pdf = [float(x) for x in areas * inv]
    avg = 1.0 / n
    prob, alias = np.zeros(n, D), np.arange(n, dtype=np.int32)
    small = [i for i in range(n) if not pdf[i] >= avg]
    large = [i for i in range(n) if pdf[i] >= avg]
    while small and large:                               # msh_std.h:1884-1897
        l, g = small.pop(), large.pop()
        prob[l] = pdf[l] * n
        alias[l] = g
        pdf[g] = (pdf[g] + pdf[l]) - avg
        (large if pdf[g] >= avg else small).append(g)
    for i in small + large:
        prob[i] = 1.0
    return n_samples, float(total), prob, alias


# ---- the samples -------------------------------------------------------------------------------------------------------------

def weights(first, count):
    """The barycentric weights (w0, w1, w2) of samples first .. first + count - 1 (:1114-1130): they depend on the index alone."""
    i = np.arange(first, first + count, dtype=U64)
    st, inc = pcg_seed(SEED_BARYCENTRIC)
    s = advance(st, inc, U64(2) * i)
    u1, s = pcg_draw(s, inc)
    u2, s = pcg_draw(s, inc)
    a, b = unit_float(u1).astype(D), unit_float(u2).astype(D)
    flip = a + b > 1.0
    a = np.where(flip, 1.0 - a, a); b = np.where(flip, 1.0 - b, b)
    q = 1.0 - a - b
    return q.astype(F), a.astype(F), b.astype(F), flip


def sampled_faces(first, count, n_faces, prob, alias):
    i = np.arange(first, first + count, dtype=U64)
    st, inc = pcg_seed(SEED_ALIAS)
    s = advance(st, inc, U64(2) * i)
    u1, s = pcg_draw(s, inc)
    u2, s = pcg_draw(s, inc)
    column = (unit_float(u1) * F(n_faces)).astype(np.int32)      # msh_rand_range's fp32 product (msh_std.h:1468)
    return np.where(unit_float(u2).astype(D) < prob[column], column, alias[column]).astype(np.int32)


def _mix(v, f, w0, w1, w2):
    return (v[f[:, 0]] * w0 + v[f[:, 1]] * w1) + v[f[:, 2]] * w2


def resample(mesh, first=0, count=None, the_plan=None):
    """mesh: dict with pos, faces and any of nor, col, radii, cls, inst.  Returns the window's arrays (and face, n_samples,
    flipped: the draws with s + t > 1, tie: samples whose two smallest weights are equal)."""
    pos = np.ascontiguousarray(mesh["pos"], F).reshape(-1, 3); faces = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    n_samples, total, prob, alias = the_plan if the_plan is not None else plan(pos, faces)
    if count is None:
        count = n_samples - first
    assert 0 <= first and 0 <= count and first + count <= n_samples
    w0, w1, w2, flip = weights(first, count)
    face = sampled_faces(first, count, len(faces), prob, alias)
    f = faces[face]
    W0, W1, W2 = w0[:, None], w1[:, None], w2[:, None]
    out = dict(n_samples=n_samples, total_area=total, face=face, flipped=flip)
    out["pos"] = _mix(pos, f, W0, W1, W2)
    if mesh.get("nor") is not None:
        v = _mix(np.ascontiguousarray(mesh["nor"], F).reshape(-1, 3), f, W0, W1, W2)
        with np.errstate(divide="ignore", invalid="ignore"):
            denom = F(1.0) / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])     # msh_vec_math.h:868
            out["nor"] = v * denom[:, None]
    if mesh.get("col") is not None:
        out["col"] = _mix(np.ascontiguousarray(mesh["col"], F).reshape(-1, 3), f, W0, W1, W2)
    if mesh.get("radii") is not None:
        r = np.ascontiguousarray(mesh["radii"], F)
        out["radii"] = (((r[f[:, 0]] * w0).astype(D) + (r[f[:, 1]] * w1).astype(D)) + (r[f[:, 2]] * w2).astype(D)).astype(F)   # :1195-1198
    m = np.minimum(np.minimum(w0, w1), w2)
    pick = np.where(w0 == m, 0, np.where(w1 == m, 1, 2))                                                  # :1200-1222
    out["tie"] = ((w0 == m).astype(int) + (w1 == m) + (w2 == m)) >= 2
    out["pick"] = pick
    for key in ("cls", "inst"):
        if mesh.get(key) is not None:
            out[key] = np.ascontiguousarray(mesh[key], np.int32)[f[np.arange(count), pick]]
    return out


def same_bits(got, want):
    """uint32 bit equality; an entry that is NaN in `want` only has to be NaN in `got` (x86 and gfx950 produce different NaNs)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool((got == want).all())
    g, w = got.view(np.uint32 if got.itemsize == 4 else np.uint64), want.view(np.uint32 if want.itemsize == 4 else np.uint64)
    nan = np.isnan(want)
    return bool(((g == w) | (nan & np.isnan(got))).all())
