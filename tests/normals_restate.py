"""rs_pointcloud__compute_normals (lib/rs/rs_pointcloud.h:556-596) and the loader's pass over its result (:743-751), restated in
NumPy with every operation in fp32 and in the reference's order.  tests/test_normals_cpu.py checks it bit for bit against what the
reference's own function wrote (tests/golden/normals_*.npz); the GPU tests use it where no recording exists.

A vertex normal is a running mean over the corners that name the vertex, in face order.  One vertex's chain is sequential, but the
chains are independent, so step k of the loop below applies every vertex's k-th corner at once: the loop is as long as the highest
valence, not as the face list."""
import numpy as np

F = np.float32
E_ARG = -2
INT32_MAX = (1 << 31) - 1


class Refused(Exception):
    def __init__(self, code, what):
        super().__init__(what)
        self.code = code


def same_bits(got, want):
    """The comparison rule: bit for bit where the reference's value is not NaN, NaN where it is."""
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != F:
        return bool((got == want).all())
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all())


def face_normals(pos, faces):
    """cross( p2 - p1, p3 - p1 ), not normalised (msh_vec3_cross, msh_vec_math.h:974-979)."""
    with np.errstate(all="ignore"):
        p1, p2, p3 = pos[faces[:, 0]], pos[faces[:, 1]], pos[faces[:, 2]]
        a, b = p2 - p1, p3 - p1
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def normalize(n):
    """msh_vec3_normalize (msh_vec_math.h:868-872)."""
    with np.errstate(all="ignore"):
        d = F(1.0) / np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        return n * d[:, None]


def vertex_normals(pos, faces, loader_pass=False):
    """(normals (n, 3) float32, counts (n,) int32: the corners that name each vertex)."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3); faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nv, nf = len(pos), len(faces)
    if nv <= 0 or nv > INT32_MAX: raise Refused(E_ARG, "vertices")
    if nf <= 0 or 3 * nf > INT32_MAX: raise Refused(E_ARG, "faces")
    if (faces < 0).any() or (faces >= nv).any(): raise Refused(E_ARG, "index")
    fn = face_normals(pos, faces)
    vert = faces.ravel().astype(np.int64)
    order = np.argsort(vert, kind="stable")                 # by vertex, ascending corner id inside a vertex: the reference's order
    sv, face = vert[order], order // 3
    counts = np.bincount(vert, minlength=nv)
    start = np.cumsum(counts) - counts
    rank = np.arange(3 * nf) - start[sv]
    # counts[v] advances after a face's three corners (:580-583): every corner of a (vertex, face) group sees the rank of the group's first
    head = np.ones(3 * nf, bool); head[1:] = (sv[1:] != sv[:-1]) | (face[1:] != face[:-1])
    before = rank[np.maximum.accumulate(np.where(head, np.arange(3 * nf), 0))]
    t = F(1.0) / (before.astype(F) + F(1.0))
    u = F(1.0) - t
    by_valence = np.argsort(-counts, kind="stable")
    active = np.searchsorted(-counts[by_valence], -np.arange(counts.max()), side="left")      # vertices with counts > k
    n = np.zeros((nv, 3), F)
    with np.errstate(all="ignore"):
        for k in range(int(counts.max())):
            v = by_valence[:active[k]]
            j = start[v] + k
            n[v] = t[j, None] * fn[face[j]] + u[j, None] * n[v]                               # msh_vec3_lerp, msh_vec_math.h:1032-1036
        # :586-592
        s = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
        norm = np.sqrt(s.astype(np.float64)).astype(F)
        out = np.where((norm > 0.0)[:, None], normalize(n), np.array([0.0, 1.0, 0.0], F)[None, :]).astype(F)
        if loader_pass:                                                                       # :743-751
            out = normalize(out)
            out[np.isnan(out).any(1)] = 0.0
    return np.ascontiguousarray(out), counts.astype(np.int32)
