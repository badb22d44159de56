"""NumPy restatements of the model fusion that closes a timestep (rsdu_augment_database, apps/segment_transfer/database_update.cpp:22-91):
the selection of rs_pointcloud_copy_by_ids (lib/rs/rs_pointcloud.h:239-297), the permutation of rs_pointcloud_merge's shuffle
(:427-442) and the merge itself with rs_pointcloud_transform's arithmetic (:1367-1378, msh_vec_math.h:1554-1561).

Not the product's code and not the reference's: a third statement of the same semantics, checked bit for bit against the
reference's recorded output (tests/test_fuse_cpu.py) and then used where no recording exists.  The PCG32 stream is
resample_restate's."""
import numpy as np

import resample_restate as R

F = np.float32
SEED_MERGE = 12346                                         # rs_pointcloud.h:428
MAX_POINTS = 1 << 24
E_ARG, E_CAPACITY = R.E_ARG, R.E_CAPACITY
Refused = R.Refused


def select(point_ids, ids):
    """The indices, increasing, of the points whose id is among ids (each id listed once)."""
    ids = np.asarray(ids, np.int32).ravel()
    if len(np.unique(ids)) != len(ids):
        raise Refused(E_ARG, "an id is listed twice")
    return np.flatnonzero(np.isin(np.asarray(point_ids, np.int32).ravel(), ids)).astype(np.int32)


def draws(n, seed=SEED_MERGE):
    """j[i] for the steps i = 1 .. n-1 (j[0] unused, 0): step i takes draw n-1-i of the stream; j = (int32)( nextf * i ) in fp32."""
    j = np.zeros(max(n, 1), np.int64)
    if n < 2:
        return j
    i = np.arange(1, n, dtype=np.int64)
    state, inc = R.pcg_seed(seed)
    u, _ = R.pcg_draw(R.advance(state, inc, (n - 1 - i).astype(np.uint64)), inc)
    j[1:] = (R.unit_float(u) * i.astype(F)).astype(np.int32)
    return j


def plan(n, seed=SEED_MERGE):
    """perm[i]: the index in "A then B" of the element the shuffle leaves at i — the sequential loop of :430-442."""
    if n < 0:
        raise Refused(E_ARG, "a negative count")
    if n > MAX_POINTS:
        raise Refused(E_CAPACITY, "more than 2^24 points")
    perm = list(range(n))
    j = draws(n, seed).tolist()
    for i in range(n - 1, 0, -1):
        perm[i], perm[j[i]] = perm[j[i]], perm[i]
    return np.array(perm, np.int32).reshape(n)


def transform(xform, v, w):
    """msh_mat4_vec3_mul( xform, v, w ) row by row: three fp32 products added left to right, then (float)w times the translation."""
    m = np.ascontiguousarray(xform, F).ravel(); v = np.ascontiguousarray(v, F).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    w = F(w)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([m[0] * x + m[4] * y + m[8] * z + w * m[12],
                         m[1] * x + m[5] * y + m[9] * z + w * m[13],
                         m[2] * x + m[6] * y + m[10] * z + w * m[14]], axis=1).astype(F)


def merge(a_pos, a_nor, xform, b_pos, b_nor, seed=SEED_MERGE):
    """(pos, nor, source) of rs_pointcloud_transform( A, xform ) followed by rs_pointcloud_merge( A, B )."""
    a_pos = np.ascontiguousarray(a_pos, F).reshape(-1, 3); b_pos = np.ascontiguousarray(b_pos, F).reshape(-1, 3)
    a_nor = np.ascontiguousarray(a_nor, F).reshape(-1, 3); b_nor = np.ascontiguousarray(b_nor, F).reshape(-1, 3)
    source = plan(len(a_pos) + len(b_pos), seed)
    pos = np.concatenate([transform(xform, a_pos, 1), b_pos])[source]
    nor = np.concatenate([transform(xform, a_nor, 0), b_nor])[source]
    return pos, nor, source


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64)


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a) == bits(b)).all())
