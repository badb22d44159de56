"""The meshes the resampler's tests and fixtures are made of (tools/resample_fixture/gen.py, tests/test_resample_cpu.py,
tests/test_gpu_resample.py, tools/resample_timing.py).  Deterministic: every call gives the same arrays.

A mesh is a dict: pos (n, 3) float32, faces (m, 3) int32, and per vertex nor, col (n, 3) float32, radii float32, cls, inst int32."""
import numpy as np

F = np.float32
SAMPLES_PER_AREA = 6400.0          # rs_pointcloud.h:1151-1158: 0.5 * 12800 samples per unit of the reference's "area", the norm of a face's cross product
SMALL_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
# Samples of the reference's sequence whose two smallest barycentric weights are equal (the weights depend on the index alone):
# w1 == w2 < w0, w0 == w2 < w1, w0 == w1 < w2.  Found by scanning the restatement; tests assert them again.
TIE_INDICES = (853896, 2188471, 2436935)


def attributes(n, seed):
    """Random unit normals, colours, radii, class and instance ids for n vertices."""
    rng = np.random.default_rng(seed)
    nor = rng.normal(size=(n, 3)); nor /= np.linalg.norm(nor, axis=1, keepdims=True)
    return dict(nor=nor.astype(F), col=rng.random((n, 3)).astype(F), radii=rng.uniform(0.001, 0.02, n).astype(F),
                cls=rng.integers(0, 40, n).astype(np.int32), inst=rng.integers(0, 1000, n).astype(np.int32))


def mesh(pos, faces, seed):
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    return dict(pos=pos, faces=np.ascontiguousarray(faces, np.int32).reshape(-1, 3), **attributes(len(pos), seed))


def grid(nx, ny, size, bump, seed):
    """An (nx x ny)-vertex height field over size x size metres, two triangles per cell, heights +- bump."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.linspace(0, size, nx), np.linspace(0, size, ny), indexing="ij")
    pos = np.stack([x.ravel(), rng.uniform(-bump, bump, nx * ny), y.ravel()], 1)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (i * ny + j).ravel(); b = a + 1; c = a + ny; d = c + 1
    return pos, np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])


def patch():
    """A bumpy 9 x 9 grid, one large triangle and two zero-area faces ([v, v, v] and [a, b, b]): 131 faces, about 6 000 samples."""
    pos, faces = grid(9, 9, 0.45, 0.015, 41)
    n = len(pos)
    pos = np.concatenate([pos, [[0.7, 0.0, 0.0], [1.42, 0.0, 0.07], [0.92, 0.65, 0.29]]])
    faces = np.concatenate([faces, [[n, n + 1, n + 2], [7, 7, 7], [3, 30, 30]]])
    return mesh(pos, faces, 42)


def skew():
    """About 200 faces whose areas span six decades; one holds more than 99 % of the area: most alias columns point at it.  ~3 000 samples."""
    rng = np.random.default_rng(43)
    n_small = 199
    side = 10.0 ** rng.uniform(-4.2, -2.0, n_small)            # areas (side^2) 4e-9 .. 1e-4 against the big face's 0.46
    org = rng.uniform(-1.0, 1.0, (n_small, 3))
    e1 = rng.normal(size=(n_small, 3)); e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(e1, rng.normal(size=(n_small, 3))); e2 /= np.linalg.norm(e2, axis=1, keepdims=True)
    pos = np.concatenate([np.stack([org, org + e1 * side[:, None], org + e2 * side[:, None]], 1).reshape(-1, 3),
                          [[0.0, 0.0, 0.0], [0.68, 0.0, 0.0], [0.0, 0.0, 0.68]]])
    faces = np.arange(3 * (n_small + 1)).reshape(-1, 3)
    order = np.random.default_rng(44).permutation(n_small + 1)     # the big face somewhere in the middle
    return mesh(pos, faces[order], 45)


def long():
    """Two triangles whose areas (cross-product norms) sum to about 11: more than 65 536 samples, so sample indices exceed 2^16."""
    return mesh([[0, 0, 0], [2.4, 0, 0], [2.4, 0.15, 2.33], [0, 0.1, 2.26]], [[0, 1, 2], [0, 2, 3]], 46)


def triangle(n_samples):
    """One right triangle whose sample count is n_samples: cross-product norm leg^2 = (n + 0.5) / 6400."""
    leg = np.sqrt((n_samples + 0.5) / SAMPLES_PER_AREA)
    return mesh([[0.1, 0.2, 0.3], [0.1 + leg, 0.2, 0.3], [0.1, 0.2, 0.3 + leg]], [[0, 1, 2]], 47 + n_samples)


def mostly_degenerate():
    """Forty faces, all but one of exactly zero area: repeated vertices, and collinear vertices a dyadic step apart (their fp32
    cross product is exactly zero)."""
    pos = np.concatenate([[[0, 0, 0], [0.5, 0, 0], [0, 0.6, 0.1]], 1.0 + np.arange(12)[:, None] * np.array([0.25, 0.5, 0.75])])
    faces = [[3 + k % 12, 3 + k % 12, 3 + (k + 1) % 12] for k in range(20)] + [[0, 1, 2]] + [[3, 5 + k % 9, 4] for k in range(19)]
    return mesh(pos, faces, 48)


def equal_pair():
    """Two faces of exactly equal area (a unit-free square cut along its diagonal): every prob is 1.0."""
    return mesh([[0, 0, 0], [0.5, 0, 0], [0.5, 0, 0.5], [0, 0, 0.5]], [[0, 1, 2], [0, 2, 3]], 49)


def huge():
    """Two triangles whose areas sum to about 3.4e5: n_samples lies in (2^31 - 2^10, INT32_MAX], so 2 * i does not fit 32 bits near
    the end.  512 x b metres with 512 * b exact in fp32; b is chosen so that 6400 * 2 * 512 * b falls inside that window."""
    b = F(327.67992)
    return mesh([[0, 0, 0], [512, 0, 0], [512, b, 0], [0, b, 0]], [[0, 1, 2], [0, 2, 3]], 50)


def big(n_side=1001, seed=51):
    """A height field of n_side^2 vertices and 2 (n_side - 1)^2 faces over 8.8 x 8.8 m: about 1 M vertices, 2 M faces, ~1 M samples
    (tools/resample_timing.py)."""
    pos, faces = grid(n_side, n_side, 8.8, 0.004, seed)
    return mesh(pos, faces, seed + 1)
