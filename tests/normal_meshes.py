"""The meshes the vertex-normal tests and fixtures are made of (tools/normals_fixture/gen.py, tests/test_normals_cpu.py,
tests/test_gpu_normals.py), beside those of tests/hard_meshes.py.  Deterministic: every call gives the same arrays.

A mesh here is (pos (n, 3) float32, faces (m, 3) int32): normals are what is computed."""
import numpy as np

import hard_meshes as H

F = np.float32
FAN_FACES = 3000


def _mesh(pos, faces):
    return np.ascontiguousarray(pos, F).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)


def patch():
    m = H.patch()
    return m["pos"], m["faces"]


def fan(hub_last=False, n=FAN_FACES, seed=61):
    """One hub vertex named by n faces: more than a wave, more than a workgroup, and long enough for the running mean to depend on the
    face order in its last bits.  The rim vertices stand at random angles, so consecutive face normals point anywhere.  Face k is
    (hub, rim k, rim k + 1) rotated by k % 3: the hub sits in every corner position.  hub_last: the hub is the last vertex, not the first."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0.0, 2.0 * np.pi, n); rad = rng.uniform(0.5, 2.0, n); hgt = rng.normal(0.0, 0.3, n)
    rim = np.stack([rad * np.cos(ang), hgt, rad * np.sin(ang)], 1)
    hub = np.array([[0.0, 0.2, 0.0]])
    k = np.arange(n)
    if hub_last:
        pos, h, r0 = np.concatenate([rim, hub]), n, 0
    else:
        pos, h, r0 = np.concatenate([hub, rim]), 0, 1
    tri = np.stack([np.full(n, h), r0 + k, r0 + (k + 1) % n], 1)
    faces = np.stack([np.roll(tri[i], i % 3) for i in range(n)])
    return _mesh(pos, faces)


def fan_shuffled(hub_last=False, seed=62):
    pos, faces = fan(hub_last)
    return pos, np.ascontiguousarray(faces[np.random.default_rng(seed).permutation(len(faces))])


def quirks():
    """Every corner of the reference's function on a handful of vertices; the comments name the vertices."""
    nan = np.nan
    pos = [
        [0.0, 0.0, 0.0], [0.3, 0.0, 0.1], [0.1, 0.2, 0.4],          # 0-2   two opposite faces on one triple: the mean cancels exactly -> +y
        [1.0, 0.0, 0.0], [1.2, 0.1, 0.0],                           # 3-4   faces (a,a,b), (a,b,a), (a,a,a): zero cross products, counts 7 and 2
        [2.0, 0.0, 0.0], [2.5, 0.0, 0.1], [2.1, 0.4, 0.0], [2.2, 0.1, 0.6],   # 5-8   5: ordinary, doubled, ordinary (one t for both corners); 8: doubled first
        [3.0, 3.0, 3.0],                                            # 9     no face names it
        [0.0, 0.0, 0.0], [1e20, 0.0, 0.0], [0.0, 1e20, 0.0],        # 10-12 the cross product overflows to (0, 0, inf): NaN after the finish
        [4.0, nan, 0.0], [4.5, 0.0, 0.0], [4.0, 0.0, 0.5],          # 13-15 a NaN coordinate: NaN fails the compare -> +y
        [0.0, 0.0, 0.0], [1e-23, 0.0, 0.0], [0.0, 0.0, 1e-23],      # 16-18 edge 1e-23: the products underflow to zero
        [0.0, 0.0, 0.0], [1e-20, 0.0, 0.0], [0.0, 1e-20, 0.0],      # 19-21 edge 1e-20: the products are denormal, their squares zero
        [0.0, 0.0, 0.0], [2e-10, 1e-10, 0.0], [0.0, 2e-10, 1e-10],  # 22-24 edge 2e-10: the squares are denormal, the sum positive
    ]
    faces = [
        [0, 1, 2], [0, 2, 1],
        [3, 3, 4], [3, 4, 3], [3, 3, 3],
        [5, 6, 7], [8, 5, 8], [5, 7, 5], [5, 8, 6], [8, 6, 7],
        [10, 11, 12],
        [13, 14, 15],
        [16, 17, 18], [19, 20, 21], [22, 23, 24],
    ]
    return _mesh(pos, faces)


def single():
    return _mesh([[0.1, 0.2, 0.3], [0.6, 0.2, 0.3], [0.1, 0.2, 0.9]], [[0, 1, 2]])


def grid(nx, ny, seed=63):
    pos, faces = H.grid(nx, ny, 0.01 * nx, 0.004, seed)
    return _mesh(pos, faces)


def ends(n=70001):
    """n vertices of which faces name only the first three and the last three: a sort key cut to 16 bits folds the last onto others."""
    rng = np.random.default_rng(64)
    pos = rng.uniform(-1.0, 1.0, (n, 3))
    faces = [[0, 1, 2], [n - 1, n - 2, n - 3], [2, n - 1, 0], [n - 3, 1, n - 2], [1, 0, n - 1]]
    return _mesh(pos, faces)
