"""Hostile inputs for the fuse row's merge kernel: transforms whose products underflow, overflow, cancel to -0 or meet Inf and NaN, and
points with +-0, subnormal, Inf and NaN coordinates.  Plain NumPy, deterministic.  tests/golden/fuse_hostile.npz holds what the
reference's rs_pointcloud_transform makes of them (tools/fuse_fixture/gen.py); tests/test_hard_fuse_cpu.py pins
fuse_restate.transform to it and tests/test_gpu_hard_fuse.py runs k_fuse_merge on them."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(F).max
N_A, N_B = 257, 65                                       # across a block and a wave
FINITE = ("identity", "translation", "rotation")         # the merged cloud stays finite and spread: the device-cloud route indexes it


def _mat(rot, t):
    m = np.zeros(16, F)
    m[[0, 1, 2]], m[[4, 5, 6]], m[[8, 9, 10]] = rot[:, 0], rot[:, 1], rot[:, 2]      # column-major
    m[12:15] = t
    m[15] = 1
    return m


def transforms():
    """name -> 16 floats, column-major, the translation in 12..14"""
    eye = np.eye(3)
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    a = 0.7
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    rot = eye + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)                              # no entry is representable
    return dict(
        identity=_mat(eye, (0, 0, 0)),
        translation=_mat(eye, (1e4, -1e4, 1e4)),
        rotation=_mat(rot, (0.3, -1.7, 2.9)),
        tiny=_mat(eye * 1e-20, (1e-39, -1e-39, 0)),                                    # subnormal products and sums
        huge=_mat(eye * 1e20 + 1e19, (FLT_MAX, -FLT_MAX, 1e38)),                       # overflow, Inf - Inf
        negzero=_mat(np.full((3, 3), -0.0), (1.0, 2.0, 3.0)),                          # zero normals: the products sum to -0, + 0 * t makes it +0
        inf_nan=_mat(eye, (np.inf, -np.inf, np.nan)))                                  # normals NaN through 0.0f * Inf, positions Inf


SPECIAL = np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, -0.0, 0.0], [1e-45, -1e-45, 1e-40], [1e-19, -3e-19, 2e-19], [5e-39, 1.0, -1.0],
                    [FLT_MAX, -FLT_MAX, FLT_MAX], [FLT_MAX, 1.0, 0.0], [np.inf, 0.5, 0.5], [0.5, -np.inf, 0.5], [np.nan, 0.5, 0.5], [0.5, 0.5, np.nan],
                    [np.inf, -np.inf, np.nan], [1e19, 1e19, -1e19], [3e18, -0.0, 1.0], [-1.0, 1e-38, 1.1754944e-38]], F)


def points(seed=0, finite=False):
    """dict(a_pos, a_nor, b_pos, b_nor): N_A and N_B points; both ends of each array and every 16th entry come from SPECIAL (finite:
    only its finite, moderate rows), positions and normals from different rows of it."""
    rng = np.random.default_rng([81, seed])
    rows = SPECIAL[:6] if finite else SPECIAL
    out = {}
    for side, n in (("a", N_A), ("b", N_B)):
        pos = rng.uniform(-1, 1, (n, 3)).astype(F)
        nor = rng.normal(0, 1, (n, 3)); nor = (nor / np.linalg.norm(nor, axis=1, keepdims=True)).astype(F)
        at = np.unique(np.r_[0:4, n - 4:n, 0:n:16])
        pos[at] = rows[np.arange(len(at)) % len(rows)]
        nor[at] = rows[(np.arange(len(at)) + 3) % len(rows)]
        if finite:                                       # a cloud handle wants distinct, finite positions: the special rows go to the normals only
            pos[at] = rng.uniform(-1, 1, (len(at), 3)).astype(F) * F(1e-3)
            pos[at[0]] = (0.0, -0.0, 1e-40)
        out[side + "_pos"], out[side + "_nor"] = np.ascontiguousarray(pos), np.ascontiguousarray(nor)
    return out
