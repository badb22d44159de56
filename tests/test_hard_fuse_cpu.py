"""CPU: fuse_restate.transform reproduces what the reference's rs_pointcloud_transform made of the hostile points under every hostile
transform (tests/golden/fuse_hostile.npz, tools/fuse_fixture/gen.py; inputs: tests/hard_fuse.py), and the recordings hold what the
transforms are for.  Comparisons are uint32 bit equality; where both sides are NaN the payload is not compared (the sign and payload
of a NaN that an operation makes differ between processors and mean nothing to a consumer)."""
import numpy as np
import pytest

from conftest import load_golden
import fuse_restate as R
import hard_fuse as H

F = np.float32


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    nan = np.isnan(a)
    return a.shape == b.shape and bool((nan == np.isnan(b)).all()) and bool((R.bits(a)[~nan] == R.bits(b)[~nan]).all())


@pytest.fixture(scope="module")
def golden():
    return load_golden("fuse_hostile.npz")


def test_fixture_holds_the_generators_points_and_transforms(golden):
    assert golden["names"].tolist() == list(H.transforms())
    for tag, pts in (("", H.points()), ("finite_", H.points(finite=True))):
        assert same(golden[tag + "a_pos"], pts["a_pos"]) and same(golden[tag + "a_nor"], pts["a_nor"]) and len(pts["a_pos"]) == 257 and len(pts["b_pos"]) == 65
        for name, x in H.transforms().items():
            assert same(golden[f"{tag}{name}_xform"], x), name
    p = H.points()
    for what in (np.isnan, np.isinf, lambda a: (a == 0) & np.signbit(a), lambda a: (a != 0) & (np.abs(a) < np.finfo(F).tiny)):
        assert what(p["a_pos"]).any() and what(p["a_nor"]).any() and what(p["b_pos"]).any()
    f = H.points(finite=True)
    assert np.isfinite(f["a_pos"]).all() and np.isfinite(f["b_pos"]).all() and len(np.unique(f["a_pos"], axis=0)) == 257


@pytest.mark.parametrize("name", list(H.transforms()))
def test_restatement_reproduces_the_transform(golden, name):
    for tag in ("", "finite_"):
        x = golden[f"{tag}{name}_xform"]
        assert same(R.transform(x, golden[tag + "a_pos"], 1), golden[f"{tag}{name}_pos"]), (tag, name)
        assert same(R.transform(x, golden[tag + "a_nor"], 0), golden[f"{tag}{name}_nor"]), (tag, name)


def test_recordings_hold_what_the_transforms_are_for(golden):
    a_pos, a_nor = golden["a_pos"], golden["a_nor"]
    assert same(golden["identity_pos"][np.isfinite(a_pos).all(axis=1)], a_pos[np.isfinite(a_pos).all(axis=1)] + F(0))
    # the -0 matrix on zero normals: the three products sum to -0 and the kept 0 * t makes it +0; without that term it stays -0
    zero = (a_nor == 0).all(axis=1) & ~np.signbit(a_nor).any(axis=1)
    x = golden["negzero_xform"].copy()
    assert zero.sum() >= 1 and (golden["negzero_nor"][zero] == 0).all() and not np.signbit(golden["negzero_nor"][zero]).any()
    m = x.astype(F); v = a_nor[zero]
    dropped = np.stack([m[0] * v[:, 0] + m[4] * v[:, 1] + m[8] * v[:, 2]], axis=1)
    assert np.signbit(dropped).all()
    # Inf and NaN translations: every normal is NaN (0.0f * Inf and 0.0f * NaN), finite positions become +-Inf and NaN
    fin = np.isfinite(a_pos).all(axis=1)
    assert np.isnan(golden["inf_nan_nor"]).all()
    assert (golden["inf_nan_pos"][fin, 0] == np.inf).all() and (golden["inf_nan_pos"][fin, 1] == -np.inf).all() and np.isnan(golden["inf_nan_pos"][fin, 2]).all()
    # the scale of 1e-20: subnormal results that a flush to zero would lose; the scale of 1e20: overflow
    t = golden["tiny_pos"]
    assert ((t != 0) & (np.abs(t) < np.finfo(F).tiny)).sum() >= 20
    assert np.isinf(golden["huge_pos"]).any() and np.isnan(golden["huge_pos"][fin]).any() and np.isinf(golden["huge_nor"]).any()
    # a translation of 1e4 swallows the low bits: distinct points stay distinct, but not the same floats shifted back
    assert (golden["translation_pos"][fin] - golden["translation_xform"][12:15] != a_pos[fin]).any()
