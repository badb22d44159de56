"""The brute-force rows of tests/hard_clouds.py against the CPU oracle's msh_hash_grid_radius_search on every hard family: the
GPU tests hold the device to the brute force, so the brute force must itself be the reference's answer.  No GPU needed.

Every family agrees exactly (counts, totals, distance rows bit for bit; indices up to exact ties, ties across the k-th slot
included), so the reference's own float bin arithmetic drops no point on any of them, not even 1e4 m from the origin or on
exact d² == r² lattices.  The GPU tests can therefore hold the device to the brute force directly."""
import numpy as np
import pytest

import hard_clouds as hc


@pytest.fixture(scope="module")
def rows():
    cache = {}

    def get(name):
        if name not in cache:
            f = hc.make(name)
            cache[name] = f, hc.brute_rows(f["points"], f["queries"], f["radius"], 1024)
        return cache[name]
    return get


@pytest.mark.parametrize("name", hc.FAMILIES)
def test_brute_force_equals_the_oracle(name, rows, oracle):
    f, full = rows(name)
    assert f["radius"] <= 2 * f["grid_radius"]                 # cell >= radius: at most 27 bins, the 512-bin cap never applies
    g = oracle.grid_create(f["points"], f["grid_radius"])
    try:
        for k in (1, 3, 16, 17, 64, 1024):
            d, i, nn, tot, _ = hc.truncate(full, k)
            od, oi, onn, otot = oracle.radius_search(g, f["queries"], f["radius"], k, 1)
            hc.assert_rows((d, i, nn, tot), (od, oi, onn, otot), f["points"], f["queries"])
    finally:
        oracle.grid_destroy(g)


def test_families_reach_what_they_are_for(rows):
    """The properties the GPU tests rely on: the contrast family has queries with more than 1024 points within the radius, the
    lattice family has exact d² == r² pairs (excluded), the outside family holds a NaN query and queries with no neighbour."""
    f, full = rows("contrast")
    assert (full[4] > 1024).sum() > 100 and full[4].max() >= 50000
    f, full = rows("lattice")
    d2 = hc.d2_rows(f["points"], f["queries"][:256])
    r2 = hc.radius_sq(f["radius"])
    assert (d2 == r2).sum() > 256 and (full[0][:256] < r2).all()
    f, full = rows("outside")
    nan = ~np.isfinite(f["queries"]).all(axis=1)
    assert nan.sum() == 1 and full[2][nan][0] == 0
    assert (full[2] == 0).sum() > 500
    f, full = rows("two_far")
    assert len(f["points"]) == 2 and full[2].max() == 1
