"""CPU: every stream of tests/hard_split.py has the property it was made for; the reference's centroid and transformed arrays for
each (tests/golden/split_hostile.npz, written by the reference's own pointcloud_to_rsdb: tools/split_fixture) are reproduced bit for
bit by the NumPy restatement and by rs_hip_split_plan; and the block walk of rescan_amd/csrc/rs_split.hip, restated
(split_restate.chain_by_blocks), gives the sequential sum on every stream at every length the GPU tests use, taking the streams
that need the reference's order one addend at a time.

A NaN compares equal to a NaN whatever its sign and payload, and only where the reference's value is NaN too; the fixture names the
streams whose outputs hold no NaN at all, so that the allowance cannot hide a failure."""
import numpy as np
import pytest

from conftest import load_golden
import hard_split as H
import split_restate as R

F = np.float32
LENGTHS = (1, 63, 64, 65, 511, 512, 513)


@pytest.fixture(scope="module")
def capi():
    from rescan_amd import build, capi
    build.build()
    return capi


@pytest.fixture(scope="module")
def hostile():
    return load_golden("split_hostile.npz")


def bits(v):
    return H.bits64(v)


def test_every_family_has_its_property():
    m = {name: H.measure(name) for name in H.STREAMS}
    # the cancellation: the chain gives 0, the exact sum is 0.25, and the float centroids differ
    assert m["cancel"]["seq"] == 0.0 and m["cancel"]["exact"] == 0.25 and m["cancel"]["seq_centroid"] != m["cancel"]["exact_centroid"]
    # the ties round by the parity of the sum they meet: the first eight half-grid addends vanish (2^30 is even), 2^-22 makes the sum
    # odd, the ninth rounds it up to even and the last seven vanish again; the exact sum keeps all sixteen
    assert m["tie"]["seq"] == 2.0 ** 30 + 2.0 ** -21 and m["tie"]["exact"] == 2.0 ** 30 + 2.0 ** -22 + 16 * 2.0 ** -23
    x = H.stream("range")
    e = np.frexp(np.abs(x.astype(np.float64)))[1]
    assert e.min() <= -39 and e.max() >= 20 and bits(m["range"]["seq"]) != bits(m["range"]["exact"])       # wider than 53 bits: the order shows
    assert m["zero_sum"]["seq"] == 0.0 and m["zero_sum"]["exact"] == 0.0 and not np.signbit(m["zero_sum"]["seq"])
    # -0.0 only: the chain starts from +0.0 and stays there; a reduction that starts from its first addend gives -0.0
    assert bits(m["negzero"]["seq"]) == 0 and np.signbit(m["negzero"]["pairwise"])
    x = H.stream("subnormal")
    assert (np.abs(x[x != 0]) < np.finfo(F).tiny).all() and bits(m["subnormal"]["seq"]) == bits(m["subnormal"]["exact"])
    assert m["binade"]["binade_changes_first_block"] >= 5 and bits(m["binade"]["seq"]) == bits(m["binade"]["exact"])
    assert np.isposinf(m["one_inf"]["seq"]) and np.isnan(m["one_nan"]["seq"]) and np.isnan(m["both_inf"]["seq"])
    assert not m["one_inf"]["finite"] and not m["one_nan"]["finite"] and not m["both_inf"]["finite"]
    # the quotient lies exactly between two floats and rounds to the even one
    q = m["cast_tie"]["seq"] / 2.0
    assert q == 1.0 + 2.0 ** -24 and m["cast_tie"]["seq_centroid"] == F(1.0)
    for name in H.FINITE:
        assert m[name]["finite"], name


def test_the_fixture_holds_entirely_finite_streams(hostile):
    assert tuple(hostile["names"].tolist()) == H.STREAMS and tuple(hostile["finite"].tolist()) == H.FINITE
    for name in H.STREAMS:
        out = [hostile[f"stream_{name}_{k}"] for k in ("centroid", "xform", "pose", "out_pos", "out_nor")]
        assert all(np.isfinite(a).all() for a in out) == (name in H.FINITE), name
        pos, nor, _, _ = H.scan(name)
        assert R.same_bits(pos, hostile[f"stream_{name}_pos"]) and R.same_bits(nor, hostile[f"stream_{name}_nor"]), name
    # a dynamic object's -0.0 normal component comes out +0.0, and an infinite coordinate makes NaN
    z = hostile["stream_tie_out_nor"]
    assert np.signbit(hostile["stream_tie_nor"][hostile["stream_tie_nor"] == 0]).any() and not np.signbit(z[z == 0]).any()
    assert np.isnan(hostile["stream_one_inf_out_pos"]).any()


def check_stream(got, hostile, name):
    assert got["n_instances"] == 1 and got["inst_ids"].tolist() == [H.INSTANCE] and got["is_static"].tolist() == [0], name
    x = hostile[f"stream_{name}_pos"][:, 0]
    want = H.seq_sum(x)
    assert R.same_bits(got["sums"][0, :1], np.array([want])), (name, got["sums"][0, 0], want)
    cen = hostile[f"stream_{name}_centroid"].copy(); cen[1] = 0
    assert R.same_bits(got["centroids"][0], cen), name
    assert R.same_bits(got["xforms"][0], hostile[f"stream_{name}_xform"]) and R.same_bits(got["poses"][0], hostile[f"stream_{name}_pose"]), name
    assert R.same_bits(got["out_pos"], hostile[f"stream_{name}_out_pos"]) and R.same_bits(got["out_nor"], hostile[f"stream_{name}_out_nor"]), name


@pytest.mark.parametrize("name", H.STREAMS)
def test_restatement_reproduces_the_hostile_fixture(capi, hostile, name):
    pos, nor, cls, inst = H.scan(name)
    check_stream(R.plan(pos, nor, cls, inst), hostile, name)


@pytest.mark.parametrize("name", H.STREAMS)
def test_plan_reproduces_the_hostile_fixture(capi, hostile, name):
    """Fails on a library without rs_hip_split_plan."""
    pos, nor, cls, inst = H.scan(name)
    check_stream(capi.split_plan(pos, nor, cls, inst, R.STATIC_CLASSES), hostile, name)


@pytest.mark.parametrize("name", H.STREAMS)
def test_the_block_walk_gives_the_sequential_sum(name):
    """The condition of rs_split.hip's header comment, restated: where it lets a block or a row go order-free the sum is the
    reference's all the same, at the stream's own length and at every length around a row and a block."""
    x = H.stream(name)
    for n in (len(x),) + LENGTHS:
        y = H.at_length(x, n)
        s, one_by_one = R.chain_by_blocks(y)
        want = H.seq_sum(y)
        assert R.same_bits(np.array([s]), np.array([want])), (name, n, s, want)
        assert 0 <= one_by_one <= n
    full = R.chain_by_blocks(x)[1]
    if name in ("cancel", "tie", "range", "one_inf", "one_nan", "both_inf"):
        assert full > 0, name                                     # the order matters, or a value is not finite
    if name in ("zero_sum", "negzero", "subnormal", "binade", "cast_tie"):
        assert full == 0, name                                    # provably exact: never one by one
