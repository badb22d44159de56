"""Coordinate streams on which a parallel restatement of rs_pointcloud_centroid's chain is easy to get subtly wrong, each as a
one-instance dynamic scan, and the sequential reference to hold the chains of rescan_amd/csrc/rs_split.hip to.  A plain helper
module like hard_sums.py: no fixtures, no pytest hooks.

The reference adds a segment's coordinates one after the other into a double that starts at 0.0 (lib/rs/rs_pointcloud.h:1326-1332),
divides by the count and casts to float.  The order of the additions matters only where the addends span more than the 53 bits of
the accumulator; the streams below sit on both sides of that line, and on the special values:

  cancel      2^40, 4096 x 2^-14, -2^40: every small addend is a quarter of the running sum's grid and vanishes; the chain gives 0,
              the exact sum is 0.25
  tie         2^30, 8 x 2^-23, 2^-22, 8 x 2^-23: an addend of 2^-23 is exactly half the grid of 2^30 and rounds to even
  range       random 24-bit mantissas on exponents 2^-40 .. 2^20, shuffled
  zero_sum    multiples of 2^-10 and their negatives, shuffled: a sum of exactly zero
  negzero     -0.0 first, and only: the chain gives +0.0 (0.0 + -0.0), a reduction that starts from its first addend gives -0.0
  subnormal   float subnormals (exact in a double)
  binade      600 x (2^24 - 1): the running sum changes binade inside every block, all exact
  one_inf     one +Inf among finite values           one_nan     one NaN            both_inf   +Inf and -Inf: NaN
  cast_tie    1 and 1 + 2^-23: the quotient 1 + 2^-24 lies exactly between two floats

stream(name) is the x coordinate; scan(name) puts it into a scan of one instance of a dynamic class, with y and z of their own and
normals that include -0.0 components.  seq_sum is the reference (np.add.accumulate in float64 is the sequential sum), exact_sum the
correctly rounded one; measure(name) returns each family's defining property, which tests/test_hard_split_cpu.py holds it to.
"""
import math

import numpy as np

F = np.float32
STREAMS = ("cancel", "tie", "range", "zero_sum", "negzero", "subnormal", "binade", "one_inf", "one_nan", "both_inf", "cast_tie")
FINITE = ("cancel", "tie", "range", "zero_sum", "negzero", "subnormal", "binade", "cast_tie")       # the reference's output is entirely finite
DYNAMIC_CLASS = 5                   # synth.CLASS_IDX["chair"]
INSTANCE = 9


def stream(name):
    rng = np.random.default_rng(2100 + STREAMS.index(name))
    if name == "cancel":
        x = [2.0 ** 40] + [2.0 ** -14] * 4096 + [-(2.0 ** 40)]
    elif name == "tie":
        x = [2.0 ** 30] + [2.0 ** -23] * 8 + [2.0 ** -22] + [2.0 ** -23] * 8
    elif name == "range":
        e = np.repeat(np.arange(-40, 21), 12)
        m = rng.integers(1 << 23, 1 << 24, len(e)) * rng.choice([-1, 1], len(e))
        x = rng.permutation(np.ldexp(m.astype(np.float64), e - 23))
    elif name == "zero_sum":
        h = rng.integers(1, 1 << 20, 300) / 1024.0
        x = rng.permutation(np.concatenate([h, -h]))
    elif name == "negzero":
        x = [-0.0] * 5
    elif name == "subnormal":
        x = np.ldexp(rng.integers(-(1 << 22), 1 << 22, 200).astype(np.float64), -149)
    elif name == "binade":
        x = [2.0 ** 24 - 1] * 600
    elif name == "one_inf":
        x = list(rng.uniform(-2, 2, 99).astype(F).astype(np.float64)); x.insert(40, np.inf)
    elif name == "one_nan":
        x = list(rng.uniform(-2, 2, 99).astype(F).astype(np.float64)); x.insert(70, np.nan)
    elif name == "both_inf":
        x = list(rng.uniform(-2, 2, 98).astype(F).astype(np.float64)); x.insert(10, np.inf); x.insert(80, -np.inf)
    elif name == "cast_tie":
        x = [1.0, 1.0 + 2.0 ** -23]
    else:
        raise KeyError(name)
    x64 = np.asarray(x, np.float64)
    out = x64.astype(F)
    assert np.array_equal(out.astype(np.float64), x64, equal_nan=True), name          # every addend is a float as written
    return out


def at_length(x, n):
    """The stream cut or repeated to n addends."""
    return np.resize(np.asarray(x, F), n)


def scan(name, x=None):
    """(pos, nor, class_ids, instance_ids) of a one-instance dynamic scan whose x coordinates are the stream."""
    x = stream(name) if x is None else np.asarray(x, F)
    n = len(x)
    k = np.arange(n)
    pos = np.stack([x, (k % 7 - 3) * F(0.125), (k % 5) * F(0.5) - F(0.75)], axis=1).astype(F)
    nor = np.zeros((n, 3), F); nor[:, 1] = 1.0; nor[k % 3 == 0, 0] = -0.0; nor[k % 4 == 1, 2] = -0.0
    return pos, nor, np.full(n, DYNAMIC_CLASS, np.int32), np.full(n, INSTANCE, np.int32)


def seq_sum(x):
    """The reference's chain: double c = 0; c += (double)x[i], in order."""
    x = np.asarray(x, F).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.add.accumulate(np.concatenate([np.zeros(1), x]))[-1]


def seq_prefixes(x):
    x = np.asarray(x, F).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.add.accumulate(np.concatenate([np.zeros(1), x]))[1:]


def exact_sum(x):
    """The correctly rounded sum (math.fsum); NaN where an addend is not finite."""
    x = np.asarray(x, F).astype(np.float64)
    return math.fsum(x.tolist()) if np.isfinite(x).all() else float("nan")


def pairwise_sum(x):
    """A plain parallel fp64 reduction: a tree over the addends, the first addend as the start."""
    v = list(np.asarray(x, F).astype(np.float64))
    with np.errstate(all="ignore"):
        while len(v) > 1:
            v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0]


def centroid_of(total, n):
    with np.errstate(all="ignore"):
        return F(np.float64(total) / np.float64(n))


def bits64(v):
    return int(np.float64(v).view(np.uint64))


def measure(name):
    """The family's defining property, as a dict of measured values."""
    x = stream(name)
    s, e, p = seq_sum(x), exact_sum(x), pairwise_sum(x)
    pre = seq_prefixes(x)
    with np.errstate(all="ignore"):
        expo = np.frexp(pre)[1]
    return dict(n=len(x), seq=s, exact=e, pairwise=p, seq_centroid=centroid_of(s, len(x)), exact_centroid=centroid_of(e, len(x)),
                binade_changes_first_block=int((np.diff(expo[:64]) != 0).sum()), finite=bool(np.isfinite(x).all()))
