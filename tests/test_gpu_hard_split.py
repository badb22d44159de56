"""GPU: the centroid chains of rescan_amd/csrc/rs_split.hip on the streams of tests/hard_split.py.  The reference is the sequential
fp64 sum (hard_split.seq_sum), compared as `sums` in all 64 bits, not only through the cast; a NaN compares equal to a NaN and only
where the reference's value is NaN too.  Every stream at the lengths around a row (64) and a block of the chain, the three axes
carrying different families, the same stream twice in one call; the whole hostile fixture through rs_hip_scan_to_objects is in
tests/test_gpu_split.py.  A plain parallel fp64 reduction fails here (hard_split.pairwise_sum differs on these streams:
tests/test_hard_split_cpu.py).  The GPU work runs in a child process under its own time limit; the inputs are hostile to the
arithmetic, not to the addressing."""
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PRELUDE = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from rescan_amd import capi
import split_restate as R
import hard_split as H
capi.init(0)
B = capi.split_layout()["chain_block"]
LENGTHS = (1, 63, 64, 65, B - 1, B, B + 1)
def segments():
    # (x stream, y stream, z stream, length): every stream on x at every length, two other families on y and z
    names = H.STREAMS
    out = []
    for k, name in enumerate(names):
        for n in LENGTHS + (len(H.stream(name)),):
            out.append((name, names[(k + 3) % len(names)], names[(k + 7) % len(names)], n))
    return out
def build(segs):
    pos, off = [], [0]
    for a, b, c, n in segs:
        pos.append(np.stack([H.at_length(H.stream(s), n) for s in (a, b, c)], axis=1)); off.append(off[-1] + n)
    return np.concatenate(pos).astype(np.float32), np.array(off, np.int64)
def reference(pos, off):
    sums = np.array([[H.seq_sum(pos[off[k]:off[k + 1], a]) for a in range(3)] for k in range(len(off) - 1)])
    with np.errstate(all="ignore"):
        cen = (sums / np.diff(off)[:, None].astype(np.float64)).astype(np.float32)
    return sums, cen
"""


def run_child(body, limit=120):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", PRELUDE + body, ROOT], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


def test_chains_on_every_stream_at_every_length():
    run_child(r"""
segs = segments()
segs = segs + segs[::5]                                   # the same streams twice in one call, as further instances
pos, off = build(segs)
want_sums, want_cen = reference(pos, off)
rng = np.random.default_rng(11)
for order in (np.arange(len(pos), dtype=np.int32),):
    sums, cen = capi.segment_centroids(pos, order, off)
    bad = [(segs[k], a, sums[k, a], want_sums[k, a]) for k in range(len(segs)) for a in range(3) if not R.same_bits(sums[k, a:a + 1], want_sums[k, a:a + 1])]
    assert not bad, bad[:5]
    assert R.same_bits(cen, want_cen)
assert capi.split_chains_sequential() > 0
# through a permutation of the points: the chain follows `order`, not the memory
perm = rng.permutation(len(pos)).astype(np.int32)
inv = np.empty_like(perm); inv[perm] = np.arange(len(pos), dtype=np.int32)
sums2, cen2 = capi.segment_centroids(pos[perm], inv, off)
assert sums2.tobytes() == sums.tobytes() and cen2.tobytes() == cen.tobytes()
# the lone-lane form gives the same doubles; two runs give identical bytes
before = capi.split_chains_form(1)
try:
    lone = capi.segment_centroids(pos, np.arange(len(pos), dtype=np.int32), off)[0]
finally:
    capi.split_chains_form(before)
assert R.same_bits(lone, want_sums)
assert capi.segment_centroids(pos, np.arange(len(pos), dtype=np.int32), off)[0].tobytes() == sums.tobytes()
print("ok")
""")


def test_the_diagnostic_counts_what_went_one_by_one():
    """0 on the room (every step is provably exact there), positive on the cancellation stream, all of a stream that is not finite
    from its first Inf on; an empty segment sums to +0.0."""
    run_child(r"""
g = dict(np.load(os.path.join(sys.argv[1], "tests", "golden", "split_room.npz")))
inst, off, order = capi.split_by_instance(g["scan_inst"])
sums, cen = capi.segment_centroids(g["scan_pos"], order, off)
assert capi.split_chains_sequential() == 0
assert R.same_bits(cen, g["centroids"])
for name in ("cancel", "tie", "range"):
    x = H.stream(name)
    pos = np.stack([x, np.zeros_like(x), np.ones_like(x)], axis=1)
    sums, _ = capi.segment_centroids(pos, np.arange(len(x)), [0, len(x)])
    n_seq = capi.split_chains_sequential()
    assert 0 < n_seq <= len(x), (name, n_seq)
    assert R.same_bits(sums[0], np.array([H.seq_sum(x), 0.0, float(len(x))])), name
    assert n_seq == R.chain_by_blocks(x)[1], (name, n_seq)            # the restated walk takes the same rows one by one
x = H.stream("one_inf")
pos = np.stack([x, x, x], axis=1)
sums, _ = capi.segment_centroids(pos, np.arange(len(x)), [0, len(x)])
assert np.isposinf(sums).all() and capi.split_chains_sequential() == 3 * len(x)       # one block, one row with the Inf, then S is not finite
sums, cen = capi.segment_centroids(pos, np.arange(len(x)), [0, 0, len(x)])
assert sums[0].tobytes() == np.zeros(3).tobytes() and np.isnan(cen[0]).all() and np.isposinf(sums[1]).all()
print("ok")
""")
