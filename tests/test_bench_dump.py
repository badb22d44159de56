"""bench.py --dump-outputs (no device): what the last timed step returned, written as float32 .npy files — every array whole while
they fit the budget, a fixed, seeded sample of the per-point rows when they do not; and the inputs a dump is compared on are the
same from run to run."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _step_outputs(rng, n, sharded=False):
    o = dict(err=np.float32(rng.random()), T=rng.random(16).astype(np.float32), scores=rng.random(256).astype(np.float32),
             labels=rng.integers(-1, 40, n).astype(np.int8), min_dists=rng.random(n).astype(np.float32))
    if sharded:
        o["Ts"] = rng.random((3, 16)).astype(np.float32)
        o["errs"] = rng.random(3).astype(np.float32)
    return o


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_writes_every_output_as_float32(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    o0, o1 = _step_outputs(rng, 1000), _step_outputs(rng, 900, sharded=True)
    bench.dump_outputs(str(tmp_path), [o0, o1])
    got = _read(str(tmp_path))
    assert sorted(got) == sorted(n + s for n in ("icp_poses", "icp_errors", "scores", "labels", "min_dists") for s in ("", "_pair1"))
    assert all(a.dtype == np.float32 for a in got.values())
    assert (got["icp_poses"] == o0["T"].reshape(1, 16)).all() and (got["icp_errors"] == [o0["err"]]).all()
    assert (got["icp_poses_pair1"] == o1["Ts"]).all() and (got["icp_errors_pair1"] == o1["errs"]).all()
    assert (got["scores"] == o0["scores"]).all() and (got["min_dists_pair1"] == o1["min_dists"]).all()
    assert (got["labels"] == o0["labels"].astype(np.float32)).all()


def test_dump_samples_the_same_rows_within_the_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 << 10)
    o = _step_outputs(np.random.default_rng(2), 50_000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [o])
    a, b = _read(str(tmp_path / "a")), _read(str(tmp_path / "b"))
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))) <= 64 << 10
    rows = a["sample_rows"].astype(np.int64)
    assert len(rows) > 0 and (np.diff(rows) > 0).all() and (a["sample_rows"] == b["sample_rows"]).all()
    assert (a["labels"] == o["labels"][rows]).all() and (a["min_dists"] == o["min_dists"][rows]).all()
    assert (a["scores"] == o["scores"]).all()


def test_inputs_are_the_same_from_run_to_run():
    import bench
    a, b = bench.build_inputs(20_000, 11), bench.build_inputs(20_000, 11)
    for k in ("icp_T0s", "score_poses", "plc_poses"):
        assert (a[k] == b[k]).all()
    for s in ("s0", "s1"):
        assert (a[s]["points"] == b[s]["points"]).all() and (a[s]["normals"] == b[s]["normals"]).all()
    assert all((p["np"][0] == q["np"][0]).all() for p, q in zip(a["plc"], b["plc"]))
