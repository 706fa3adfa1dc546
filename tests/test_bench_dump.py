"""bench.py --dump-outputs: what the timed path returned in its last step, as float64 .npy files within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_what_the_caller_receives(tmp_path):
    import bench
    labels = np.arange(1000, dtype=np.int64) % 7 - 1
    names = bench.dump_outputs(str(tmp_path / "d"), (labels, 1, np.array([412], dtype=np.int64)))
    got = _files(tmp_path / "d")
    assert names == sorted(got) == ["changed_per_sweep", "labels", "sweeps"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["labels"], labels) and got["sweeps"].tolist() == [1.0]
    assert got["changed_per_sweep"].tolist() == [412.0]


def test_dump_outputs_samples_beyond_the_budget(tmp_path):
    import bench
    rng = np.random.default_rng(5)
    labels = rng.integers(0, 64, size=200_000)
    budget = 256 << 10
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), (labels, 1, np.array([9])), budget=budget)
    sizes = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert sizes <= budget
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    idx = a["labels_index"].astype(np.int64)
    assert np.array_equal(a["labels_index"], idx) and np.all(np.diff(idx) > 0)      # exact row numbers, ascending
    assert np.array_equal(a["labels"], labels[idx])
    assert idx.size > 10_000
    assert all(np.array_equal(a[k], b[k]) for k in a)                                 # the sample is fixed


@pytest.mark.gpu
def test_bench_dump_outputs_equal_the_oracle_sweep(tmp_path):
    """Two runs with different step counts dump the same arrays, and they are the oracle's sweep of the same inputs."""
    from oracle import oracle as O
    import chbin_amd
    N, B, m = 3000, 8, 5
    outs = {}
    for steps in (1, 3):
        d = tmp_path / f"s{steps}"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--contigs", str(N), "--bins", str(B),
                            "--steps", str(steps), "--warmup", "1", "--cpu-sample", "0", "--no-e2e", "--no-extra",
                            "--dump-outputs", str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = p.stdout.splitlines()
        assert len(lines) == 1 and json.loads(lines[0])["steps"] == steps
        outs[steps] = _files(d)
    assert sorted(outs[1]) == ["changed_per_sweep", "labels", "sweeps"]
    assert all(np.array_equal(outs[1][k], outs[3][k]) for k in outs[1])
    X, initial, _ = chbin_amd.synth.make_synthetic(N, 136, B, S=1, seed=0, mix=0.0, sigma=1.5e-3)   # bench.py's inputs
    perms = chbin_amd.synth.draw_permutations(initial, 10, seed=0)
    want, _ = O.sweep(X, B, initial, perms[0], m)
    assert np.array_equal(outs[1]["labels"], want)
    assert outs[1]["sweeps"].tolist() == [1.0]
    assert outs[1]["changed_per_sweep"].tolist() == [float((want != initial).sum())]
