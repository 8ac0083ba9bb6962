"""CPU: bench.py's own options -- what --dump-outputs writes (whole arrays, the seeded sample of one over the budget) and
the refusal of a run without timed steps -- and its start-up in a tree it cannot write."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_keeps_small_arrays_whole_and_samples_a_large_one(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 << 10)
    small = torch.arange(10, dtype=torch.float64)
    jac = torch.linspace(0.0, 1.0, 30, dtype=torch.float64).reshape(6, 5)
    big = torch.from_numpy(np.random.default_rng(1).standard_normal((64, 1000)))
    bench.dump_outputs(str(tmp_path / "a"), [("small", small), ("jac", jac), ("U", big)])
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["U_sample.npy", "jac.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BYTES
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())
    j = np.load(tmp_path / "a" / "jac.npy")
    assert j.shape == (6, 5) and np.array_equal(j, jac.numpy())
    u = np.load(tmp_path / "a" / "U_sample.npy")
    assert u.dtype == np.float64 and 0 < u.size < big.numel()
    # the sample is a subset of the array's elements, in index order, and the same on every run
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(big.numel(), u.size, replace=False))
    assert np.array_equal(u, big.numpy().reshape(-1)[idx])
    bench.dump_outputs(str(tmp_path / "b"), [("small", small), ("jac", jac), ("U", big)])
    assert np.array_equal(np.load(tmp_path / "b" / "U_sample.npy"), u)


def test_bench_refuses_a_run_without_timed_steps():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                         timeout=120, env=env)
    assert out.returncode == 2 and "--steps must be >= 1" in out.stderr


def test_up_to_date_artefacts_are_used_without_writing_into_the_tree(monkeypatch):
    """The benchmark (and smoke(), and --full's CPU baseline) may run as another user than the one whose build() made the
    tree: with everything up to date, none of them takes a build lock or starts a compiler."""
    import __graft_entry__ as G
    from oracle import oracle as O
    G.build()   # everything is up to date from here on
    O.build()
    real_open = os.open

    def no_lock(path, *a, **k):
        assert not str(path).endswith(".build.lock"), "build lock taken although nothing is out of date: %s" % path
        return real_open(path, *a, **k)

    def no_compiler(cmd, *a, **k):
        raise AssertionError("compiler started although nothing is out of date: %s" % cmd)
    monkeypatch.setattr(os, "open", no_lock)
    monkeypatch.setattr(subprocess, "check_call", no_compiler)
    bench.use_built_library()
    G.build()
    O.build()
