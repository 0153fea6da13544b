"""bench.py's multi-GPU launch contract on CPU: `--gpus N` without WORLD_SIZE re-launches itself
under torch.distributed.run with N ranks; the dry run takes the collective path of the sharded
step (histogram all-reduce + exact-size gather to rank 0) over gloo and prints one JSON line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    return p


@pytest.mark.parametrize("n", [2, 3])
def test_bench_spawns_n_ranks(n):
    p = _run(["--gpus", str(n), "--dry-run"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == n
    assert d["collectives_ok"] is True
    assert sum(d["slab_planes"]) == 512 and all(z % 8 == 0 for z in d["slab_planes"])


def test_bench_rejects_world_mismatch():
    p = _run(["--gpus", "2", "--dry-run"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0
    assert "WORLD_SIZE" in p.stderr


def test_dump_sample_is_fixed_and_within_budget(tmp_path):
    """--dump-outputs: an array over its share is a fixed seeded sample; float64 stays float64,
    everything else is written as float32 (int64 sizes as float64)."""
    import importlib.util

    import numpy as np
    import torch

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    big = torch.arange(5_000_000, dtype=torch.float32)
    a1, a2 = b.sample_for_dump(big, 1000), b.sample_for_dump(big, 1000)
    assert a1.shape == (1000,) and np.array_equal(a1, a2) and np.all(np.diff(a1) >= 0)
    assert np.array_equal(b.sample_for_dump(big[:1000], 1000), big[:1000].numpy())
    arrays = {"f64": torch.arange(3_000_000, dtype=torch.float64), "bytes": torch.zeros(30_000_000, dtype=torch.uint8),
              "n": torch.tensor([7], dtype=torch.int64)}
    b.dump_outputs(str(tmp_path), 1, 0, arrays)
    got = {k: np.load(tmp_path / f"{k}.npy") for k in arrays}
    assert got["f64"].dtype == np.float64 and got["bytes"].dtype == np.float32 and got["n"].dtype == np.float64
    assert got["n"][0] == 7.0 and got["f64"].size < 3_000_000 and got["bytes"].size < 30_000_000
    assert sum(a.nbytes for a in got.values()) <= b.DUMP_BUDGET
    b.dump_outputs(str(tmp_path), 2, 1, {"n": arrays["n"]})
    assert (tmp_path / "n_rank1.npy").exists()
