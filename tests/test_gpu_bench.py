"""bench.py on the GPU: the zero-copy archive view RCCL sends from, the plain and the --full run
(tiny field), and --dump-outputs."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import cusz_amd as cz
from cusz_amd import datagen
from gpu_util import d2h

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_archive_view_is_the_archive():
    b = _bench()
    dims = (256, 40, 24)
    x = datagen.smooth3d_torch(dims, seed=4)
    r = cz.Resource(cz.F4, dims, stream=torch.cuda.current_stream().cuda_stream)
    ptr, nb, _ = r.compress(x.data_ptr(), 1e-4)
    view, scratch = b.archive_view(ptr, nb, x.device, None)
    assert view.numel() == nb and view.dtype == torch.uint8
    np.testing.assert_array_equal(view.cpu().numpy(), d2h(ptr, nb))
    print("zero-copy" if view.data_ptr() == ptr else "copied")
    r.close()


def _run_bench(b, monkeypatch, capsys, argv):
    monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    assert b.main() == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_steps_outputs(tmp_path, monkeypatch, capsys):
    """A plain run prints the headline fields only and --dump-outputs writes the last timed step's
    reconstruction and archive; a second run with the same arguments writes the same arrays."""
    b = _bench()
    dims, eb, steps = (96, 64, 40), 1e-4, 5
    argv = ["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--dims", "96x64x40"]
    d = _run_bench(b, monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "a")])
    assert d["steps"] == steps and d["full"] is False and d["unit"] == "GB/s" and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and d["higher_is_better"] is True
    np.testing.assert_allclose(d["value"], 4 * 96 * 64 * 40 / (d["ms_per_step"] * 1e-3) / 1e9, rtol=1e-2)
    assert "stages_ms" not in d and "roofline" not in d and "cpu_baseline" not in d
    _run_bench(b, monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "b")])
    got = {}
    for name in ("decompressed", "archive", "archive_nbytes"):
        got[name] = np.load(tmp_path / "a" / f"{name}.npy")
        assert got[name].dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(got[name], np.load(tmp_path / "b" / f"{name}.npy"))
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    # step k of the timed loop reads field k mod 3 (seeds 2, 1002, 2002): the last one's input
    x = datagen.smooth3d_torch(dims, seed=2 + 1000 * ((steps - 1) % 3)).cpu().numpy()
    assert got["decompressed"].shape == x.shape
    assert np.max(np.abs(got["decompressed"].astype(np.float64) - x)) <= 1.001 * eb + 2.0 ** -23 * np.abs(x).max()
    assert got["archive"].size == int(got["archive_nbytes"][0])
    assert abs(d["compression_ratio"] - x.nbytes / got["archive"].size) < 1e-3


def test_full_run_keeps_the_extra_fields(monkeypatch, capsys):
    b = _bench()
    d = _run_bench(b, monkeypatch, capsys, ["--gpus", "1", "--steps", "2", "--warmup", "1", "--dims", "96x64x40",
                                            "--full", "--no-cpu-baseline"])
    assert d["full"] is True and d["steps"] == 2 and d["ms_per_step"] > 0
    for k in ("stages_ms", "roofline", "same_field_value", "host_phases_ms", "e2e_host_gbps", "max_abs_err"):
        assert k in d, k
    assert d["max_abs_err"] <= 1.001e-4 + 2.0 ** -23 * 2
