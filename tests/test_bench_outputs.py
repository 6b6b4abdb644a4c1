"""bench.py's plain and ``--full`` runs and ``--dump-outputs``: the plain line carries
the contract fields and none of the legs that take runs of their own, ``--full`` adds
them, and both write the same band flux for the same arguments (seeded inputs)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

FULL_ONLY = ("cpu_baseline", "unfused", "end_to_end", "end_to_end_band",
             "max_rel_err_vs_cpu_restatement", "band_fused_vs_unfused_max_rel")


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    band = torch.arange(50 * 9 * 2, dtype=torch.float64).reshape(50, 9, 2)
    bench.dump_outputs(str(tmp_path / "a"), band)
    assert sorted(os.listdir(tmp_path / "a")) == ["band_flux.npy"]
    got = np.load(tmp_path / "a" / "band_flux.npy")
    assert got.dtype == np.float64 and np.array_equal(got, band.numpy())
    # over the limit: a fixed sample of whole columns, the same in every run
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 10 * (9 * 2 * 8 + 8))
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), band)
    cols = np.load(tmp_path / "b" / "band_flux_columns.npy")
    got = np.load(tmp_path / "b" / "band_flux.npy")
    assert cols.dtype == np.float64 and len(cols) == 10 and len(set(cols)) == 10
    assert np.array_equal(got, band.numpy()[cols.astype(int)])
    assert np.array_equal(cols, np.load(tmp_path / "c" / "band_flux_columns.npy"))
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) \
        <= bench.DUMP_LIMIT_BYTES


def _run(tmp_path, name, *extra):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "3", "--warmup", "1", "--ncol", "37", "--ngpoint", "5",
                        "--nlyr", "12", "--dump-outputs", str(out), *extra],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    return json.loads(lines[0]), np.load(out / "band_flux.npy")


@pytest.mark.gpu
def test_plain_and_full_runs(tmp_path):
    plain, band = _run(tmp_path, "plain")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0
    # value = solves per step / the step's time (ms_per_step is printed to 1e-3 ms)
    ms = plain["ms_per_step"]
    assert abs(plain["value"] - 37 * 5 / (ms * 1e-3)) <= (1e-3 / ms + 1e-6) * plain["value"]
    assert all(plain[k] is None for k in FULL_ONLY)
    assert band.dtype == np.float64 and band.shape == (37, 13, 2)
    assert np.isfinite(band).all() and np.abs(band).max() > 0
    assert abs(band.sum() - plain["band_flux_sum"]) <= 1e-12 * np.abs(band).sum()

    full, band_full = _run(tmp_path, "full", "--full", "--no-cpu-baseline")
    assert all(full[k] is not None for k in FULL_ONLY if "cpu" not in k)
    assert full["band_fused_vs_unfused_max_rel"] <= 1e-12  # summation order only
    # same arguments, same inputs, same kernels: the same band flux to rounding (the
    # fused band sum's order over g-points may differ between runs)
    assert np.abs(band_full - band).max() <= 1e-12 * np.abs(band).max()
