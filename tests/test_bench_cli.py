"""bench.py's command line (CPU): a plain run selects the timed steps only, --full brings back
every secondary measurement with its own switches, and --dump-outputs writes the step's
return value as float32 (a fixed seeded sample above the size cap)."""
import sys

import numpy as np
import torch


def _parse(monkeypatch, argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_selects_no_secondary_measurement(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (5, 2, False, None)
    assert a.no_roofline and a.no_psnr and a.no_cpu_baseline
    assert a.modes == "none" and a.lines == "none"
    # the secondary switches are inert without --full
    a = _parse(monkeypatch, ["--lines", "mixed8", "--modes", "bf16"])
    assert a.modes == "none" and a.lines == "none"


def test_full_run_keeps_every_measurement_and_its_switches(monkeypatch):
    a = _parse(monkeypatch, ["--full"])
    assert not (a.no_roofline or a.no_psnr or a.no_cpu_baseline)
    assert a.modes == "bf16" and a.lines == "mixed8,wild-ir,fp8,fp16-b16,fp32"
    a = _parse(monkeypatch, ["--full", "--no-psnr", "--lines", "fp8", "--dump-outputs", "d"])
    assert a.no_psnr and not a.no_roofline and a.lines == "fp8" and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import bench
    x = torch.arange(2 * 3 * 4 * 4, dtype=torch.float16).reshape(2, 3, 4, 4)
    bench.dump_outputs(x, str(tmp_path / "a"))
    a = np.load(tmp_path / "a" / "restored.npy")
    assert a.dtype == np.float32 and np.array_equal(a, x.float().numpy())
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 128)          # 96 elements x 4 B > 128 B
    bench.dump_outputs(x, str(tmp_path / "b"))
    bench.dump_outputs(x, str(tmp_path / "c"))
    b, c = np.load(tmp_path / "b" / "restored.npy"), np.load(tmp_path / "c" / "restored.npy")
    assert b.dtype == np.float32 and b.nbytes <= 128 and b.size == 16
    assert np.array_equal(b, c)
    idx = np.sort(np.random.default_rng(0).integers(0, x.numel(), 16))
    assert np.array_equal(b, x.float().numpy().reshape(-1)[idx])
