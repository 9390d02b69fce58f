"""The bench-line contract (utils/metrics.py): what bench.py prints is what the round driver parses."""
import json
import os
import subprocess
import sys

import pytest

from parallel_c_programs_amd.utils.metrics import BENCH_KEYS, bench_line, validate_bench_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {"model": "SGEMM 8192x8192x8192 fp32", "global_batch": 1, "seq_len": None, "parallelism": "dp1"}


def _line(**kw):
    args = dict(metric="m", value=150.0, unit="TFLOPS", n_gpus=1, steps=10, warmup=3, ms_per_step=7.2, dtype="fp32",
                data="synthetic", config=dict(CFG))
    args.update(kw)
    return bench_line(**args)


def test_bench_line_keys_order_and_extras():
    line = _line(sgemm_tflops_per_gpu=150.0)
    assert list(line)[:len(BENCH_KEYS)] == list(BENCH_KEYS)
    assert line["vs_baseline"] is None and line["sgemm_tflops_per_gpu"] == 150.0
    assert _line(baseline=100.0)["vs_baseline"] == pytest.approx(1.5)
    json.dumps(line)


@pytest.mark.parametrize("bad", [dict(value=float("nan")), dict(value=-1.0), dict(scaling="linear"), dict(n_gpus=0),
                                 dict(steps=True), dict(config={"model": "x"}), dict(value=None)])
def test_bench_line_rejects(bad):
    with pytest.raises(ValueError):
        _line(**bad)


def test_bench_line_partial_and_shadowing():
    assert _line(value=None, ms_per_step=None, partial=True)["value"] is None
    with pytest.raises(ValueError, match="shadow"):
        _line(vs_baseline=2.0)  # an extra field may not overwrite a contract key
    with pytest.raises(ValueError, match="missing"):
        validate_bench_line({"metric": "m"})


def test_bench_small_cpu_prints_a_valid_line():
    """bench.py --small on the CPU (one rank): the one JSON line passes the contract check."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--small", "--device", "cpu",
                        "--steps", "1", "--warmup", "0", "--sections", "sgemm,reduce"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    validate_bench_line(line)
    assert line["n_gpus"] == 1 and line["value"] > 0


def test_bench_prints_line_with_contract_error(monkeypatch, capsys):
    """A line that fails the contract is still printed (with the reason) and bench.main returns 1."""
    import importlib

    import parallel_c_programs_amd.utils.metrics as M

    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")

    def broken(**kw):
        raise ValueError("bench line violates the driver contract: test")

    monkeypatch.setattr(M, "bench_line", broken)
    rc = bench.main(["--full", "--small", "--device", "cpu", "--steps", "1", "--warmup", "0", "--sections", "reduce"])
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert rc == 1 and "test" in line["contract_error"] and line["vs_baseline"] is None and "reduce_weak_gbps" in line


def _bench_main(capsys, *argv):
    import importlib

    sys.path.insert(0, ROOT)
    rc = importlib.import_module("bench").main(list(argv))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return rc, json.loads(lines[0])


def test_bench_plain_run_times_only_the_headline_and_dumps_its_output(tmp_path, capsys):
    """Without --full: the SGEMM alone (no other section's field, no check, no verdict), EXACTLY --steps timed steps,
    ms_per_step in the line; --dump-outputs writes the timed C (float32), the product of the seeded operands, and
    a second run with the same arguments writes the same bytes."""
    import numpy as np

    from parallel_c_programs_amd.models import workloads as W
    from parallel_c_programs_amd.parallel.dist import Context

    args = ("--gpus", "1", "--small", "--device", "cpu", "--steps", "3", "--warmup", "1")
    rc, line = _bench_main(capsys, *args, "--dump-outputs", str(tmp_path / "a"))
    validate_bench_line(line)
    assert rc == 0 and line["full"] is False and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["sgemm_device_ms_median"] > 0
    assert line["value"] == pytest.approx(2.0 * 256 ** 3 / (line["ms_per_step"] * 1e-3) / 1e12, rel=1e-2)
    assert "checks_passed" not in line and "sgemm_max_rel_err_vs_fp64" not in line
    assert not [k for k in line if k.split("_")[0] in ("reduce", "scan", "axpy", "stencil", "spmv", "hipblaslt")]
    c = np.load(tmp_path / "a" / "sgemm_c.npy")
    assert os.listdir(tmp_path / "a") == ["sgemm_c.npy"] and c.dtype == np.float32 and c.shape == (256, 256)
    g = W.Sgemm(Context(), n=256)
    g.step()
    assert np.array_equal(c, g.c.numpy())
    rc, _ = _bench_main(capsys, *args, "--dump-outputs", str(tmp_path / "b"))
    assert rc == 0 and np.array_equal(np.load(tmp_path / "b" / "sgemm_c.npy"), c)


def test_bench_dump_samples_an_output_above_the_budget(tmp_path, monkeypatch):
    """An output larger than the byte budget is written as a fixed seeded sample: the same flat indices every time,
    the tensor's own values at them, within the budget."""
    import importlib

    import numpy as np
    import torch

    from parallel_c_programs_amd.parallel.dist import Context

    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 1000)
    t = torch.arange(300 * 70, dtype=torch.float32).reshape(300, 70)
    bench.dump_output(str(tmp_path), "x", t, Context())
    bench.dump_output(str(tmp_path), "y", t * 2, Context())
    x, y = np.load(tmp_path / "x.npy"), np.load(tmp_path / "y.npy")
    assert x.dtype == np.float32 and x.shape == (1000,) and np.array_equal(y, 2 * x)  # (x holds its own flat indices)
    assert len(np.unique(x)) > 900 and x.min() >= 0 and x.max() < t.numel() and x.max() - x.min() > t.numel() / 2


@pytest.mark.parametrize("extra", [("--sections", "reduce"), ("--inject-fault", "sgemm:0:perturb")])
def test_bench_plain_run_refuses_full_only_options(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--small", "--device", "cpu", *extra],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 2 and "needs --full" in r.stderr and not r.stdout.strip()
