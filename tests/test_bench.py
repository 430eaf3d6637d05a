"""bench.py's plain run, --full and --dump-outputs (the launcher and the work models are
covered by test_distributed.py)."""
import importlib
import json
import os

import numpy as np
import pytest

from conftest import rel

FULL_KEYS = ("roofline", "kernels_ms", "mstep_roofline", "estep_roofline", "status_trials",
             "nonhpd_trials", "cpu_baseline", "cpu_baseline_reference_structured")


def _bench():
    return importlib.import_module("bench")


def test_bench_full_and_dump_options_default_off():
    b = _bench()
    a = b.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = b.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_bench_dump_outputs_float64_and_seeded_sample(tmp_path, monkeypatch):
    """dump_outputs writes float64 .npy files (complex as a trailing re / im axis); past the
    byte budget every array keeps the same seeded rows, the same from call to call."""
    import torch
    b = _bench()
    th = torch.arange(40 * 6, dtype=torch.float64).reshape(40, 6).to(torch.complex128) * (1 + 2j)
    st = torch.arange(40, dtype=torch.int32)
    b.dump_outputs(str(tmp_path / "a"), {"theta": th, "status": st})
    t = np.load(tmp_path / "a" / "theta.npy")
    assert t.dtype == np.float64 and t.shape == (40, 6, 2)
    assert np.array_equal(t[..., 0] + 1j * t[..., 1], th.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "status.npy"), np.arange(40.0))
    total = t.nbytes + 40 * 8
    monkeypatch.setattr(b, "DUMP_BUDGET_BYTES", total // 4)
    for d in ("b", "c"):
        b.dump_outputs(str(tmp_path / d), {"theta": th, "status": st})
    tb, sb = np.load(tmp_path / "b" / "theta.npy"), np.load(tmp_path / "b" / "status.npy")
    assert tb.shape == (10, 6, 2) and sb.shape == (10,)
    assert tb.nbytes + sb.nbytes <= total // 4
    assert np.array_equal(np.sort(sb), sb) and np.array_equal(tb, t[sb.astype(int)])
    assert np.array_equal(tb, np.load(tmp_path / "c" / "theta.npy"))
    assert np.array_equal(sb, np.load(tmp_path / "c" / "status.npy"))


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_timed_path_theta(sbce, tmp_path, capsys):
    """A plain run (plumbing shape) prints the headline line without the --full figures and
    --dump-outputs holds the theta of EMEngine.run on the same seeded batch; a second run and a
    --full run (whose kernel timings overwrite theta afterwards) dump the same theta."""
    b = _bench()
    argv = ["--gpus", "1", "--config", "plumbing", "--steps", "2", "--warmup", "1"]
    lines = []
    for d, extra in (("a", []), ("b", []), ("c", ["--full", "--no-cpu-baseline"])):
        b.main(argv + extra + ["--dump-outputs", str(tmp_path / d)])
        lines.append(json.loads(capsys.readouterr().out.strip().splitlines()[-1]))
    for line in lines:
        assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["unit"] == "EM-iterations/s" and line["dtype"] == "f64"
        assert line["higher_is_better"] is True
        assert line["value"] == pytest.approx(10 * 10 / (line["ms_per_step"] * 1e-3))
    assert not [k for k in FULL_KEYS if k in lines[0]]
    assert lines[2]["roofline"] and lines[2]["kernels_ms"]["estep"] > 0
    assert lines[2]["nmse_mean"] == pytest.approx(lines[0]["nmse_mean"], rel=1e-9)
    n_tx, n_rx, N, T_p, T_d, M, B, iters = b.CONFIGS["plumbing"]
    varn = float(sbce.signal_model.snr_to_varn(20.0))
    batch = sbce.signal_model.synthetic_batch(B, n_tx, n_rx, N, T_p, T_d, M, varn, seed=0)
    ref = sbce.EMEngine(batch, varn).run(iters).cpu().numpy()
    t = np.load(tmp_path / "a" / "theta.npy")
    assert t.dtype == np.float64 and t.shape == ref.shape + (2,)
    assert np.load(tmp_path / "a" / "status.npy").shape == (B,)
    # float64 kernels on identical inputs: the bar of the suite's other same-path comparisons
    assert rel(t[..., 0] + 1j * t[..., 1], ref) < 1e-12
    for d in ("b", "c"):
        assert rel(np.load(tmp_path / d / "theta.npy"), t) < 1e-12
