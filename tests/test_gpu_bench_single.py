"""GPU: bench.py at N = 1 as every later change runs it -- a plain run
(inputs, W warmup steps, K timed steps, the line), --dump-outputs (what the
last timed step returned, the same from run to run) and --full (everything
else the bench measures, after the timed region)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB, STEPS, WARMUP, SETS = 1, 3, 2, 2          # 5 steps over 2 sets: the last one lands on set 0
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
           "--warmup", str(WARMUP), "--mib", str(MIB), "--sets", str(SETS)] + list(extra)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(line) == 1, p.stdout[-2000:]
    return json.loads(line[0])


@pytest.fixture(scope="module")
def expected():
    """the inout vector of the last of WARMUP + STEPS steps, from bench.py's
    own inputs: float32 adds on the host round as the kernel's do"""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    dev = torch.device("cuda:0")
    n = MIB * bench.MIB // 4
    x_in = [bench.synth_f32(n, 0x9E3779B9 ^ (2 * s * 1000003 + 1), dev).cpu().numpy() for s in range(SETS)]
    x_io = [bench.synth_f32(n, 0x9E3779B9 ^ ((2 * s + 1) * 1000003 + 1), dev).cpu().numpy() for s in range(SETS)]
    for i in range(WARMUP + STEPS):
        x_io[i % SETS] = x_in[i % SETS] + x_io[i % SETS]
    return x_io[(WARMUP + STEPS - 1) % SETS]


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path, expected):
    d = _bench("--dump-outputs", str(tmp_path / "a"))
    assert all(k in d for k in HEADLINE), sorted(d)
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - MIB / 1024 / (d["ms_per_step"] * 1e-3)) <= 0.01 * d["value"], d
    # nothing but the headline's own work ran
    assert d["full"] is False and d["parity"] is None
    assert "cpu_baseline" not in d and "combine_kernels" not in d and "mix_ceiling" not in d["roofline"]
    assert d["step_ms"]["evented_median"] is None
    assert sorted(os.listdir(tmp_path / "a")) == ["inout.npy"]
    got = np.load(tmp_path / "a" / "inout.npy")
    assert got.dtype == np.float32 and got.shape == expected.shape
    assert np.array_equal(got.view(np.uint32), expected.view(np.uint32))


def test_full_run_keeps_every_other_figure_and_the_same_dump(tmp_path, expected):
    d = _bench("--full", "--cpu-seconds", "0.2", "--dump-outputs", str(tmp_path / "b"))
    assert all(k in d for k in HEADLINE), sorted(d)
    assert d["full"] is True and d["parity"].startswith("bit-exact"), d["parity"]
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] == 1
    assert [r["config"] for r in d["combine_kernels"]] == ["C3", "C4", "C5"]
    assert d["roofline"]["mix_ceiling"]["additive_GBs"] > 0, d["roofline"]["mix_ceiling"]
    assert d["step_ms"]["evented_median"] >= d["step_ms"]["evented_min"] > 0
    # the evented pass and the parity step come after the dump is taken
    got = np.load(tmp_path / "b" / "inout.npy")
    assert np.array_equal(got.view(np.uint32), expected.view(np.uint32))
