"""bench.py's contract with the driver: stdout carries exactly ONE line, a JSON object with the agreed keys."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_prints_one_json_line_with_roofline_and_legs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-duplex"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines          # the batch-CLI leg's own summary must not reach stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["dtype"] == "f32" and d["vs_baseline"] is None
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9 and 0.3 < rf["frac"] < 1.0
    cfg = d["config"]
    assert cfg["receptive_field_trimmed"]["codes_identical_to_full_windows"] is True
    assert cfg["bf16_mfma_opt_in"]["bf16_hi_lo_split"]["code_ids_equal_to_f32_path"] > 0.99
    assert cfg["batch_cli"]["value"] > 0


def _plain_run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", out_dir],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), np.load(os.path.join(out_dir, "codes.npy"))


def test_plain_bench_times_only_the_headline_and_dumps_the_last_step(tmp_path):
    """Without --full the line carries the headline alone (no roofline, legs or baselines); --dump-outputs writes the code ids of the
    last timed step, and two runs with the same arguments give the same ids."""
    d, codes = _plain_run(str(tmp_path / "a"))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0
    for k in ("roofline", "roofline_bf16", "duplex", "cpu_baseline"):
        assert k not in d, k
    assert d["config"]["bf16_mfma_opt_in"] is None and d["config"]["receptive_field_trimmed"] is None and "batch_cli" not in d["config"]
    # one step = 128 chunk positions x 5 frames per 0.1 s chunk, both channels; the codebook has 131072 entries
    assert codes.dtype == np.float64 and codes.shape == (2, 640)
    assert codes.min() >= 0 and codes.max() < 131072 and np.array_equal(codes, np.round(codes)) and len(np.unique(codes)) > 1
    _, again = _plain_run(str(tmp_path / "b"))
    assert np.array_equal(codes, again)
