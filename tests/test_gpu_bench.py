# coding: utf-8
"""bench.py on the GPU: a plain run measures the headline alone; what --full adds stays out of its line."""
import json
import os
import subprocess
import sys

import pytest

from tests.util import ROOT

# the fields only `bench.py --full` measures
FULL_ONLY = ("eager", "input_pipeline", "host_buffers", "value_exact_f32", "configs", "roofline", "roofline_wgrad",
             "roofline_exact_f32", "roofline_bf16_c8", "cpu_baseline")


@pytest.mark.gpu
def test_plain_bench_line_is_the_headline_alone():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                       universal_newlines=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "dtype", "config", "step_flop_frac"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "mel-frames/s" and d["dtype"] in ("f16x3", "bf16x3", "f32", "bf16")
    assert abs(d["value"] - d["config"]["global_batch"] * 800 / (d["ms_per_step"] * 1e-3)) < 0.02 * d["value"]
    assert not set(FULL_ONLY) & set(d), sorted(set(FULL_ONLY) & set(d))
