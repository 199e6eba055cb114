"""GPU: a plain `bench.py` run measures the headline only and times exactly --steps steps; --dump-outputs writes the scores the timed
path returned in its last step (checked against the oracle on the same seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ivos_w_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16_SCORE_RTOL = 4e-3      # the bf16 mode's stated tolerance (tests/test_gpu_assess.py)


def test_plain_bench_line_and_dumped_scores(tmp_path):
    out = tmp_path / "outputs"
    B, steps = 8, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--min-warm-s", "0",
                        "--batch", str(B), "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert (d["metric"], d["unit"], d["higher_is_better"], d["dtype"]) == ("assessed_frames_per_sec", "frames/s", True, "bf16")
    assert d["steps"] == steps and d["warmup"] == 1 and d["n_gpus"] == 1
    assert abs(d["value"] - B * 1e3 / d["ms_per_step"]) < 0.01 * d["value"]          # value and ms_per_step describe the same timed steps
    moved = {"roofline", "sustained", "checked", "check", "front", "fp32", "bf16x3", "dqn", "recommend_frame", "jf", "seg_epilogue", "cpu_baseline"}
    assert not moved & set(d), moved & set(d)                                          # those belong to a --full run
    scores = np.load(out / "scores.npy")
    assert scores.dtype == np.float32 and scores.shape == (B, 1)
    from oracle import assess_oracle as ao
    tf, tp = synth.assess_inputs(B, seed=1234)                                         # bench.py's rank-0 inputs (one block of <= 32 frames)
    ref = ao.assess_forward(ao.to_torch_sd(synth.assessnet_state_dict(0)), tf, tp).reshape(-1)
    np.testing.assert_allclose(scores.reshape(-1), ref, rtol=BF16_SCORE_RTOL)
