"""A plain bench.py run on the GPU: the headline line only (no companion lines, no CPU baseline), --steps timed
steps, and --dump-outputs writing what the last timed step returned (small batch, two steps)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, M, T_MAX = 64, 1024, 512, 25


def test_plain_run_dumps_last_step_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SG_AMP_")}
    dump = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", str(B), "--dump-outputs", str(dump), "--detail-dir", str(tmp_path / "detail")],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["unit"] == "codewords/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - B) < 1e-6 * B
    assert line["companions"] == {} and line["cpu_baseline"] is None
    assert sorted(os.listdir(dump)) == ["error_counts.npy", "map_idx.npy", "t_final.npy"]
    mi, tf, cnt = (np.load(dump / f) for f in ("map_idx.npy", "t_final.npy", "error_counts.npy"))
    assert mi.dtype == np.float32 and mi.shape == (B, L) and tf.dtype == np.float32 and tf.shape == (B,)
    assert cnt.dtype == np.float64 and cnt.shape == (4,)
    assert np.array_equal(mi, np.round(mi)) and mi.min() >= 0 and mi.max() < M
    assert tf.min() >= 1 and tf.max() <= T_MAX
    # the counters belong to the same step as the decisions: section errors <= B L, codeword errors <= B
    assert 0 <= cnt[0] <= B * L and 0 <= cnt[2] <= B
    with open(tmp_path / "detail" / os.path.basename(line["detail"])) as f:
        full = json.load(f)
    assert full["amp"]["section_errors"] == int(cnt[0]) and full["amp"]["codeword_errors"] == int(cnt[2])
    assert not any(k in full for k in ("amp_r13", "amp_f64", "bp", "sc", "sc_notebook", "concat"))
