"""GPU: a plain `python bench.py` run -- set-up, warm-up, the timed steps, the outputs of the last one (--dump-outputs) and the
headline line, nothing else (the secondary measurements need --full) -- and the reproducibility of what it dumps."""
import os
import sys

import numpy as np
import pytest

from _child import GPU, json_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDARY = ("sync_actions", "h2d_inclusive", "plugin_path", "cpu_baseline", "weak", "phases", "allreduce_exposed")


def _plain(out_dir):
    # 64 actors = two actor slices on two streams, as at the headline size
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--actors", "64", "--rollout", "8", "--steps", "2",
           "--warmup", "1", "--dump-outputs", out_dir]
    r = GPU.run(cmd, drop=("RANK", "WORLD_SIZE", "LOCAL_RANK"), limit=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = json_lines(r)
    assert len(lines) == 1, r.stdout[-3000:]
    return lines[0]


def test_plain_bench_run_dumps_the_last_step_reproducibly(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = _plain(a)
    assert line["unit"] == "env-frames/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["metric"].startswith("env-frames/sec") and line["steps"] == 2 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and abs(line["value"] - 8 * 64 / (line["ms_per_step"] * 1e-3)) <= 1e-2 * line["value"]
    assert not any(k in line for k in SECONDARY), sorted(line)
    names = sorted(os.listdir(a))
    assert names == sorted(n + ".npy" for n in ("policy_params", "actions", "log_probs", "values", "returns", "advantages",
                                                 "hidden_state", "features_sample", "loss")), names
    assert sum(os.path.getsize(os.path.join(a, n)) for n in names) < 64 << 20
    got = {n: np.load(os.path.join(a, n)) for n in names}
    assert got["actions.npy"].shape == (8, 64) and got["values.npy"].shape == (9, 64)
    # the whole flat parameter vector: 3,480,775 parameters (+ the flat layout's padding), not a sample
    assert 3_480_775 <= got["policy_params.npy"].shape[0] < 3_480_775 + 64 and got["loss.npy"].dtype == np.float64
    assert set(np.unique(got["actions.npy"])) <= set(range(6))
    assert all(np.isfinite(v).all() for v in got.values())
    assert np.abs(got["features_sample.npy"]).max() > 0
    # same arguments -> same inputs; the step is bit-reproducible (tests/test_gpu_engine.py), so the outputs are equal
    _plain(b)
    for n in names:
        assert np.array_equal(got[n], np.load(os.path.join(b, n))), n
