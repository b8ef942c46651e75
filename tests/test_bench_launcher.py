"""bench.py's multi-rank launcher: ``python bench.py --gpus N`` must run N
ranks and report n_gpus = N, never silently one.  CPU only: the --dry-run mode goes through the
same launch (torch.distributed.run child), rendezvous (gloo), barrier and max-over-ranks timing as
the GPU run, around a CPU stand-in step.  One GPU case: a plain run prints the headline only and
``--dump-outputs`` writes the last timed step's arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK",
                                                             "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=240)


def _line(out):
    return json.loads([ln for ln in out.strip().splitlines() if ln.startswith("{")][-1])


def test_gpus2_launches_two_ranks():
    r = _run(["--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = _line(r.stdout)
    assert d["n_gpus"] == 2 and d["dry_run"] and d["ranks_launched_by_bench"]
    assert d["steps"] == 3 and d["value"] > 0


def test_gpus1_runs_in_process():
    r = _run(["--gpus", "1", "--dry-run", "--steps", "2", "--warmup", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = _line(r.stdout)
    assert d["n_gpus"] == 1 and not d["ranks_launched_by_bench"]


def test_world_size_must_agree_with_gpus():
    r = _run(["--gpus", "2", "--dry-run"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "disagrees with WORLD_SIZE" in r.stderr


def test_too_few_gpus_refused():
    # this container has no GPU: a real (non dry-run) --gpus 2 must refuse before launching anything
    r = _run(["--gpus", "2"])
    assert r.returncode != 0 and "GPU(s) visible" in r.stderr


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dumps_outputs(tmp_path):
    """Without --full no other leg runs (their objects are absent from the line); --steps sets the
    timed steps; the dump holds what tt2_synthesize_dev returned: float32, every decoded frame."""
    B, n = 3, 8
    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", str(B), "--chars", "20",
              "--ref-frames", "64", "--t-out", str(n), "--dump-outputs", str(tmp_path / "out")])
    assert r.returncode == 0, r.stderr[-2000:]
    d = _line(r.stdout)
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "mel-frames/s" and d["higher_is_better"] and d["dtype"] == "f32" and not d["full"]
    for leg in ("roofline", "cpu_baseline", "wavenet", "e2e", "griffin_lim", "train", "variants"):
        assert leg not in d, leg
    frames = int(np.load(str(tmp_path / "out" / "decoded_frames.npy"))[0])
    assert frames == d["config"]["decoded_steps"] and 1 <= frames <= n
    mel = np.load(str(tmp_path / "out" / "mel_outputs.npy"))
    stop = np.load(str(tmp_path / "out" / "stop_tokens.npy"))
    assert mel.dtype == np.float32 and mel.shape == (B, frames, 80) and np.isfinite(mel).all()
    assert stop.dtype == np.float32 and stop.shape == (B, frames) and np.isfinite(stop).all()
    # clip_outputs: [-max_abs_value - lower_bound_decay, max_abs_value]; and not a blank buffer
    assert np.abs(mel).max() <= 4.1 and mel.std() > 0
