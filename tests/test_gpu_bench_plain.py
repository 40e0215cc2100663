"""GPU: a plain `bench.py` run (no --full) times exactly --steps steps in one window, prints the headline fields, and with
--dump-outputs writes what its last timed step returned -- the same ids the line's `captions_sha256` hashes, identical from run to run."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "8", "--warmup", "2", "--batch", "16",
                        "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs(tmp_path):
    from conette_amd.dist import trim_captions
    d = _run(tmp_path / "a")
    assert d["metric"] == "clips_per_sec" and d["unit"] == "clips/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["steps"] == 8 and d["repeat"] == 1 and d["full"] is False
    assert "roofline" not in d and "cpu_baseline" not in d and "parity" not in d and "also_pipelined" not in d
    assert abs(d["timed_region_s"] * 1e3 - 8 * d["ms_per_step"]) < 0.01 * d["timed_region_s"] * 1e3 + 1e-3
    assert abs(d["value"] - 16 * 8 / d["timed_region_s"]) < 1e-2 * d["value"]
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("preds", "lprobs", "clip_probs")}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["clip_probs.npy", "lprobs.npy", "preds.npy"]
    assert got["preds"].shape == (16, 20) and got["lprobs"].shape == (16,) and got["clip_probs"].shape == (16, 527)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert np.all((got["clip_probs"] >= 0) & (got["clip_probs"] <= 1)) and np.all(got["lprobs"] <= 0)
    ids = trim_captions(torch.from_numpy(got["preds"].astype(np.int32)))
    assert hashlib.sha256(ids.to(torch.int32).contiguous().numpy().tobytes()).hexdigest() == d["captions_sha256"]
    d2 = _run(tmp_path / "b")
    assert d2["captions_sha256"] == d["captions_sha256"]
    for n, a in got.items():
        assert np.array_equal(np.load(tmp_path / "b" / (n + ".npy")), a), n
