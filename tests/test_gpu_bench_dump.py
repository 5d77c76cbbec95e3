"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` run, as a
fresh process on a tiny TD update: the learner took K timed updates after W warm-ups, the
line carries ms_per_step and none of --full's legs, and DIR holds what the last
timed step returned (plus the stepped parameters) as finite float32 arrays of the
update's shapes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.gpu_util import require_gpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_dumps_the_last_steps_outputs(tmp_path):
    require_gpu()
    B, T, A, K = 16, 6, 8, 3
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "1",
           "--batch", str(B), "--T", str(T), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == K and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["updates_done"] == K + 1  # counted by the learner (its Adam step count): 1 warm-up + K timed updates
    assert d["ms_per_step"] > 0 and abs(d["value"] - B * T * A / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert not {"cpu_baseline", "fp32_companion", "configs"} & set(d)
    got = {p.name[:-4]: np.load(p) for p in out.iterdir()}
    assert set(got) == {"td_errors_abs", "loss_sum", "mask_sum", "grad_norm", "qtot", "targets", "params"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["qtot"].shape == (B, T) and got["targets"].shape == (B, T) and got["td_errors_abs"].size == B
    assert float(got["mask_sum"].reshape(-1)[0]) == B * T  # the synthetic batch: every step filled, none terminal
    assert got["params"].ndim == 1 and float(got["grad_norm"].reshape(-1)[0]) > 0
    assert sum(a.nbytes for a in got.values()) <= 64 * 2 ** 20
    print("bench --dump-outputs:", {k: v.shape for k, v in sorted(got.items())})
