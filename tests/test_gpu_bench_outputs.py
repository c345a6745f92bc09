"""A plain bench.py run and its --dump-outputs files.

One small run (2 048 envs, 1 warm-up + 2 timed launches of 2 048 ticks) as a
child process; the files it writes are compared bit for bit with the same
launches made here on a fresh handle (non-finite elements of diverged envs: 0 in
the file, their kind in <name>_nonfinite), and the result line holds the headline
keys and none of the --full legs.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, BUDGET, CAP, CHUNK, SEED, WARMUP, STEPS = 2048, 2048, 4, 64, 3, 1, 2
FLOATING = ("obs", "obs_before", "actions", "rewards", "state")
NAMES = FLOATING + tuple(n + "_nonfinite" for n in FLOATING) + ("dones", "steps_done", "env_ids")


@pytest.mark.gpu
@pytest.mark.timeout(180)
def test_plain_run_dumps_what_the_timed_path_computed(tmp_path):
    import torch
    from grasp_lab_salp_amd._abi import NUM_FIELDS, default_params
    from grasp_lab_salp_amd.batched_env import BatchedSalpEnv

    out = tmp_path / "dump"
    env_vars = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
           str(WARMUP), "--n-envs", str(N), "--tick-budget", str(BUDGET), "--capacity", str(CAP), "--chunk",
           str(CHUNK), "--seed", str(SEED), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=150, env=env_vars, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    res = json.loads(lines[0])
    assert res["steps"] == STEPS and res["warmup"] == WARMUP and res["full"] is False
    assert res["unit"] == "env-steps/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["value"] > 0 and res["ms_per_step"] > 0
    for leg in ("parity_sampled", "ppo", "cpu_baseline", "divergence"):
        assert leg not in res
    assert not res["lockstep_env_steps_per_sec"] and res["steady_state_env_steps_per_sec"] is None

    got = {name: np.load(out / (name + ".npy")) for name in NAMES}
    assert sorted(os.listdir(out)) == sorted(name + ".npy" for name in NAMES)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    ids = got["env_ids"].astype(np.int64)
    assert np.array_equal(ids, np.arange(N))   # a batch this small is written whole

    # the same launches on a fresh handle
    dev = torch.device("cuda", 0)
    env = BatchedSalpEnv(N, params=default_params(), seed=SEED, device=0)
    bufs = {"obs": torch.zeros((CAP, N, env.obs_dim), dtype=torch.float32, device=dev),
            "obs_before": torch.zeros((CAP, N, env.obs_dim), dtype=torch.float32, device=dev),
            "actions": torch.zeros((CAP, N, 3), dtype=torch.float32, device=dev),
            "rewards": torch.zeros((CAP, N), dtype=torch.float32, device=dev),
            "dones": torch.zeros((CAP, N), dtype=torch.uint8, device=dev)}
    done = torch.zeros(N, dtype=torch.int64, device=dev)
    for _ in range(WARMUP + STEPS):
        env.rollout(BUDGET, buffers=bufs, steps_done=done, chunk=CHUNK)
    want = {k: v.cpu().numpy() for k, v in bufs.items()}
    want["steps_done"] = done.cpu().numpy()
    want["state"] = env.get_state().cpu().numpy()
    env.close()
    assert got["state"].shape == (NUM_FIELDS, N) and got["steps_done"].sum() > 0
    for name, w in want.items():
        assert got[name].shape == w.shape, name
        if name not in FLOATING:
            assert np.array_equal(got[name], w.astype(got[name].dtype)), name
            continue
        assert got[name].dtype == w.dtype, name
        code = np.select([np.isnan(w), w == np.inf, w == -np.inf], [1.0, 2.0, 3.0], 0.0).astype(np.float32)
        assert np.array_equal(got[name + "_nonfinite"], code), name
        assert np.array_equal(got[name], np.where(code == 0, w, 0).astype(w.dtype)), name
    # the run is long enough for some env to diverge, so the non-finite path is exercised
    assert got["state_nonfinite"].any() and got["obs_nonfinite"].any()
