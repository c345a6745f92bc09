"""What k_rollout carries across its call of wave_ticks in registers.

wave_ticks<false> saves no register for its caller (csrc/salp_kernels.hip:
local linkage plus [[clang::not_tail_called]], so LLVM's interprocedural
register allocation drops the callee saves and tells the caller exactly what
the callee clobbers).  The kernel therefore keeps its slot, env index, pending /
active flags and step count in registers that only the compiler's clobber mask
protects, where the build before kept them safe behind 132 saved registers.  A
wrong mask would show as an env continuing in another slot, a lost or doubled
env-step, or a rollout-buffer row written for the wrong env.

Every handle selects k_rollout explicitly (set_rollout_kernel(0)): at these
sizes the auto choice is the two-wave kernel, which has no such call.

* 257 envs (a full workgroup, then one lane beside 255 empty slots) and 64
  envs (one wave beside three empty ones), chunk 8 and 64, three launches on
  one handle with max_cycles = 2 so that episodes end and envs reset inside
  the run, a 3-slot buffer that wraps: state, steps_done and buffer rows of
  every env against the C oracle bit for bit (oracle/sampled.py);
* the same with max_steps, so that workgroups leave through all_done;
* salp_collect on kernel 0 (k_rollout<false, true>, the instance whose call
  site once carried the `tail` marker), every env replayed on the oracle.

Reference path: src/salp_robot_env.py:196-299 per env-step, src/robot.py:740-777
per cycle.
"""
import numpy as np
import pytest
import torch

from grasp_lab_salp_amd._abi import default_params
from grasp_lab_salp_amd.batched_env import BatchedSalpEnv
from grasp_lab_salp_amd.ppo import DIVERGED_OBS_ABS, DIVERGED_REWARD_ABS, ActorCritic, pack_policy
from oracle import sampled

pytestmark = pytest.mark.gpu

SEED = 11
MAX_CYCLES = 2   # an episode is truncated after two env-steps: every launch crosses episode ends


def _params():
    p = default_params()
    p.max_cycles = MAX_CYCLES
    return p


def _buffers(cap, n, obs_dim):
    return {"obs": torch.zeros((cap, n, obs_dim), dtype=torch.float32, device="cuda"),
            "obs_before": torch.zeros((cap, n, obs_dim), dtype=torch.float32, device="cuda"),
            "actions": torch.zeros((cap, n, 3), dtype=torch.float32, device="cuda"),
            "rewards": torch.zeros((cap, n), dtype=torch.float32, device="cuda"),
            "dones": torch.zeros((cap, n), dtype=torch.uint8, device="cuda")}


def _check(env, done, bufs, p, n):
    st = env.get_state().cpu().numpy()
    dn = done.cpu().numpy()
    res = sampled.check(st, dn, {k: v.cpu().numpy() for k, v in bufs.items()}, p, SEED, ids=np.arange(n))
    print(res)
    assert res["envs_checked"] == n
    assert res["buffer_rows_checked"] > 0
    assert res["ok"], res
    return res, dn


@pytest.mark.parametrize("chunk", [8, 64])
@pytest.mark.parametrize("n", [257, 64])
def test_rollout_across_episode_ends_matches_oracle(n, chunk):
    p = _params()
    env = BatchedSalpEnv(n, params=p, seed=SEED)
    env.set_rollout_kernel(0)   # k_rollout<false, false>
    bufs = _buffers(3, n, env.obs_dim)
    done = torch.zeros(n, dtype=torch.int64, device="cuda")
    for _ in range(3):
        env.rollout(1024, buffers=bufs, steps_done=done, chunk=chunk)
    torch.cuda.synchronize()
    res, dn = _check(env, done, bufs, p, n)
    assert (dn > MAX_CYCLES).any(), "no env got past its first episode"
    assert int(bufs["dones"].sum()) > 0, "no episode end among the last buffer rows"
    assert res["pending_checked"] > 0, "cycles in flight at the end of the third launch"


@pytest.mark.parametrize("chunk", [8, 64])
def test_rollout_with_max_steps_leaves_through_all_done(chunk):
    n, steps = 257, 5
    p = _params()
    env = BatchedSalpEnv(n, params=p, seed=SEED)
    env.set_rollout_kernel(0)
    bufs = _buffers(3, n, env.obs_dim)
    done = torch.zeros(n, dtype=torch.int64, device="cuda")
    env.rollout(10**6, buffers=bufs, steps_done=done, max_steps=steps, chunk=chunk)
    torch.cuda.synchronize()
    res, dn = _check(env, done, bufs, p, n)
    assert int(dn.min()) == steps and int(dn.max()) == steps
    assert res["buffer_rows_checked"] == 3 * n


def test_collect_on_the_plain_kernel_matches_oracle():
    n, n_steps = 257, 6
    p = _params()
    env = BatchedSalpEnv(n, params=p, seed=SEED)
    env.set_rollout_kernel(0)   # k_rollout<false, true>
    torch.manual_seed(1)
    pol = ActorCritic(env.obs_dim, 3).cuda()
    with torch.no_grad():
        pol.action_net.weight.mul_(60.0)   # actions spread over the box: cycles of many lengths
        pol.log_std.copy_(torch.tensor([-0.7, -0.4, -0.2]))
    w = pack_policy(pol)
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")  # noqa: E731
    bufs = {"obs": z(n_steps, n, env.obs_dim), "actions": z(n_steps, n, 3), "rewards": z(n_steps, n),
            "episode_starts": z(n_steps, n), "values": z(n_steps, n), "log_probs": z(n_steps, n)}
    ep_start = torch.ones(n, dtype=torch.float32, device="cuda")
    last_obs = env.reset()
    state0, obs0 = env.get_state().cpu().numpy(), last_obs.cpu().numpy()
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    div = torch.zeros(1, dtype=torch.int64, device="cuda")
    env.collect(w, n_steps, bufs, ep_start, last_obs, stats, div, noise_seed=7, gamma=0.99,
                diverged_obs_abs=DIVERGED_OBS_ABS, diverged_reward_abs=DIVERGED_REWARD_ABS)
    torch.cuda.synchronize()
    res = sampled.check_collect(state0, obs0, {k: bufs[k].cpu().numpy() for k in ("obs", "actions", "rewards",
                                                                                  "episode_starts")},
                                last_obs.cpu().numpy(), env.get_state().cpu().numpy(), p, SEED, block=n,
                                guard=(DIVERGED_OBS_ABS, DIVERGED_REWARD_ABS))
    print(res)
    assert res["envs_checked"] == n and res["env_steps_replayed"] == n * n_steps
    assert float(bufs["episode_starts"][1:].sum()) > 0, "no episode ended inside the collection"
    assert res["ok"], res
