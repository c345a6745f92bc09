"""The four-role env-step boundary of k_rollout<false, false>.

At every chunk boundary the workgroup packs the envs that finish or start an
env-step ("jobs", in lane order) onto lanes, 64 to a pass: job j of a pass is
lane j of every wave.  Wave 0 finishes the env-step (salp::finish_core, the
actions / rewards / dones rows, after the barrier the reset with the draw
wave 3 left in LDS, salp::apply_step, the stores); wave 1 computes the
observation from the slot and the cold block, stores the obs row, fills the
float32 geometry cache of the next step and, after the barrier, stores the
obs_before row: the same observation when wave 0 says the episode goes on,
the reset state's, computed from the draw, when it ended; wave 2 plans the
next step's nozzle angles and direction; wave 3 draws the reset of every
finishing job
(csrc/salp_kernels.hip, role_boundary).  A lane that took the wrong slot, an
observation of the wrong state or in the wrong row, a draw of the wrong
episode, an obs_before row written for an episode that ended (or not written
for one that went on), a plan or a row past a max_steps end, or a wave that
misses a barrier shows as a state, steps_done or buffer row that differs from
the C oracle (oracle/sampled.py), checked here for every env bit for bit.

Every handle selects k_rollout explicitly (set_rollout_kernel(0)): at these
sizes the auto choice is the two-wave kernel, which has no such boundary.

Shapes (max_cycles = 2, so nearly every boundary holds a reset; a 3-slot
buffer that wraps; three launches of 1 024 ticks on one handle, chunk 8 and
64):

* 64 envs: a launch's first boundary is exactly one full pass;
* 65 envs: a second pass with a single job;
* 129 envs: three passes, the last with a single job;
* 257 envs: four full passes in the first workgroup, and a second workgroup
  with one env beside 255 empty slots;
* 257 envs with max_steps = 5: the fifth env-step gets no plan and no
  obs_before row, and the workgroups leave through all_done;
* 129 envs with `obs` but no `obs_before`, and with `obs_before` but no
  `obs`: the observe wave stores only the rows that exist; the state, the
  step counts and the four buffers the run has are checked against the oracle.

Chained zero-tick cycles (a new cycle that has already ended takes another
round on its lanes) need an action whose contraction and coast time are both
zero; the uniform random actions of these seeds need not contain one, and the
oracle's replay reports ticks per env, not per cycle, so these tests do not
claim to cover the extra rounds.

Reference path: src/salp_robot_env.py:196-299 per env-step, :114-155 and
:449-559 per reset, :651-670 per observation.
"""
import numpy as np
import pytest
import torch

from grasp_lab_salp_amd._abi import default_params
from grasp_lab_salp_amd.batched_env import BatchedSalpEnv
from oracle import sampled

pytestmark = pytest.mark.gpu

SEED = 11
MAX_CYCLES = 2   # an episode is truncated after two env-steps: every launch crosses episode ends
ALL = ("obs", "obs_before", "actions", "rewards", "dones")


def _params():
    p = default_params()
    p.max_cycles = MAX_CYCLES
    return p


def _buffers(cap, n, obs_dim, names=ALL):
    shapes = {"obs": ((cap, n, obs_dim), torch.float32), "obs_before": ((cap, n, obs_dim), torch.float32),
              "actions": ((cap, n, 3), torch.float32), "rewards": ((cap, n), torch.float32),
              "dones": ((cap, n), torch.uint8)}
    return {k: torch.zeros(shapes[k][0], dtype=shapes[k][1], device="cuda") for k in names}


def _check(env, done, bufs, p, n):
    st = env.get_state().cpu().numpy()
    dn = done.cpu().numpy()
    res = sampled.check(st, dn, {k: v.cpu().numpy() for k, v in bufs.items()}, p, SEED, ids=np.arange(n))
    print(res)
    assert res["envs_checked"] == n
    assert res["buffer_rows_checked"] > 0
    assert res["ok"], res
    return res, dn


def _run(n, chunk, names=ALL):
    p = _params()
    env = BatchedSalpEnv(n, params=p, seed=SEED)
    env.set_rollout_kernel(0)   # k_rollout<false, false>
    bufs = _buffers(3, n, env.obs_dim, names)
    done = torch.zeros(n, dtype=torch.int64, device="cuda")
    for _ in range(3):
        env.rollout(1024, buffers=bufs, steps_done=done, chunk=chunk)
    torch.cuda.synchronize()
    return env, done, bufs, p


def _check_launches(env, done, bufs, p, n):
    res, dn = _check(env, done, bufs, p, n)
    assert int(dn.min()) > 0, "an env finished no env-step"
    assert (dn > MAX_CYCLES).any(), "no env got past its first episode"
    assert res["pending_checked"] > 0, "cycles in flight at the end of the third launch"
    return dn


@pytest.mark.parametrize("chunk", [8, 64])
@pytest.mark.parametrize("n", [64, 65, 129, 257])
def test_four_roles_across_episode_ends_match_oracle(n, chunk):
    env, done, bufs, p = _run(n, chunk)
    dn = _check_launches(env, done, bufs, p, n)
    assert (dn[256:] > MAX_CYCLES).any() or n <= 256, "no env of the second workgroup got past its first episode"
    assert int(bufs["dones"].sum()) > 0, "no episode end among the last buffer rows"


@pytest.mark.parametrize("chunk", [8, 64])
def test_four_roles_with_max_steps_plan_nothing_past_the_last_step(chunk):
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
    assert res["pending_checked"] == 0, "an env began a step past max_steps"


@pytest.mark.parametrize("names", [("obs", "actions", "rewards", "dones"),
                                   ("obs_before", "actions", "rewards", "dones")],
                         ids=["obs_only", "obs_before_only"])
def test_observe_role_stores_only_the_rows_that_exist(names):
    n, chunk = 129, 8
    # the run with every buffer, checked against the oracle, lends the missing buffer
    # to the oracle's check of the run without it (sampled.check reads all five)
    env, done, full, p = _run(n, chunk)
    _check_launches(env, done, full, p, n)
    env, done, bufs, p = _run(n, chunk, names)
    missing = [k for k in ALL if k not in names]
    assert len(missing) == 1 and missing[0] not in bufs
    _check_launches(env, done, {**full, **bufs}, p, n)
