"""salp_collect_episodes and salp_episode_window_push_log on the GPU.

The chained kernels' episode log is checked against a twin handle stepped in
lock-step with salp_step on the collection's clipped actions, as
tests/test_gpu_collect.py replays the buffers: every finished episode's window
row, the step it ended in and the per-env counts must match the twin's info
rows bit for bit, and the merged window must equal the window the lock-step
callback's per-step pushes build whenever the merge reports nothing lost.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from grasp_lab_salp_amd import _lib
from grasp_lab_salp_amd._abi import FIELD, INFO, default_params
from grasp_lab_salp_amd.batched_env import BatchedSalpEnv
from grasp_lab_salp_amd.callbacks import DetailedMetricsCallback
from grasp_lab_salp_amd.metrics import EpisodeLog, EpisodeWindow, torch_episode_window_push_log
from grasp_lab_salp_amd.ppo import DIVERGED_OBS_ABS, DIVERGED_REWARD_ABS, PPO, pack_policy
from grasp_lab_salp_amd.vec_env import SalpVecEnv
from test_gpu_bounds import Guarded
from test_gpu_collect import ALL_RAND, _buffers, _cpu, _equal_up_to_nan_payload, _policy

pytestmark = pytest.mark.gpu

COLS = _lib.EPWIN_COLS
N_STEPS = 24
NEAR = (0, 3, 64)    # envs whose target is put beside the body: they terminate at once
FAR = 7              # an env put far outside the world: its first step trips the divergence guard
_FIRST, _LAST = INFO["path_length"], INFO["avg_rewards_obstacle"]


def _pair(n, rand=False, max_cycles=3, seed=23):
    """Two handles in one state: a few targets beside the body (episodes that
    terminate), one env far away (a step the guard drops)."""
    p = default_params()
    p.max_cycles = max_cycles
    env = BatchedSalpEnv(n, params=p, seed=seed)
    twin = BatchedSalpEnv(n, params=p, seed=seed)
    if rand:
        env.set_randomization(**ALL_RAND)
        twin.set_randomization(**ALL_RAND)
    obs0 = env.reset()
    s = env.get_state()
    for i in NEAR:
        if i < n:
            s[FIELD["target0"], i] = s[FIELD["pos0"], i] + 0.05
            s[FIELD["target1"], i] = s[FIELD["pos1"], i]
    s[FIELD["pos0"], FAR] = 1.0e6
    env.set_state(s)
    twin.set_state(s)
    return env, twin, obs0


class _Call:
    """The in/out tensors of one salp_collect call sequence on a handle."""

    def __init__(self, env, obs0, n_steps=N_STEPS):
        n = env.n_envs
        self.env, self.n_steps = env, n_steps
        self.bufs = _buffers(n_steps, n, env.obs_dim)
        self.ep_start = torch.ones(n, dtype=torch.float32, device="cuda")
        self.last_obs = obs0.clone()
        self.ep_stats = torch.zeros(4, dtype=torch.float64, device="cuda")
        self.diverged = torch.zeros(1, dtype=torch.int64, device="cuda")

    def collect(self, w, log=None):
        self.env.collect(w, self.n_steps, self.bufs, self.ep_start, self.last_obs, self.ep_stats, self.diverged,
                         noise_seed=99, gamma=0.99, diverged_obs_abs=DIVERGED_OBS_ABS,
                         diverged_reward_abs=DIVERGED_REWARD_ABS, episode_log=log)
        torch.cuda.synchronize()
        self.env.check_pair()   # no partner wait of a two-wave collection may give up


def _window_rows(info, term, trunc):
    """The window row of include/salp.h from one env-step's info rows (bit copies)."""
    t = term.bool()
    return torch.cat([info[:, INFO["ep_return"]:INFO["ep_return"] + 1], info[:, INFO["ep_len"]:INFO["ep_len"] + 1],
                      t.double().unsqueeze(1), (trunc.bool() & ~t).double().unsqueeze(1), info[:, _FIRST:_LAST + 1]], 1)


def _twin_steps(twin, actions, windows):
    """Step the twin on the buffer's clipped actions with the learner's guard;
    after every step push into each of ``windows`` as the lock-step callback
    does.  Returns the finished episodes [(t, env, row [20])] in push order and
    what kinds of step were seen."""
    clipped = torch.clamp(actions, torch.tensor([0.0, 0.0, -1.0], device="cuda"),
                          torch.tensor([1.0, 1.0, 1.0], device="cuda"))
    episodes, seen = [], {"terminated": 0, "truncated": 0, "dropped": 0, "dropped_at_an_end": 0}
    for t in range(actions.shape[0]):
        r = twin.step(clipped[t].contiguous(), auto_reset=True, want_terminal_obs=True)
        tob = r.terminal_obs
        bad = (~torch.isfinite(tob).all(1) | (tob.abs() > DIVERGED_OBS_ABS).any(1)
               | ~(r.reward.abs() <= DIVERGED_REWARD_ABS))
        done = r.terminated.bool() | r.truncated.bool()
        for win in windows:
            win.push(r.info, r.terminated.to(torch.uint8), r.truncated.to(torch.uint8), skip=bad.to(torch.uint8))
        ended = done & ~bad
        rows = _cpu(_window_rows(r.info, r.terminated, r.truncated))
        for i in np.flatnonzero(_cpu(ended)):
            episodes.append((t, int(i), rows[i].copy()))
        seen["terminated"] += int((ended & r.terminated.bool()).sum())
        seen["truncated"] += int((ended & ~r.terminated.bool()).sum())
        seen["dropped"] += int(bad.sum())
        seen["dropped_at_an_end"] += int((bad & done).sum())
        twin.reset(mask=bad & ~done)
    return episodes, seen


def _expected_log(episodes, n, K):
    rows = np.full((n, K, COLS), np.nan)
    step = np.full((n, K), -1, np.int32)
    count = np.zeros(n, np.int32)
    for t, i, row in episodes:
        rows[i, count[i] % K], step[i, count[i] % K] = row, t
        count[i] += 1
    return rows, step, count


@pytest.mark.parametrize("n,kernel,rand", [(65, 0, False), (65, 1, False), (65, 2, False), (300, 0, False),
                                           (300, 1, False), (300, 2, False), (300, -1, True)])
def test_log_and_window_replay_on_the_lockstep_path(n, kernel, rand):
    """rand: every randomisation switch on (k_rollout_log<true>)."""
    w = pack_policy(_policy(1))
    twin_windows = {W: EpisodeWindow(W) for W in (1, 7, 100)}
    episodes = seen = None
    some_lost = some_exact_beyond_the_window = False
    for K in (1, 3, N_STEPS):
        env, twin, obs0 = _pair(n, rand)
        env.set_rollout_kernel(kernel)
        call = _Call(env, obs0)
        log = EpisodeLog(n, K)
        call.collect(w, log)
        if episodes is not None:
            twin.close()
        else:   # the twin's replay is the same for every K: once
            episodes, seen = _twin_steps(twin, call.bufs["actions"], list(twin_windows.values()))
            # the conditions on the inputs
            assert seen["terminated"] > 0 and seen["truncated"] > 0, seen
            assert seen["dropped_at_an_end"] > 0, seen      # an episode end the guard dropped: it must not be logged
            assert max(np.bincount([i for _, i, _ in episodes], minlength=n)) > 3   # the rings of K = 1 and 3 wrap
            assert all(i != FAR or t > 0 for t, i, _ in episodes)
        D = len(episodes)
        want_rows, want_step, want_count = _expected_log(episodes, n, K)
        assert np.array_equal(_cpu(log.count), want_count)
        assert np.array_equal(_cpu(log.step), want_step)           # -1 where nothing was written
        assert _equal_up_to_nan_payload(_cpu(log.rows), want_rows)   # NaN where nothing was written
        assert int(call.ep_stats[1]) == D
        for W, twin_win in twin_windows.items():
            win = EpisodeWindow(W)
            win.push_log(log)
            assert int(win.count) == int(twin_win.count) == int(call.ep_stats[1])
            lost = int(win.lost)
            if K == N_STEPS:
                assert lost == 0 and D > W          # nothing can be dropped: exact beyond the window's length
                some_exact_beyond_the_window = True
            if lost == 0:
                assert _equal_up_to_nan_payload(_cpu(win.rows), _cpu(twin_win.rows)), (K, W)
            else:
                some_lost = True
            # the readable restatement agrees with the kernel bit for bit, lost or not
            ref = EpisodeWindow(W, fused=False)
            torch_episode_window_push_log(ref.rows, ref.count, ref.lost, log.rows, log.step, log.count)
            assert _equal_up_to_nan_payload(_cpu(win.rows), _cpu(ref.rows)), (K, W)
            assert int(ref.count) == int(win.count) and int(ref.lost) == lost
        env.close()
    assert some_lost and some_exact_beyond_the_window


def test_two_calls_on_one_handle_accumulate():
    """count is rewritten by the second call; the window accumulates across a count that is no multiple of W."""
    n, W, K = 65, 7, N_STEPS
    w = pack_policy(_policy(1))
    env, twin, obs0 = _pair(n)
    env.set_rollout_kernel(2)
    call, log, win, twin_win = _Call(env, obs0), EpisodeLog(n, K), EpisodeWindow(W), EpisodeWindow(W)
    total = 0
    for k in range(2):
        call.collect(w, log)
        episodes, _ = _twin_steps(twin, call.bufs["actions"], [twin_win])
        want_rows, want_step, want_count = _expected_log(episodes, n, K)
        assert np.array_equal(_cpu(log.count), want_count)      # this call's episodes alone
        kept = want_step >= 0
        assert np.array_equal(_cpu(log.step)[kept], want_step[kept])
        assert _equal_up_to_nan_payload(_cpu(log.rows)[kept], want_rows[kept])
        win.push_log(log)
        total += len(episodes)
        assert int(win.count) == int(twin_win.count) == total == int(call.ep_stats[1])
        assert int(win.lost) == 0
        assert _equal_up_to_nan_payload(_cpu(win.rows), _cpu(twin_win.rows))
        if k == 0:
            assert total % W != 0
    assert _equal_up_to_nan_payload(_cpu(env.get_state()), _cpu(twin.get_state()))


@pytest.mark.parametrize("kernel", [0, 2])
def test_log_off_equals_log_on(kernel):
    n = 300
    w = pack_policy(_policy(1))
    calls = []
    for logged in (False, True):
        env, twin, obs0 = _pair(n)
        twin.close()
        env.set_rollout_kernel(kernel)
        call = _Call(env, obs0)
        call.collect(w, EpisodeLog(n, 3) if logged else None)
        calls.append(call)
    off, on = calls
    for k in off.bufs:
        assert _equal_up_to_nan_payload(_cpu(off.bufs[k]), _cpu(on.bufs[k])), k
    assert _equal_up_to_nan_payload(_cpu(off.last_obs), _cpu(on.last_obs))
    assert torch.equal(off.ep_start, on.ep_start)
    assert int(off.diverged) == int(on.diverged) > 0
    # fp64 atomics arrive in another order
    assert np.allclose(_cpu(off.ep_stats), _cpu(on.ep_stats), rtol=1e-12, atol=1e-9) and float(off.ep_stats[1]) > 0
    assert _equal_up_to_nan_payload(_cpu(off.env.get_state()), _cpu(on.env.get_state()))


def _guarded_run(n, K, W, kernel):
    w = pack_policy(_policy(1))
    env, twin, obs0 = _pair(n)
    twin.close()
    env.set_rollout_kernel(kernel)
    call, log = _Call(env, obs0), EpisodeLog(n, K)
    g = {"rows": Guarded((n, K, COLS), torch.float64, math.nan), "step": Guarded((n, K), torch.int32, -1),
         "count": Guarded((n,), torch.int32, 77), "win_rows": Guarded((W, COLS), torch.float64, math.nan),
         "win_count": Guarded((1,), torch.int64, 5), "lost": Guarded((1,), torch.int64, 0)}
    log.rows, log.step, log.count = g["rows"].t, g["step"].t, g["count"].t
    call.collect(w, log)
    cw = _lib.SalpEpisodeWindow(W, 0, g["win_rows"].t.data_ptr(), g["win_count"].t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().salp_episode_window_push_log(ctypes.byref(cw), ctypes.byref(log.c_struct()), n,
                                                        g["lost"].ptr(), st))
    torch.cuda.synchronize()
    assert all(v.intact() for v in g.values()), [k for k, v in g.items() if not v.intact()]
    count = g["count"].t
    assert int(count.min()) >= 0 and int(count.max()) <= N_STEPS        # every env's 77 was rewritten
    unwritten = torch.arange(K, device="cuda").unsqueeze(0) >= count.unsqueeze(1)
    assert bool((g["step"].t[unwritten] == -1).all()) and bool(g["rows"].t[unwritten].isnan().all())
    assert bool((g["step"].t[~unwritten] >= 0).all()) and not bool(g["rows"].t[~unwritten][:, :4].isnan().any())
    assert int(g["win_count"].t) == 5 + int(count.sum()) == 5 + int(call.ep_stats[1])
    return {k: _cpu(v.t).copy() for k, v in g.items()}


@pytest.mark.parametrize("n,K,W,kernel", [(300, 3, 100, 0), (65, 1, 7, 2), (65, N_STEPS, 100, 1)])
def test_log_and_merge_write_inside_their_buffers_and_repeat(n, K, W, kernel):
    a, b = _guarded_run(n, K, W, kernel), _guarded_run(n, K, W, kernel)
    for k in a:
        assert _equal_up_to_nan_payload(a[k], b[k]), k   # no atomics on the log's path: the same bits


def test_entry_point_rejects_a_bad_log():
    """include/salp.h: per_env < 1 or a NULL member of a non-NULL log is SALP_EINVAL, with a message, no launch."""
    n = 64
    env = BatchedSalpEnv(n, seed=1)
    call = _Call(env, env.reset(), n_steps=4)
    w = pack_policy(_policy(0))
    for field, value in (("per_env", 0), ("per_env", -1), ("rows", None), ("step", None), ("count", None)):
        log = EpisodeLog(n, 2)
        c = log.c_struct()
        setattr(c, field, value)
        log.c_struct = lambda c=c: c
        with pytest.raises(_lib.SalpError, match="salp_collect_episodes"):
            call.collect(w, log)
    assert int(call.ep_stats[1]) == 0 and bool((call.bufs["obs"] == -7.0).all())   # nothing ran
    with pytest.raises(ValueError):
        call.collect(w, EpisodeLog(n + 1, 2))


def test_learner_runs_the_detailed_metrics_on_the_chained_collection(tmp_path):
    p = default_params()
    p.max_cycles = 3
    n, n_steps = 64, 16
    venv = SalpVecEnv(n, params=p, seed=5)
    model = PPO("MlpPolicy", venv, n_steps=n_steps, batch_size=256, n_epochs=1, seed=3, collect="chained",
                episode_log=True)
    assert model.episode_log == 100 and model._episode_log.per_env == n_steps
    cb = DetailedMetricsCallback(log_freq=n_steps)
    model.learn(3 * n_steps * n, callback=cb)
    assert len(model.history) == 3
    so_far = 0
    for row in model.history:
        so_far += row["episodes"]
        for key in ("custom/navigation/success_rate", "custom/path/efficiency", "reward/stats/total_mean"):
            assert key in row and np.isfinite(row[key]), (key, row)
        assert not row.get("custom/episodes_lost")
    assert cb.last_summary["n"] == min(100, so_far)
    assert int(cb.window.count) == so_far > 100 and int(cb.window.lost) == 0
    assert model.locals == {"episode_log": model._episode_log}
    path = model.save(tmp_path / "m")
    again = PPO.load(path, env=venv)
    assert again.episode_log == 100 and again._episode_log is not None
    assert PPO.load(path, env=venv, episode_log=0)._episode_log is None
    # without the log the callback is refused as before
    plain = PPO("MlpPolicy", venv, n_steps=n_steps, batch_size=256, n_epochs=1, seed=3, collect="chained")
    with pytest.raises(ValueError, match='DetailedMetricsCallback.*collect="lockstep"'):
        plain.learn(n_steps * n, callback=DetailedMetricsCallback(log_freq=n_steps))
    assert plain.locals == {}
