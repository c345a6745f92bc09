"""grasp_lab_salp_amd/callbacks.py on the host: when each callback fires, the
SB3 file names, the best-model rule and the evaluations file, on a stub model
that counts ``save`` and ``evaluate`` calls (no GPU, no simulator)."""
import os

import numpy as np
import pytest
import torch

from grasp_lab_salp_amd import callbacks as cbs
from grasp_lab_salp_amd._abi import INFO_DIM


class _Model:
    """What the callbacks use of a learner: 4 envs per call."""

    n_envs, fused, device = 4, False, torch.device("cpu")

    def __init__(self, eval_means=()):
        self.num_timesteps = 0
        self.env = object()
        self.saved, self.replays, self.evals = [], [], []
        self.callback_metrics, self.locals, self.last_eval = {}, {}, None
        self._means = list(eval_means)

    def record(self, key, value):
        self.callback_metrics[key] = value

    def save(self, path):
        path = path if os.path.splitext(path)[1] else path + ".zip"
        open(path, "w").close()
        self.saved.append((self.num_timesteps, path))

    def save_replay_buffer(self, path):
        open(path, "w").close()
        self.replays.append(path)

    def evaluate(self, env, n_eval_episodes=10, deterministic=True, return_episode_rewards=False):
        mean = self._means[len(self.evals)]
        self.evals.append((self.num_timesteps, env, n_eval_episodes, deterministic))
        returns = [mean - 1.0, mean + 1.0] + [mean] * (n_eval_episodes - 2)
        self.last_eval = {"successes": [True] + [False] * (n_eval_episodes - 1)}
        assert return_episode_rewards
        return returns, list(range(1, n_eval_episodes + 1))

    def step(self, terminated=None):
        n = self.n_envs
        self.num_timesteps += n
        z = torch.zeros(n, dtype=torch.uint8)
        self.locals = {"info": torch.ones((n, INFO_DIM), dtype=torch.float64),
                       "terminated": z if terminated is None else terminated, "truncated": z, "diverged": z}


def _run(model, cb, calls, **kw):
    cb.init_callback(model)
    cb.on_training_start({}, {})
    out = []
    for _ in range(calls):
        model.step(**kw)
        out.append(cb.on_step())
    cb.on_training_end()
    return out


class _EvalEnv:
    """Passes for a vector env of this package: the attributes EvalCallback looks for."""

    n_envs, obs_dim, params, device = 5, 10, None, torch.device("cpu")

    def step(self):
        pass

    def reset(self):
        pass


def test_checkpoint_callback_fires_every_save_freq_with_sb3_names(tmp_path):
    m = _Model()
    cb = cbs.CheckpointCallback(save_freq=3, save_path=str(tmp_path / "models"), name_prefix="salp_robot_v5")
    assert all(_run(m, cb, 10))
    assert cb.n_calls == 10 and cb.num_timesteps == 40
    names = [f"salp_robot_v5_{t}_steps.zip" for t in (12, 24, 36)]                # calls 3, 6, 9 of 4 envs
    assert [(t, os.path.basename(p)) for t, p in m.saved] == list(zip((12, 24, 36), names))
    assert sorted(os.listdir(tmp_path / "models")) == sorted(names) and not m.replays
    m = _Model()
    cb = cbs.CheckpointCallback(2, str(tmp_path / "b"), save_replay_buffer=True)
    _run(m, cb, 4)
    assert sorted(os.listdir(tmp_path / "b")) == ["rl_model_16_steps.zip", "rl_model_8_steps.zip",
                                                  "rl_model_replay_buffer_16_steps.pt",
                                                  "rl_model_replay_buffer_8_steps.pt"]


def test_eval_callback_keeps_the_best_model_and_grows_the_log(tmp_path):
    m = _Model(eval_means=[1.0, 3.0, 3.0, 2.0, 5.0])
    env = _EvalEnv()
    cb = cbs.EvalCallback(env, best_model_save_path=str(tmp_path / "best"), log_path=str(tmp_path / "logs"),
                          eval_freq=2, deterministic=True, render=False, n_eval_episodes=5, verbose=0)
    cb.init_callback(m)
    cb.on_training_start({}, {})
    rows = []
    for call in range(1, 11):
        m.step()
        assert cb.on_step()
        if call % 2 == 0:
            rows.append(call * 4)
            z = np.load(tmp_path / "logs" / "evaluations.npz")
            assert z["timesteps"].tolist() == rows                                  # one row per evaluation
            assert z["results"].shape == (len(rows), 5) and z["ep_lengths"].shape == (len(rows), 5)
            assert z["ep_lengths"][-1].tolist() == [1, 2, 3, 4, 5]
    assert [e[0] for e in m.evals] == [8, 16, 24, 32, 40] and all(e[1:] == (env, 5, True) for e in m.evals)
    # saved on 1.0, 3.0 and 5.0: an equal or lower mean is no improvement
    assert [t for t, _ in m.saved] == [8, 16, 40]
    assert all(p == str(tmp_path / "best" / "best_model.zip") for _, p in m.saved)
    assert cb.best_mean_reward == 5.0 and cb.last_mean_reward == 5.0
    assert m.callback_metrics == {"eval/mean_reward": 5.0, "eval/mean_ep_length": 3.0, "eval/success_rate": 0.2}


def test_eval_callback_rejects_rendering_and_a_single_env():
    with pytest.raises(NotImplementedError):
        cbs.EvalCallback(_EvalEnv(), render=True)
    with pytest.raises(TypeError, match=r"SalpVecEnv\(n_eval_episodes\)"):
        cbs.EvalCallback(object())


class _StopAt(cbs.BaseCallback):
    def __init__(self, at):
        super().__init__()
        self.at = at

    def _on_step(self):
        return self.n_calls != self.at


def test_callback_list_stops_when_any_member_does():
    m = _Model()
    a, b, c = _StopAt(0), _StopAt(3), _StopAt(0)
    cl = cbs.CallbackList([a, b, c])
    assert _run(m, cl, 4) == [True, True, False, True]
    assert (a.n_calls, b.n_calls, c.n_calls) == (4, 4, 4) and c.model is m      # every member sees every step
    assert c.num_timesteps == 16
    with pytest.raises(TypeError):
        cbs.CallbackList([a, object()])


def test_detailed_metrics_records_nothing_while_the_window_is_empty():
    m = _Model()
    cb = cbs.DetailedMetricsCallback(log_freq=2, window=10)
    _run(m, cb, 6)
    assert m.callback_metrics == {} and int(cb.window.count) == 0 and not cb.window.fused
    # then two envs end their episodes with a success: the next log_freq call records
    m.step(terminated=torch.tensor([1, 0, 1, 0], dtype=torch.uint8))
    assert cb.on_step() and m.callback_metrics == {} and cb.n_calls == 7
    m.step()
    assert cb.on_step()
    got = m.callback_metrics
    assert got["custom/navigation/success_rate"] == 1.0 and got["custom/navigation/truncation_rate"] == 0.0
    assert got["reward/stats/total_mean"] == 1.0 and got["reward/stats/total_std"] == 0.0
    assert got["custom/performance/cycles_to_success"] == 1.0 and got["reward/components/track"] == 1.0
    assert len(got) == 26 and int(cb.window.count) == 2


def test_evaluate_policy_delegates_to_the_model():
    m = _Model(eval_means=[2.0])
    assert cbs.evaluate_policy(m, "env", n_eval_episodes=4, return_episode_rewards=True)[0] == [1.0, 3.0, 2.0, 2.0]
    assert m.evals == [(0, "env", 4, True)]
