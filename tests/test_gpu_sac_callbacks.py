"""The rest of the reference's training script on the GPU
(src/train_robot.py:71-122): SAC.learn with the callbacks of
grasp_lab_salp_amd/callbacks.py, SAC.evaluate, SAC.save / SAC.load and the
replay buffer's save / load.  64 envs whose episodes last at most 4 steps
(max_cycles = 4), so a few env-steps end hundreds of episodes."""
import os

import numpy as np
import pytest
import torch

import metrics_ref
from sac_state import assert_same_state, learner_state
from grasp_lab_salp_amd import callbacks as cbs
from grasp_lab_salp_amd import metrics, sac
from grasp_lab_salp_amd._abi import INFO, default_params

pytestmark = pytest.mark.gpu

N, MAX_CYCLES = 64, 4


def _env(n=N, seed=3):
    from grasp_lab_salp_amd.vec_env import SalpVecEnv
    return SalpVecEnv(n, params=default_params(max_cycles=MAX_CYCLES), seed=seed)


def _model(env=None, **kw):
    return sac.SAC("MlpPolicy", env or _env(), learning_starts=64, batch_size=64, buffer_size=512, seed=1, **kw)


def _same_bits(a, b):
    return a.dtype == b.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64))


def _summary_index(name):
    if "/" in name:
        col, stat = name.split("/")
        return 1 + 4 * metrics.ROW_KEYS.index(col) + metrics.SUMMARY_STATS.index(stat)
    return {"distance_per_cycle": 81, "cycles_to_success": 82}[name]


class _Recorder(cbs.BaseCallback):
    """Copies each step's locals to the host and feeds the deque restatement;
    at every ``log_freq``-th call keeps that restatement's summary and what
    the metrics callback (which ran just before) recorded."""

    def __init__(self, window, log_freq):
        super().__init__()
        self.ref, self.log_freq, self.logs, self.finished = metrics_ref.DequeWindow(window), log_freq, [], 0
        self.shapes = None

    def _on_step(self):
        lo = {k: v.cpu().numpy() for k, v in self.locals.items()}
        self.shapes = {k: v.shape for k, v in lo.items()}
        self.ref.push(lo["info"], lo["terminated"], lo["truncated"], skip=lo["diverged"].astype(np.uint8))
        if self.n_calls % self.log_freq == 0:
            self.logs.append((self.ref.summary(), dict(self.model.callback_metrics)))
        return True


def test_metrics_callback_end_to_end():
    m = _model()
    det, rec = cbs.DetailedMetricsCallback(log_freq=8), _Recorder(100, 8)
    m.learn(24 * N, callback=[det, rec], log_interval=8)
    assert det.n_calls == rec.n_calls == 24 and det.num_timesteps == 24 * N and det.window.fused
    assert rec.shapes == {"obs": (N, m.obs_dim), "actions": (N, 3), "rewards": (N,), "terminated": (N,),
                          "truncated": (N,), "dones": (N,), "info": (N, len(INFO)), "diverged": (N,)}
    # every episode ends within 4 steps: the window of 100 wrapped several times
    assert rec.ref.count >= 24 // MAX_CYCLES * N and int(det.window.count) == rec.ref.count
    got, want = det.window.rows.cpu().numpy(), rec.ref.rows()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert len(rec.logs) == 3
    for (want, scale), recorded in rec.logs:
        assert len(recorded) >= 25
        for key, name in cbs._SUMMARY_KEYS:
            k = _summary_index(name)
            if np.isnan(want[k]):       # no success in the window: no cycles to success
                assert name == "cycles_to_success" and key not in recorded, key
                continue
            print(f"[callbacks] {key}: {recorded[key]!r} against {want[k]!r} (bound {metrics_ref.BOUND * scale[k]:.3g})")
            if k in metrics_ref.EXACT:
                assert recorded[key] == want[k], key
            else:
                assert abs(recorded[key] - want[k]) <= metrics_ref.BOUND * scale[k], key
    assert len(m.history) == 3 and m.history[-1] is m.logger
    for row in m.history:
        assert "critic_loss" in row and "reward/stats/total_mean" in row and "custom/navigation/success_rate" in row
    assert m.history[-1]["reward/stats/total_mean"] == rec.logs[-1][1]["reward/stats/total_mean"]


@pytest.fixture(scope="module")
def trained():
    """A learner after 8 env-steps (6 gradient steps), library GEMMs."""
    m = _model()
    m.learn(8 * N)
    return m


@pytest.mark.parametrize("n_eval_envs", [5, 3])
def test_evaluate_equals_a_host_loop_on_a_twin_env(trained, n_eval_envs):
    m = trained
    before = m.sim.get_state().clone(), m.sample_gen.get_state().clone(), learner_state(m)
    returns, lengths = m.evaluate(_env(n_eval_envs, seed=11), n_eval_episodes=5, return_episode_rewards=True)
    assert len(returns) == len(lengths) == 5 and all(1 <= l <= MAX_CYCLES for l in lengths)
    assert m.last_eval["returns"] == returns and len(m.last_eval["successes"]) == 5
    mean, std = m.evaluate(_env(n_eval_envs, seed=11), n_eval_episodes=5)
    assert mean == float(np.mean(returns)) and std == float(np.std(returns))
    assert cbs.evaluate_policy(m, _env(n_eval_envs, seed=11), n_eval_episodes=5, return_episode_rewards=True) == (
        returns, lengths)
    # the same policy, stepped from the host with the bookkeeping in Python
    twin = _env(n_eval_envs, seed=11).sim
    ref = metrics_ref.EvalLoop(5, n_eval_envs)
    obs = twin.reset()
    for _ in range(max(ref.target) * MAX_CYCLES):
        r = twin.step(sac.unscale_action(m._eval_action(obs, True), m.low, m.high), auto_reset=True)
        ref.push(r.info.cpu().numpy(), r.terminated.cpu().numpy(), r.truncated.cpu().numpy())
        obs = r.obs
        if ref.remaining == 0:
            break
    assert ref.remaining == 0 and ref.done == ref.target
    assert np.array_equal(np.asarray(returns).view(np.uint64), ref.ep_return.view(np.uint64))
    assert lengths == ref.ep_len.astype(int).tolist()
    assert m.last_eval["successes"] == ref.success.astype(bool).tolist()
    # the training env, the generator and the learner are where they were
    assert _same_bits(m.sim.get_state(), before[0]) and torch.equal(m.sample_gen.get_state(), before[1])
    assert_same_state(learner_state(m), before[2], "after evaluate")


def test_evaluate_rejects_what_it_cannot_step(trained):
    with pytest.raises(TypeError, match="SalpVecEnv"):
        trained.evaluate(object())


class _BestPredictions(cbs.BaseCallback):
    """What the live model predicts on fixed observations, kept whenever the EvalCallback before it found a new best."""

    def __init__(self, eval_cb, obs):
        super().__init__()
        self.eval_cb, self.obs, self.best, self.actions, self.at = eval_cb, obs, -np.inf, None, []

    def _on_step(self):
        if self.eval_cb.best_mean_reward > self.best:
            self.best = self.eval_cb.best_mean_reward
            self.actions = self.model.predict(self.obs)[0]
            self.at.append(self.n_calls)
        return True


def test_eval_and_checkpoint_callbacks_inside_learn(tmp_path):
    m = _model()
    obs = np.random.default_rng(0).normal(size=(7, m.obs_dim)).astype(np.float32)
    ev = cbs.EvalCallback(_env(5, seed=11), best_model_save_path=str(tmp_path / "best"),
                          log_path=str(tmp_path / "logs"), eval_freq=4, deterministic=True, render=False,
                          n_eval_episodes=5, verbose=0)
    ck = cbs.CheckpointCallback(save_freq=6, save_path=str(tmp_path / "models"), name_prefix="salp",
                                save_replay_buffer=True)
    best = _BestPredictions(ev, obs)
    m.learn(12 * N, callback=cbs.CallbackList([ev, ck, best]))
    assert sorted(os.listdir(tmp_path / "models")) == sorted(
        [f"salp_{t}_steps.zip" for t in (6 * N, 12 * N)] + [f"salp_replay_buffer_{t}_steps.pt" for t in (6 * N, 12 * N)])
    z = np.load(tmp_path / "logs" / "evaluations.npz")
    assert z["timesteps"].tolist() == [4 * N, 8 * N, 12 * N] and z["results"].shape == z["ep_lengths"].shape == (3, 5)
    means = [float(np.mean(r)) for r in z["results"].tolist()]
    assert ev.last_mean_reward == means[-1] and ev.best_mean_reward == max(means)
    assert best.at and best.at[0] == 4 and os.listdir(tmp_path / "best") == ["best_model.zip"]
    for key in ("eval/mean_reward", "eval/mean_ep_length", "eval/success_rate"):
        assert key in m.callback_metrics and key in m.history[-1]
    # the best model, loaded for prediction only and onto an env, predicts what the live model did then
    path = str(tmp_path / "best" / "best_model")
    for loaded in (sac.SAC.load(path), sac.SAC.load(path, env=_env())):
        assert np.array_equal(loaded.predict(obs)[0], best.actions)
        assert loaded.num_timesteps == best.at[-1] * N and loaded.device == m.device
    if best.at[-1] != 12:
        assert not np.array_equal(m.predict(obs)[0], best.actions)      # the live model has moved on since


def _resume(tmp_path, **kw):
    m = _model(**kw)
    m.learn(6 * N)
    saved = learner_state(m)
    path, rb = m.save(str(tmp_path / "model")), m.save_replay_buffer(str(tmp_path / "replay.pt"))
    m2 = sac.SAC.load(path, env=_env())
    assert (m2.fused, m2.fused_mlp) == (m.fused, m.fused_mlp)
    ptrs = [getattr(m2.replay, k).data_ptr() for k in sac._REPLAY_TENSORS]
    m2.load_replay_buffer(rb)
    assert ptrs == [getattr(m2.replay, k).data_ptr() for k in sac._REPLAY_TENSORS]
    for k in sac._REPLAY_TENSORS:
        assert torch.equal(getattr(m.replay, k), getattr(m2.replay, k)), k
    assert_same_state(learner_state(m2), saved, "loaded")
    pol = m2.policy
    assert pol.actor.is_flat() and pol.critic.is_flat() and pol.critic_target.is_flat()
    return m, m2


def test_resume_with_fused_mlp_continues_bit_equal(tmp_path):
    """Every kernel of the fused_mlp gradient step is deterministic: three more
    steps on the learner that never stopped and on the one loaded from its
    files leave parameters, targets, optimiser states, log_ent_coef, the
    update counter and the generator bit-equal."""
    m, m2 = _resume(tmp_path, fused_mlp=True)
    assert m.n_updates == 5
    m.train(3)
    m2.train(3)
    assert m2.n_updates == 8
    assert_same_state(m, m2, "3 more gradient steps")
    m2.learn(2 * N)                          # and the loaded learner collects and trains on its env
    assert m2.num_timesteps == 8 * N and m2.n_updates == 10


def test_resume_on_the_default_path_restores_the_saved_state(tmp_path):
    _resume(tmp_path)


class _StopAtThird(cbs.BaseCallback):
    def _on_step(self):
        return self.n_calls < 3


def test_a_callback_that_returns_false_stops_learn():
    m = _model()
    cb = _StopAtThird()
    assert m.learn(100 * N, callback=cb) is m
    # three env-steps; the second was followed by a gradient step, the third by none
    assert cb.n_calls == 3 and m.num_timesteps == 3 * N and m.n_updates == 1
    assert len(m.history) == 1 and m.history[0]["timesteps"] == 3 * N          # the closing row


class _Passive(cbs.BaseCallback):
    pass


def test_a_passive_callback_changes_nothing():
    """learn(callback=None) and learn with a callback that does nothing end in
    the same bits (fused_mlp: every kernel of the step is deterministic)."""
    a, b = _model(fused_mlp=True), _model(fused_mlp=True)
    a.learn(6 * N)
    cb = _Passive()
    b.learn(6 * N, callback=cb)
    assert cb.n_calls == 6 and b.callback_metrics == {} and a.history[-1].keys() == b.history[-1].keys()
    assert_same_state(a, b, "with and without a passive callback")
    assert _same_bits(a.sim.get_state(), b.sim.get_state())
    with pytest.raises(TypeError):
        a.learn(N, callback="not a callback")
