"""The rest of the reference's recurrent training script on the GPU
(src/train_robot_recurrent_ppo.py:110-165): RecurrentPPO.learn with the
callbacks of grasp_lab_salp_amd/callbacks.py, evaluate, save / load, and the
fused policy step (``fused_step=True``, salp_lstm_policy_step) under all of
them.  64 envs whose episodes last at most 4 steps (max_cycles = 4)."""
import os

import numpy as np
import pytest
import torch

import metrics_ref
from grasp_lab_salp_amd import callbacks as cbs
from grasp_lab_salp_amd import metrics
from grasp_lab_salp_amd._abi import INFO, default_params
from grasp_lab_salp_amd.recurrent_ppo import RecurrentPPO
from recurrent_stub import assert_same, state_of

pytestmark = pytest.mark.gpu

N, MAX_CYCLES, T = 64, 4, 32


def _env(n=N, seed=3):
    from grasp_lab_salp_amd.vec_env import SalpVecEnv
    return SalpVecEnv(n, params=default_params(max_cycles=MAX_CYCLES), seed=seed)


def _model(env=None, **kw):
    return RecurrentPPO("MlpLstmPolicy", env or _env(), n_steps=T, batch_size=256, n_epochs=1, seq_len=16, seed=1, **kw)


def _same_bits(a, b):
    return a.dtype == b.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_fused_collection_is_replayed_by_the_update():
    """The check and the figure of test_recurrent_ppo_replays_its_collection_and_learns,
    with the collection's steps on salp_lstm_policy_step: the update's pass over
    the stored sequences (k_lstm_fwd, torch's GEMMs and tanh) reproduces the
    values and log-probs the fused step stored, so the first ratios are 1."""
    m = _model(fused_step=True)
    checked = []
    inner = m.train

    def train():
        if not checked:
            b = m.buf
            with torch.no_grad():
                for k in range(m.n_seq):
                    sl = slice(k * m.seq_len, (k + 1) * m.seq_len)
                    v, lp, _ = m.policy.evaluate(b.obs[sl], b.actions[sl], m.seq_states[k], b.episode_starts[sl])
                    checked.append((float((v - b.values[sl]).abs().max()), float((lp - b.log_probs[sl]).abs().max())))
            assert b.episode_starts[0].sum() == N and 0 < b.episode_starts[1:].sum() < (T - 1) * N
            assert bool((m.seq_states[1] != 0).any())
        return inner()

    m.train = train
    m.learn(3 * T * N)
    print(f"[recurrent fused replay] (|dv|, |dlogp|) per sequence: {checked}")
    assert len(checked) == 2
    for dv, dlp in checked:
        assert dv <= 1e-4 and dlp <= 1e-4, checked
    assert len(m.history) == 3 and m.num_timesteps == 3 * T * N
    for row in m.history:
        assert np.isfinite(row["vf_loss"]) and np.isfinite(row["pg_loss"])
    assert all(bool(torch.isfinite(p).all()) for p in m.policy.parameters())


def test_fused_and_unfused_collections_agree():
    """One collection from the same seed on both paths: the same noise is
    drawn, so values, log-probs and actions agree within the kernel test's
    tolerance for as long as the envs see the same actions (the first step)."""
    a, b = _model(fused_step=False), _model(fused_step=True)
    a.collect_rollouts()
    b.collect_rollouts()
    for name in ("obs", "actions", "values", "log_probs"):
        x, y = getattr(a.buf, name)[0], getattr(b.buf, name)[0]
        assert torch.allclose(x, y, rtol=1e-4, atol=1e-5), name
    assert torch.equal(a.sample_gen.get_state(), b.sample_gen.get_state())


def _summary_index(name):
    if "/" in name:
        col, stat = name.split("/")
        return 1 + 4 * metrics.ROW_KEYS.index(col) + metrics.SUMMARY_STATS.index(stat)
    return {"distance_per_cycle": 81, "cycles_to_success": 82}[name]


class _Recorder(cbs.BaseCallback):
    """Copies each step's locals to the host and feeds the deque restatement."""

    def __init__(self, window, log_freq):
        super().__init__()
        self.ref, self.log_freq, self.logs, self.shapes, self.steps = metrics_ref.DequeWindow(window), log_freq, [], None, []

    def _on_step(self):
        lo = {k: v.cpu().numpy() for k, v in self.locals.items()}
        self.shapes = {k: v.shape for k, v in lo.items()}
        self.steps.append(self.model.num_timesteps)
        self.ref.push(lo["info"], lo["terminated"], lo["truncated"], skip=lo["diverged"].astype(np.uint8))
        if self.n_calls % self.log_freq == 0:
            self.logs.append((self.ref.summary(), dict(self.model.callback_metrics)))
        return True


@pytest.mark.parametrize("fused_step", [False, True])
def test_metrics_callback_end_to_end(fused_step):
    m = _model(fused_step=fused_step)
    det, rec = cbs.DetailedMetricsCallback(log_freq=8), _Recorder(100, 8)
    m.learn(2 * T * N, callback=[det, rec])
    assert det.n_calls == rec.n_calls == 2 * T and det.num_timesteps == 2 * T * N == m.num_timesteps
    assert rec.steps == [k * N for k in range(1, 2 * T + 1)] and det.window.fused
    assert rec.shapes == {"obs": (N, m.obs_dim), "actions": (N, 3), "rewards": (N,), "terminated": (N,),
                          "truncated": (N,), "dones": (N,), "info": (N, len(INFO)), "diverged": (N,)}
    assert rec.ref.count >= 2 * T // MAX_CYCLES * N and int(det.window.count) == rec.ref.count
    got, want = det.window.rows.cpu().numpy(), rec.ref.rows()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert len(rec.logs) == 8
    earlier = {}
    for (want, scale), recorded in rec.logs:
        assert len(recorded) >= 25
        for key, name in cbs._SUMMARY_KEYS:
            k = _summary_index(name)
            if np.isnan(want[k]):       # no success in the window: no cycles to success recorded at this call
                assert name == "cycles_to_success" and recorded.get(key) == earlier.get(key), key
                continue
            if k in metrics_ref.EXACT:
                assert recorded[key] == want[k], key
            else:
                assert abs(recorded[key] - want[k]) <= metrics_ref.BOUND * scale[k], key
        earlier = recorded
    assert len(m.history) == 2
    for row in m.history:
        assert "vf_loss" in row and "reward/stats/total_mean" in row and "custom/navigation/success_rate" in row
    assert m.history[-1]["reward/stats/total_mean"] == rec.logs[-1][1]["reward/stats/total_mean"]


@pytest.fixture(scope="module")
def trained():
    """A fused-step learner after one iteration."""
    m = _model(fused_step=True)
    m.learn(T * N)
    return m


@pytest.mark.parametrize("n_eval_envs", [5, 3])
def test_evaluate_equals_a_host_loop_on_a_twin_env(trained, n_eval_envs):
    m = trained
    before = (m.sim.get_state().clone(), m.sample_gen.get_state().clone(), state_of(m), m._lstm_state.clone(),
              m._lstm_state.data_ptr())
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
    state = m.policy.initial_state(n_eval_envs, m.device)
    starts = torch.ones(n_eval_envs, device=m.device)
    for _ in range(max(ref.target) * MAX_CYCLES):
        a, state = m._eval_action(obs, state, starts, True)
        r = twin.step(torch.clamp(a, m.low, m.high), auto_reset=True)
        ref.push(r.info.cpu().numpy(), r.terminated.cpu().numpy(), r.truncated.cpu().numpy())
        starts = (r.terminated | r.truncated).float()
        obs = r.obs
        if ref.remaining == 0:
            break
    assert ref.remaining == 0 and ref.done == ref.target
    assert np.array_equal(np.asarray(returns).view(np.uint64), ref.ep_return.view(np.uint64))
    assert lengths == ref.ep_len.astype(int).tolist()
    assert m.last_eval["successes"] == ref.success.astype(bool).tolist()
    # the training env, the generator, the learner and its recurrent state are where they were
    assert _same_bits(m.sim.get_state(), before[0]) and torch.equal(m.sample_gen.get_state(), before[1])
    assert_same(state_of(m), before[2], "after evaluate")
    assert torch.equal(m._lstm_state, before[3]) and m._lstm_state.data_ptr() == before[4]


def test_eval_action_paths_agree_and_predict_clips(trained):
    m = trained
    obs = torch.randn(7, m.obs_dim, device=m.device)
    state = 0.3 * torch.randn(4, 7, 256, device=m.device)
    starts = (torch.arange(7, device=m.device) % 3 == 0).float()
    a1, s1 = m._eval_action(obs, state, starts, True)
    m.fused_step = False
    try:
        a0, s0 = m._eval_action(obs, state, starts, True)
    finally:
        m.fused_step = True
    assert torch.allclose(a1, a0, rtol=1e-4, atol=1e-5) and torch.allclose(s1, s0, rtol=1e-4, atol=1e-5)
    assert torch.equal(s1[2:], state[2:])
    a, s = m.predict(obs.cpu().numpy(), state=state, episode_start=starts)
    assert isinstance(a, np.ndarray) and np.array_equal(a, torch.clamp(a1, m.low, m.high).cpu().numpy())
    assert torch.equal(s, s1) and m.predict(obs[0])[0].shape == (3,)


def test_eval_and_checkpoint_callbacks_inside_learn(tmp_path):
    m = _model(fused_step=True)
    ev = cbs.EvalCallback(_env(5, seed=11), best_model_save_path=str(tmp_path / "best"),
                          log_path=str(tmp_path / "logs"), eval_freq=16, deterministic=True, render=False,
                          n_eval_episodes=5, verbose=0)
    ck = cbs.CheckpointCallback(save_freq=24, save_path=str(tmp_path / "models"), name_prefix="recurrent_ppo_salp")
    m.learn(2 * T * N, callback=cbs.CallbackList([ev, ck]), tb_log_name="recurrent_ppo", progress_bar=True)
    assert sorted(os.listdir(tmp_path / "models")) == sorted(f"recurrent_ppo_salp_{t}_steps.zip"
                                                             for t in (24 * N, 48 * N))
    z = np.load(tmp_path / "logs" / "evaluations.npz")
    assert z["timesteps"].tolist() == [16 * N, 32 * N, 48 * N, 64 * N]
    assert z["results"].shape == z["ep_lengths"].shape == (4, 5)
    means = [float(np.mean(r)) for r in z["results"].tolist()]
    assert ev.last_mean_reward == means[-1] and ev.best_mean_reward == max(means)
    assert os.listdir(tmp_path / "best") == ["best_model.zip"]
    for key in ("eval/mean_reward", "eval/mean_ep_length", "eval/success_rate"):
        assert key in m.callback_metrics and key in m.history[-1]
    # a checkpoint taken mid-collection loads, for prediction only and onto an env
    path = str(tmp_path / "models" / f"recurrent_ppo_salp_{24 * N}_steps")
    obs = np.random.default_rng(0).normal(size=(7, m.obs_dim)).astype(np.float32)
    p, q = RecurrentPPO.load(path), RecurrentPPO.load(path, env=_env())
    assert p.predict_only and p.fused_step and q.fused_step and p.num_timesteps == q.num_timesteps == 24 * N
    assert np.array_equal(p.predict(obs)[0], q.predict(obs)[0])
    m.save(str(tmp_path / "final"))                                                   # the script's last line


def test_load_and_resume_with_the_fused_step(tmp_path):
    m = _model(fused_step=True)
    m.learn(T * N)
    path = m.save(str(tmp_path / "model"))
    m2 = RecurrentPPO.load(path, env=_env())
    assert m2.fused_step and m2.num_timesteps == T * N
    assert_same(state_of(m), state_of(m2), "loaded")
    for name in ("obs", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
        getattr(m2.buf, name).copy_(getattr(m.buf, name))
    m2.seq_states.copy_(m.seq_states)
    m.train()
    m2.train()
    torch.cuda.synchronize()
    assert_same(state_of(m), state_of(m2), "one more train()")
    m2.learn(2 * T * N)                          # and the loaded learner collects and trains on its env
    assert m2.num_timesteps == 2 * T * N and np.isfinite(m2.history[-1]["vf_loss"])


class _StopAt(cbs.BaseCallback):
    def __init__(self, k):
        super().__init__()
        self.k = k

    def _on_step(self):
        return self.n_calls < self.k


@pytest.mark.parametrize("k", [5, T + 5])
def test_a_callback_that_returns_false_stops_learn(k):
    m = _model(fused_step=True)
    updates = []
    inner = m.train
    m.train = lambda: updates.append(m.num_timesteps) or inner()
    cb = _StopAt(k)
    assert m.learn(100 * T * N, callback=cb) is m
    assert cb.n_calls == k and m.num_timesteps == k * N
    assert updates == [T * N] * (k // T) and len(m.history) == k // T      # no update for the iteration that was cut
