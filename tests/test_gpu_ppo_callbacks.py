"""PPO's learner surface on the GPU: predict, evaluate, save / load and
``learn(callback=...)`` over both collections, with the fused policy step
(``fused_act=True``, salp_ppo_mlp_act) under them.  64 envs whose episodes last
at most 4 steps (max_cycles = 4), n_steps 16, batch_size 256, 2 epochs."""
import os

import numpy as np
import pytest
import torch

import metrics_ref
from grasp_lab_salp_amd import _lib
from grasp_lab_salp_amd import callbacks as cbs
from grasp_lab_salp_amd._abi import default_params
from grasp_lab_salp_amd.ppo import PPO

pytestmark = pytest.mark.gpu

N, MAX_CYCLES, T = 64, 4, 16


def _env(n=N, seed=3):
    from grasp_lab_salp_amd.vec_env import SalpVecEnv
    return SalpVecEnv(n, params=default_params(max_cycles=MAX_CYCLES), seed=seed)


def _model(env=None, **kw):
    return PPO("MlpPolicy", env or _env(), n_steps=T, batch_size=256, n_epochs=2, seed=1, **kw)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8).reshape(-1),
                                                                     b.contiguous().view(torch.uint8).reshape(-1))


@pytest.fixture(scope="module")
def trained():
    """A lock-step learner with the fused policy step after one iteration."""
    m = _model(collect="lockstep", fused_act=True)
    m.learn(T * N)
    with torch.no_grad():     # the action head's init (gain 0.01) would leave every action near the box's corner
        m.policy.action_net.weight.mul_(100.0)
    return m


def test_fused_and_torch_paths_agree(trained):
    """predict's and evaluate's one action function on both paths, on random
    observations and on those an evaluation visits, within the policy's bound
    for the action.  Two evaluations' returns are printed and not compared:
    the simulator counts an action's contraction and coast times in whole
    ticks, so an episode's return is not continuous in the action, and actions
    2e-7 apart gave returns 7e-3 apart (of -97; lengths equal) on one MI355X.
    That evaluate is the host loop on predict's actions is the next test's, on
    either path, bit for bit."""
    m = trained
    twin, seen = _env(5, seed=11).sim, []
    o = twin.reset()
    for _ in range(2 * MAX_CYCLES):
        seen.append(o.clone())
        o = twin.step(m.predict(o)[0].contiguous(), auto_reset=True).obs
    obs = torch.cat([torch.randn(70, m.obs_dim, device=m.device), *seen])
    a1, none = m.predict(obs)
    raw1 = m._eval_action(obs).clone()
    m.fused_act = False
    try:
        a0, _ = m.predict(obs)
        raw0 = m._eval_action(obs)
        ret0, len0 = m.evaluate(_env(5, seed=11), n_eval_episodes=5, return_episode_rewards=True)
    finally:
        m.fused_act = True
    ret1, len1 = m.evaluate(_env(5, seed=11), n_eval_episodes=5, return_episode_rewards=True)
    print(f"[ppo fused_act] |d action| {float((raw1 - raw0).abs().max()):.3e}, "
          f"|d return| {np.abs(np.asarray(ret1) - np.asarray(ret0)).max():.3e}, lengths {len0} {len1}")
    assert none is None and torch.allclose(raw1, raw0, rtol=1e-5, atol=1e-5)
    assert torch.allclose(a1, a0, rtol=1e-5, atol=1e-5) and not torch.equal(a1, raw1)       # the clip did something
    assert bool((a1 >= m.low).all()) and bool((a1 <= m.high).all())
    assert len(ret0) == len(ret1) == 5 and all(1 <= l <= MAX_CYCLES for l in len0 + len1)
    # numpy in, numpy out; one observation in, one action out; noise only when asked for
    before = m.sample_gen.get_state().clone()
    an, _ = m.predict(obs.cpu().numpy())
    assert isinstance(an, np.ndarray) and an.dtype == np.float32 and np.array_equal(an, a1.cpu().numpy())
    one, _ = m.predict(obs[3])
    assert one.shape == (3,) and torch.equal(one, a1[3])
    assert torch.equal(m.sample_gen.get_state(), before)
    noisy, _ = m.predict(obs, deterministic=False)
    assert not torch.equal(m.sample_gen.get_state(), before) and not torch.equal(noisy, a1)


@pytest.fixture(params=[True, False], ids=["fused_act", "torch"])
def either_path(request, trained):
    trained.fused_act = request.param
    yield trained
    trained.fused_act = True


@pytest.mark.parametrize("n_eval_envs", [5, 3])
def test_evaluate_equals_a_host_loop_on_a_twin_env(either_path, n_eval_envs):
    m = either_path
    before = (m.sim.get_state().clone(), m.sample_gen.get_state().clone(), _flat_state(m), m._obs.clone(),
              m._obs.data_ptr())
    returns, lengths = m.evaluate(_env(n_eval_envs, seed=11), n_eval_episodes=5, return_episode_rewards=True)
    assert len(returns) == len(lengths) == 5 and all(1 <= l <= MAX_CYCLES for l in lengths)
    assert m.last_eval["returns"] == returns and len(m.last_eval["successes"]) == 5
    mean, std = m.evaluate(_env(n_eval_envs, seed=11), n_eval_episodes=5)
    assert mean == float(np.mean(returns)) and std == float(np.std(returns))
    assert cbs.evaluate_policy(m, _env(n_eval_envs, seed=11), n_eval_episodes=5, return_episode_rewards=True) == (
        returns, lengths)
    # the same policy, stepped from the host on predict's actions with the bookkeeping in Python
    twin = _env(n_eval_envs, seed=11).sim
    ref = metrics_ref.EvalLoop(5, n_eval_envs)
    obs = twin.reset()
    for _ in range(max(ref.target) * MAX_CYCLES):
        a, _ = m.predict(obs)
        r = twin.step(a.contiguous(), auto_reset=True)
        ref.push(r.info.cpu().numpy(), r.terminated.cpu().numpy(), r.truncated.cpu().numpy())
        obs = r.obs
        if ref.remaining == 0:
            break
    assert ref.remaining == 0 and ref.done == ref.target
    assert np.array_equal(np.asarray(returns).view(np.uint64), ref.ep_return.view(np.uint64))
    assert lengths == ref.ep_len.astype(int).tolist()
    assert m.last_eval["successes"] == ref.success.astype(bool).tolist()
    # the training env, its observation, the generator and the learner are where they were
    assert _same_bits(m.sim.get_state(), before[0]) and torch.equal(m.sample_gen.get_state(), before[1])
    assert all(_same_bits(v, before[2][k]) for k, v in _flat_state(m).items())
    assert torch.equal(m._obs, before[3]) and m._obs.data_ptr() == before[4]
    # the errors of SAC.evaluate
    with pytest.raises(TypeError, match="SalpVecEnv"):
        m.evaluate(object())
    with pytest.raises(ValueError, match="obs_dim"):
        from grasp_lab_salp_amd.vec_env import SalpVecEnv
        m.evaluate(SalpVecEnv(2, params=default_params(num_obstacles=1), seed=1))


class _StopAfter(cbs.BaseCallback):
    def __init__(self, k):
        super().__init__()
        self.k, self.spans = k, []

    def _on_steps(self, first, last):
        self.spans.append((first, last, self.num_timesteps, dict(self.locals)))
        return len(self.spans) < self.k


def test_chained_learn_with_eval_and_checkpoint_callbacks(tmp_path):
    m = _model(collect="chained", fused_act=True)
    assert m.fused_update and m.use_graphs
    ev = cbs.EvalCallback(_env(5, seed=11), eval_freq=24, n_eval_episodes=5, log_path=str(tmp_path / "logs"),
                          best_model_save_path=str(tmp_path / "best"), verbose=0)
    ck = cbs.CheckpointCallback(save_freq=16, save_path=str(tmp_path / "models"), name_prefix="ppo_salp")
    assert m.learn(3 * T * N, callback=[ev, ck], tb_log_name="ppo", progress_bar=True) is m
    assert sorted(os.listdir(tmp_path / "models")) == sorted(f"ppo_salp_{t}_steps.zip" for t in (16 * N, 32 * N, 48 * N))
    assert ev.evaluations_timesteps == [32 * N, 48 * N] and (ev.n_calls, ck.n_calls) == (48, 48)
    z = np.load(tmp_path / "logs" / "evaluations.npz")
    assert z["timesteps"].tolist() == [32 * N, 48 * N] and z["results"].shape == z["ep_lengths"].shape == (2, 5)
    assert os.listdir(tmp_path / "best") == ["best_model.zip"]
    assert m.num_timesteps == 3 * T * N and [r["timesteps"] for r in m.history] == [16 * N, 32 * N, 48 * N]
    assert "eval/mean_reward" not in m.history[0]
    for row in m.history[1:]:     # the evaluation ran before that collection's update: it is in that row
        assert "eval/mean_reward" in row and "eval/success_rate" in row and np.isfinite(row["vf_loss"])
    assert m.history[2]["eval/mean_reward"] == float(np.mean(z["results"][1]))
    # a checkpoint written between a collection and its update loads, for prediction only and onto an env
    path = str(tmp_path / "models" / f"ppo_salp_{32 * N}_steps")
    obs = np.random.default_rng(0).normal(size=(7, m.obs_dim)).astype(np.float32)
    p, q = PPO.load(path), PPO.load(path, env=_env())
    assert p.predict_only and p.fused_act and q.fused_act and q.fused_update and q.collect == "chained"
    assert p.num_timesteps == q.num_timesteps == 32 * N
    assert np.array_equal(p.predict(obs)[0], q.predict(obs)[0])
    # learn() without a callback goes on as before, per collection
    m.learn(4 * T * N)
    assert m.num_timesteps == 4 * T * N and len(m.history) == 4 and ck.n_calls == 48


def test_chained_learn_refuses_per_step_callbacks_and_stops_on_false():
    m = _model(collect="chained")
    collected = []
    inner = m.collect_rollouts
    m.collect_rollouts = lambda: collected.append(1) or inner()
    with pytest.raises(ValueError, match='DetailedMetricsCallback.*collect="lockstep"'):
        m.learn(T * N, callback=[cbs.BaseCallback(), cbs.DetailedMetricsCallback(log_freq=8)])
    assert collected == [] and m.num_timesteps == 0
    updates = []
    train = m.train
    m.train = lambda: updates.append(m.num_timesteps) or train()
    cb = _StopAfter(2)
    m.learn(100 * T * N, callback=cb)
    # the second collection's callback ended training: no GAE, no update, no history row for it
    assert cb.spans == [(1, T, T * N, {}), (T + 1, 2 * T, 2 * T * N, {})]
    assert updates == [T * N] and len(m.history) == 1 and m.num_timesteps == 2 * T * N


def _copy_buffer(dst, src):
    for name in ("obs", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
        getattr(dst.buf, name).copy_(getattr(src.buf, name))


def _flat_state(m):
    return {"m": m._f_m.clone(), "v": m._f_v.clone(), "step": m._f_step.clone(),
            **{f"p{i}": p.detach().clone() for i, p in enumerate(m.policy.parameters())}}


def _cuts(m):
    """The fused step's flat moments cut per parameter, in policy.parameters() order."""
    L = _lib.load()
    where = {id(t): k for k, t in enumerate(m._mlp_tensors)}
    out = []
    for p in m.policy.parameters():
        off = L.salp_ppo_mlp_offset(m.obs_dim, where[id(p)])
        out.append((m._f_m[off:off + p.numel()].view(p.shape), m._f_v[off:off + p.numel()].view(p.shape)))
    return out


def test_save_and_load_with_the_fused_update(tmp_path):
    m = _model(collect="chained", fused_update=True)
    m.learn(2 * T * N)
    assert m._epoch_graph is not None                    # the epoch graphs are kept across updates
    ptrs = [p.data_ptr() for p in m.policy.parameters()]
    path = m.save(str(tmp_path / "model"))
    m2 = PPO.load(path, env=_env())
    assert m2.fused_update and m2.collect == "chained" and m2.num_timesteps == 2 * T * N
    for k, v in _flat_state(m).items():
        assert _same_bits(v, _flat_state(m2)[k]), k
    assert torch.equal(m.gen.get_state(), m2.gen.get_state())
    _copy_buffer(m2, m)
    m.train()             # replays the kept graphs
    m2.train()            # captures its own over the loaded tensors
    torch.cuda.synchronize()
    assert float(m._f_step) == float(m2._f_step) == 3 * 2 * (T * N // 256)
    for k, v in _flat_state(m).items():
        assert _same_bits(v, _flat_state(m2)[k]), ("one more train()", k)
    assert ptrs == [p.data_ptr() for p in m.policy.parameters()]

    # one file layout for both update paths: fused -> torch Adam
    path = m.save(str(tmp_path / "fused"))
    m3 = PPO.load(path, env=_env(), fused_update=False)
    assert not m3.fused_update and not hasattr(m3, "_f_m")
    st = m3.opt.state_dict()["state"]
    assert sorted(st) == list(range(len(list(m3.policy.parameters()))))
    for i, (em, ev) in enumerate(_cuts(m)):
        assert _same_bits(st[i]["exp_avg"], em) and _same_bits(st[i]["exp_avg_sq"], ev), i
        assert float(st[i]["step"]) == float(m._f_step)
    for p, q in zip(m.policy.parameters(), m3.policy.parameters()):
        assert _same_bits(p.detach(), q.detach())
    # ... and torch Adam -> fused, after the torch path has moved on
    _copy_buffer(m3, m)
    m3.train()
    torch.cuda.synchronize()
    path = m3.save(str(tmp_path / "torch"))
    m4 = PPO.load(path, env=_env(), fused_update=True)
    st = m3.opt.state_dict()["state"]
    assert m4.fused_update and float(m4._f_step) == float(st[0]["step"]) > float(m._f_step)
    for i, (em, ev) in enumerate(_cuts(m4)):
        assert _same_bits(st[i]["exp_avg"], em) and _same_bits(st[i]["exp_avg_sq"], ev), i
    _copy_buffer(m4, m)
    m4.train()            # and the fused step goes on from them
    assert all(bool(torch.isfinite(p).all()) for p in m4.policy.parameters())


def test_lockstep_learn_with_the_fused_step_and_a_metrics_callback():
    """The update's torch pass over the stored rows reproduces the values and
    log-probs salp_ppo_mlp_act stored: the first ratios are 1."""
    m = _model(collect="lockstep", fused_act=True)
    checked = []
    inner = m.train

    def train():
        if not checked:
            b = m.buf
            with torch.no_grad():
                v, lp, _ = m.policy.evaluate(b.obs.reshape(T * N, -1), b.actions.reshape(T * N, 3))
            checked.append((float((v - b.values.reshape(-1)).abs().max()),
                            float((lp - b.log_probs.reshape(-1)).abs().max())))
            assert b.episode_starts[0].sum() == N and 0 < b.episode_starts[1:].sum() < (T - 1) * N
        return inner()

    m.train = train
    det = cbs.DetailedMetricsCallback(log_freq=8)
    m.learn(2 * T * N, callback=det)
    print(f"[ppo fused_act replay] (|dv|, |dlogp|): {checked}")
    assert len(checked) == 1 and checked[0][0] <= 1e-4 and checked[0][1] <= 1e-4, checked
    assert det.n_calls == 2 * T and det.num_timesteps == 2 * T * N == m.num_timesteps and det.window.fused
    assert int(det.window.count) >= 2 * T // MAX_CYCLES * N
    assert len(m.history) == 2 and all("custom/navigation/success_rate" in r for r in m.history)
    assert all(bool(torch.isfinite(p).all()) for p in m.policy.parameters())
