"""RecurrentPPO's learner surface on the CPU (a stub env, torch ops):
``predict``'s call shape, and the callback protocol inside ``learn``."""
import numpy as np
import pytest
import torch

from grasp_lab_salp_amd import callbacks as cbs
from grasp_lab_salp_amd._abi import INFO_DIM
from grasp_lab_salp_amd.recurrent_ppo import RecurrentPPO
from recurrent_stub import StubEnv

N, D, H = 4, 10, 32


def _model(**kw):
    kw.setdefault("n_steps", 16)
    kw.setdefault("batch_size", 32)
    return RecurrentPPO("MlpLstmPolicy", StubEnv(n_envs=N, obs_dim=D), n_epochs=1, seq_len=8, seed=2,
                        policy_kwargs={"lstm_hidden_size": H}, **kw)


@pytest.fixture(scope="module")
def model():
    m = _model()
    with torch.no_grad():     # the action head's init (gain 0.01) would leave every action inside the box
        m.policy.action_net.weight.mul_(300.0)
    return m


def test_predict_shapes_and_types(model):
    m = model
    obs = np.random.default_rng(0).normal(size=(6, D)).astype(np.float32)
    a, s = m.predict(obs)
    assert isinstance(a, np.ndarray) and a.shape == (6, 3) and a.dtype == np.float32
    assert torch.is_tensor(s) and s.shape == (4, 6, H)
    a1, s1 = m.predict(obs[0])
    assert a1.shape == (3,) and s1.shape == (4, 1, H)
    assert np.allclose(a1, a[0], atol=1e-6)       # (a GEMM of one row rounds otherwise than one of six)
    at, st = m.predict(torch.from_numpy(obs), deterministic=True)
    assert torch.is_tensor(at) and np.array_equal(at.numpy(), a) and torch.equal(st, s)
    # clipped to Box([0, 0, -1], [1, 1, 1]), and the clipping did something
    raw, _ = m._eval_action(torch.from_numpy(obs), m.policy.initial_state(6), torch.zeros(6))
    assert np.array_equal(a, np.clip(raw.numpy(), [0, 0, -1], [1, 1, 1])) and not np.array_equal(a, raw.numpy())
    # the actor's half moved, the critic's half is carried as it was
    assert bool((s[:2] != 0).any()) and bool((s[2:] == 0).all())


def test_predict_state_round_trip_and_reset(model):
    m = model
    g = torch.Generator().manual_seed(1)
    obs = [torch.randn(3, D, generator=g) for _ in range(3)]
    # handing the state back equals the policy run over the sequence
    s, acts = None, []
    for o in obs:
        a, s = m.predict(o, state=s)
        acts.append(a)
    with torch.no_grad():
        lat, _, new = m.policy.forward_seq(torch.stack(obs), m.policy.initial_state(3), torch.zeros(3, 3), critic=False)
        want = torch.clamp(m.policy._dist(lat).mean, m.low, m.high)
    assert torch.allclose(torch.stack(acts), want, atol=1e-6) and torch.allclose(s, new, atol=1e-6)
    # a viewer that discards the state gets the answer from a fresh one
    assert torch.equal(m.predict(obs[2])[0], m.predict(obs[2], state=None, episode_start=None)[0])
    assert not torch.equal(m.predict(obs[2])[0], acts[2])
    # episode_start = 1 resets that env's state before the step, and only that env's
    a_reset, s_reset = m.predict(obs[2], state=s, episode_start=np.array([0, 1, 0]))
    a_keep, s_keep = m.predict(obs[2], state=s)
    a_fresh, s_fresh = m.predict(obs[2])
    assert torch.equal(a_reset[1], a_fresh[1]) and torch.equal(s_reset[:2, 1], s_fresh[:2, 1])
    assert torch.equal(a_reset[[0, 2]], a_keep[[0, 2]]) and not torch.equal(a_reset[1], a_keep[1])
    # a NumPy state is taken too
    assert torch.equal(m.predict(obs[2], state=s.numpy())[0], a_keep)


def test_deterministic_predict_leaves_the_generator(model):
    m = model
    before = m.sample_gen.get_state().clone()
    obs = torch.zeros(2, D)
    a, _ = m.predict(obs)
    assert torch.equal(m.sample_gen.get_state(), before)
    b, _ = m.predict(obs, deterministic=False)
    assert not torch.equal(m.sample_gen.get_state(), before) and not torch.equal(a, b)


class _Recorder(cbs.BaseCallback):
    def __init__(self, stop_at=None, record_at=()):
        super().__init__()
        self.stop_at, self.record_at, self.seen, self.started, self.ended = stop_at, record_at, [], 0, 0

    def _on_training_start(self):
        self.started += 1

    def _on_training_end(self):
        self.ended += 1

    def _on_step(self):
        lo = self.locals
        self.seen.append((self.n_calls, self.num_timesteps, self.model.num_timesteps,
                          {k: (tuple(v.shape), v.dtype) for k, v in lo.items()}))
        if self.n_calls in self.record_at:
            self.logger.record("probe/calls", self.n_calls)
        return self.stop_at is None or self.n_calls < self.stop_at


def test_callback_protocol():
    m = _model()
    cb = _Recorder(record_at=(3, 20))
    assert m.learn(2 * 16 * N, callback=cb, tb_log_name="x", progress_bar=True) is m
    assert (cb.started, cb.ended, cb.n_calls) == (1, 1, 32)
    assert [s[:3] for s in cb.seen] == [(k, k * N, k * N) for k in range(1, 33)]
    assert cb.seen[-1][3] == {"obs": ((N, D), torch.float32), "actions": ((N, 3), torch.float32),
                              "rewards": ((N,), torch.float64), "terminated": ((N,), torch.uint8),
                              "truncated": ((N,), torch.uint8), "dones": ((N,), torch.bool),
                              "info": ((N, INFO_DIM), torch.float64), "diverged": ((N,), torch.uint8)}
    assert m.num_timesteps == 2 * 16 * N and len(m.history) == 2
    assert [r["timesteps"] for r in m.history] == [16 * N, 32 * N]
    # what was recorded reaches the next history row, once
    assert m.history[0]["probe/calls"] == 3 and m.history[1]["probe/calls"] == 20
    assert m.callback_metrics == {"probe/calls": 20}
    m.learn(3 * 16 * N)                                   # no callback: the counter moves per iteration, as before
    assert m.num_timesteps == 3 * 16 * N and "probe/calls" not in m.history[2] and cb.n_calls == 32
    with pytest.raises(TypeError):
        m.learn(N, callback="not a callback")


def test_a_list_of_callbacks_and_an_early_stop():
    m = _model()
    updates = []
    inner = m.train
    m.train = lambda: updates.append(m.num_timesteps) or inner()
    a, b = _Recorder(), _Recorder(stop_at=19)
    m.learn(100 * 16 * N, callback=[a, b])
    # the first iteration's update ran; the env-step that stopped training was followed by none
    assert a.n_calls == b.n_calls == 19 and m.num_timesteps == 19 * N and updates == [16 * N]
    assert len(m.history) == 1 and (a.ended, b.ended) == (1, 1)


def test_passive_callback_changes_nothing():
    a, b = _model(), _model()
    a.learn(2 * 16 * N)
    b.learn(2 * 16 * N, callback=cbs.BaseCallback())
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
    assert a.history[-1].keys() == b.history[-1].keys() and a.num_timesteps == b.num_timesteps
    assert all(torch.equal(x, y) for x, y in zip(a.sim.actions, b.sim.actions))
