"""PPO's callback protocol on the CPU: ``learn(callback=...)`` over the
lock-step collection (a stub env, torch ops), and the host logic of
``on_steps`` (what the chained collection calls once per collection) with a
fake model."""
import os

import pytest
import torch

from grasp_lab_salp_amd import callbacks as cbs
from grasp_lab_salp_amd._abi import INFO_DIM
from grasp_lab_salp_amd.ppo import PPO
from recurrent_stub import StubEnv

N, D = 4, 10


def _model(**kw):
    return PPO("MlpPolicy", StubEnv(n_envs=N, obs_dim=D), n_steps=16, batch_size=32, n_epochs=1, seed=2, **kw)


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
    assert m.collect == "lockstep"
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
    m.learn(4 * 16 * N, 1)                                # log_interval stays the second positional argument
    assert m.num_timesteps == 4 * 16 * N
    with pytest.raises(TypeError):
        m.learn(N, callback="not a callback")
    with pytest.raises(TypeError):
        m.learn(N, 1, cb)                                 # callback is keyword-only


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


# ------------------------------------------------------------ on_steps
class _FakeModel:
    """What the callbacks touch of a learner whose collection is chained."""

    collect = "chained"
    device = torch.device("cpu")
    env = None

    def __init__(self, n_envs=64):
        self.n_envs, self.num_timesteps, self.saved, self.evaluated, self.recorded = n_envs, 0, [], [], {}
        self.last_eval, self.locals = None, {}

    def collect_once(self, n_steps):
        self.num_timesteps += n_steps * self.n_envs

    def save(self, path):
        self.saved.append(os.path.basename(path))

    def evaluate(self, env, n_eval_episodes, deterministic, return_episode_rewards):
        self.evaluated.append(self.num_timesteps)
        self.last_eval = {"successes": [True] * n_eval_episodes}
        return [1.0] * n_eval_episodes, [7] * n_eval_episodes

    def record(self, key, value):
        self.recorded[key] = value


class _EvalEnv:
    step = reset = params = None
    n_envs, obs_dim, device = 5, D, torch.device("cpu")


class _Spans(cbs.BaseCallback):
    def __init__(self):
        super().__init__()
        self.spans = []

    def _on_steps(self, first, last):
        self.spans.append((first, last, self.n_calls, self.num_timesteps, dict(self.locals)))
        return last < 48


def test_on_steps_fires_once_per_span(tmp_path):
    m = _FakeModel()
    ck = cbs.CheckpointCallback(save_freq=16, save_path=str(tmp_path / "ck"), name_prefix="ppo")
    ev = cbs.EvalCallback(_EvalEnv(), n_eval_episodes=5, eval_freq=24, log_path=str(tmp_path / "ev"), verbose=0)
    spans = _Spans()
    both = cbs.CallbackList([ck, ev, spans])
    both.init_callback(m)
    went_on = []
    for _ in range(3):
        m.collect_once(16)
        went_on.append(both.on_steps(16))
    # calls {16, 32, 48} and {32, 48}: once each, under the timesteps at the end of the collection
    assert m.saved == [f"ppo_{k * 64}_steps.zip" for k in (16, 32, 48)]
    assert m.evaluated == [32 * 64, 48 * 64] == ev.evaluations_timesteps
    assert m.recorded["eval/mean_reward"] == 1.0 and m.recorded["eval/success_rate"] == 1.0
    assert (ck.n_calls, ev.n_calls, both.n_calls) == (48, 48, 48)
    # the list forwards the span, and a member's False comes back
    assert spans.spans == [(1, 16, 16, 16 * 64, {}), (17, 32, 32, 32 * 64, {}), (33, 48, 48, 48 * 64, {})]
    assert went_on == [True, True, False]


def test_on_steps_frequencies_that_do_not_divide_the_span(tmp_path):
    m = _FakeModel(n_envs=1)
    ck = cbs.CheckpointCallback(save_freq=5, save_path=str(tmp_path))
    ck.init_callback(m)
    fired = []
    for k in (4, 1, 3, 12, 1):            # calls 1-4, 5, 6-8, 9-20 (two multiples: once), 21
        m.collect_once(k)
        before = len(m.saved)
        assert ck.on_steps(k) is True
        fired.append(len(m.saved) - before)
    assert fired == [0, 1, 0, 1, 0]
    # on_step is what it was
    before = len(m.saved)
    for _ in range(4):
        ck.on_step()
    assert ck.n_calls == 25 and len(m.saved) == before + 1


class _PerStep(cbs.BaseCallback):
    def _on_step(self):
        return True


class _Both(_PerStep):
    def _on_steps(self, first, last):
        return True


def test_per_step_callbacks_are_refused_by_a_chained_model():
    m = _FakeModel()
    for cb, names in ((cbs.DetailedMetricsCallback(log_freq=1), ("DetailedMetricsCallback",)),
                      (cbs.CallbackList([cbs.BaseCallback(), _PerStep()]), ("_PerStep",)),
                      ([cbs.DetailedMetricsCallback(), _PerStep()], ("DetailedMetricsCallback", "_PerStep"))):
        with pytest.raises(ValueError, match='collect="lockstep"') as e:
            PPO._as_callback(m, cb)       # what learn() does first, before anything is collected
        assert all(n in str(e.value) for n in names) and m.num_timesteps == 0
    assert PPO._as_callback(m, [cbs.BaseCallback(), _Both()]).per_step_only() == []
    lock = _FakeModel()
    lock.collect = "lockstep"
    assert isinstance(PPO._as_callback(lock, _PerStep()), _PerStep)
