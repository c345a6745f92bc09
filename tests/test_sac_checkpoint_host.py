"""SAC.save / SAC.load and the replay buffer's save / load on the CPU
(fused=False, a stub env as tests/test_sac_host.py's): what is saved comes
back bit for bit, in place, and a resumed learner goes on exactly as the one
that never stopped."""
import json
import os
import zipfile

import numpy as np
import pytest
import torch

from grasp_lab_salp_amd import sac
from sac_state import assert_same_state as _assert_same


class _Sim:
    n_envs, obs_dim, device = 8, 10, torch.device("cpu")


class _Env:
    def __init__(self):
        self.sim = _Sim()


def _fill(m, steps, seed):
    g = torch.Generator().manual_seed(seed)
    n, d = m.n_envs, m.obs_dim
    for _ in range(steps):
        m.replay.add(torch.randn(n, d, generator=g), torch.rand(n, 3, generator=g) * 2 - 1,
                     torch.randn(n, d, generator=g), torch.randn(n, d, generator=g),
                     torch.randn(n, generator=g, dtype=torch.float64), (torch.rand(n, generator=g) < 0.2).to(torch.uint8),
                     torch.zeros(n, dtype=torch.uint8))


def _steps(m, k):
    for _ in range(k):
        m.gradient_step(m.replay.sample(m.batch_size, m._update))


@pytest.fixture
def trained(tmp_path_factory):
    m = sac.SAC("MlpPolicy", _Env(), batch_size=32, buffer_size=64, learning_rate=1e-3, seed=3)
    assert not m.fused
    _fill(m, 5, seed=0)
    _steps(m, 3)
    m.num_timesteps = 40
    d = tmp_path_factory.mktemp("ckpt")
    path = m.save(str(d / "model"))
    rb = m.save_replay_buffer(str(d / "replay.pt"))
    return m, path, rb, d


def test_save_applies_the_zip_suffix_rule(trained):
    m, path, _, d = trained
    assert path == str(d / "model.zip") and os.path.exists(path)
    assert m.save(str(d / "other.zip")) == str(d / "other.zip")
    assert m.save(str(d / "sub" / "name.ckpt")) == str(d / "sub" / "name.ckpt")     # a suffix is kept, folders made
    with zipfile.ZipFile(path) as z:
        assert set(z.namelist()) == {"data.json", "policy.pth", "actor.optimizer.pth", "critic.optimizer.pth",
                                     "ent_coef_optimizer.pth", "pytorch_variables.pth", "rng.pth"}
        data = json.loads(z.read("data.json"))
    assert data["format"] == "grasp_lab_salp_amd.SAC" and data["version"] == 1
    assert data["n_updates"] == 3 and data["update"] == 3 and data["num_timesteps"] == 40 and data["seed"] == 3
    assert data["obs_dim"] == 10 and data["fused"] is False and data["fused_mlp"] is False
    assert data["hyperparameters"]["batch_size"] == 32 and data["hyperparameters"]["learning_rate"] == 1e-3
    assert data["hyperparameters"]["ent_coef"] == "auto"


def test_round_trip_is_bit_equal_and_flat(trained):
    m, path, _, _ = trained
    m2 = sac.SAC.load(path[:-4], env=_Env())        # the suffix rule applies to load's path too
    _assert_same(m, m2, "loaded")
    assert (m2.num_timesteps, m2.n_updates, int(m2._update)) == (40, 3, 3)
    assert m2.batch_size == 32 and m2.learning_rate == 1e-3 and m2.replay.capacity == 8
    pol = m2.policy
    assert pol.actor.is_flat() and pol.critic.is_flat() and pol.critic_target.is_flat()
    assert not any(p.requires_grad for p in pol.critic_target.parameters())
    assert sac.SAC.load(path, env=_Env(), learning_rate=5e-4).learning_rate == 5e-4       # kwargs override


def test_resumed_learner_continues_bit_equal(trained):
    m, path, rb, _ = trained
    m2 = sac.SAC.load(path, env=_Env())
    ptrs = {k: getattr(m2.replay, k).data_ptr() for k in sac._REPLAY_TENSORS}
    m2.load_replay_buffer(rb)
    assert ptrs == {k: getattr(m2.replay, k).data_ptr() for k in sac._REPLAY_TENSORS}      # in place
    for k in sac._REPLAY_TENSORS:
        assert torch.equal(getattr(m.replay, k), getattr(m2.replay, k)), k
    assert m2.replay.seed == m.replay.seed
    _steps(m, 3)
    _steps(m2, 3)
    _assert_same(m, m2, "3 more steps")
    assert int(m2._update) == 6 and m2.n_updates == 6
    # a learner that had forgotten the update counter (which keys the sampler) would not have followed
    m3 = sac.SAC.load(path, env=_Env())
    m3.load_replay_buffer(rb)
    m3._update.zero_()
    _steps(m3, 3)
    assert not torch.equal(m3.policy.critic.flat, m.policy.critic.flat)


def test_replay_file_of_another_shape_is_rejected(trained):
    _, _, rb, _ = trained
    other = sac.SAC("MlpPolicy", _Env(), batch_size=32, buffer_size=128)
    with pytest.raises(ValueError, match="capacity"):
        other.load_replay_buffer(rb)


def test_predict_only_model(trained):
    m, path, _, _ = trained
    p = sac.SAC.load(path, env=None, device="cpu")
    assert p.predict_only and p.env is None and p.device.type == "cpu"
    obs = np.random.default_rng(0).normal(size=(6, 10)).astype(np.float32)
    want, _ = m.predict(obs)
    got, _ = p.predict(obs)
    assert np.array_equal(got, want) and got.shape == (6, 3)
    assert np.array_equal(p.predict(obs[0])[0], want[0])
    for call in (lambda: p.learn(8), p.collect_step, lambda: p.evaluate(_Env())):
        with pytest.raises(RuntimeError, match="env"):
            call()


def test_load_rejects_a_foreign_file(tmp_path):
    f = tmp_path / "x.zip"
    with zipfile.ZipFile(f, "w") as z:
        z.writestr("data.json", json.dumps({"format": "something else", "version": 1}))
    with pytest.raises(ValueError, match="grasp_lab_salp_amd.SAC"):
        sac.SAC.load(str(f), env=_Env())
