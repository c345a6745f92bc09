"""RecurrentPPO.save / RecurrentPPO.load on the CPU (a stub env as
tests/test_sac_checkpoint_host.py's): what is saved comes back bit for bit,
in place, and a resumed learner goes on exactly as the one that never
stopped."""
import json
import os
import zipfile

import numpy as np
import pytest
import torch

from grasp_lab_salp_amd.recurrent_ppo import RecurrentPPO
from recurrent_stub import StubEnv, assert_same, fill, state_of

N, D, H = 4, 10, 32


def _model(env=None, **kw):
    return RecurrentPPO("MlpLstmPolicy", env or StubEnv(n_envs=N, obs_dim=D), n_steps=16, batch_size=32, n_epochs=2,
                        seq_len=8, seed=5, learning_rate=1e-3, policy_kwargs={"lstm_hidden_size": H}, **kw)


@pytest.fixture
def trained(tmp_path):
    m = _model()
    m.learn(2 * 16 * N)
    m.predict(torch.zeros(1, D), deterministic=False)
    return m, m.save(str(tmp_path / "model")), tmp_path


def test_zip_members_and_data(trained):
    m, path, d = trained
    assert path == str(d / "model.zip") and os.path.exists(path)
    assert m.save(str(d / "sub" / "name.ckpt")) == str(d / "sub" / "name.ckpt")     # a suffix is kept, folders made
    with zipfile.ZipFile(path) as z:
        assert set(z.namelist()) == {"data.json", "policy.pth", "policy.optimizer.pth", "rng.pth"}
        assert all(i.compress_type == zipfile.ZIP_STORED for i in z.infolist())
        data = json.loads(z.read("data.json"))
    assert data["format"] == "grasp_lab_salp_amd.RecurrentPPO" and data["version"] == 1
    assert data["num_timesteps"] == 2 * 16 * N and data["seed"] == 5 and data["obs_dim"] == D
    assert data["fused_step"] is False and data["device_type"] == "cpu"
    hp = data["hyperparameters"]
    assert (hp["seq_len"], hp["lstm_hidden_size"], hp["net_arch"]) == (8, H, [64, 64])
    assert (hp["n_steps"], hp["batch_size"], hp["n_epochs"], hp["learning_rate"]) == (16, 32, 2, 1e-3)
    for k in ("gamma", "gae_lambda", "clip_range", "ent_coef", "vf_coef", "max_grad_norm"):
        assert isinstance(hp[k], float), k


def test_round_trip_is_bit_equal_and_in_place(trained, monkeypatch):
    m, path, _ = trained
    ptrs = []
    inner = torch.nn.Module.load_state_dict

    def spy(self, *a, **kw):
        ptrs.append([p.data_ptr() for p in self.parameters()])
        return inner(self, *a, **kw)

    monkeypatch.setattr(torch.nn.Module, "load_state_dict", spy)
    m2 = RecurrentPPO.load(path[:-4], env=StubEnv(n_envs=N, obs_dim=D))      # the suffix rule applies to load too
    assert ptrs and ptrs[0] == [p.data_ptr() for p in m2.policy.parameters()]      # copied into, not replaced
    assert [id(p) for g in m2.opt.param_groups for p in g["params"]] == [id(p) for p in m2.policy.parameters()]
    assert_same(state_of(m), state_of(m2), "loaded")
    assert m2.num_timesteps == m.num_timesteps and (m2.seq_len, m2.policy.hidden, m2.n_steps) == (8, H, 16)
    m3 = RecurrentPPO.load(path, env=StubEnv(n_envs=N, obs_dim=D), learning_rate=5e-4)     # kwargs override
    assert m3.learning_rate == 5e-4 and m3.opt.param_groups[0]["lr"] == 5e-4


def test_resumed_learner_continues_bit_equal(trained):
    m, path, _ = trained
    m2 = RecurrentPPO.load(path, env=StubEnv(n_envs=N, obs_dim=D))
    fill(m, 11)
    fill(m2, 11)
    m.train()
    m2.train()
    assert_same(state_of(m), state_of(m2), "one more train()")
    # a learner that had forgotten the permutation generator would not have followed
    m3 = RecurrentPPO.load(path, env=StubEnv(n_envs=N, obs_dim=D))
    m3.gen.manual_seed(99)
    fill(m3, 11)
    m3.train()
    assert not all(torch.equal(p, q) for p, q in zip(m.policy.parameters(), m3.policy.parameters()))


def test_predict_only_model(trained):
    m, path, _ = trained
    p = RecurrentPPO.load(path, env=None, device="cpu")
    assert p.predict_only and p.env is None and p.device.type == "cpu" and p.fused_step is False
    obs = np.random.default_rng(0).normal(size=(6, D)).astype(np.float32)
    want, ws = m.predict(obs)
    got, gs = p.predict(obs)
    assert np.array_equal(got, want) and got.shape == (6, 3) and torch.equal(ws, gs)
    assert np.array_equal(p.predict(obs[0])[0], m.predict(obs[0])[0])
    for call in (lambda: p.learn(8), lambda: p.evaluate(StubEnv())):
        with pytest.raises(RuntimeError, match="env"):
            call()


def test_load_rejects_a_foreign_file(tmp_path, trained):
    for tag in ({"format": "grasp_lab_salp_amd.SAC", "version": 1}, {"format": "grasp_lab_salp_amd.RecurrentPPO",
                                                                     "version": 2}):
        f = tmp_path / "x.zip"
        with zipfile.ZipFile(f, "w") as z:
            z.writestr("data.json", json.dumps(tag))
        with pytest.raises(ValueError, match="grasp_lab_salp_amd.RecurrentPPO"):
            RecurrentPPO.load(str(f), env=StubEnv())
