"""The SAC learner's host side and its plain torch restatements on the CPU
(grasp_lab_salp_amd/sac.py): the sampler's integer draw against Philox, the
index-op replay ring against the NumPy one (tests/sac_ref.py), the torch_*
heads in float64 against the closed-form gradients of include/salp.h, and the
constructor's SB3 surface."""
import numpy as np
import pytest
import torch

import sac_ref
from grasp_lab_salp_amd import sac


def test_numpy_philox_equals_the_oracle():
    from oracle.oracle import philox
    ctrs = [(0, 0, 0, 0), (1, 2, 3, 4), (0xFFFFFFFF,) * 4, (123456789, 7, 77, sac.REPLAY_STREAM),
            (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344)]
    for key in ((0, 0), (0xDEADBEEF, 0x12345678), (0xFFFFFFFF, 0xFFFFFFFF)):
        got = sac_ref.philox4x32_10(ctrs, key)
        for c, g in zip(ctrs, got):
            assert [int(x) for x in g] == [int(x) for x in philox(c, key)], (c, key)
    # the torch restatement the fused=False sampler uses
    c = torch.tensor(ctrs, dtype=torch.int64)
    out = torch.stack(sac._philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], 0xDEADBEEF, 0x12345678), 1)
    assert np.array_equal(out.numpy().astype(np.uint64), sac_ref.philox4x32_10(ctrs, (0xDEADBEEF, 0x12345678)))


@pytest.mark.parametrize("size", [[4, 0, 2], [0, 0, 5], [1, 1, 1, 1, 1, 1, 1], [3]])
def test_torch_sample_indices_equal_the_restatement(size):
    for update in (0, 1, (1 << 32) + 5):
        for seed in (0, 7, -3, (1 << 63) + 11):
            env, slot = sac.torch_replay_indices(torch.tensor(size), torch.tensor([update]), seed, 257)
            e, s = sac_ref.sample_indices(size, update, seed, 257)
            assert np.array_equal(env.numpy(), e) and np.array_equal(slot.numpy(), s)
            assert all(size[i] > 0 for i in e) and (s < np.asarray(size)[e]).all()
    a = sac_ref.sample_indices(size, 0, 0, 257)
    b = sac_ref.sample_indices(size, 1, 0, 257)
    if sum(size) > 3:
        assert not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


@pytest.mark.parametrize("obs_dim", [10, 14])
def test_index_op_ring_equals_the_restatement(obs_dim):
    n, cap = 3, 4
    rb = sac.ReplayBuffer(cap * n, n, obs_dim, "cpu", seed=5)
    assert rb.capacity == cap and not rb.fused
    ref = sac_ref.Ring(cap, n, obs_dim)
    for t, s in enumerate(sac_ref.replay_script(n, obs_dim, 7)):
        bad = rb.add(*(torch.from_numpy(s[k]) for k in ("obs", "actions", "obs_after", "terminal_obs", "reward",
                                                         "terminated", "truncated")))
        want = ref.add(**s)
        assert np.array_equal(bad.numpy(), want), t
        for k in ("obs", "next_obs", "actions", "rewards", "dones", "pos", "size"):
            assert np.array_equal(getattr(rb, k).numpy(), getattr(ref, k), equal_nan=True), (t, k)
    # the last env never stored; env 0 stored 4 of 7 steps, env 1 5 of 7 (wrapped around, cursors apart)
    assert ref.size.tolist() == [cap, cap, 0] and ref.pos.tolist() == [0, 1, 0]
    upd = torch.tensor([3])
    *rows, env, slot = rb.sample(257, upd, return_indices=True)
    e, sl = sac_ref.sample_indices(ref.size, 3, 5, 257)
    assert np.array_equal(env.numpy(), e) and np.array_equal(slot.numpy(), sl) and (e != n - 1).all()
    for got, want in zip(rows, ref.rows(e, sl)):
        assert np.array_equal(got.numpy(), want)


def test_capacity_rule():
    for size, n, want in ((100000, 8, 12500), (100000, 4096, 24), (10, 64, 1), (512, 64, 8)):
        assert sac.ReplayBuffer(size, n, 6, "cpu").capacity == want


def test_action_scaling_round_trip():
    low, high = torch.tensor([0.0, 0.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    a = torch.rand(100, 3, generator=torch.Generator().manual_seed(0)) * (high - low) + low
    s = sac.scale_action(a, low, high)
    assert float(s.min()) >= -1 and float(s.max()) <= 1
    assert torch.allclose(sac.unscale_action(s, low, high), a, atol=1e-6)
    assert torch.equal(sac.unscale_action(torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), low, high), torch.stack([low, high]))


def _head_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    mu = (torch.rand(B, 3, generator=g, dtype=torch.float64) * 2 - 1) * 3
    ls = torch.rand(B, 3, generator=g, dtype=torch.float64) * 28 - 25      # -25 .. 3: both clamp regions
    ls[0] = torch.tensor([-20.0, 2.0, -20.0])                              # the closed ends pass the gradient
    eps = torch.randn(B, 3, generator=g, dtype=torch.float64)
    return mu, ls, eps, g


def test_torch_squashed_gaussian_gradients_are_the_closed_form():
    B = 64
    mu, ls, eps, g = _head_inputs(B, 1)
    assert (ls < -20).any() and (ls > 2).any() and ((ls > -20) & (ls < 2)).any()
    mu.requires_grad_(True)
    ls.requires_grad_(True)
    a, logp = sac.torch_squashed_gaussian(mu, ls, eps)
    da, dlogp = torch.randn(B, 3, generator=g, dtype=torch.float64), torch.randn(B, generator=g, dtype=torch.float64)
    torch.autograd.backward((a, logp), (da, dlogp))
    want_lp, dmu, dls = sac_ref.actor_head(ls.detach().numpy(), eps.numpy(), a.detach().numpy(), da.numpy(),
                                           dlogp.numpy())
    np.testing.assert_allclose(logp.detach().numpy(), want_lp, rtol=1e-12, atol=1e-12)
    # Both sides form 1 - a^2 in float64 from the same a, in their own operation order: a^2 rounds
    # by <= 1.1e-16, which the 1 / (1 - a^2 + 1e-6) of the log term's gradient amplifies by up to
    # 1e6 and 2 |dlogp| <= 10: 1e-8 absolute on du, times |d u / d ls| = exp(ls) |eps| on dls.
    np.testing.assert_allclose(mu.grad.numpy(), dmu, rtol=1e-10, atol=1e-8)
    scale = 1 + np.exp(np.clip(ls.detach().numpy(), -20, 2)) * np.abs(eps.numpy())
    assert (np.abs(ls.grad.numpy() - dls) <= 1e-10 * np.abs(dls) + 1e-8 * scale).all()
    outside = ((ls < -20) | (ls > 2)).detach().numpy()
    assert (ls.grad.numpy()[outside] == 0).all() and (ls.grad.numpy()[0] != 0).all()


def test_torch_td_and_pi_heads_are_the_closed_form():
    B = 33
    g = torch.Generator().manual_seed(2)
    r, q1t, q2t, lpn, q1, q2, lp = (torch.randn(B, generator=g, dtype=torch.float64) * 3 for _ in range(7))
    d = (torch.rand(B, generator=g) < 0.3).double()
    q2t[:5] = q1t[:5]
    la = torch.tensor([-0.7], dtype=torch.float64, requires_grad=True)
    q1.requires_grad_(True)
    q2.requires_grad_(True)
    closs, eloss, target, alpha = sac.torch_td_head(r, d, q1t, q2t, lpn, q1, q2, lp, la, 0.99, -3.0)
    (closs + eloss).backward()
    t, dq1, dq2, cl, el, dla, al = sac_ref.td_head(*(x.detach().numpy() for x in (r, d, q1t, q2t, lpn, q1, q2, lp)),
                                                   -0.7, 0.99, -3.0)
    for got, want in ((target, t), (q1.grad, dq1), (q2.grad, dq2), (closs, cl), (eloss, el), (la.grad, dla),
                      (alpha, al)):
        np.testing.assert_allclose(got.detach().numpy().reshape(-1), np.asarray(want).reshape(-1), rtol=1e-12)
    # pi head, with q1 == q2 ties: the whole -1/B goes to q1
    q1p, q2p = (torch.randn(B, generator=g, dtype=torch.float64) for _ in range(2))
    q2p[:7] = q1p[:7]
    lp2 = lp.clone().requires_grad_(True)
    q1p.requires_grad_(True)
    q2p.requires_grad_(True)
    loss = sac.torch_pi_head(alpha, lp2, q1p, q2p)
    loss.backward()
    want = sac_ref.pi_head(al, lp.numpy(), q1p.detach().numpy(), q2p.detach().numpy())
    for got, w in zip((loss, lp2.grad, q1p.grad, q2p.grad), want):
        np.testing.assert_allclose(got.detach().numpy().reshape(-1), np.asarray(w).reshape(-1), rtol=1e-12)
    assert (q1p.grad[:7] == -1.0 / B).all() and (q2p.grad[:7] == 0).all()


def test_torch_polyak():
    p, t = [torch.ones(5, dtype=torch.float64)], [torch.zeros(5, dtype=torch.float64)]
    sac.torch_polyak(p, t, 0.005)
    sac.torch_polyak(p, t, 0.005)
    np.testing.assert_allclose(t[0].numpy(), 0.005 * 0.995 + 0.005, rtol=1e-15)


class _Sim:
    n_envs, obs_dim, device = 8, 10, torch.device("cpu")


class _Env:
    sim = _Sim()


def test_constructor_takes_the_training_scripts_keywords():
    """src/train_robot.py:62-69, unchanged."""
    m = sac.SAC("MlpPolicy", _Env(), verbose=1, tensorboard_log="../experiments/v5/logs", learning_rate=3e-4,
                buffer_size=100000, learning_starts=1000, batch_size=256, tau=0.005, gamma=0.99, train_freq=1,
                gradient_steps=1, device="auto")
    assert not m.fused and m.replay.capacity == 12500 and m.target_entropy == -3.0
    assert float(m.log_ent_coef.detach()) == 0.0 and m.ent_coef_opt is not None
    pol = m.policy
    assert [tuple(p.shape) for p in pol.actor.parameters()] == [(256, 10), (256,), (256, 256), (256,), (3, 256), (3,),
                                                                (3, 256), (3,)]
    assert [tuple(p.shape) for p in pol.critic.qf1.parameters()] == [(256, 13), (256,), (256, 256), (256,), (1, 256),
                                                                     (1,)]
    assert pol.critic.is_flat() and pol.critic_target.is_flat()
    assert torch.equal(pol.critic.flat, pol.critic_target.flat) and not any(
        p.requires_grad for p in pol.critic_target.parameters())
    with pytest.raises(ValueError):
        sac.SAC("MlpPolicy", _Env(), fused=True)     # HIP kernels need a GPU: no quiet fall-back
    with pytest.raises(ValueError):
        sac.SAC("MlpPolicy", _Env(), train_freq=(1, "episode"))
    assert sac.SAC("MlpPolicy", _Env(), ent_coef=0.2).ent_coef_opt is None
    assert abs(float(sac.SAC("MlpPolicy", _Env(), ent_coef="auto_0.1").log_ent_coef.detach()) - np.log(0.1)) < 1e-6


def test_plain_gradient_step_moves_everything_once():
    """fused=False on the CPU: one gradient step changes actor, critics, alpha
    and (by tau) the target, which stays a view of its flat buffer."""
    m = sac.SAC("MlpPolicy", _Env(), batch_size=32, buffer_size=64)
    g = torch.Generator().manual_seed(0)
    for _ in range(3):
        m.replay.add(torch.randn(8, 10, generator=g), torch.rand(8, 3, generator=g) * 2 - 1,
                     torch.randn(8, 10, generator=g), torch.randn(8, 10, generator=g),
                     torch.randn(8, generator=g, dtype=torch.float64), torch.zeros(8, dtype=torch.uint8),
                     torch.zeros(8, dtype=torch.uint8))
    before = {k: v.clone() for k, v in m.policy.state_dict().items()}
    t0 = m.policy.critic_target.flat.clone()
    c0 = m.policy.critic.flat.clone()
    m.gradient_step(m.replay.sample(32, m._update))
    after = m.policy.state_dict()
    assert all(not torch.equal(before[k], after[k]) for k in before)
    assert float(m.log_ent_coef.detach()) != 0.0 and int(m._update) == 1
    assert m.policy.critic_target.is_flat()
    want = t0 * (1 - 0.005) + 0.005 * m.policy.critic.flat
    assert torch.allclose(m.policy.critic_target.flat, want, rtol=1e-6, atol=1e-9) and not torch.equal(c0, m.policy.critic.flat)
    a, _ = m.predict(np.zeros((4, 10), np.float32))
    assert a.shape == (4, 3) and (a >= [0, 0, -1]).all() and (a <= [1, 1, 1]).all()


def test_plain_log_alpha_gradient_does_not_accumulate(monkeypatch):
    """Three plain gradient steps: after each, log_ent_coef.grad is
    -mean(logp + target_entropy) of that step's batch alone, and the
    coefficient's Adam has stepped once per gradient step."""
    m = sac.SAC("MlpPolicy", _Env(), batch_size=32, buffer_size=64)
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        m.replay.add(torch.randn(8, 10, generator=g), torch.rand(8, 3, generator=g) * 2 - 1,
                     torch.randn(8, 10, generator=g), torch.randn(8, 10, generator=g),
                     torch.randn(8, generator=g, dtype=torch.float64), torch.zeros(8, dtype=torch.uint8),
                     torch.zeros(8, dtype=torch.uint8))
    states, orig = [], sac.critic_phase

    def recording(*a, **kw):
        states.append(orig(*a, **kw))
        return states[-1]

    monkeypatch.setattr(sac, "critic_phase", recording)
    grads = []
    for k in range(3):
        m.gradient_step(m.replay.sample(32, m._update))
        want = -(states[-1]["logp"].detach() + m.target_entropy).mean()
        assert torch.allclose(m.log_ent_coef.grad, want.reshape(1), rtol=1e-6, atol=0), (k, m.log_ent_coef.grad, want)
        grads.append(float(m.log_ent_coef.grad))
    assert len(states) == 3 and max(grads) < 1.5 * min(grads)       # a running sum would triple
    assert int(m.ent_coef_opt.state[m.log_ent_coef]["step"]) == 3


def test_building_a_learner_leaves_the_global_generator_alone():
    torch.manual_seed(123)
    want = torch.rand(4)
    torch.manual_seed(123)
    a = sac.SAC("MlpPolicy", _Env(), seed=5)
    assert torch.equal(torch.rand(4), want)
    b = sac.SAC("MlpPolicy", _Env(), seed=5)
    assert all(torch.equal(p, q) for p, q in zip(a.policy.parameters(), b.policy.parameters()))
    c = sac.SAC("MlpPolicy", _Env(), seed=6)
    assert not torch.equal(next(a.policy.parameters()), next(c.policy.parameters()))
