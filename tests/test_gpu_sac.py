"""The SAC kernels (csrc/salp_sac.hip) and the learner (grasp_lab_salp_amd/
sac.py) on the GPU: the replay ring and sampler bit for bit against the NumPy
restatement (tests/sac_ref.py), the heads and Polyak against float64 closed
forms within bounds counted in float32 roundings (u = 2^-24), one gradient
step against plain torch in float32 and float64, and a short run.

Inputs come from seeded CPU generators.  Lines starting with "[sac]"
(pytest -s) print the measured figures."""
import copy

import numpy as np
import pytest
import torch

import sac_ref
from grasp_lab_salp_amd import sac

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24


def _np(t):
    return t.detach().cpu().numpy()


# -------------------------------------------------------------------- replay
@pytest.mark.parametrize("obs_dim", [10, 14])
def test_replay_ring_and_sampler_are_bit_equal_to_the_restatement(obs_dim):
    """3 envs x 4 slots, 7 adds (sac_ref.replay_script: terminated-only,
    truncated-only and both-flag rows, staggered divergence, the last env
    never stores): rings and cursors after every add, wrap-around included;
    then batches of 1 and 257 rows for two update values."""
    n, cap = 3, 4
    rb = sac.ReplayBuffer(cap * n, n, obs_dim, DEV, seed=5)
    assert rb.fused and rb.capacity == cap
    ref = sac_ref.Ring(cap, n, obs_dim)
    keys = ("obs", "actions", "obs_after", "terminal_obs", "reward", "terminated", "truncated")
    for t, s in enumerate(sac_ref.replay_script(n, obs_dim, 7)):
        bad = rb.add(*(torch.from_numpy(s[k]).to(DEV) for k in keys))
        want = ref.add(**s)
        assert np.array_equal(_np(bad).astype(bool), want), t
        for k in ("obs", "next_obs", "actions", "rewards", "dones", "pos", "size"):
            assert np.array_equal(_np(getattr(rb, k)), getattr(ref, k), equal_nan=True), (t, k)
    assert ref.size.tolist() == [cap, cap, 0] and ref.pos.tolist() == [0, 1, 0]
    upd = torch.zeros(1, dtype=torch.int64, device=DEV)
    seen = {}
    for B in (1, 257):
        for u in (3, (1 << 32) + 9):
            upd.fill_(u)
            *rows, env, slot = rb.sample(B, upd, return_indices=True)
            e, sl = sac_ref.sample_indices(ref.size, u, 5, B)
            assert np.array_equal(_np(env), e) and np.array_equal(_np(slot), sl), (B, u)
            assert (e != n - 1).all()                     # no row from the env that never stored
            for got, want in zip(rows, ref.rows(e, sl)):
                assert np.array_equal(_np(got), want), (B, u)
            plain = rb.sample(B, upd)                      # without the index outputs: the same rows
            assert all(torch.equal(a, b) for a, b in zip(plain, rows))
            seen[(B, u)] = (e, sl)
    a, b = seen[(257, 3)], seen[(257, (1 << 32) + 9)]
    assert not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


# ---------------------------------------------------------------- actor head
@pytest.mark.parametrize("B", [1, 63, 257])
def test_actor_head_equals_the_closed_form(B):
    """|mu| <= 10, |eps| <= 5, raw log-std over -25 .. 3 with exact -20 and 2.
    a against float64 tanh(mu + exp(ls) eps) within the rtol 1e-5 / atol 1e-6 of
    test_lstm_cell_kernels_equal_torch_lstm; logp and both gradients against
    the float64 formula evaluated at the kernel's own a (a tanh difference is
    not amplified through log(1 - a^2)) within 3e-5 (1 + |ref|): about 16
    float32 roundings on terms bounded by 32.  dls is exactly 0 outside the
    clamp."""
    g = torch.Generator().manual_seed(100 + B)
    mu = (torch.rand(B, 3, generator=g) * 2 - 1) * 10
    eps = (torch.rand(B, 3, generator=g) * 2 - 1) * 5
    ls = torch.rand(B, 3, generator=g) * 28 - 25
    ls[0, 0], ls[0, 1] = -20.0, 2.0
    da, dlogp = torch.randn(B, 3, generator=g), torch.randn(B, generator=g)
    mu_d, ls_d = mu.to(DEV).requires_grad_(True), ls.to(DEV).requires_grad_(True)
    a, logp = sac.squashed_gaussian(mu_d, ls_d, eps.to(DEV))
    torch.autograd.backward((a, logp), (da.to(DEV), dlogp.to(DEV)))
    a_k, ls64 = _np(a).astype(np.float64), np.clip(ls.double().numpy(), -20, 2)
    a_ref = np.tanh(mu.double().numpy() + np.exp(ls64) * eps.double().numpy())
    print(f"[sac] actor head B={B}: max |a - tanh64| {np.abs(a_k - a_ref).max():.3g}")
    np.testing.assert_allclose(a_k, a_ref, rtol=1e-5, atol=1e-6)
    lp_ref, dmu_ref, dls_ref = sac_ref.actor_head(ls.numpy(), eps.numpy(), a_k, da.numpy(), dlogp.numpy())
    for name, got, ref in (("logp", logp, lp_ref), ("dmu", mu_d.grad, dmu_ref), ("dls", ls_d.grad, dls_ref)):
        err = np.abs(_np(got).astype(np.float64) - ref) / (1 + np.abs(ref))
        print(f"[sac] actor head B={B}: {name} worst error / (1 + |ref|) {err.max():.3g} (bound 3e-5)")
        assert (err <= 3e-5).all(), name
    outside = (ls.numpy() < -20) | (ls.numpy() > 2)
    assert (B == 1 or outside.any()) and (_np(ls_d.grad)[outside] == 0).all()
    assert _np(ls_d.grad)[0, 0] != 0 and _np(ls_d.grad)[0, 1] != 0      # the closed ends pass the gradient


# ------------------------------------------------------------- TD / pi heads
# (the heads cap their grid at 64 blocks of 256 rows: 16385 and 49153 are the second and fourth stride passes)
@pytest.mark.parametrize("B", [1, 257, 4097, 16385, 49153])
def test_td_and_pi_heads_equal_fp64(B):
    """Mixed dones, q1 == q2 ties in the target critics and in the actor pass.
    Float32 roundings per element, u = 2^-24, against float64 on the same
    float32 inputs, with M = |r| + gamma (|min q_t| + alpha |logp'|):
      target  expf (2 ulp = 4 u on alpha logp'), the inner fmaf, float32 gamma,
              the outer fmaf: <= 7 u M, bound 8 u M;
      dq      target's error, the subtraction, 1 / B and the product:
              (8 u M + 3 u (|q| + |t|)) / B;
      dlogp   expf, 1 / B, the product: 8 u alpha / B;  -1 / B: 2 u / B.
    Scalar losses within 1e-6 relative (fp64 sums of exact row terms).  A
    second launch on the same inputs gives the same bits."""
    g = torch.Generator().manual_seed(200 + B)
    r, q1t, q2t, lpn, q1, q2, lp, q1p, q2p = (torch.randn(B, generator=g) * 3 for _ in range(9))
    d = (torch.rand(B, generator=g) < 0.3).float()
    tie = torch.rand(B, generator=g) < 0.2
    q2t = torch.where(tie, q1t, q2t)
    q2p = torch.where(tie, q1p, q2p)
    if B == 1:
        q2p = q1p.clone()
    la, gamma, tent = -0.7, 0.99, -3.0
    dv = lambda *ts: [t.to(DEV) for t in ts]  # noqa: E731
    args = dv(r, d, q1t, q2t, lpn, q1, q2, lp) + [torch.tensor([la], device=DEV), gamma, tent]
    out, target, dq1, dq2, alpha = sac.td_head(*args)
    again = sac.td_head(*args)
    assert all(torch.equal(x, y) for x, y in zip((out, target, dq1, dq2, alpha), again))
    n64 = [x.double().numpy() for x in (r, d, q1t, q2t, lpn, q1, q2, lp)]
    t_ref, dq1_ref, dq2_ref, cl, el, dla, al = sac_ref.td_head(*n64, np.float32(la), gamma, tent)
    M = np.abs(n64[0]) + gamma * (np.abs(np.minimum(n64[2], n64[3])) + al * np.abs(n64[4]))
    assert abs(float(alpha) - al) <= 4 * U * al
    et = np.abs(_np(target) - t_ref)
    print(f"[sac] td head B={B}: target worst error / (u M) {(et / (U * M)).max():.3g} (bound 8)")
    assert (et <= 8 * U * M).all()
    for q, dq, ref in ((n64[5], dq1, dq1_ref), (n64[6], dq2, dq2_ref)):
        lim = (8 * U * M + 3 * U * (np.abs(q) + np.abs(t_ref))) / B
        assert (np.abs(_np(dq) - ref) <= lim).all()
    for name, got, ref in (("critic_loss", out[0], cl), ("ent_coef_loss", out[1], el), ("d_log_alpha", out[2], dla)):
        rel = abs(float(got) - ref) / abs(ref)
        print(f"[sac] td head B={B}: {name} relative error {rel:.3g} (bound 1e-6)")
        assert rel <= 1e-6, (name, float(got), ref)
    # pi head on the coefficient the td head wrote
    pargs = [alpha] + dv(lp, q1p, q2p)
    pout, dlogp, dp1, dp2 = sac.pi_head(*pargs)
    assert all(torch.equal(x, y) for x, y in zip((pout, dlogp, dp1, dp2), sac.pi_head(*pargs)))
    loss, dlp_ref, d1_ref, d2_ref = sac_ref.pi_head(float(alpha), lp.numpy(), q1p.numpy(), q2p.numpy())
    rel = abs(float(pout[0]) - loss) / abs(loss)
    print(f"[sac] pi head B={B}: actor_loss relative error {rel:.3g} (bound 1e-6)")
    assert rel <= 1e-6
    assert (np.abs(_np(dlogp) - dlp_ref) <= 8 * U * float(alpha) / B).all()
    assert (np.abs(_np(dp1) - d1_ref) <= 2 * U / B).all() and (np.abs(_np(dp2) - d2_ref) <= 2 * U / B).all()
    ties = (q1p == q2p).numpy()
    assert ties.any() and (_np(dp1)[ties] != 0).all() and (_np(dp2)[ties] == 0).all()
    assert ((_np(dp1) != 0) ^ (_np(dp2) != 0)).all()     # exactly one of the two gets the row's -1 / B


# -------------------------------------------------------------------- polyak
# (the grid is capped at 1024 blocks of 256 elements: 262145 and 524295 are the second and third stride passes)
@pytest.mark.parametrize("n", [1, 255, 70003, 262145, 524295])
def test_polyak_equals_fp64(n):
    """Within 2 ulp (float32) of target (1 - tau) + tau param in float64, the
    ulp taken at max(|target|, |param|): 1 - tau rounded from double (0.5), the
    product (0.5) and the fused multiply-add (0.5), tau's own rounding on the
    smaller addend."""
    g = torch.Generator().manual_seed(300 + n)
    p, t = torch.randn(n, generator=g), torch.randn(n, generator=g) * 2
    for tau in (0.005, 1.0, 0.3):
        ref = t.double() * (1 - tau) + tau * p.double()
        out = sac.polyak(p.to(DEV), t.clone().to(DEV), tau).cpu()
        big = torch.maximum(t.abs(), p.abs())
        ulp = (torch.nextafter(big, torch.full_like(big, float("inf"))) - big).double()
        err = ((out.double() - ref).abs() / ulp).max()
        print(f"[sac] polyak n={n} tau={tau}: worst error {float(err):.3g} ulp (bound 2)")
        assert float(err) <= 2.0
    same = sac.polyak(p.to(DEV), t.clone().to(DEV), 0.0).cpu()
    assert torch.equal(same, t)


# ------------------------------------------------------------------- learner
@pytest.fixture(scope="module")
def learner():
    """SAC on 64 envs after three collected env-steps (192 transitions, no update yet)."""
    from grasp_lab_salp_amd.vec_env import SalpVecEnv
    m = sac.SAC("MlpPolicy", SalpVecEnv(64, seed=3), learning_starts=128, batch_size=64, buffer_size=512, seed=1)
    assert m.fused and m.replay.capacity == 8
    for _ in range(3):
        m.collect_step()
    torch.cuda.synchronize()
    return m


def _grads_of(pol, la):
    out = {"actor." + k: p.grad for k, p in pol.actor.named_parameters()}
    out.update({"critic." + k: p.grad for k, p in pol.critic.named_parameters()})
    out["log_alpha"] = la.grad
    return {k: v.detach().double().clone() for k, v in out.items()}


def _three_losses_and_grads(pol, la, batch, eps, fused):
    for p in list(pol.parameters()) + [la]:
        p.grad = None
    st = sac.critic_phase(pol, la, batch, eps[0], eps[1], 0.99, -3.0, fused)
    actor_loss = sac.actor_phase(pol, st, fused)
    losses = {"critic_loss": st["critic_loss"], "ent_coef_loss": st["ent_coef_loss"], "actor_loss": actor_loss}
    return {k: float(v) for k, v in losses.items()}, _grads_of(pol, la)


def test_one_gradient_step_equals_plain_torch_and_fp64(learner):
    """The three losses and every actor / critic / alpha gradient of one
    sampled batch, before any optimizer step: fused, plain torch in float32 and
    plain torch on a float64 copy.  Per tensor, the fused path's error against
    float64 over the tensor's largest float64 entry (test_gpu_ppo_mlp_ref.
    _check_grads) is at most 4 x the plain float32 path's (another, fixed,
    summation order) plus a floor of 4 u = 2.4e-7: on a tensor where plain
    torch happens to round luckily (the first run had it at 2.2e-8 on a bias)
    the fused path still may differ by a few roundings of the top entry.  The
    first run's fused errors were 2.2e-8 .. 5.0e-7 against 2.2e-8 .. 1.5e-6, so
    above the floor it is the ratio that decides."""
    m = learner
    assert m.n_updates == 0 and int(m.replay.size.min()) == 3
    batch = m.replay.sample(64, m._update)
    g = torch.Generator().manual_seed(7)
    eps = [torch.randn(64, 3, generator=g).to(DEV) for _ in range(2)]
    la = torch.full((1,), -0.7, device=DEV, requires_grad=True)
    pol64 = copy.deepcopy(m.policy).double()
    la64 = la.detach().double().requires_grad_(True)
    l_f, g_f = _three_losses_and_grads(m.policy, la, batch, eps, True)
    l_p, g_p = _three_losses_and_grads(m.policy, la, batch, eps, False)
    l_d, g_d = _three_losses_and_grads(pol64, la64, tuple(t.double() for t in batch), [e.double() for e in eps],
                                       False)
    for p in m.policy.parameters():
        p.grad = None
    bad = []
    for k in l_d:
        ef, ep = abs(l_f[k] - l_d[k]) / abs(l_d[k]), abs(l_p[k] - l_d[k]) / abs(l_d[k])
        print(f"[sac] gradient step: {k} {l_d[k]:.6g}: fused {ef:.3g}, float32 torch {ep:.3g}")
        if not ef <= 4 * ep + 4 * U:
            bad.append((k, ef, ep))
    for k, ref in g_d.items():
        top = float(ref.abs().max())
        assert top > 0, k
        ef, ep = float((g_f[k] - ref).abs().max()) / top, float((g_p[k] - ref).abs().max()) / top
        print(f"[sac] gradient step: {k}: fused {ef:.3g}, float32 torch {ep:.3g}")
        if not ef <= 4 * ep + 4 * U:
            bad.append((k, ef, ep))
    assert not bad, f"(tensor, fused error, float32 torch error) against fp64: {bad}"


def test_log_alpha_gradient_is_one_batch_on_both_paths(learner):
    """critic_phase twice in a row with nothing clearing log_alpha.grad between:
    after the second call it holds -mean(logp + target_entropy) of that batch
    alone, fused and plain alike (a plain path that accumulated would hold
    twice that).  Against the float64 mean of the path's own float32 logp: 8 u
    relative (plain torch adds target_entropy per row, sums 64 same-signed
    float32 terms in a tree, log2(64) = 6 roundings, and divides; the fused
    head's sum is fp64 and rounds once)."""
    m = learner
    batch = m.replay.sample(64, m._update)
    g = torch.Generator().manual_seed(11)
    eps = [torch.randn(64, 3, generator=g).to(DEV) for _ in range(2)]
    got = {}
    for fused in (True, False):
        la = torch.full((1,), -0.7, device=DEV, requires_grad=True)
        for _ in range(2):
            st = sac.critic_phase(m.policy, la, batch, eps[0], eps[1], 0.99, -3.0, fused)
        want = -float((st["logp"].detach().double() - 3.0).mean())
        got[fused] = float(la.grad)
        assert abs(got[fused] - want) <= 8 * U * abs(want), (fused, got[fused], want)
    for p in m.policy.parameters():
        p.grad = None
    assert abs(got[True] - got[False]) <= 1e-5 * abs(got[False])     # the two heads' logp differ by roundings


def test_short_run(learner):
    """40 env-steps with one gradient step each after learning_starts."""
    m = learner
    target0 = m.policy.critic_target.flat.clone()
    log, add = [], m.replay.add

    def recording_add(*a, **kw):
        bad = add(*a, **kw)
        log.append((a[6].bool().cpu().numpy(), bad.bool().cpu().numpy()))   # truncated, dropped
        return bad

    m.replay.add = recording_add
    try:
        m.learn(40 * 64)
    finally:
        m.replay.add = add
    torch.cuda.synchronize()
    assert m.num_timesteps == 43 * 64 and m.n_updates == 40 and int(m._update) == 40
    assert all(bool(torch.isfinite(p).all()) for p in m.policy.parameters()) and bool(torch.isfinite(m.log_ent_coef))
    assert float(m.log_ent_coef.detach()) != 0.0
    pol = m.policy
    assert pol.critic.is_flat() and pol.critic_target.is_flat()
    assert not torch.equal(pol.critic_target.flat, pol.critic.flat)
    assert not torch.equal(pol.critic_target.flat, target0)
    rb = m.replay
    size, pos = _np(rb.size), _np(rb.pos)
    assert (size <= rb.capacity).all() and size.max() == rb.capacity
    # chronology per env from the recorded flags: where a stored transition did not end its episode
    # and the env's next step was stored too, its next_obs is that step's obs
    obs, nxt, dones = _np(rb.obs), _np(rb.next_obs), _np(rb.dones)
    checked = 0
    for e in range(m.n_envs):
        stored = [t for t, (_, dropped) in enumerate(log) if not dropped[e]]
        assert len(stored) >= size[e] == rb.capacity
        held = stored[len(stored) - size[e]:]                       # the ring keeps the last size[e] of them
        slot = {t: (pos[e] - (len(held) - i)) % rb.capacity for i, t in enumerate(held)}
        for t0, t1 in zip(held, held[1:]):
            if t1 == t0 + 1 and dones[slot[t0], e] == 0 and not log[t0][0][e]:
                assert np.array_equal(nxt[slot[t0], e], obs[slot[t1], e]), (e, t0)
                checked += 1
    assert checked >= 64 * 4
    low, high = np.array([0, 0, -1], np.float32), np.array([1, 1, 1], np.float32)
    a, _ = m.predict(_np(m._obs), deterministic=True)
    assert a.shape == (64, 3) and (a >= low).all() and (a <= high).all()
    one, _ = m.predict(_np(m._obs)[0])
    assert one.shape == (3,) and (one >= low).all() and (one <= high).all()
    assert m.history and m.history[-1]["timesteps"] == m.num_timesteps and m.timing["update_s"] > 0
