"""salp_lstm_policy_step (csrc/salp_lstm.hip) against the module it fuses,
``RecurrentActorCritic.act`` / ``predict_values``.

Reference: a float64 copy of the same module on the CPU with the same noise.
Bound: per tensor, the largest error over the tensor's largest
float64 magnitude is at most 4 x the same figure of the float32 torch path on
the GPU, plus 4 u, u = 2^-24.  Rows: 1, 4, 31, 32, 33, 65 (below, at and past
one and two tiles of 32 rows) and 1057 = 33 tiles + 1 row: the cell kernel
splits the rows over at most 32 workgroups per unit group, so from 33 tiles on
a workgroup loops over row tiles with its weights kept (here workgroups 0 and 1
take two tiles, the second of workgroup 1 a ragged one)."""
import copy
import ctypes

import pytest
import torch

from grasp_lab_salp_amd import _lib
from grasp_lab_salp_amd.recurrent_ppo import FusedPolicyStep, RecurrentActorCritic

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
H = 256
ROWS = (1, 4, 31, 32, 33, 65, 1057)
OBS_DIMS = (6, 10, 16)
PAD, SENTINEL = 7, 12345.0
NAMES = ("action", "log_prob", "value", "actor_h", "actor_c", "critic_h", "critic_c")


def _policy(obs_dim):
    torch.manual_seed(100 + obs_dim)
    pol = RecurrentActorCritic(obs_dim, 3)
    with torch.no_grad():
        pol.log_std.uniform_(-2.0, 0.5)
        for m in (pol.pi_net[0], pol.pi_net[2], pol.vf_net[0], pol.vf_net[2], pol.action_net, pol.value_net):
            m.bias.uniform_(-0.1, 0.1)      # (the module's init zeroes them: a bias bug would not show)
    return pol


@pytest.fixture(scope="module")
def policies():
    """obs_dim -> (float64 CPU module, float32 GPU module)."""
    out = {}
    for d in OBS_DIMS:
        pol = _policy(d)
        out[d] = (copy.deepcopy(pol).double(), copy.deepcopy(pol).cuda())
    return out


def _inputs(rows, obs_dim, keep_mode):
    g = torch.Generator().manual_seed(rows * 31 + obs_dim)
    obs = torch.randn(rows, obs_dim, generator=g)
    state = 0.5 * torch.randn(4, rows, H, generator=g)
    eps = torch.randn(rows, 3, generator=g)
    keep = {"ones": torch.ones(rows), "zeros": torch.zeros(rows),
            "mixed": (torch.rand(rows, generator=g) < 0.5).float()}[keep_mode]
    return obs, state, eps, keep


def _module_step(pol, obs, state, eps, keep):
    """act() with the given noise: (action, log_prob, value, new state)."""
    with torch.no_grad():
        lp, lv, new = pol.forward_seq(obs.unsqueeze(0), state, (1.0 - keep).unsqueeze(0))
        d = pol._dist(lp[0])
        a = d.mean if eps is None else d.mean + d.stddev * eps
        return a, d.log_prob(a).sum(-1), pol._value(lv[0]), new


class _Guarded:
    """A NaN-filled [rows, ...] tensor between two canary blocks."""

    def __init__(self, *shape):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, device="cuda")
        self.t = self.buf[PAD:PAD + n].view(*shape)
        self.t.fill_(float("nan"))

    def intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[-PAD:] == SENTINEL).all())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.t).all())


def _run(pol, obs, state, keep=None, eps=None, actor=True, critic=True, advance=True):
    """One salp_lstm_policy_step call into guarded buffers: {name: _Guarded}."""
    rows, od = obs.shape
    fs = FusedPolicyStep(pol, rows, obs.device)
    out = {"action": _Guarded(rows, 3), "log_prob": _Guarded(rows), "value": _Guarded(rows),
           "state": _Guarded(4, rows, H), "latent": _Guarded(2, rows, H)}
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    s = _lib.SalpLstmPolicyStep(rows=rows, obs_dim=od, act_dim=3, obs=ptr(obs), keep=ptr(keep), state_in=ptr(state),
                                state_out=ptr(out["state"].t) if advance else None, latent=ptr(out["latent"].t),
                                log_std=ptr(pol.log_std), eps=ptr(eps), action=ptr(out["action"].t) if actor else None,
                                log_prob=ptr(out["log_prob"].t) if actor else None,
                                value=ptr(out["value"].t) if critic else None)
    if actor:
        s.actor = fs._net(pol.lstm_actor, pol.pi_net, pol.action_net)
    if critic:
        s.critic = fs._net(pol.lstm_critic, pol.vf_net, pol.value_net)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().salp_lstm_policy_step(ctypes.byref(s), st))
    torch.cuda.synchronize()
    return out


def _tensors(out):
    s = out["state"].t
    return dict(zip(NAMES, (out["action"].t, out["log_prob"].t, out["value"].t, s[0], s[1], s[2], s[3])))


def _rel(x, ref64):
    return float((x.double().cpu() - ref64).abs().max() / ref64.abs().max())


@pytest.mark.parametrize("keep_mode", ["ones", "zeros", "mixed"])
@pytest.mark.parametrize("obs_dim", OBS_DIMS)
@pytest.mark.parametrize("rows", ROWS)
def test_step_against_the_module(policies, rows, obs_dim, keep_mode):
    pol64, pol = policies[obs_dim]
    obs, state, eps, keep = _inputs(rows, obs_dim, keep_mode)
    a64, lp64, v64, new64 = _module_step(pol64, obs.double(), state.double(), eps.double(), keep.double())
    ref = dict(zip(NAMES, (a64, lp64, v64, new64[0], new64[1], new64[2], new64[3])))
    g = [t.cuda() for t in (obs, state, eps, keep)]
    a32, lp32, v32, new32 = _module_step(pol, *g[:3], g[3])
    torch32 = dict(zip(NAMES, (a32, lp32, v32, new32[0], new32[1], new32[2], new32[3])))
    out = _run(pol, g[0], g[1], keep=g[3], eps=g[2])
    got = _tensors(out)
    for name in NAMES:
        e_k, e_t = _rel(got[name], ref[name]), _rel(torch32[name], ref[name])
        print(f"[lstm_policy_step] rows {rows} obs_dim {obs_dim} keep {keep_mode} {name}: kernel {e_k:.3e} "
              f"torch f32 {e_t:.3e} (bound {4 * e_t + 4 * U:.3e})")
        assert bool(torch.isfinite(got[name]).all()), name          # every row was written
        assert e_k <= 4 * e_t + 4 * U, (name, e_k, e_t)
        # and the unfused path directly (the figures of tests/test_gpu_recurrent_ppo.py)
        assert torch.allclose(got[name], torch32[name], rtol=1e-4, atol=1e-5), name
    for name in ("action", "log_prob", "value", "state"):
        assert out[name].intact(), name
    assert out["latent"].untouched()               # h goes to state_out when there is one
    # keep = NULL is keep = 1
    if keep_mode == "ones":
        again = _tensors(_run(pol, g[0], g[1], keep=None, eps=g[2]))
        assert all(torch.equal(again[k].view(torch.int32), got[k].view(torch.int32)) for k in NAMES)
    # a second run gives the same bits
    again = _tensors(_run(pol, g[0], g[1], keep=g[3], eps=g[2]))
    for name in NAMES:
        assert torch.equal(again[name].view(torch.int32), got[name].view(torch.int32)), name


@pytest.mark.parametrize("rows,obs_dim", [(4, 10), (33, 6), (65, 16), (1057, 10)])
def test_call_variants(policies, rows, obs_dim):
    pol64, pol = policies[obs_dim]
    obs, state, eps, keep = (t.cuda() for t in _inputs(rows, obs_dim, "mixed"))
    full = _run(pol, obs, state, keep=keep, eps=eps)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    # eps = NULL: the action is the mean's bits, the log-prob the mean's
    det = _run(pol, obs, state, keep=keep, eps=None)
    zero = _run(pol, obs, state, keep=keep, eps=torch.zeros_like(eps))
    assert torch.equal(bits(det["action"].t), bits(zero["action"].t))
    a64, lp64, _, _ = _module_step(pol64, obs.double().cpu(), state.double().cpu(), None, keep.double().cpu())
    # the log-prob of the mean is -sum(log sigma) - 3 log sqrt(2 pi): three terms |log sigma| <= 2, each
    # logf(expf(.)) within a few ulp of 2: <= ~1.5e-6 absolute
    assert _rel(det["action"].t, a64) <= 1e-5
    assert float((det["log_prob"].t.double().cpu() - lp64).abs().max()) <= 2e-6
    assert bool((det["log_prob"].t == det["log_prob"].t[0]).all())
    assert torch.equal(bits(det["state"].t), bits(full["state"].t)) and torch.equal(bits(det["value"].t),
                                                                                    bits(full["value"].t))
    # critic only, the state not advanced: the same value bits, nothing else written
    cr = _run(pol, obs, state, keep=keep, actor=False, advance=False)
    assert torch.equal(bits(cr["value"].t), bits(full["value"].t))
    assert cr["action"].untouched() and cr["log_prob"].untouched() and cr["state"].untouched()
    assert cr["latent"].intact() and bool(torch.isnan(cr["latent"].t[0]).all())
    assert torch.equal(bits(cr["latent"].t[1]), bits(full["state"].t[2]))
    # critic only with the state advanced: the critic's half alone
    cr = _run(pol, obs, state, keep=keep, actor=False)
    assert torch.equal(bits(cr["value"].t), bits(full["value"].t)) and cr["state"].intact()
    assert torch.equal(bits(cr["state"].t[2:]), bits(full["state"].t[2:])) and bool(torch.isnan(cr["state"].t[:2]).all())
    # actor only, likewise
    ac = _run(pol, obs, state, keep=keep, eps=eps, critic=False, advance=False)
    assert torch.equal(bits(ac["action"].t), bits(full["action"].t))
    assert torch.equal(bits(ac["log_prob"].t), bits(full["log_prob"].t))
    assert ac["value"].untouched() and ac["state"].untouched() and bool(torch.isnan(ac["latent"].t[1]).all())
    ac = _run(pol, obs, state, keep=keep, eps=eps, critic=False)
    assert torch.equal(bits(ac["state"].t[:2]), bits(full["state"].t[:2])) and bool(torch.isnan(ac["state"].t[2:]).all())
    assert torch.equal(bits(ac["action"].t), bits(full["action"].t)) and ac["value"].untouched()


def test_wrapper_alternates_its_buffers_and_checks_shapes(policies):
    _, pol = policies[10]
    fs = FusedPolicyStep(pol, 4, torch.device("cuda", torch.cuda.current_device()))
    obs, state, eps, keep = (t.cuda() for t in _inputs(4, 10, "mixed"))
    new = torch.empty_like(state)
    a, lp, v = fs(obs, keep, state, new, eps)
    want = _tensors(_run(pol, obs, state, keep=keep, eps=eps))
    assert torch.equal(a, want["action"]) and torch.equal(lp, want["log_prob"]) and torch.equal(v, want["value"])
    assert torch.equal(new[3], want["critic_c"])
    tv = fs(obs, None, new, actor=False)[2]
    assert tv.data_ptr() != v.data_ptr() and torch.equal(v, want["value"])       # the step's value is left alone
    with pytest.raises(_lib.SalpError, match="overlap"):
        fs(obs, keep, state, state, eps)
    with pytest.raises(ValueError, match="obs"):
        fs(obs[:3], keep, state, new, eps)
