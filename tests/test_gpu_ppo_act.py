"""salp_ppo_mlp_act (csrc/salp_ppo_act.hip) against the module it fuses,
``ActorCritic.act`` / ``value``, and against the in-kernel policy of
salp_collect, whose operation order it restates.

Reference: a float64 copy of the same module on the CPU with the same noise.
Bounds: the project's own for this policy (tests/test_gpu_collect.py): action
and value rtol 1e-5, atol 1e-5; log-prob rtol 1e-5, atol 1e-4.  Rows: 1, 5, 63,
64, 65 (below, at and past one tile of 64 rows) and 257 (four tiles and one
row); a workgroup takes one tile and does not loop over tiles.  Largest errors
measured on one MI355X over all cases (kernel / float32 torch path): action
2.71e-7 / 3.00e-7, log-prob 1.53e-6 / 1.08e-6, value 3.47e-7 / 6.52e-7."""
import copy
import ctypes

import pytest
import torch

from grasp_lab_salp_amd import _lib
from grasp_lab_salp_amd._abi import default_params
from grasp_lab_salp_amd.batched_env import BatchedSalpEnv
from grasp_lab_salp_amd.ppo import ActorCritic, FusedMlpAct, _mlp_tensors, pack_policy

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 63, 64, 65, 257)
OBS_DIMS = (6, 10, 14)
PAD, SENTINEL = 7, 12345.0
NAMES = ("action", "log_prob", "value")
TOL = {"action": (1e-5, 1e-5), "value": (1e-5, 1e-5), "log_prob": (1e-5, 1e-4)}     # (rtol, atol)


def _policy(obs_dim):
    torch.manual_seed(200 + obs_dim)
    pol = ActorCritic(obs_dim, 3)
    with torch.no_grad():
        pol.log_std.uniform_(-2.0, 0.5)
        pol.action_net.weight.mul_(60.0)     # means spread over the box, not ~ 0
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


def _inputs(rows, obs_dim):
    g = torch.Generator().manual_seed(rows * 31 + obs_dim)
    return torch.randn(rows, obs_dim, generator=g), torch.randn(rows, 3, generator=g)


def _module_step(pol, obs, eps):
    """act() with the given noise: (action, log_prob, value)."""
    with torch.no_grad():
        d = pol.dist(obs)
        a = d.mean if eps is None else d.mean + d.stddev * eps
        return a, d.log_prob(a).sum(-1), pol.value(obs)


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


def _run(pol, obs, eps=None, actor=True, critic=True, log_prob=True):
    """One salp_ppo_mlp_act call into guarded buffers: {name: _Guarded}."""
    rows, od = obs.shape
    out = {"action": _Guarded(rows, 3), "log_prob": _Guarded(rows), "value": _Guarded(rows)}
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    a = _lib.SalpPpoMlpAct(rows=rows, obs_dim=od, obs=ptr(obs), eps=ptr(eps),
                           action=ptr(out["action"].t) if actor else None,
                           log_prob=ptr(out["log_prob"].t) if actor and log_prob else None,
                           value=ptr(out["value"].t) if critic else None)
    for i, t in enumerate(_mlp_tensors(pol)):
        a.params[i] = t.data_ptr()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().salp_ppo_mlp_act(ctypes.byref(a), st))
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def largest(policies):
    """(obs, eps, outputs) of the largest case per obs_dim, computed once."""
    out = {}
    for d in OBS_DIMS:
        obs, eps = (t.cuda() for t in _inputs(ROWS[-1], d))
        out[d] = (obs, eps, _run(policies[d][1], obs, eps))
    return out


@pytest.mark.parametrize("obs_dim", OBS_DIMS)
@pytest.mark.parametrize("rows", ROWS)
def test_against_the_float64_module(policies, rows, obs_dim):
    p64, p32 = policies[obs_dim]
    obs, eps = _inputs(rows, obs_dim)
    want = dict(zip(NAMES, _module_step(p64, obs.double(), eps.double())))
    obs, eps = obs.cuda(), eps.cuda()
    out = _run(p32, obs, eps)
    torch32 = dict(zip(NAMES, _module_step(p32, obs, eps)))
    for name in NAMES:
        got = out[name].t.cpu().double()
        err = float((got - want[name]).abs().max())
        err32 = float((torch32[name].cpu().double() - want[name]).abs().max())
        print(f"rows {rows} obs_dim {obs_dim} {name}: kernel {err:.3e} torch-f32 {err32:.3e}")
        assert out[name].intact(), name
        rtol, atol = TOL[name]
        assert torch.allclose(got, want[name], rtol=rtol, atol=atol), (name, err)
    # a second call gives the same bits (no atomics, nothing carried over)
    again = _run(p32, obs, eps)
    assert all(_same_bits(out[n].t, again[n].t) for n in NAMES)


@pytest.mark.parametrize("obs_dim", OBS_DIMS)
def test_row_invariance(policies, largest, obs_dim):
    """Row r of the 257-row call equals a 1-row call on that observation: a
    row's bits depend neither on the row count nor on its place in a tile."""
    pol = policies[obs_dim][1]
    obs, eps, big = largest[obs_dim]
    for r in (0, 1, 63, 64, 130, 255, 256):
        one = _run(pol, obs[r:r + 1].contiguous(), eps[r:r + 1].contiguous())
        for name in NAMES:
            assert _same_bits(one[name].t, big[name].t[r:r + 1]), (r, name)


@pytest.mark.parametrize("obs_dim", OBS_DIMS)
def test_one_network_alone_and_absent_outputs(policies, largest, obs_dim):
    pol = policies[obs_dim][1]
    obs, eps, both = largest[obs_dim]
    critic = _run(pol, obs, None, actor=False)
    assert _same_bits(critic["value"].t, both["value"].t) and critic["value"].intact()
    assert critic["action"].untouched() and critic["log_prob"].untouched()
    actor = _run(pol, obs, eps, critic=False)
    assert _same_bits(actor["action"].t, both["action"].t) and _same_bits(actor["log_prob"].t, both["log_prob"].t)
    assert actor["value"].untouched() and actor["action"].intact() and actor["log_prob"].intact()
    no_lp = _run(pol, obs, eps, critic=False, log_prob=False)
    assert _same_bits(no_lp["action"].t, both["action"].t) and no_lp["log_prob"].untouched()


@pytest.mark.parametrize("obs_dim", OBS_DIMS)
def test_no_noise_gives_the_mean(policies, largest, obs_dim):
    """eps NULL: the action is the mean's bits, which a zero eps gives too
    wherever mean + 0 is the mean (all but a mean of -0)."""
    pol = policies[obs_dim][1]
    obs, eps, _ = largest[obs_dim]
    det = _run(pol, obs, None)
    zero = _run(pol, obs, torch.zeros_like(eps))
    assert _same_bits(det["action"].t, zero["action"].t) and _same_bits(det["log_prob"].t, zero["log_prob"].t)
    assert _same_bits(det["value"].t, zero["value"].t)
    # and the wrapper: deterministic actor-only calls are the mean; its two value buffers are kept apart
    fa = FusedMlpAct(pol, obs.shape[0], obs.device)
    a, lp, v = fa(obs, eps)
    v_step = v.clone()
    a2, _, none = fa(obs, critic=False)
    assert none is None and _same_bits(a2, det["action"].t)
    _, _, v_only = fa(obs[:].flip(0).contiguous(), actor=False)
    assert v_only.data_ptr() != v.data_ptr() and _same_bits(v, v_step) and _same_bits(v_only.flip(0), v_step)


@pytest.mark.parametrize("kernel", [0, 2])
def test_values_are_the_collections_bit_for_bit(kernel):
    """salp_collect at 64 envs x 8 steps on either rollout kernel (0: one env
    per lane, 2: two waves per env), then salp_ppo_mlp_act on the observations
    it stored: the same values, bit for bit."""
    n, n_steps = 64, 8
    p = default_params()
    p.max_cycles = 3        # timeouts inside the collection
    env = BatchedSalpEnv(n, params=p, seed=23)
    obs0 = env.reset()
    env.set_rollout_kernel(kernel)
    torch.manual_seed(1)
    pol = ActorCritic(env.obs_dim, 3).cuda()
    with torch.no_grad():
        pol.action_net.weight.mul_(60.0)
        pol.log_std.copy_(torch.tensor([-0.7, -0.4, -0.2]))
        for m in (pol.vf_net[0], pol.vf_net[2], pol.value_net):
            m.bias.uniform_(-0.1, 0.1)
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")  # noqa: E731
    bufs = {"obs": z(n_steps, n, env.obs_dim), "actions": z(n_steps, n, 3), "rewards": z(n_steps, n),
            "episode_starts": z(n_steps, n), "values": z(n_steps, n), "log_probs": z(n_steps, n)}
    env.collect(pack_policy(pol), n_steps, bufs, torch.ones(n, dtype=torch.float32, device="cuda"), obs0.clone(),
                torch.zeros(4, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"),
                noise_seed=99, gamma=0.99)
    torch.cuda.synchronize()
    env.check_pair()
    flat = bufs["obs"].reshape(-1, env.obs_dim)
    assert bool(torch.isfinite(flat).all()) and bool((bufs["values"] != -7.0).all())
    out = _run(pol, flat, None, actor=False)
    assert _same_bits(out["value"].t, bufs["values"].reshape(-1))
