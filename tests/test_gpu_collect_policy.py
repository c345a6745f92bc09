"""The policy side of salp_collect (csrc/salp_kernels.hip policy_act, in
k_rollout, k_rollout_pair with the actor's second layer staged in LDS, and
k_rollout_split) against independent references.

(a) every action, log-prob and value of the collection equals, bit for bit,
    salp_ppo_mlp_act on the recorded observations with the oracle's
    exploration noise (oracle.policy_noise, pinned on the CPU by
    tests/test_policy_noise.py) for (noise_seed, env_id_offset + i, the env's
    step counter before the call + t);
(b) one call of 8 steps equals calls of 3 and then 5 steps;
(c) envs 32..64 as a handle of their own equal the parent's rows;
(d) the log-prob against float64 at the kernel's own mean, action and log-std;
(e) the timeout bootstrap rew + float32(gamma) V(terminal obs), exactly.

Shapes: 65 envs (one full wave plus one lane, an empty seat in the two-wave
kernels; 65 * 8 = 520 rows, past eight tiles of the act kernel), 8 steps,
max_cycles 3 so that timeouts occur, gamma 0.9, means spread over the box and
every bias nonzero.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from grasp_lab_salp_amd._abi import FIELD, default_params
from grasp_lab_salp_amd.batched_env import BatchedSalpEnv
from grasp_lab_salp_amd.ppo import DIVERGED_OBS_ABS, DIVERGED_REWARD_ABS, pack_policy
from oracle import oracle
from test_gpu_ppo_act import _policy, _run

pytestmark = pytest.mark.gpu

N, T, GAMMA, SIM_SEED = 65, 8, 0.9, 23
KERNELS = pytest.mark.parametrize("kernel", [0, 1, 2], ids=["lane", "pair", "split"])
BUFFERS = ("obs", "actions", "rewards", "episode_starts", "values", "log_probs")
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def no_pair_timeouts():
    """Every pair launch of the test met its partner wave on every tick: no
    wait gave up (salp_pair_timeouts, read and cleared; process-wide)."""
    probe = BatchedSalpEnv(64, seed=0)
    probe.pair_timeouts()
    yield
    assert probe.pair_timeouts() == 0
    probe.close()


def _np(t):
    return t.detach().cpu().numpy()


def _differ(a, b):
    """Elements whose bit patterns differ, NaN payloads aside."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind != "f":
        return a != b
    iv = np.int64 if a.dtype == np.float64 else np.int32
    return (a.view(iv) != b.view(iv)) & ~(np.isnan(a) & np.isnan(b))


def _assert_same(what, a, b):
    d = _differ(a, b)
    if d.any():
        where = np.argwhere(d)[:4].tolist()
        raise AssertionError(f"{what}: {int(d.sum())} of {d.size} differ, first at {where}: "
                             f"{np.asarray(a)[d][:4]} != {np.asarray(b)[d][:4]}")


@functools.lru_cache(maxsize=None)
def _pol(zero_tick=False):
    pol = _policy(10).cuda()
    if zero_tick:
        # tests/test_gpu_collect.py: contraction and coast clipped to 0 for about
        # half the draws each, so many cycles of zero ticks, a few lanes at a
        # time: boundary rounds chain and leave lanes to the next chunk boundary
        with torch.no_grad():
            pol.action_net.weight.mul_(0.01)
            pol.action_net.bias.copy_(torch.tensor([0.0, 0.0, 0.0]))
            pol.log_std.copy_(torch.tensor([-1.0, -1.0, -3.0]))
    return pol


class _Handle:
    """An env handle with what salp_collect carries between calls."""

    def __init__(self, kernel, n=N, offset=0, state=None, obs0=None):
        p = default_params()
        p.max_cycles = 3
        self.env = BatchedSalpEnv(n, params=p, seed=SIM_SEED, env_id_offset=offset)
        self.n, self.offset = n, offset
        reset_obs = self.env.reset()
        if state is not None:
            self.env.set_state(state)
        self.env.set_rollout_kernel(kernel)
        self.last_obs = (reset_obs if obs0 is None else obs0).clone().contiguous()
        self.ep_start = torch.ones(n, dtype=torch.float32, device="cuda")
        self.ep_stats = torch.zeros(4, dtype=torch.float64, device="cuda")
        self.diverged = torch.zeros(1, dtype=torch.int64, device="cuda")

    def collect(self, pol, n_steps, noise_seed):
        """One salp_collect call: the six buffers, the step counters before the
        call and what the call left, as numpy arrays."""
        n, od = self.n, self.env.obs_dim
        z = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")  # noqa: E731
        bufs = {"obs": z(n_steps, n, od), "actions": z(n_steps, n, 3), "rewards": z(n_steps, n),
                "episode_starts": z(n_steps, n), "values": z(n_steps, n), "log_probs": z(n_steps, n)}
        before = _np(self.env.get_state())
        first_obs = self.last_obs.clone()
        self.env.collect(pack_policy(pol), n_steps, bufs, self.ep_start, self.last_obs, self.ep_stats, self.diverged,
                         noise_seed=noise_seed, gamma=GAMMA, diverged_obs_abs=DIVERGED_OBS_ABS,
                         diverged_reward_abs=DIVERGED_REWARD_ABS)
        torch.cuda.synchronize()
        self.env.check_pair()
        out = {k: _np(v) for k, v in bufs.items()}
        assert all((out[k] != -7.0).all() for k in BUFFERS), "a buffer row was not written"
        out.update(state_before=before, first_obs=first_obs, base=before[FIELD["step_count"]].astype(np.int64),
                   state=_np(self.env.get_state()), last_obs=_np(self.last_obs), episode_start=_np(self.ep_start),
                   ep_stats=_np(self.ep_stats), diverged=_np(self.diverged), noise_seed=noise_seed,
                   offset=self.offset)
        return out


@functools.lru_cache(maxsize=None)
def _first(kernel):
    """The collection most tests share: offset 0, noise_seed 99, from reset."""
    h = _Handle(kernel)
    return h, h.collect(_pol(), T, 99)


def _noise(run, n_steps):
    """The oracle's noise for the rows of a collection: float32 [n_steps, n, 3]."""
    base = run["base"]
    eps = np.empty((n_steps, len(base), 3), np.float32)
    for b in np.unique(base):
        idx = np.nonzero(base == b)[0]
        z = oracle.policy_noise(run["noise_seed"], [run["offset"] + int(i) for i in idx],
                                [int(b) + t for t in range(n_steps)])
        eps[:, idx] = z.transpose(1, 0, 2)
    return eps


def _assert_collection_is_the_act_kernels(pol, run):
    n_steps, n, od = run["obs"].shape
    assert np.isfinite(run["obs"]).all()
    eps = torch.tensor(_noise(run, n_steps).reshape(-1, 3), device="cuda")
    obs = torch.tensor(run["obs"].reshape(-1, od), device="cuda")
    out = _run(pol, obs, eps)
    for name, key in (("action", "actions"), ("log_prob", "log_probs"), ("value", "values")):
        assert out[name].intact()
        _assert_same(key, run[key], _np(out[name].t).reshape(run[key].shape))


# ------------------------------------------------ (a) against the act kernel
@KERNELS
def test_collection_equals_the_act_kernel_on_the_oracles_noise(kernel):
    """From reset (every counter 0) at env_id_offset 0, noise_seed 99, then a
    second collection on the same handle, whose counters start at 8."""
    h, run = _first(kernel)
    assert (run["base"] == 0).all()
    _assert_collection_is_the_act_kernels(_pol(), run)
    again = h.collect(_pol(), T, 99)
    assert (again["base"] == T).all()
    _assert_same("the second call starts on the first's last observation", _np(again["first_obs"]), run["last_obs"])
    _assert_collection_is_the_act_kernels(_pol(), again)


@KERNELS
def test_collection_uses_the_global_env_id_and_the_whole_seed(kernel):
    """env ids 2^32 - 32 .. 2^32 + 32 with a seed above 2^32; and on one start
    state the seeds 99 / 2^32 + 99 and 99 / 100 move every action."""
    _, run = _first(kernel)
    h = _Handle(kernel, offset=2 ** 32 - 32)
    _assert_collection_is_the_act_kernels(_pol(), h.collect(_pol(), T, 2 ** 32 + 99))
    for seed in (2 ** 32 + 99, 100):
        other = _Handle(kernel, state=run["state_before"], obs0=run["first_obs"]).collect(_pol(), 1, seed)
        _assert_same("the same start", other["obs"][0], run["obs"][0])
        assert (other["actions"][0] != run["actions"][0]).all(), seed
        _assert_collection_is_the_act_kernels(_pol(), other)


@KERNELS
def test_zero_tick_policy_equals_the_act_kernel(kernel):
    """Many zero-tick cycles: several boundary rounds per chunk boundary, and
    lanes left to the next one (SALP_COLLECT_REP_MIN)."""
    pol = _pol(True)
    run = _Handle(kernel).collect(pol, T, 99)
    clipped = np.clip(run["actions"], np.float32([0, 0, -1]), np.float32([1, 1, 1]))
    zero = (clipped[..., 0] == 0) & (clipped[..., 1] == 0)
    assert zero.mean() > 0.1, float(zero.mean())
    _assert_collection_is_the_act_kernels(pol, run)


# ------------------------------------------------------ (b) split invariance
def _assert_runs_equal(a, b, keys):
    for k in keys:
        _assert_same(k, a[k], b[k])


@KERNELS
def test_one_call_equals_calls_of_three_and_five_steps(kernel):
    _, one = _first(kernel)
    twin = _Handle(kernel, state=one["state_before"], obs0=one["first_obs"])
    p3, p5 = twin.collect(_pol(), 3, 99), twin.collect(_pol(), 5, 99)
    for k in BUFFERS:
        _assert_same(k, one[k], np.concatenate([p3[k], p5[k]]))
    _assert_runs_equal(one, p5, ("last_obs", "episode_start", "diverged", "state"))
    # float64 atomics: the summation order follows the scheduling (tests/test_gpu_pair.py)
    assert np.allclose(one["ep_stats"], p5["ep_stats"], rtol=1e-12, atol=0), (one["ep_stats"], p5["ep_stats"])
    assert one["ep_stats"][1] > 0


# -------------------------------------------------------------- (c) sharding
@KERNELS
def test_envs_32_to_64_as_their_own_handle_equal_the_parents_rows(kernel):
    _, parent = _first(kernel)
    lo = 32
    shard = _Handle(kernel, n=N - lo, offset=lo, state=np.ascontiguousarray(parent["state_before"][:, lo:]),
                    obs0=parent["first_obs"][lo:])
    got = shard.collect(_pol(), T, 99)
    for k in BUFFERS:
        _assert_same(k, got[k], parent[k][:, lo:])
    _assert_same("last_obs", got["last_obs"], parent["last_obs"][lo:])
    _assert_same("episode_start", got["episode_start"], parent["episode_start"][lo:])
    _assert_same("state", got["state"], parent["state"][:, lo:])


# ---------------------------------------------- (d) the log-prob against fp64
@KERNELS
def test_log_prob_against_float64_at_the_kernels_own_numbers(kernel):
    """lp = sum_c -(d d) / (2 (sd sd)) - logf(sd) - 0.918..., d = a - mean, sd =
    expf(log_std), against float64 with the mean of an eps = NULL act call on
    the recorded observations (test_no_noise_gives_the_mean: the mean's bits),
    the buffer's action and sd = exp(log_std) in float64.

    First-order count in float32 roundings, u = 2^-24 (one rounding <= u
    relative, 1 ulp <= 2 u), per component with T1 = d^2 / (2 sd^2),
    T2 = |log_std|, T3 = 0.918...:
    * expf <= 2 ulp as tests/test_gpu_sac.py counts it: sd within 4 u;
    * d one rounding (u), d d 3 u; sd sd 9 u; the factor 2 exact; the quotient
      one more: 13 u T1;
    * logf at the perturbed sd: 4 u absolute, and its own 1 ulp: 2 u T2;
    * the float32 constant: u T3;
    * the sums: (-T1 - T2) <= u (T1 + T2), (... - T3) <= u (T1 + T2 + T3), and
      lp += ... <= u (sum of all terms so far), exact for the first component.
    With M the sum of all nine absolute terms this is at most 17 u M + 12 u;
    the bound used is the count itself, term by term."""
    _, run = _first(kernel)
    pol = _pol()
    n_steps, n, od = run["obs"].shape
    obs = torch.tensor(run["obs"].reshape(-1, od), device="cuda")
    mean = _np(_run(pol, obs, None, critic=False, log_prob=False)["action"].t).astype(np.float64)
    a = run["actions"].reshape(-1, 3).astype(np.float64)
    ls = _np(pol.log_std).astype(np.float64)
    sd = np.exp(ls)
    t3 = float(np.float32(0.91893853320467274))
    t1, t2 = (a - mean) ** 2 / (2.0 * sd * sd), np.abs(ls)[None, :] + 0.0 * a
    ref = (-t1 - np.log(sd) - 0.5 * np.log(2.0 * np.pi)).sum(1)
    term = 13 * t1 + (4 + 2 * t2) + t3
    comp = t1 + t2 + t3                                  # a component's absolute terms
    before = np.cumsum(comp, 1)                          # ... of the components so far
    sums = (t1 + t2) + comp + np.where(np.arange(3)[None, :] > 0, before, 0.0)
    bound = U * (term + sums).sum(1)
    err = np.abs(run["log_probs"].reshape(-1).astype(np.float64) - ref)
    print(f"kernel {kernel}: log-prob worst error / bound {float((err / bound).max()):.3f}, "
          f"worst error {float(err.max()):.3e}, |ref| up to {float(np.abs(ref).max()):.3e}")
    assert (t1.max() > 1.0) and (err <= bound).all(), float((err / bound).max())


# --------------------------------------------------- (e) the timeout bootstrap
def _f32_nearest(x):
    """The float32 nearest to the Fraction x (ties to even)."""
    f = np.float32(float(x))
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    best = min(abs(Fraction(float(c)) - x) for c in cands)
    near = [c for c in cands if abs(Fraction(float(c)) - x) == best]
    if len(near) > 1:
        near = [c for c in near if int(c.view(np.int32)) % 2 == 0]
    return near[0]


FORMS = {}     # kernel -> the rounding form its bootstrapped rows showed


@KERNELS
def test_timeout_bootstrap_is_exactly_one_float32_expression(kernel):
    """The collection replayed lock-step on a twin (tests/test_gpu_collect.py)
    gives each timeout's float32 reward and terminal observation, and
    salp_ppo_mlp_act V(terminal obs).  Every bootstrapped reward is then
    fl(rew + g V) (one rounding, a fused multiply-add) or fl(rew + fl(g V))
    (two), g = float32(gamma), both computed exactly; the rows that tell the
    two apart all show one form, the same on the three kernels."""
    _, run = _first(kernel)
    pol = _pol()
    p = default_params()
    p.max_cycles = 3
    twin = BatchedSalpEnv(N, params=p, seed=SIM_SEED)
    twin.reset()
    twin.set_state(run["state_before"])
    clipped = np.clip(run["actions"], np.float32([0, 0, -1]), np.float32([1, 1, 1]))
    g = Fraction(float(np.float32(GAMMA)))
    one, two, n_boot = 0, 0, 0
    for t in range(T):
        r = twin.step(torch.tensor(clipped[t], device="cuda"), auto_reset=True, want_terminal_obs=True)
        tob = r.terminal_obs
        bad = (~torch.isfinite(tob).all(1) | (tob.abs() > DIVERGED_OBS_ABS).any(1)
               | ~(r.reward.abs() <= DIVERGED_REWARD_ABS))
        done = r.terminated.bool() | r.truncated.bool()
        boot = _np(r.truncated.bool() & ~r.terminated.bool() & ~bad)
        rew32 = _np(r.reward.float())
        want = np.where(_np(bad), np.float32(0), rew32)
        _assert_same(f"step {t}: rewards without a bootstrap", run["rewards"][t][~boot], want[~boot])
        twin.reset(mask=bad & ~done)
        if not boot.any():
            continue
        v = _np(_run(pol, tob[torch.tensor(boot, device="cuda")].contiguous(), None, actor=False)["value"].t)
        for got, rew, val in zip(run["rewards"][t][boot], rew32[boot], v):
            rew_q, val_q = Fraction(float(rew)), Fraction(float(val))
            fused = _f32_nearest(rew_q + g * val_q)
            split = _f32_nearest(rew_q + Fraction(float(_f32_nearest(g * val_q))))
            assert got in (fused, split), (t, got, fused, split)
            n_boot += 1
            if fused != split:
                one, two = one + (got == fused), two + (got == split)
    _assert_same("final state", run["state"], _np(twin.get_state()))
    print(f"kernel {kernel}: {n_boot} bootstrapped rewards, {one + two} tell the forms apart: "
          f"{one} one rounding, {two} two roundings")
    assert n_boot > 0
    assert one == 0 or two == 0, (one, two)
    if one or two:
        FORMS[kernel] = "one" if one else "two"
    assert len(set(FORMS.values())) <= 1, FORMS
