"""On-device SAC over the batched simulator: the learner of the reference's
production training script, ``src/train_robot.py:62-69``
(``SAC("MlpPolicy", vec_env, learning_rate=3e-4, buffer_size=100000,
learning_starts=1000, batch_size=256, tau=0.005, gamma=0.99, train_freq=1,
gradient_steps=1)``).

Stable-Baselines3 (>= 2.0) is not installed here: its semantics are restated,
and parity with it is unpinned.  What is kept:

* policy: SB3's SAC ``MlpPolicy``: a 256-256 ReLU actor with a mean head and a
  state-dependent log-std head (clamped to [-20, 2]), a tanh-squashed diagonal
  Gaussian, two 256-256 ReLU Q-networks on ``cat(obs, action)`` and a target
  copy of them; torch's default init, as SB3 uses for SAC;
* the policy acts in [-1, 1]; the env receives the action unscaled to
  ``Box([0, 0, -1], [1, 1, 1])`` and the replay buffer keeps the scaled one;
* actions are uniform in the Box until ``learning_starts`` transitions;
* the replay buffer holds ``max(buffer_size // n_envs, 1)`` slots per env;
  ``next_obs`` is the terminal observation where an episode ended, and a
  truncation does not cut the bootstrap (``handle_timeout_termination``);
* ``ent_coef="auto"``: ``log_ent_coef`` starts at 0 with its own Adam and
  ``target_entropy = -3``; the coefficient of before its step serves the whole
  gradient step;
* per gradient step: sample, actor(obs), [no grad] actor(next_obs) and the
  target critics, critics(obs, a), TD head, critic Adam and alpha Adam,
  critics(obs, a_pi), pi head, actor Adam, Polyak.

The GEMMs are library calls through torch.  With ``fused=True`` (the default
on a GPU) everything around them is the HIP kernels of csrc/salp_sac.hip
(include/salp.h "SAC"): replay add / sample, the squashed-Gaussian head and
its backward, the TD and pi heads with their gradients, and Polyak in one
launch over flat parameter buffers.  ``fused=False`` runs the same step from
the plain torch expressions below (``torch_squashed_gaussian``,
``torch_td_head``, ``torch_pi_head``, index-op add / sample): the readable
restatement, and the one that runs on the CPU.  Both draw the same batches.
``fused_mlp=True`` (default off) replaces the library GEMMs too: the actor and
the critics run as the kernels of csrc/salp_sac_mlp.hip (``fused_actor``,
``fused_critic``), forward and backward, over the same ``nn.Module`` parameters.

Collection is lock-step ``salp_step`` on a stream of its own, with the
divergence guard, episode statistics and HIP-event phase timings of
:class:`~grasp_lab_salp_amd.ppo.PPO`.

The rest of the reference script (``src/train_robot.py:71-122``) runs too:
``learn(callback=...)`` drives the callbacks of
:mod:`grasp_lab_salp_amd.callbacks` after every env-step, on the collection
stream and on the step's device tensors (``model.locals``; no list of info
dicts is built); :meth:`SAC.evaluate` runs deterministic episodes on a second
vector env with its bookkeeping in one launch per step
(:class:`~grasp_lab_salp_amd.metrics.EvalAccount`); :meth:`SAC.save` /
:meth:`SAC.load` and :meth:`SAC.save_replay_buffer` /
:meth:`SAC.load_replay_buffer` keep everything a resumed run needs (parameters,
targets, optimiser states, the entropy coefficient, the counters and the
sampling generator) in a zip of this project's own layout, which is not SB3's.

Not built: the actor inside the chained simulation kernel, HIP-graph capture
of the step (the kernels read what changes per step from device memory, so
they are ready for it), several GPUs, TensorBoard event files
(``tensorboard_log`` is accepted and unused), rendering during evaluation, and
reading or writing SB3's own model files.
"""
import copy
import ctypes
import io
import json
import math
import os
import zipfile

import numpy as np
import torch
from torch import nn

from . import _lib
from .ppo import DIVERGED_OBS_ABS, DIVERGED_REWARD_ABS, diverged_mask, sampling_generator
from ._abi import INFO, INFO_DIM

__all__ = ["SAC", "SACPolicy", "ReplayBuffer", "squashed_gaussian", "td_head", "pi_head", "polyak",
           "torch_squashed_gaussian", "torch_td_head", "torch_pi_head", "torch_polyak", "torch_replay_add",
           "torch_replay_indices", "scale_action", "unscale_action", "critic_phase", "actor_phase",
           "fused_nets", "fused_actor", "fused_critic",
           "LOG_STD_MIN", "LOG_STD_MAX", "REPLAY_STREAM"]

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0     # SB3 sac/policies.py
SQUASH_EPS = 1e-6                         # SB3 SquashedDiagGaussianDistribution.epsilon
REPLAY_STREAM = 0x52504C59                # csrc/salp_sac.hip SP_STREAM_REPLAY
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
_EP_RETURN = INFO["ep_return"]
_EP_LEN = INFO["ep_len"]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _f32(name, t, shape):
    if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected a float32 CUDA tensor of shape {tuple(shape)}, got "
                         f"{t.dtype} {tuple(t.shape)} on {t.device}")
    return t.contiguous()


# ------------------------------------------------------------ action scaling
def scale_action(action, low, high):
    """SB3 ``BasePolicy.scale_action``: Box [low, high] -> [-1, 1]."""
    return 2.0 * ((action - low) / (high - low)) - 1.0


def unscale_action(scaled, low, high):
    """SB3 ``BasePolicy.unscale_action``: [-1, 1] -> Box [low, high]."""
    return low + 0.5 * (scaled + 1.0) * (high - low)


# ------------------------------------------------- plain torch restatements
def torch_squashed_gaussian(mu, log_std, eps):
    """SB3 ``SquashedDiagGaussianDistribution`` of SAC's actor from the raw
    log-std and N(0, 1) noise ``eps``: (action in [-1, 1], log-probability)."""
    ls = torch.clamp(log_std, LOG_STD_MIN, LOG_STD_MAX)
    a = torch.tanh(mu + ls.exp() * eps)
    logp = (-0.5 * eps * eps - ls - _HALF_LOG_2PI).sum(-1) - torch.log(1.0 - a * a + SQUASH_EPS).sum(-1)
    return a, logp


def torch_td_head(rewards, dones, q1_target, q2_target, logp_next, q1, q2, logp, log_alpha, gamma, target_entropy):
    """SB3 ``SAC.train``: (critic_loss, ent_coef_loss, target, alpha).  The
    target and alpha carry no gradient; critic_loss is differentiable in q1,
    q2 and ent_coef_loss in log_alpha ([1])."""
    with torch.no_grad():
        alpha = log_alpha.exp()
        nq = torch.minimum(q1_target, q2_target) - alpha * logp_next
        target = rewards + (1.0 - dones) * gamma * nq
    critic_loss = 0.5 * (((q1 - target) ** 2).mean() + ((q2 - target) ** 2).mean())
    ent_coef_loss = -(log_alpha * (logp.detach() + target_entropy)).mean()
    return critic_loss, ent_coef_loss, target, alpha


def torch_pi_head(alpha, logp, q1_pi, q2_pi):
    """SB3 ``SAC.train``'s actor loss, mean(alpha logp - min(q1_pi, q2_pi));
    ``torch.min`` over a dimension gives a tie's gradient to the first, q1."""
    min_q = torch.min(torch.stack([q1_pi, q2_pi], dim=1), dim=1).values
    return (alpha.detach() * logp - min_q).mean()


def torch_polyak(params, targets, tau):
    """SB3 ``polyak_update``: target = target (1 - tau) + tau param."""
    with torch.no_grad():
        for p, t in zip(params, targets):
            t.mul_(1.0 - tau)
            t.add_(p, alpha=tau)


def _mulhilo(a, b):
    """(high, low) 32-bit halves of a * b for a constant a < 2^32 and an int64
    tensor b of values < 2^32, without leaving int64."""
    bh, bl = b >> 16, b & 0xFFFF
    ph, pl = a * bh, a * bl                     # < 2^48 each
    hi = (ph + (pl >> 16)) >> 16
    lo = (((ph & 0xFFFF) << 16) + pl) & 0xFFFFFFFF
    return hi, lo


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (csrc/salp_philox.h sp_philox4x32_10) on int64 tensors
    holding 32-bit words; k0, k1 Python ints."""
    m32 = 0xFFFFFFFF
    for _ in range(10):
        hi0, lo0 = _mulhilo(0xD2511F53, c0)
        hi1, lo1 = _mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & m32, (k1 + 0xBB67AE85) & m32
    return c0, c1, c2, c3


def torch_replay_indices(size, update, seed, batch):
    """The (env, slot) draw of ``salp_replay_sample`` (include/salp.h) as torch
    integer ops, without a host sync: ``size`` [n_envs] int64, ``update`` a
    [1] int64 tensor, ``seed`` a Python int.  Bit-equal to the kernel."""
    dev = size.device
    n = size.numel()
    u = update.reshape(1).to(torch.int64)
    b = torch.arange(batch, dtype=torch.int64, device=dev)
    zero = torch.zeros_like(b)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    v0, v1, _, _ = _philox4x32_10(zero + (u & 0xFFFFFFFF), zero + ((u >> 32) & 0xFFFFFFFF), b, zero + REPLAY_STREAM,
                                  seed & 0xFFFFFFFF, seed >> 32)
    env = (v0 * n) >> 32
    # the first env at or after `env` (cyclically) that has stored something
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    have = torch.where(size > 0, ids, torch.full_like(ids, 2 * n))
    two = torch.cat([have, have + n])
    nxt = torch.flip(torch.cummin(torch.flip(two, [0]), 0).values, [0])[:n]
    env = torch.where(nxt[env] < 2 * n, nxt[env] % n, env)
    slot = (v1 * size[env]) >> 32
    return env, slot


def torch_replay_add(rb, obs, actions, obs_after, terminal_obs, reward, terminated, truncated, guard=True):
    """``salp_replay_add`` (include/salp.h) as torch index ops, without a host
    sync; returns the diverged mask (bool [n_envs])."""
    term = terminated.bool()
    done = term | truncated.bool()
    nxt = torch.where(done.unsqueeze(1), terminal_obs, obs_after)
    rew = reward.to(torch.float32)
    bad = diverged_mask(nxt, rew) if guard else torch.zeros_like(done)
    keep = ~bad
    env = torch.arange(rb.n_envs, device=obs.device)
    p = rb.pos
    for ring, new in ((rb.obs, obs), (rb.next_obs, nxt), (rb.actions, actions)):
        ring[p, env] = torch.where(keep.unsqueeze(1), new.to(ring.dtype), ring[p, env])
    rb.rewards[p, env] = torch.where(keep, rew.to(rb.rewards.dtype), rb.rewards[p, env])
    rb.dones[p, env] = torch.where(keep, term.to(rb.dones.dtype), rb.dones[p, env])
    rb.pos.copy_(torch.where(keep, (p + 1) % rb.capacity, p))
    rb.size.copy_(torch.where(keep, torch.clamp(rb.size + 1, max=rb.capacity), rb.size))
    return bad


# ------------------------------------------------------ HIP-kernel wrappers
class _ActorHeadFn(torch.autograd.Function):
    """The squashed-Gaussian head through salp_sac_actor_head_forward /
    _backward (include/salp.h): one kernel each way."""

    @staticmethod
    def forward(ctx, mu, log_std, eps):
        B = mu.shape[0]
        a = torch.empty_like(mu)
        logp = torch.empty(B, dtype=mu.dtype, device=mu.device)
        _lib.check(_lib.load().salp_sac_actor_head_forward(B, _ptr(mu), _ptr(log_std), _ptr(eps), _ptr(a),
                                                           _ptr(logp), _stream(mu.device)))
        ctx.save_for_backward(log_std, eps, a)
        return a, logp

    @staticmethod
    def backward(ctx, da, dlogp):
        log_std, eps, a = ctx.saved_tensors
        da = None if da is None else da.contiguous()
        dlogp = None if dlogp is None else dlogp.contiguous()
        dmu, dls = torch.empty_like(a), torch.empty_like(a)
        _lib.check(_lib.load().salp_sac_actor_head_backward(a.shape[0], _ptr(log_std), _ptr(eps), _ptr(a), _ptr(da),
                                                            _ptr(dlogp), _ptr(dmu), _ptr(dls), _stream(a.device)))
        return dmu, dls, None


def squashed_gaussian(mu, log_std, eps):
    """Fused :func:`torch_squashed_gaussian` (differentiable in mu, log_std);
    float32 CUDA tensors [B, 3]."""
    shape = (mu.shape[0], 3)
    return _ActorHeadFn.apply(_f32("mu", mu, shape), _f32("log_std", log_std, shape), _f32("eps", eps, shape))


def td_head(rewards, dones, q1_target, q2_target, logp_next, q1, q2, logp, log_alpha, gamma, target_entropy):
    """``salp_sac_td_head``: (out [3] = critic_loss, ent_coef_loss,
    d ent_coef_loss / d log_alpha; target [B]; dq1, dq2 [B] = d critic_loss /
    d q; alpha_used [1]).  No autograd: the caller feeds dq into backward."""
    B = rewards.shape[0]
    rows = [_f32(n, t.detach(), (B,)) for n, t in (("rewards", rewards), ("dones", dones), ("q1_target", q1_target),
                                                   ("q2_target", q2_target), ("logp_next", logp_next), ("q1", q1),
                                                   ("q2", q2), ("logp", logp))]
    la = _f32("log_alpha", log_alpha.detach(), (1,))
    dev = rewards.device
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
    target, dq1, dq2, out, alpha = new(B), new(B), new(B), new(3), new(1)
    ws = torch.empty(_lib.SAC_WORKSPACE_DOUBLES, dtype=torch.float64, device=dev)
    t = _lib.SalpSacTd(B, *(r.data_ptr() for r in rows), la.data_ptr(), float(gamma), float(target_entropy),
                       ws.data_ptr(), target.data_ptr(), dq1.data_ptr(), dq2.data_ptr(), out.data_ptr(),
                       alpha.data_ptr())
    _lib.check(_lib.load().salp_sac_td_head(ctypes.byref(t), _stream(dev)))
    return out, target, dq1, dq2, alpha


def pi_head(alpha_used, logp, q1_pi, q2_pi):
    """``salp_sac_pi_head``: (out [1] = actor_loss; dlogp, dq1, dq2 [B] = its
    gradient in logp, q1_pi, q2_pi).  No autograd, as :func:`td_head`."""
    B = logp.shape[0]
    al = _f32("alpha_used", alpha_used.detach(), (1,))
    rows = [_f32(n, t.detach(), (B,)) for n, t in (("logp", logp), ("q1_pi", q1_pi), ("q2_pi", q2_pi))]
    dev = logp.device
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
    out, dlogp, dq1, dq2 = new(1), new(B), new(B), new(B)
    ws = torch.empty(_lib.SAC_WORKSPACE_DOUBLES, dtype=torch.float64, device=dev)
    p = _lib.SalpSacPi(B, al.data_ptr(), *(r.data_ptr() for r in rows), ws.data_ptr(), out.data_ptr(),
                       dlogp.data_ptr(), dq1.data_ptr(), dq2.data_ptr())
    _lib.check(_lib.load().salp_sac_pi_head(ctypes.byref(p), _stream(dev)))
    return out, dlogp, dq1, dq2


def polyak(params_flat, target_flat, tau):
    """``salp_sac_polyak`` in place on ``target_flat`` (flat float32 CUDA vectors)."""
    n = params_flat.numel()
    for name, t in (("params_flat", params_flat), ("target_flat", target_flat)):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"polyak: {name} must be a contiguous flat float32 CUDA vector of {n} elements")
    _lib.check(_lib.load().salp_sac_polyak(n, _ptr(params_flat), _ptr(target_flat), float(tau),
                                           _stream(target_flat.device)))
    return target_flat


class _NetFn(torch.autograd.Function):
    """One pass of up to four 256-256 ReLU networks of one shape through
    salp_sac_net_forward / _backward (include/salp.h): a launch forward, the
    row kernel and the reduction backward.  ``params``: every network's
    tensors in the kernel's flat order, views into one buffer per network
    (``_Actor.net_params``, ``_Critic.net_params``).  The activations are kept
    only if ``keep`` (something asks for a gradient); the parameter gradients come back
    as views of one flat gradient buffer per pass, and ``x1``'s (the action
    columns) summed over the networks.  ``x0`` gets no gradient."""

    @staticmethod
    def forward(ctx, x0, x1, n_nets, out_dim, keep, *params):
        B, d0 = x0.shape
        d1 = 0 if x1 is None else x1.shape[1]
        per = len(params) // n_nets
        dev = x0.device
        outs = [torch.empty((B, out_dim), dtype=torch.float32, device=dev) for _ in range(n_nets)]
        h = torch.empty((2, n_nets, B, _lib.SAC_HIDDEN), dtype=torch.float32, device=dev) if keep else None
        f = _lib.SalpSacNetForward(batch=B, d0=d0, d1=d1, out_dim=out_dim, n_nets=n_nets)
        for i in range(n_nets):
            f.params[i] = params[i * per].data_ptr()
            f.x0[i] = x0.data_ptr()
            f.x1[i] = x1.data_ptr() if d1 else None
            f.out[i] = outs[i].data_ptr()
            if keep:
                f.h1[i], f.h2[i] = h[0, i].data_ptr(), h[1, i].data_ptr()
        _lib.check(_lib.load().salp_sac_net_forward(ctypes.byref(f), _stream(dev)))
        if keep:
            ctx.save_for_backward(x0, x1, h, *params)
            ctx.dims = (n_nets, out_dim, per)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        x0, x1, h, *params = ctx.saved_tensors
        n_nets, out_dim, per = ctx.dims
        if ctx.needs_input_grad[0]:
            raise RuntimeError("the fused networks give no gradient to their first input")
        B, d0 = x0.shape
        d1 = 0 if x1 is None else x1.shape[1]
        dev = x0.device
        want_x1 = ctx.needs_input_grad[1]
        want_p = any(ctx.needs_input_grad[5:])
        lib = _lib.load()
        P = lib.salp_sac_net_num_params(d0 + d1, out_dim)
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        douts = [torch.zeros((B, out_dim), dtype=torch.float32, device=dev) if d is None else d.contiguous()
                 for d in douts]
        gflat = new(n_nets, P) if want_p else None
        dx1 = new(B, d1) if want_x1 else None
        ws = new(lib.salp_sac_net_workspace_floats(B, d0, d1, out_dim, n_nets))
        b = _lib.SalpSacNetBackward(batch=B, d0=d0, d1=d1, out_dim=out_dim, n_nets=n_nets,
                                    dx1=dx1.data_ptr() if want_x1 else None, workspace=ws.data_ptr())
        for i in range(n_nets):
            b.params[i] = params[i * per].data_ptr()
            b.x0[i] = x0.data_ptr()
            b.x1[i] = x1.data_ptr() if d1 else None
            b.h1[i], b.h2[i] = h[0, i].data_ptr(), h[1, i].data_ptr()
            b.dout[i] = douts[i].data_ptr()
            b.dparams[i] = gflat[i].data_ptr() if want_p else None
        _lib.check(lib.salp_sac_net_backward(ctypes.byref(b), _stream(dev)))
        grads = [None] * len(params)
        if want_p:
            for i in range(n_nets):
                off = 0
                for k in range(per):
                    p = params[i * per + k]
                    grads[i * per + k] = gflat[i, off:off + p.numel()].view_as(p)
                    off += p.numel()
        return (None, dx1, None, None, None, *grads)


def fused_nets(x0, x1, nets, out_dim):
    """``nets`` (lists of parameter tensors in the kernel's flat order, each
    list contiguous in one buffer) evaluated on ``concat(x0, x1)`` (``x1`` may
    be None) in one launch: a tuple of [B, out_dim] outputs, differentiable
    in the parameters and in ``x1``."""
    B = x0.shape[0]
    x0 = _f32("x0", x0, (B, x0.shape[1]))
    if x1 is not None:
        x1 = _f32("x1", x1, (B, x1.shape[1]))
    params = [p for net in nets for p in net]
    keep = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x0, x1, *params))
    return _NetFn.apply(x0, x1, len(nets), out_dim, keep, *params)


def fused_actor(actor, obs):
    """``actor(obs)`` through the fused network: (mean, raw log-std)."""
    out, = fused_nets(obs, None, [actor.net_params()], 2 * actor.mu.out_features)
    k = actor.mu.out_features
    return out[:, :k], out[:, k:]


def fused_critic(critic, obs, action, detach=False):
    """``critic(obs, action)`` through the fused network, both Q-networks in
    one launch.  ``detach``: the parameters get no gradient (the backward then
    computes the action's gradient alone)."""
    nets = critic.net_params()
    if detach:
        nets = [[p.detach() for p in net] for net in nets]
    q1, q2 = fused_nets(obs, action, nets, 1)
    return q1.squeeze(-1), q2.squeeze(-1)


# ------------------------------------------------------------- replay buffer
class ReplayBuffer:
    """SB3 ``ReplayBuffer`` in device memory: rings [capacity, n_envs, ...]
    with ``capacity = max(buffer_size // n_envs, 1)`` and per-env cursors
    ``pos`` / ``size`` (an env whose step diverged stores nothing, so the
    cursors differ between envs and the rings have no holes).  ``fused``:
    the HIP kernels ``salp_replay_add`` / ``salp_replay_sample`` (CUDA only),
    else torch index ops; both store and draw the same rows."""

    def __init__(self, buffer_size, n_envs, obs_dim, device, act_dim=3, seed=0, fused=None, dtype=torch.float32):
        if act_dim != 3:
            raise ValueError("the replay kernels store the simulator's 3 action dimensions")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.fused = self.device.type == "cuda" if fused is None else bool(fused)
        if self.fused and (self.device.type != "cuda" or dtype != torch.float32):
            raise ValueError("fused=True runs HIP kernels: it needs a ROCm GPU device and float32")
        self.n_envs, self.obs_dim = int(n_envs), int(obs_dim)
        self.capacity = max(int(buffer_size) // self.n_envs, 1)
        self.seed = int(seed)
        z = lambda *s: torch.zeros(s, dtype=dtype, device=self.device)  # noqa: E731
        c, n = self.capacity, self.n_envs
        self.obs, self.next_obs = z(c, n, self.obs_dim), z(c, n, self.obs_dim)
        self.actions, self.rewards, self.dones = z(c, n, 3), z(c, n), z(c, n)
        self.pos = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.size = torch.zeros(n, dtype=torch.int64, device=self.device)
        self._c = None
        if self.fused:
            self._c = _lib.SalpReplay(c, n, self.obs_dim, 0, self.obs.data_ptr(), self.next_obs.data_ptr(),
                                      self.actions.data_ptr(), self.rewards.data_ptr(), self.dones.data_ptr(),
                                      self.pos.data_ptr(), self.size.data_ptr())

    def add(self, obs, actions, obs_after, terminal_obs, reward, terminated, truncated, guard=True, diverged_out=None):
        """One env-step of every env (what ``BatchedSalpEnv.step(auto_reset=
        True, out=...)`` wrote: fp64 reward, u8 flags).  Returns the diverged
        mask (u8 [n_envs] when fused, else bool), written to ``diverged_out``
        when given."""
        if not self.fused:
            bad = torch_replay_add(self, obs, actions, obs_after, terminal_obs, reward, terminated, truncated, guard)
            if diverged_out is not None:
                diverged_out.copy_(bad)
                return diverged_out
            return bad
        n, D = self.n_envs, self.obs_dim
        for name, t, shape, dt in (("obs", obs, (n, D), torch.float32), ("actions", actions, (n, 3), torch.float32),
                                   ("obs_after", obs_after, (n, D), torch.float32),
                                   ("terminal_obs", terminal_obs, (n, D), torch.float32),
                                   ("reward", reward, (n,), torch.float64),
                                   ("terminated", terminated, (n,), torch.uint8),
                                   ("truncated", truncated, (n,), torch.uint8)):
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"ReplayBuffer.add: {name!r} must be a contiguous {dt} tensor of shape {shape} on "
                                 f"{self.device}")
        if diverged_out is None:
            diverged_out = torch.empty(n, dtype=torch.uint8, device=self.device)
        a = _lib.SalpReplayAdd(obs.data_ptr(), actions.data_ptr(), obs_after.data_ptr(), terminal_obs.data_ptr(),
                               reward.data_ptr(), terminated.data_ptr(), truncated.data_ptr(),
                               DIVERGED_OBS_ABS if guard else 0.0, DIVERGED_REWARD_ABS if guard else 0.0,
                               diverged_out.data_ptr())
        _lib.check(_lib.load().salp_replay_add(ctypes.byref(self._c), ctypes.byref(a), _stream(self.device)))
        return diverged_out

    def sample(self, batch_size, update, return_indices=False):
        """``batch_size`` transitions (obs, actions, next_obs, rewards, dones)
        drawn for gradient step ``update`` (a [1] int64 device tensor: a
        replayed graph sees its new value).  At least one env must have stored
        a transition.  ``return_indices``: also the (env, slot) pairs."""
        B = int(batch_size)
        if not self.fused:
            env, slot = torch_replay_indices(self.size, update, self.seed, B)
            out = (self.obs[slot, env], self.actions[slot, env], self.next_obs[slot, env], self.rewards[slot, env],
                   self.dones[slot, env])
            return out + ((env, slot) if return_indices else ())
        if update.dtype != torch.int64 or update.numel() != 1 or update.device != self.device:
            raise ValueError("ReplayBuffer.sample: update must be a one-element int64 tensor on the buffer's device")
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)  # noqa: E731
        obs, nxt, act, rew, done = new(B, self.obs_dim), new(B, self.obs_dim), new(B, 3), new(B), new(B)
        env = slot = None
        if return_indices:
            env = torch.empty(B, dtype=torch.int64, device=self.device)
            slot = torch.empty(B, dtype=torch.int64, device=self.device)
        s = _lib.SalpReplaySample(B, self.seed & 0xFFFFFFFFFFFFFFFF, update.data_ptr(), obs.data_ptr(),
                                  nxt.data_ptr(), act.data_ptr(), rew.data_ptr(), done.data_ptr(),
                                  env.data_ptr() if return_indices else None,
                                  slot.data_ptr() if return_indices else None)
        _lib.check(_lib.load().salp_replay_sample(ctypes.byref(self._c), ctypes.byref(s), _stream(self.device)))
        return (obs, act, nxt, rew, done) + ((env, slot) if return_indices else ())


# -------------------------------------------------------------------- policy
def _mlp(d_in, hidden, d_out=None):
    layers, d = [], d_in
    for h in hidden:
        layers += [nn.Linear(d, h), nn.ReLU()]
        d = h
    if d_out is not None:
        layers.append(nn.Linear(d, d_out))
    return nn.Sequential(*layers)


def _flatten(ps):
    """Make the parameters views into one new flat buffer, back to back in the given order."""
    flat = torch.cat([p.detach().reshape(-1) for p in ps])
    off = 0
    for p in ps:
        p.data = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    return flat


def _is_flat(flat, ps):
    if flat is None:
        return False
    off = 0
    for p in ps:
        if p.data_ptr() != flat.data_ptr() + off * flat.element_size() or not p.is_contiguous():
            return False
        off += p.numel()
    return off == flat.numel()


class _Actor(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden):
        super().__init__()
        self.latent_pi = _mlp(obs_dim, hidden)
        self.mu = nn.Linear(hidden[-1], act_dim)
        self.log_std = nn.Linear(hidden[-1], act_dim)
        self.flat = None

    def forward(self, obs):
        """(mean, raw log-std); the heads clamp the log-std."""
        z = self.latent_pi(obs)
        return self.mu(z), self.log_std(z)

    def net_params(self):
        """The parameters in the fused network's flat order (include/salp.h
        SalpSacNetTensor): the two heads are one 2 act_dim-row layer, mu's rows
        first."""
        return [*self.latent_pi.parameters(), self.mu.weight, self.log_std.weight, self.mu.bias, self.log_std.bias]

    def flatten_(self):
        self.flat = _flatten(self.net_params())
        return self

    def is_flat(self):
        return _is_flat(self.flat, self.net_params())


class _Critic(nn.Module):
    """SB3 ``ContinuousCritic`` with n_critics = 2.  After :meth:`flatten_`
    every parameter is a view into ``flat``, so Polyak is one launch."""

    def __init__(self, obs_dim, act_dim, hidden):
        super().__init__()
        self.qf0 = _mlp(obs_dim + act_dim, hidden, 1)
        self.qf1 = _mlp(obs_dim + act_dim, hidden, 1)
        self.flat = None

    def forward(self, obs, action):
        x = torch.cat([obs, action], dim=1)
        return self.qf0(x).squeeze(-1), self.qf1(x).squeeze(-1)

    def net_params(self):
        """Each Q-network's parameters in the fused network's flat order (torch's own)."""
        return [list(self.qf0.parameters()), list(self.qf1.parameters())]

    def flatten_(self):
        self.flat = _flatten(list(self.parameters()))
        return self

    def is_flat(self):
        return _is_flat(self.flat, list(self.parameters()))


class SACPolicy(nn.Module):
    """SB3's SAC ``MlpPolicy`` (``net_arch=[256, 256]``, ReLU, two critics, a
    target copy of the critics; torch's default init).  Built on ``device``:
    the critics' parameters are views into one flat buffer each (``critic.flat``,
    ``critic_target.flat``); after moving or copying the module call
    :meth:`flatten_` again."""

    def __init__(self, obs_dim, act_dim=3, hidden=(256, 256), device=None):
        super().__init__()
        self.obs_dim, self.act_dim, self.hidden = int(obs_dim), int(act_dim), tuple(hidden)
        self.actor = _Actor(obs_dim, act_dim, hidden)
        self.critic = _Critic(obs_dim, act_dim, hidden)
        self.critic_target = copy.deepcopy(self.critic)
        for p in self.critic_target.parameters():
            p.requires_grad_(False)
        if device is not None:
            self.to(device)
        self.flatten_()

    def flatten_(self):
        self.actor.flatten_()
        self.critic.flatten_()
        self.critic_target.flatten_()
        return self

    def forward(self, obs, eps=None):
        """Action in [-1, 1]: the mean's tanh (deterministic), or a sample with noise ``eps``."""
        mu, log_std = self.actor(obs)
        if eps is None:
            return torch.tanh(mu)
        return torch_squashed_gaussian(mu, log_std, eps)[0]


# ------------------------------------------------------------- gradient step
def _check_fused_mlp(policy, fused, device):
    """``fused_mlp=True`` needs the HIP heads, a GPU and the 256-256 networks in their flat buffers."""
    if torch.device(device).type != "cuda":
        raise ValueError("fused_mlp=True runs HIP kernels: it needs a ROCm GPU device")
    if not fused:
        raise ValueError("fused_mlp=True needs fused=True: the networks' kernels feed the fused heads")
    if tuple(policy.hidden) != (_lib.SAC_HIDDEN, _lib.SAC_HIDDEN):
        raise ValueError(f"fused_mlp=True is built for hidden sizes (256, 256), not {tuple(policy.hidden)}")
    if policy.obs_dim + policy.act_dim > _lib.SAC_NET_IN_MAX or 2 * policy.act_dim > _lib.SAC_NET_OUT_MAX:
        raise ValueError("fused_mlp=True: obs_dim + act_dim <= 17 and act_dim <= 3")
    if not (policy.actor.is_flat() and policy.critic.is_flat() and policy.critic_target.is_flat()):
        raise ValueError("fused_mlp=True: the networks' parameters must be views into their flat buffers: "
                         "SACPolicy.flatten_()")


def critic_phase(policy, log_alpha, batch, eps_pi, eps_next, gamma, target_entropy, fused, fused_mlp=False):
    """First half of SB3 ``SAC.train``'s gradient step, up to the backward of
    the critic and entropy-coefficient losses (no optimizer step).  The
    critics' gradients are added to their ``.grad`` as autograd does;
    ``log_alpha.grad`` is overwritten with this batch's gradient on both paths.  ``batch`` = (obs,
    actions, next_obs, rewards, dones); ``eps_*`` [B, 3] N(0, 1) noise for the
    actions at obs and next_obs.  ``fused_mlp``: the networks run as
    :func:`fused_actor` / :func:`fused_critic` launches instead of torch
    modules.  Returns what :func:`actor_phase` needs."""
    obs, act, next_obs, rew, done = batch
    head = squashed_gaussian if fused else torch_squashed_gaussian
    if fused_mlp:
        _check_fused_mlp(policy, fused, obs.device)
        actor, critic, critic_target = (lambda o: fused_actor(policy.actor, o),
                                        lambda o, a: fused_critic(policy.critic, o, a),
                                        lambda o, a: fused_critic(policy.critic_target, o, a))
    else:
        actor, critic, critic_target = policy.actor, policy.critic, policy.critic_target
    a_pi, logp = head(*actor(obs), eps_pi)
    with torch.no_grad():
        a_next, logp_next = head(*actor(next_obs), eps_next)
        q1t, q2t = critic_target(next_obs, a_next)
    q1, q2 = critic(obs, act)
    if fused:
        out, target, dq1, dq2, alpha = td_head(rew, done, q1t, q2t, logp_next, q1, q2, logp, log_alpha, gamma,
                                               target_entropy)
        torch.autograd.backward((q1, q2), (dq1, dq2))
        if log_alpha.requires_grad:
            log_alpha.grad = out[2:3]
        critic_loss, ent_coef_loss = out[0], out[1]
    else:
        critic_loss, ent_coef_loss, target, alpha = torch_td_head(rew, done, q1t, q2t, logp_next, q1, q2, logp,
                                                                  log_alpha, gamma, target_entropy)
        log_alpha.grad = None   # as the fused branch: this batch's gradient alone, never a running sum
        (critic_loss + ent_coef_loss if log_alpha.requires_grad else critic_loss).backward()
        critic_loss, ent_coef_loss = critic_loss.detach(), ent_coef_loss.detach()
    return {"obs": obs, "a_pi": a_pi, "logp": logp, "alpha": alpha, "target": target,
            "critic_loss": critic_loss, "ent_coef_loss": ent_coef_loss}


def actor_phase(policy, st, fused, fused_mlp=False):
    """Second half: critics(obs, a_pi), the actor loss and its backward into
    the actor's parameters only (SB3 lets it reach the critics too and zeroes
    those gradients before their next step; ``fused_mlp`` does not compute
    them).  Returns the actor loss."""
    if fused_mlp:
        _check_fused_mlp(policy, fused, st["obs"].device)
        q1_pi, q2_pi = fused_critic(policy.critic, st["obs"], st["a_pi"], detach=True)
    else:
        q1_pi, q2_pi = policy.critic(st["obs"], st["a_pi"])
    params = list(policy.actor.parameters())
    if fused:
        out, dlogp, dq1, dq2 = pi_head(st["alpha"], st["logp"], q1_pi, q2_pi)
        torch.autograd.backward((q1_pi, q2_pi, st["logp"]), (dq1, dq2, dlogp), inputs=params)
        return out[0]
    loss = torch_pi_head(st["alpha"], st["logp"], q1_pi, q2_pi)
    loss.backward(inputs=params)
    return loss.detach()


# ------------------------------------------------------------------- learner
class SAC:
    """SB3-style SAC on a :class:`~grasp_lab_salp_amd.vec_env.SalpVecEnv` (or
    anything exposing ``.sim`` = :class:`BatchedSalpEnv`).  Constructor
    arguments and defaults follow SB3's ``SAC``; every keyword of
    ``src/train_robot.py:62-69`` is accepted.

    ``train_freq``: lock-step env-steps (of all envs) between updates, an int
    or ``(n, "step")``; ``gradient_steps=-1``: as many gradient steps as
    transitions collected.  ``ent_coef``: ``"auto"``, ``"auto_<init>"`` or a
    fixed value.  ``fused``: HIP kernels around the GEMMs (default on a GPU) or
    plain torch.  ``fused_mlp`` (default off; needs ``fused``, a GPU and the
    256-256 networks): the networks themselves run as the HIP kernels of
    csrc/salp_sac_mlp.hip, forward and backward, in the collection too.  ``tensorboard_log`` is accepted and unused (``history`` holds
    the rows a logger would get); ``device`` other than ``None`` / ``"auto"``
    must be the simulator's device.  ``seed`` seeds the policy's init (without
    moving the process-wide generator), the exploration noise and the sampler.
    One GPU only."""

    def __init__(self, policy, env, learning_rate=3e-4, buffer_size=1_000_000, learning_starts=100, batch_size=256,
                 tau=0.005, gamma=0.99, train_freq=1, gradient_steps=1, ent_coef="auto", target_entropy="auto",
                 seed=0, fused=None, verbose=0, tensorboard_log=None, device="auto", reset_nonfinite=True,
                 fused_mlp=False):
        if policy not in ("MlpPolicy", None) and not isinstance(policy, SACPolicy):
            raise ValueError("policy must be 'MlpPolicy' or a SACPolicy")
        self.env = env
        self.sim = getattr(env, "sim", env)
        self.device = torch.device(self.sim.device)
        if device not in (None, "auto") and torch.device(device).type != self.device.type:
            raise ValueError(f"device={device!r}: the learner runs on the simulator's device, {self.device}")
        self.n_envs, self.obs_dim, self.act_dim = int(self.sim.n_envs), int(self.sim.obs_dim), 3
        on_gpu = self.device.type == "cuda"
        if fused and not on_gpu:
            raise ValueError("fused=True runs HIP kernels: it needs a ROCm GPU device")
        self.fused = on_gpu if fused is None else bool(fused)
        if isinstance(train_freq, (tuple, list)):
            if len(train_freq) != 2 or train_freq[1] not in ("step", "steps"):
                raise ValueError("train_freq: an int or (n, 'step'); episode-based collection is not built")
            train_freq = train_freq[0]
        self.train_freq, self.gradient_steps = int(train_freq), int(gradient_steps)
        if self.train_freq < 1:
            raise ValueError("train_freq must be >= 1")
        self.learning_rate, self.learning_starts = float(learning_rate), int(learning_starts)
        self.buffer_size, self.ent_coef = int(buffer_size), ent_coef
        self.batch_size, self.tau, self.gamma = int(batch_size), float(tau), float(gamma)
        self.verbose, self.tensorboard_log, self.reset_nonfinite = verbose, tensorboard_log, bool(reset_nonfinite)
        self.seed = int(seed)
        if isinstance(policy, SACPolicy):
            self.policy = policy
        else:
            # the init draws come from the global CPU generator seeded with `seed`, inside a fork:
            # building a learner leaves the process-wide generator where it was
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(self.seed)
                self.policy = SACPolicy(self.obs_dim, self.act_dim, device=self.device)
        if self.fused and not (self.policy.critic.is_flat() and self.policy.critic_target.is_flat()):
            raise ValueError("the critics' parameters must be views into their flat buffers: SACPolicy.flatten_()")
        self.fused_mlp = bool(fused_mlp)
        if self.fused_mlp:
            _check_fused_mlp(self.policy, self.fused, self.device)
        self.target_entropy = -float(self.act_dim) if target_entropy == "auto" else float(target_entropy)
        init, auto = 1.0, isinstance(ent_coef, str)
        if auto:
            if not ent_coef.startswith("auto"):
                raise ValueError("ent_coef: 'auto', 'auto_<initial value>' or a float")
            if "_" in ent_coef:
                init = float(ent_coef.split("_")[1])
        else:
            init = float(ent_coef)
        if not init > 0:
            raise ValueError("the entropy coefficient must be positive")
        self.log_ent_coef = torch.full((1,), math.log(init), dtype=torch.float32, device=self.device,
                                       requires_grad=auto)
        adam = lambda ps: torch.optim.Adam(ps, lr=self.learning_rate, fused=on_gpu or None)  # noqa: E731
        self.actor_opt = adam(self.policy.actor.parameters())
        self.critic_opt = adam(self.policy.critic.parameters())
        self.ent_coef_opt = adam([self.log_ent_coef]) if auto else None
        self.sample_gen = sampling_generator(self.seed, self.device)
        self.replay = ReplayBuffer(buffer_size, self.n_envs, self.obs_dim, self.device, seed=self.seed,
                                   fused=self.fused)
        self.low = torch.tensor([0.0, 0.0, -1.0], device=self.device)
        self.high = torch.tensor([1.0, 1.0, 1.0], device=self.device)
        self._update = torch.zeros(1, dtype=torch.int64, device=self.device)   # gradient steps so far
        self._obs = None
        self._out = None
        self._nonfinite = torch.zeros((), dtype=torch.int64, device=self.device)
        self._ep_stats = torch.zeros(4, dtype=torch.float64, device=self.device)
        self._loss_acc = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._collect_stream = None
        self._events = []
        self.num_timesteps = 0
        self.n_updates = 0
        self.logger = {}
        self.timing = {"collect_s": 0.0, "sample_s": 0.0, "update_s": 0.0}
        self.history = []
        self.locals = {}               # the last env-step's device tensors, for callbacks
        self.callback_metrics = {}     # the latest value of every key a callback recorded
        self._recorded = {}            # ... those since the last history row
        self.last_eval = None          # the per-episode results of the last evaluate()
        self.predict_only = False      # SAC.load(path, env=None): no env to learn on

    # -------------------------------------------------------- collection
    def _need_env(self, what):
        if self.predict_only:
            raise RuntimeError(f"{what}: this model was loaded without an env (SAC.load(path, env=None)): it can "
                               "only predict; load it with env=... to train or evaluate")
    def _step_out(self):
        """Two sets of step outputs, used in turn: the observation the next
        action is taken on stays valid while the step after it is written."""
        if self._out is None:
            n, od, dev = self.n_envs, self.obs_dim, self.device
            mk = lambda: {"obs": torch.empty((n, od), dtype=torch.float32, device=dev),  # noqa: E731
                          "reward": torch.empty(n, dtype=torch.float64, device=dev),
                          "terminated": torch.empty(n, dtype=torch.uint8, device=dev),
                          "truncated": torch.empty(n, dtype=torch.uint8, device=dev),
                          "terminal_obs": torch.empty((n, od), dtype=torch.float32, device=dev),
                          "info": torch.empty((n, INFO_DIM), dtype=torch.float64, device=dev)}
            self._out = [mk(), mk()]
        self._out.reverse()
        return self._out[0]

    @torch.no_grad()
    def _sample_action(self, obs):
        """The scaled action in [-1, 1]: uniform until learning_starts, then the policy's sample."""
        if self.num_timesteps < self.learning_starts:
            return 2.0 * torch.rand((self.n_envs, 3), generator=self.sample_gen, device=self.device) - 1.0
        eps = torch.randn((self.n_envs, 3), generator=self.sample_gen, device=self.device)
        head = squashed_gaussian if self.fused else torch_squashed_gaussian
        mu_ls = fused_actor(self.policy.actor, obs) if self.fused_mlp else self.policy.actor(obs)
        return head(*mu_ls, eps)[0]

    @torch.no_grad()
    def _eval_action(self, obs, deterministic=True):
        """The policy's scaled action in [-1, 1] on ``obs`` [n, obs_dim] (any
        n): the one action function of :meth:`evaluate`.  With ``fused_mlp``
        the actor's kernel and then the head kernel, with zero noise when
        deterministic: fmaf(exp(ls), 0, mu) is mu for the clamped log-std, so
        that is exactly tanh(mu).  Else the torch modules."""
        n = obs.shape[0]
        noise = lambda: torch.randn((n, 3), generator=self.sample_gen, device=self.device)  # noqa: E731
        if self.fused_mlp:
            eps = torch.zeros((n, 3), dtype=torch.float32, device=self.device) if deterministic else noise()
            return squashed_gaussian(*fused_actor(self.policy.actor, obs), eps)[0]
        mu, log_std = self.policy.actor(obs)
        if deterministic:
            return torch.tanh(mu)
        return (squashed_gaussian if self.fused else torch_squashed_gaussian)(mu, log_std, noise())[0]

    def collect_step(self):
        """One lock-step env-step of every env into the replay buffer.  The
        step's device tensors are left in ``self.locals`` for the callbacks:
        ``obs`` (after the step), ``actions`` (scaled to [-1, 1]), ``rewards``,
        ``terminated``, ``truncated``, ``dones``, ``info`` [n, INFO_DIM] and
        ``diverged`` (transitions the guard dropped).  They alias the two
        alternating output sets of :meth:`_step_out`: the step after the next
        overwrites them."""
        self._need_env("collect_step")
        sim = self.sim
        if self._obs is None:
            self._obs = sim.reset()
        obs = self._obs
        a = self._sample_action(obs).contiguous()
        r = sim.step(unscale_action(a, self.low, self.high), auto_reset=True, out=self._step_out())
        diverged = self.replay.add(obs, a, r.obs, r.terminal_obs, r.reward, r.terminated, r.truncated,
                                   guard=self.reset_nonfinite)
        bad = diverged.bool()
        done = (r.terminated | r.truncated).bool()
        self.locals = {"obs": r.obs, "actions": a, "rewards": r.reward, "terminated": r.terminated,
                       "truncated": r.truncated, "dones": done, "info": r.info, "diverged": diverged}
        if self.reset_nonfinite:
            # as PPO._reset_diverged: a diverged env that did not end its episode is reset on the spot
            self._nonfinite += bad.sum()
            again = bad & ~done
            fresh = sim.reset(mask=again)
            r.obs.copy_(torch.where(again.unsqueeze(1), fresh, r.obs))
        ended = done & ~bad
        ep_ret, ep_len = r.info[:, _EP_RETURN], r.info[:, _EP_LEN]
        zero = torch.zeros_like(ep_ret)
        self._ep_stats += torch.stack([torch.where(ended, ep_ret, zero).sum(), ended.sum().double(),
                                       (ended & r.terminated.bool()).sum().double(),
                                       torch.where(ended, ep_len, zero).sum()])
        self._obs = r.obs
        self.num_timesteps += self.n_envs

    @property
    def nonfinite_resets(self):
        """Envs whose transition was dropped because their state diverged (host int; syncs)."""
        return int(self._nonfinite)

    # ------------------------------------------------------------ update
    def _noise(self):
        return torch.randn((self.batch_size, 3), generator=self.sample_gen, device=self.device)

    def gradient_step(self, batch):
        """One SB3 ``SAC.train`` gradient step on ``batch`` (see the module
        docstring for the order); adds the losses to the running sums."""
        pol = self.policy
        self.critic_opt.zero_grad(set_to_none=True)
        self.actor_opt.zero_grad(set_to_none=True)
        if self.ent_coef_opt is not None:
            self.ent_coef_opt.zero_grad(set_to_none=True)
        st = critic_phase(pol, self.log_ent_coef, batch, self._noise(), self._noise(), self.gamma,
                          self.target_entropy, self.fused, self.fused_mlp)
        self.critic_opt.step()
        if self.ent_coef_opt is not None:
            self.ent_coef_opt.step()
        actor_loss = actor_phase(pol, st, self.fused, self.fused_mlp)
        self.actor_opt.step()
        if self.fused:
            polyak(pol.critic.flat, pol.critic_target.flat, self.tau)
        else:
            torch_polyak(pol.critic.parameters(), pol.critic_target.parameters(), self.tau)
        self._loss_acc += torch.stack([st["critic_loss"], actor_loss, st["ent_coef_loss"], st["alpha"][0]])
        self._update += 1
        self.n_updates += 1

    def train(self, gradient_steps, events=None):
        """``gradient_steps`` times: sample a batch, one gradient step.
        ``events``: a list that receives three HIP events of the first step,
        all on the stream the update runs on (before the sample, between the
        sample and the update, after the update), for the phase timings."""
        for k in range(gradient_steps):
            ev = events if (events is not None and k == 0) else None
            if ev is not None:
                ev.append(self._event())
            batch = self.replay.sample(self.batch_size, self._update)
            if ev is not None:
                ev.append(self._event())
            self.gradient_step(batch)
            if ev is not None:
                ev.append(self._event())

    def _event(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record(torch.cuda.current_stream(self.device))
        return e

    def _drain_events(self):
        """Resolve the recorded phase events into ``timing`` (synchronises)."""
        if not self._events:
            return
        self._events[-1][0][-1].synchronize()
        for ev, steps in self._events:
            self.timing["collect_s"] += ev[0].elapsed_time(ev[1]) / 1e3
            if len(ev) == 5:   # the first gradient step of the iteration stands for all of them
                self.timing["sample_s"] += ev[2].elapsed_time(ev[3]) / 1e3 * steps
                self.timing["update_s"] += ev[3].elapsed_time(ev[4]) / 1e3 * steps
        self._events = []

    def learn(self, total_timesteps, callback=None, tb_log_name=None, progress_bar=False, log_interval=100):
        """Collect ``train_freq`` env-steps, then train, until ``total_timesteps``
        transitions.  ``callback``: a callback of
        :mod:`grasp_lab_salp_amd.callbacks`, a list of them, or None;
        ``on_training_start`` runs once, ``on_step`` after every env-step, on
        the collection stream (which has waited for the previous update, and
        which the update waits for: evaluation and saving see a consistent
        policy), and ``on_training_end`` at the end.  An ``on_step`` that
        returns False ends training after that env-step, before its update.
        ``tb_log_name`` and ``progress_bar`` are accepted for SB3's signature
        and unused.
        Every ``log_interval`` iterations the phase timings (HIP events: the
        collection on its stream; the first gradient step's sample and update
        on the update's stream, after it has waited for the collection, scaled
        by the number of gradient steps) and a ``history`` row are resolved;
        without callbacks that is the only host synchronisation."""
        self._need_env("learn")
        cb = self._as_callback(callback)
        gpu = self.device.type == "cuda"
        if gpu and self._collect_stream is None:
            self._collect_stream = torch.cuda.Stream(self.device)
        start = self.num_timesteps
        it = 0
        go_on = True
        if cb is not None:
            cb.on_training_start({"self": self, "total_timesteps": total_timesteps}, globals())
        while go_on and self.num_timesteps - start < total_timesteps:
            ev = None
            if gpu:
                # the collection's eager GEMMs stay off the stream the update runs on (DESIGN.md §5 "HIP graphs")
                stream, cs = torch.cuda.current_stream(self.device), self._collect_stream
                cs.wait_stream(stream)
                with torch.cuda.stream(cs):
                    ev = [self._event()]
                    for _ in range(self.train_freq):
                        self.collect_step()
                        if cb is not None and not cb.on_step():
                            go_on = False
                            break
                    ev.append(self._event())
                stream.wait_stream(cs)
            else:
                for _ in range(self.train_freq):
                    self.collect_step()
                    if cb is not None and not cb.on_step():
                        go_on = False
                        break
            steps = 0
            if go_on and self.num_timesteps > self.learning_starts:
                steps = self.gradient_steps if self.gradient_steps >= 0 else self.train_freq * self.n_envs
                self.train(steps, ev)
            if ev is not None:
                self._events.append((ev, steps))
            it += 1
            logged = it % max(int(log_interval), 1) == 0
            if logged:
                self._log()
        if it and not logged:
            self._log()
        if cb is not None:
            cb.on_training_end()
        return self

    def _as_callback(self, callback):
        """None, a callback or a list of callbacks -> None or one initialised callback."""
        if callback is None:
            return None
        from .callbacks import BaseCallback, CallbackList
        if isinstance(callback, (list, tuple)):
            callback = CallbackList(list(callback))
        if not isinstance(callback, BaseCallback):
            raise TypeError("callback: a grasp_lab_salp_amd.callbacks.BaseCallback, a list of them, or None")
        callback.init_callback(self)
        return callback

    def record(self, key, value):
        """A callback's ``logger.record``: kept in ``callback_metrics`` (latest
        values) and added to the next ``history`` row."""
        self.callback_metrics[key] = value
        self._recorded[key] = value

    def _log(self):
        self._drain_events()
        ret_sum, n_ep, n_succ, len_sum = self._ep_stats.tolist()
        k = max(self.n_updates - self.logger.get("n_updates", 0), 1)
        cl, al, el, ec = (self._loss_acc / k).tolist()
        self._loss_acc.zero_()
        self._ep_stats.zero_()
        self.logger = {"timesteps": self.num_timesteps, "n_updates": self.n_updates, "critic_loss": cl,
                       "actor_loss": al, "ent_coef_loss": el, "ent_coef": ec, "episodes": int(n_ep),
                       "ep_return_mean": ret_sum / n_ep if n_ep else None,
                       "success_rate": n_succ / n_ep if n_ep else None,
                       "ep_len_mean": len_sum / n_ep if n_ep else None, "diverged_envs": self.nonfinite_resets}
        if self._recorded:   # what callbacks recorded since the last row
            self.logger.update(self._recorded)
            self._recorded = {}
        self.history.append(self.logger)
        if self.verbose:
            print(self.logger, flush=True)

    # ----------------------------------------------------------- predict
    @torch.no_grad()
    def predict(self, observation, state=None, episode_start=None, deterministic=True):
        """SB3 ``predict``: (action in the env's Box, None).  A NumPy
        observation gives a NumPy action; one observation gives one action."""
        as_numpy = not torch.is_tensor(observation)
        obs = torch.as_tensor(observation, dtype=torch.float32, device=self.device)
        single = obs.dim() == 1
        obs = obs.reshape(-1, self.obs_dim)
        eps = None if deterministic else torch.randn((obs.shape[0], 3), generator=self.sample_gen,
                                                      device=self.device)
        a = unscale_action(self.policy(obs, eps), self.low, self.high)
        a = a[0] if single else a
        return (a.cpu().numpy() if as_numpy else a), None

    # ---------------------------------------------------------- evaluate
    @torch.no_grad()
    def evaluate(self, env, n_eval_episodes=10, deterministic=True, return_episode_rewards=False, poll_every=8):
        """SB3 ``evaluate_policy`` on ``env`` (a :class:`SalpVecEnv` or
        :class:`BatchedSalpEnv` of any size, on this learner's device): reset
        it, then step all its envs in lock-step on :meth:`_eval_action`'s
        actions until env ``i`` has finished ``(n_eval_episodes + i) // n_envs``
        episodes.  The bookkeeping is one
        :class:`~grasp_lab_salp_amd.metrics.EvalAccount` launch per step; the
        number of missing episodes is copied to the host every ``poll_every``
        steps, and the loop ends at the latest after ``max(target) *
        max_cycles`` steps, by when every episode has timed out.  Returns
        (mean, std) of the episode returns (``np.std``), or (returns, lengths)
        per episode in slot order; ``last_eval`` keeps both and the successes.
        The training env is not touched, nor ``sample_gen`` when deterministic."""
        from .metrics import EvalAccount
        self._need_env("evaluate")
        sim = getattr(env, "sim", env)
        for attr in ("step", "reset", "n_envs", "obs_dim", "params", "device"):
            if not hasattr(sim, attr):
                raise TypeError("evaluate: env must be a SalpVecEnv or BatchedSalpEnv, e.g. SalpVecEnv(n_eval_episodes)")
        if int(sim.obs_dim) != self.obs_dim or torch.device(sim.device) != self.device:
            raise ValueError(f"evaluate: env has obs_dim {sim.obs_dim} on {sim.device}; the model has {self.obs_dim} "
                             f"on {self.device}")
        n, od, dev = int(sim.n_envs), self.obs_dim, self.device
        acc = EvalAccount(n_eval_episodes, n, dev, fused=self.fused)
        out = {"obs": torch.empty((n, od), dtype=torch.float32, device=dev),
               "reward": torch.empty(n, dtype=torch.float64, device=dev),
               "terminated": torch.empty(n, dtype=torch.uint8, device=dev),
               "truncated": torch.empty(n, dtype=torch.uint8, device=dev),
               "terminal_obs": None, "info": torch.empty((n, INFO_DIM), dtype=torch.float64, device=dev)}
        obs = sim.reset()
        left = acc.n_eval_episodes
        max_steps = acc.max_target * int(sim.params.max_cycles)
        poll_every = max(int(poll_every), 1)
        for t in range(1, max_steps + 1):
            a = self._eval_action(obs, deterministic).contiguous()
            r = sim.step(unscale_action(a, self.low, self.high), auto_reset=True, out=out)
            acc.push(r.info, r.terminated, r.truncated)
            obs = r.obs
            if t % poll_every == 0 or t == max_steps:
                left = acc.left()
                if left == 0:
                    break
        if left:
            raise RuntimeError(f"evaluate: {left} of {acc.n_eval_episodes} episodes did not end within {max_steps} steps")
        returns, lengths = acc.ep_return.tolist(), [int(v) for v in acc.ep_len.tolist()]
        self.last_eval = {"returns": returns, "lengths": lengths, "successes": [bool(s) for s in acc.success.tolist()]}
        if return_episode_rewards:
            return returns, lengths
        return float(np.mean(returns)), float(np.std(returns))

    # -------------------------------------------------------- save / load
    FORMAT, FORMAT_VERSION = "grasp_lab_salp_amd.SAC", 1
    _HYPERPARAMETERS = ("learning_rate", "buffer_size", "learning_starts", "batch_size", "tau", "gamma", "train_freq",
                        "gradient_steps", "ent_coef", "target_entropy", "reset_nonfinite")

    @staticmethod
    def _zip_path(path):
        path = os.fspath(path)
        return path if os.path.splitext(path)[1] else path + ".zip"

    def save(self, path):
        """Everything a resumed run needs, as a zip of this project's own
        layout (``.zip`` is appended to a ``path`` without a suffix; SB3 cannot
        read it, nor this SB3's files): ``data.json`` (format tag and version,
        hyperparameters, counters, seed, obs_dim, fused, fused_mlp),
        ``policy.pth`` (actor, critics, target critics), ``actor.optimizer.pth``,
        ``critic.optimizer.pth``, ``ent_coef_optimizer.pth``,
        ``pytorch_variables.pth`` (``log_ent_coef``) and ``rng.pth`` (the state
        of ``sample_gen``).  The replay buffer is saved apart
        (:meth:`save_replay_buffer`).  Returns the file's path; synchronises."""
        path = self._zip_path(path)
        cpu = lambda t: t.detach().to("cpu", copy=True)  # noqa: E731

        def opt_state(opt):
            if opt is None:
                return {}
            sd = opt.state_dict()
            return {"state": {k: {n: (cpu(v) if torch.is_tensor(v) else v) for n, v in s.items()}
                              for k, s in sd["state"].items()}, "param_groups": sd["param_groups"]}

        data = {"format": self.FORMAT, "version": self.FORMAT_VERSION,
                "hyperparameters": {k: getattr(self, k) for k in self._HYPERPARAMETERS},
                "num_timesteps": int(self.num_timesteps), "n_updates": int(self.n_updates),
                "update": int(self._update), "seed": self.seed, "obs_dim": self.obs_dim, "fused": self.fused,
                "fused_mlp": self.fused_mlp, "device_type": self.device.type}
        files = {"policy.pth": {k: cpu(v) for k, v in self.policy.state_dict().items()},
                 "actor.optimizer.pth": opt_state(self.actor_opt), "critic.optimizer.pth": opt_state(self.critic_opt),
                 "ent_coef_optimizer.pth": opt_state(self.ent_coef_opt),
                 "pytorch_variables.pth": {"log_ent_coef": cpu(self.log_ent_coef)},
                 "rng.pth": {"sample_gen": self.sample_gen.get_state().clone()}}
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
            z.writestr("data.json", json.dumps(data, indent=1))
            for name, obj in files.items():
                buf = io.BytesIO()
                torch.save(obj, buf)
                z.writestr(name, buf.getvalue())
        return path

    @classmethod
    def load(cls, path, env=None, device="auto", **kwargs):
        """A learner from :meth:`save`'s file (``.zip`` appended as there).
        ``kwargs`` override the saved hyperparameters, as in SB3.  Tensors are
        read with ``torch.load(weights_only=True)`` and copied into the new
        learner's flat parameter buffers, which the kernels' raw pointers stay
        valid for.  ``env=None`` gives a predict-only model on ``device``
        (``"cpu"`` too; ``"auto"``: the GPU if there is one): ``predict``
        works; ``learn``, ``collect_step`` and ``evaluate`` raise."""
        path = cls._zip_path(path)
        with zipfile.ZipFile(path) as z:
            data = json.loads(z.read("data.json"))
            if data.get("format") != cls.FORMAT or data.get("version") != cls.FORMAT_VERSION:
                raise ValueError(f"{path}: not a {cls.FORMAT} file of version {cls.FORMAT_VERSION} "
                                 f"(format {data.get('format')!r}, version {data.get('version')!r})")
            blobs = {n: torch.load(io.BytesIO(z.read(n)), map_location="cpu", weights_only=True)
                     for n in ("policy.pth", "actor.optimizer.pth", "critic.optimizer.pth", "ent_coef_optimizer.pth",
                               "pytorch_variables.pth", "rng.pth")}
        hp = dict(data["hyperparameters"])
        if isinstance(hp.get("train_freq"), list):
            hp["train_freq"] = tuple(hp["train_freq"])
        predict_only = env is None
        if predict_only:
            if device in (None, "auto"):
                device = "cuda" if torch.cuda.is_available() else "cpu"
            env = _NoEnv(data["obs_dim"], device)
            hp["buffer_size"] = 1                   # no replay buffer to speak of
            device = None
        dev_type = torch.device(getattr(env, "sim", env).device).type
        for k, saved in (("fused", data["fused"]), ("fused_mlp", data["fused_mlp"])):
            hp[k] = bool(saved) and dev_type == "cuda"      # the HIP kernels need the GPU they were saved on
        hp["seed"] = data["seed"]
        hp.update(kwargs)
        m = cls("MlpPolicy", env, device=device, **hp)
        if m.obs_dim != data["obs_dim"]:
            raise ValueError(f"{path}: saved with obs_dim {data['obs_dim']}, the env has {m.obs_dim}")
        m.predict_only = predict_only
        if predict_only:
            m.env = None
        m.policy.load_state_dict(blobs["policy.pth"], strict=True)      # in place: the flat buffers stay
        pol = m.policy
        if not (pol.actor.is_flat() and pol.critic.is_flat() and pol.critic_target.is_flat()):
            raise RuntimeError("SAC.load: the parameters left their flat buffers")
        for opt, name in ((m.actor_opt, "actor.optimizer.pth"), (m.critic_opt, "critic.optimizer.pth"),
                          (m.ent_coef_opt, "ent_coef_optimizer.pth")):
            if opt is not None and blobs[name]:
                groups = opt.state_dict()["param_groups"]   # this learner's own settings (lr may be overridden)
                opt.load_state_dict({"state": blobs[name]["state"], "param_groups": groups})
        with torch.no_grad():
            m.log_ent_coef.copy_(blobs["pytorch_variables.pth"]["log_ent_coef"])
        m._update.fill_(int(data["update"]))
        m.num_timesteps, m.n_updates = int(data["num_timesteps"]), int(data["n_updates"])
        m.logger = {"timesteps": m.num_timesteps, "n_updates": m.n_updates}
        if data.get("device_type") == m.device.type:         # a generator's state is its device type's own
            m.sample_gen.set_state(blobs["rng.pth"]["sample_gen"])
        return m

    def save_replay_buffer(self, path):
        """The replay rings, the per-env cursors and the sampler's seed to ``path`` (one ``torch.save`` file)."""
        rb = self.replay
        d = os.path.dirname(os.fspath(path))
        if d:
            os.makedirs(d, exist_ok=True)
        obj = {k: getattr(rb, k).detach().to("cpu", copy=True) for k in _REPLAY_TENSORS}
        obj.update(capacity=rb.capacity, n_envs=rb.n_envs, obs_dim=rb.obs_dim, seed=rb.seed)
        torch.save(obj, os.fspath(path))
        return os.fspath(path)

    def load_replay_buffer(self, path):
        """:meth:`save_replay_buffer`'s file into this learner's rings, in
        place (the kernels hold their raw pointers).  A file of another
        capacity, n_envs or obs_dim raises ValueError."""
        obj = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
        rb = self.replay
        for k in ("capacity", "n_envs", "obs_dim"):
            if int(obj[k]) != getattr(rb, k):
                raise ValueError(f"{path}: replay buffer with {k} = {obj[k]}, this learner's has {getattr(rb, k)}")
        for k in _REPLAY_TENSORS:
            getattr(rb, k).copy_(obj[k])
        rb.seed = int(obj["seed"])


_REPLAY_TENSORS = ("obs", "next_obs", "actions", "rewards", "dones", "pos", "size")


class _NoEnv:
    """What SAC's constructor reads of an env, for a predict-only model."""

    n_envs = 1

    def __init__(self, obs_dim, device):
        self.obs_dim = int(obs_dim)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
