"""RecurrentPPO with sb3-contrib's ``MlpLstmPolicy`` on the batched simulator:
the learner of ``/root/reference/src/train_robot_recurrent_ppo.py:85-107``
(``lstm_hidden_size=256, n_lstm_layers=1, enable_critic_lstm=True,
shared_lstm=False``; lr 3e-4, n_steps 2048, batch 64, 10 epochs, gamma 0.99,
GAE lambda 0.95, clip 0.2, ent 0, vf 0.5, max_grad_norm 0.5).

sb3-contrib (>= 2.0) is not installed here: its semantics are restated, and
parity with it is unpinned.  What is kept:

* policy: an LSTM for the actor and another for the critic on the raw
  observation, then SB3's ``net_arch`` pi=[64, 64] / vf=[64, 64] tanh MLPs, the
  action / value heads and a state-independent log-std (orthogonal init of the
  MLPs and heads as SB3; the LSTMs keep torch's default init, as sb3-contrib);
* the LSTM states are zeroed where an episode starts, before that step
  (sb3-contrib ``_process_sequence``), in collection and in training alike;
* the timeout bootstrap evaluates the terminal observation with the critic
  state after the step, episode start 0; the last value with the episode
  starts of the next step (``RecurrentPPO.collect_rollouts``);
* training re-runs the LSTMs over sequences from the states stored at their
  first step.  sb3-contrib cuts an env's rollout into sequences at episode
  starts and pads them; here every env's rollout is cut into fixed
  ``seq_len``-step sequences (the state stored every ``seq_len`` steps) and
  episode starts inside a sequence zero the state there.  Both compute the
  same forward pass per step; minibatches are ``batch_size // seq_len``
  sequences (no padding rows).

Collection is lock-step (``salp_step`` per env-step: the LSTM policy is not
evaluated inside the simulation kernel; ``salp_collect`` runs the MLP
policy), with the same divergence guard, episode statistics and HIP-event
phase timings as :class:`~grasp_lab_salp_amd.ppo.PPO`.
"""
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
from ._abi import INFO_DIM
from .ppo import PPO, SplitKLinear, _NoEnv, _ortho, allreduce_gradients, ppo_loss

__all__ = ["RecurrentActorCritic", "RecurrentPPO", "FusedPolicyStep", "lstm_cell"]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


class _LSTMCellFn(torch.autograd.Function):
    """The elementwise part of an LSTM step through the HIP kernels of
    salp_lstm_cell_forward / _backward (include/salp.h): one kernel each way
    instead of ~8 / ~12 torch kernels."""

    @staticmethod
    def forward(ctx, gates, c_prev, keep):
        m, h4 = gates.shape
        H = h4 // 4
        h = torch.empty((m, H), dtype=gates.dtype, device=gates.device)
        c = torch.empty_like(h)
        act = torch.empty_like(gates)
        st = ctypes.c_void_p(torch.cuda.current_stream(gates.device).cuda_stream)
        _lib.check(_lib.load().salp_lstm_cell_forward(m, H, _ptr(gates), _ptr(c_prev), _ptr(keep), _ptr(h), _ptr(c),
                                                      _ptr(act), st))
        ctx.save_for_backward(act, c_prev, keep, c)
        return h, c

    @staticmethod
    def backward(ctx, dh, dc):
        act, c_prev, keep, c = ctx.saved_tensors
        m, H = c.shape
        dh = torch.zeros_like(c) if dh is None else dh.contiguous()
        dc = None if dc is None else dc.contiguous()
        dg = torch.empty_like(act)
        dcp = torch.empty_like(c_prev)
        st = ctypes.c_void_p(torch.cuda.current_stream(c.device).cuda_stream)
        _lib.check(_lib.load().salp_lstm_cell_backward(m, H, _ptr(act), _ptr(c_prev), _ptr(keep), _ptr(c), _ptr(dh),
                                                       _ptr(dc), _ptr(dg), _ptr(dcp), st))
        return dg, dcp, None


class _SharedInputProjFn(torch.autograd.Function):
    """y[t, k] = x[t] @ w[k]: the input projection of every step t of the
    networks k, which share the input x [T, 1, n, K] (observations: no
    gradient); w [1, nets, K, N].  The weight gradient sum_t x_t^T dy[t, k] has
    K = 11 rows and T n = 32 768 reduction steps per minibatch: as one GEMM per
    network the library runs it on a handful of workgroups (~140 us); here the
    steps are the batch of one batched GEMM and the T products are summed
    (same math, another summation order)."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x)
        return torch.matmul(x, w)

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return None, torch.matmul(x.transpose(-1, -2), gy).sum(0, keepdim=True)


class _LSTMPairSeqFn(torch.autograd.Function):
    """Both LSTMs (actor, critic) over a whole sequence, with the backward pass
    through time written out instead of recorded step by step (CUDA float32).

    Inputs: gx [T, 2, n, 4H] (input projection + bias), w_hh [2, H, 4H],
    h0 / c0 [2, n, H], keep [T, n] and keep2 [T, 2n] (1 - episode start).
    Outputs: h of every step [T, 2, n, H] and the last c [2, n, H].
    Per step forward: G = hk W_hh (one batched GEMM for both networks), then
    the cell kernel (salp_lstm_step_forward), which adds gx and writes the
    next step's hk = h keep; backward: the cell kernel (salp_lstm_step_backward,
    dh = d_out + d hk_next keep_next), then d hk = dG W_hh^T (one batched
    GEMM).  The recurrent weight gradient
    sum_t hk_t^T dG_t is one batched GEMM over all steps at the end, and dG
    of every step is written straight into the input projection's gradient,
    where step-by-step autograd ran 16 weight-gradient GEMMs and the
    accumulations between them."""

    @staticmethod
    def forward(ctx, gx, w_hh, h0, c0, keep, keep2):
        T, _, n, H4 = gx.shape
        H = H4 // 4
        out = gx.new_empty(T, 2, n, H)
        hk = gx.new_empty(T, 2, n, H)
        act = gx.new_empty(T, 2, n, H4)
        cs = gx.new_empty(T + 1, 2, n, H)
        cs[0].copy_(c0)
        g = gx.new_empty(2, n, H4)
        lib = _lib.load()
        st = ctypes.c_void_p(torch.cuda.current_stream(gx.device).cuda_stream)
        torch.mul(h0, keep[0].view(1, n, 1), out=hk[0])
        for t in range(T):
            torch.bmm(hk[t], w_hh, out=g)
            nxt = t + 1 < T
            _lib.check(lib.salp_lstm_step_forward(2 * n, H, _ptr(g), _ptr(gx[t]), _ptr(cs[t]), _ptr(keep2[t]),
                                                  _ptr(keep2[t + 1] if nxt else None), _ptr(out[t]),
                                                  _ptr(cs[t + 1]), _ptr(act[t]), _ptr(hk[t + 1] if nxt else None), st))
        ctx.save_for_backward(w_hh, hk, act, cs, keep, keep2)
        return out, cs[T]

    @staticmethod
    def backward(ctx, d_out, d_cT):
        w_hh, hk, act, cs, keep, keep2 = ctx.saved_tensors
        T, _, n, H = hk.shape
        lib = _lib.load()
        st = ctypes.c_void_p(torch.cuda.current_stream(hk.device).cuda_stream)
        dG = torch.empty_like(act)
        d_out = torch.zeros_like(hk) if d_out is None else d_out.contiguous()
        dc = None if d_cT is None else d_cT.contiguous()
        dhk = None                         # d hk[t + 1]
        w_t = w_hh.transpose(1, 2).contiguous()
        for t in range(T - 1, -1, -1):
            dcp = torch.empty_like(d_out[t])
            _lib.check(lib.salp_lstm_step_backward(2 * n, H, _ptr(act[t]), _ptr(cs[t]), _ptr(keep2[t]),
                                                   _ptr(cs[t + 1]), _ptr(d_out[t]), _ptr(dhk),
                                                   _ptr(keep2[t + 1] if dhk is not None else None), _ptr(dc),
                                                   _ptr(dG[t]), _ptr(dcp), st))
            dhk = torch.bmm(dG[t], w_t)
            dc = dcp
        d_w = torch.matmul(hk.transpose(-1, -2), dG).sum(0)
        return dG, d_w, dhk * keep[0].view(1, n, 1), dc, None, None


def lstm_cell(gates, c_prev, keep):
    """(h, c) of one LSTM step from the gate pre-activations [m, 4H] (i, f, g,
    o), the previous cell state [m, H] and keep [m] (the state is zeroed where
    keep is 0).  CUDA float32: the HIP kernels (fails if libsalp.so is
    missing); CPU: the same equations in torch ops (the tests' path)."""
    if gates.is_cuda:
        return _LSTMCellFn.apply(gates.contiguous(), c_prev.contiguous(), keep.contiguous())
    i, f, g, o = gates.chunk(4, 1)
    c = torch.sigmoid(f) * (c_prev * keep.unsqueeze(1)) + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


class RecurrentActorCritic(nn.Module):
    """sb3-contrib ``RecurrentActorCriticPolicy`` (MlpLstmPolicy) with separate
    actor and critic LSTMs.  A recurrent state is one [4, n, H] tensor:
    (h, c) of the actor LSTM, then (h, c) of the critic LSTM."""

    def __init__(self, obs_dim, act_dim, lstm_hidden_size=256, net_arch=(64, 64)):
        super().__init__()
        self.hidden = int(lstm_hidden_size)
        self.lstm_actor = nn.LSTM(obs_dim, self.hidden)
        self.lstm_critic = nn.LSTM(obs_dim, self.hidden)

        def mlp():
            layers, d = [], self.hidden
            for h in net_arch:
                layers += [_ortho(SplitKLinear(d, h), math.sqrt(2)), nn.Tanh()]
                d = h
            return nn.Sequential(*layers), d

        self.pi_net, d_pi = mlp()
        self.vf_net, d_vf = mlp()
        self.action_net = _ortho(SplitKLinear(d_pi, act_dim), 0.01)
        self.value_net = _ortho(SplitKLinear(d_vf, 1), 1.0)
        self.log_std = nn.Parameter(torch.zeros(act_dim))

    def initial_state(self, n, device=None):
        return torch.zeros(4, n, self.hidden, device=device)

    @staticmethod
    def _run(lstm, x, h, c, starts):
        """x [T, n, D] through `lstm` (torch's LSTM equations and parameter
        layout, gates i, f, g, o) from (h, c) [n, H]; the state is zeroed where
        starts[t] (an episode starts at step t), before step t.  The input
        projection of all T steps is one GEMM; each step is one GEMM plus the
        fused cell (lstm_cell: one HIP kernel each way), all capturable in a
        HIP graph (a fused RNN library call cannot reset states inside a
        sequence).
        Returns (outputs [T, n, H], h, c)."""
        T, n, D = x.shape
        # unbind, not gx[t]: the backward of T separate selects would zero-fill
        # and add T full-size [T, n, 4H] gradients; unbind's is one stack
        gx = torch.addmm(lstm.bias_ih_l0 + lstm.bias_hh_l0, x.reshape(T * n, D),
                         lstm.weight_ih_l0.t()).view(T, n, -1).unbind(0)
        w_hh = lstm.weight_hh_l0.t()
        keeps = (1.0 - starts).unbind(0)
        outs = []
        for t in range(T):
            keep = keeps[t]
            h, c = lstm_cell(torch.addmm(gx[t], h * keep.unsqueeze(1), w_hh), c, keep)
            outs.append(h)
        return torch.stack(outs), h, c

    def _run_pair(self, x, state, starts):
        """_run of the actor and the critic LSTM together (same input, same
        episode starts): every GEMM batched over the two networks (bmm), one
        cell launch per step for both.  state [4, n, H].
        Returns (actor outputs, critic outputs [T, n, H], new state)."""
        T, n, D = x.shape
        la, lc = self.lstm_actor, self.lstm_critic
        w_hh = torch.stack([la.weight_hh_l0, lc.weight_hh_l0]).transpose(1, 2)        # [2, H, 4H]
        # input projection of all T steps, the bias folded in as a ones column
        wb = torch.stack([torch.cat([la.weight_ih_l0.t(), (la.bias_ih_l0 + la.bias_hh_l0).unsqueeze(0)]),
                          torch.cat([lc.weight_ih_l0.t(), (lc.bias_ih_l0 + lc.bias_hh_l0).unsqueeze(0)])])
        xa = torch.cat([x, x.new_ones(T, n, 1)], 2).unsqueeze(1)                       # [T, 1, n, D + 1]
        if torch.is_grad_enabled():
            gx = _SharedInputProjFn.apply(xa, wb.unsqueeze(0))
        else:
            gx = torch.matmul(xa, wb.unsqueeze(0))                                     # [T, 2, n, 4H]
        keep1 = (1.0 - starts)                                                        # [T, n]
        keep2 = keep1.repeat(1, 2)                                                    # [T, 2n]: both nets
        if x.is_cuda:
            out, c = _LSTMPairSeqFn.apply(gx, w_hh, state[0::2].contiguous(), state[1::2].contiguous(), keep1,
                                          keep2)
            h = out[T - 1]
            oa, oc = out.unbind(1)
            return oa, oc, torch.stack([h[0], c[0], h[1], c[1]])
        gx = gx.unbind(0)
        keeps = keep1.unbind(0)
        keeps2 = keep2.unbind(0)
        h, c = state[0::2], state[1::2].reshape(2 * n, -1)                            # [2, n, H], [2n, H]
        outs = []
        for t in range(T):
            g = torch.baddbmm(gx[t], h * keeps[t].view(1, n, 1), w_hh)
            hf, c = lstm_cell(g.view(2 * n, -1), c, keeps2[t])
            h = hf.view(2, n, -1)
            outs.append(h)
        out = torch.stack(outs, 1)                                                    # [2, T, n, H]
        c = c.view(2, n, -1)
        return out[0], out[1], torch.stack([h[0], c[0], h[1], c[1]])

    def forward_seq(self, obs, state, starts, critic=True):
        """Latents of a sequence: obs [T, n, D], state [4, n, H], starts [T, n].
        Returns (actor latent [T, n, H], critic latent or None, new state)."""
        if critic:
            return self._run_pair(obs, state, starts)
        lp, hp, cp = self._run(self.lstm_actor, obs, state[0], state[1], starts)
        return lp, None, torch.stack([hp, cp, state[2], state[3]])

    def _dist(self, latent_pi):
        # the heads on [rows, H] (SplitKLinear's split-K weight gradient)
        mean = self.action_net(self.pi_net(latent_pi.reshape(-1, latent_pi.shape[-1])))
        mean = mean.view(*latent_pi.shape[:-1], -1)
        return torch.distributions.Normal(mean, self.log_std.exp().expand_as(mean), validate_args=False)

    def _value(self, latent_vf):
        v = self.value_net(self.vf_net(latent_vf.reshape(-1, latent_vf.shape[-1])))
        return v.view(latent_vf.shape[:-1])

    @torch.no_grad()
    def act(self, obs, state, episode_starts, generator=None):
        """One step for every env: obs [n, D] -> (action, value, log_prob,
        new state); the Gaussian noise from `generator` when given."""
        lp, lv, new = self.forward_seq(obs.unsqueeze(0), state, episode_starts.unsqueeze(0))
        d = self._dist(lp[0])
        if generator is None:
            a = d.sample()
        else:
            a = d.mean + d.stddev * torch.randn(d.mean.shape, generator=generator, device=d.mean.device,
                                                dtype=d.mean.dtype)
        return a, self._value(lv[0]), d.log_prob(a).sum(-1), new

    @torch.no_grad()
    def predict_values(self, obs, state, episode_starts):
        """V(obs) with the critic LSTM from `state` (not advanced)."""
        lv, _, _ = self._run(self.lstm_critic, obs.unsqueeze(0), state[2], state[3], episode_starts.unsqueeze(0))
        return self._value(lv[0])

    def evaluate(self, obs, actions, state, starts):
        """Training pass over sequences: obs [T, n, D], actions [T, n, A],
        state [4, n, H] at the sequences' first step, starts [T, n].
        Returns (value, log_prob, entropy), each [T, n]."""
        lp, lv, _ = self.forward_seq(obs, state, starts)
        d = self._dist(lp)
        return self._value(lv), d.log_prob(actions).sum(-1), d.entropy().sum(-1)


def _check_fused_step(policy, device):
    """``fused_step=True`` needs a GPU and the sizes salp_lstm_policy_step is built for."""
    if torch.device(device).type != "cuda":
        raise ValueError("fused_step=True runs HIP kernels: it needs a ROCm GPU device")
    if policy.hidden != _lib.LSTM_POLICY_HIDDEN:
        raise ValueError(f"fused_step=True is built for lstm_hidden_size {_lib.LSTM_POLICY_HIDDEN}, not {policy.hidden}")
    arch = tuple(m.out_features for m in policy.pi_net if isinstance(m, nn.Linear))
    if arch != (_lib.LSTM_POLICY_MLP, _lib.LSTM_POLICY_MLP):
        raise ValueError(f"fused_step=True is built for net_arch (64, 64), not {arch}")
    if policy.lstm_actor.input_size > _lib.LSTM_POLICY_OBS_MAX:
        raise ValueError(f"fused_step=True: obs_dim <= {_lib.LSTM_POLICY_OBS_MAX}")


class FusedPolicyStep:
    """``salp_lstm_policy_step`` (include/salp.h) on a :class:`RecurrentActorCritic`'s
    own parameters for a fixed number of rows: the argument block holds the
    parameters' raw pointers (they are updated and loaded in place), and the
    outputs are allocated once.  ``value`` receives the two-network step's
    value, ``value_only`` the critic-only calls', so the timeout bootstrap
    leaves the step's value alone."""

    def __init__(self, policy, rows, device):
        _check_fused_step(policy, device)
        self.policy, self.rows, self.device = policy, int(rows), torch.device(device)
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)  # noqa: E731
        self.action, self.log_prob, self.value = z(self.rows, 3), z(self.rows), z(self.rows)
        self.value_only = z(self.rows)
        self.latent = z(2, self.rows, policy.hidden)
        self.obs_dim = policy.lstm_actor.input_size

    def _net(self, lstm, mlp, head):
        ts = (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, mlp[0].weight, mlp[0].bias,
              mlp[2].weight, mlp[2].bias, head.weight, head.bias)
        for t in ts:
            if not (t.is_contiguous() and t.dtype == torch.float32 and t.device == self.device):
                raise ValueError("fused_step: the policy's tensors must be contiguous float32 on the learner's device")
        return _lib.SalpLstmPolicyNet(*(t.data_ptr() for t in ts))

    def _check(self, name, t, shape):
        if t is None:
            return None
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
            raise ValueError(f"fused_step: {name} must be a contiguous float32 tensor of shape {shape} on {self.device}")
        return t.data_ptr()

    def __call__(self, obs, keep, state_in, state_out=None, eps=None, actor=True, critic=True):
        """One step.  ``keep`` None: all 1; ``state_out`` None: the state is
        not advanced; ``eps`` None: the action is the mean.  Returns (action,
        log_prob, value): this object's buffers (None for an absent network)."""
        pol, n, H = self.policy, self.rows, self.policy.hidden
        value = self.value if actor else self.value_only
        s = _lib.SalpLstmPolicyStep(
            rows=n, obs_dim=self.obs_dim, act_dim=3, obs=self._check("obs", obs, (n, self.obs_dim)),
            keep=self._check("keep", keep, (n,)), state_in=self._check("state_in", state_in, (4, n, H)),
            state_out=self._check("state_out", state_out, (4, n, H)), latent=self.latent.data_ptr(),
            log_std=pol.log_std.data_ptr() if actor else None, eps=self._check("eps", eps, (n, 3)),
            action=self.action.data_ptr() if actor else None, log_prob=self.log_prob.data_ptr() if actor else None,
            value=value.data_ptr() if critic else None)
        if actor:
            s.actor = self._net(pol.lstm_actor, pol.pi_net, pol.action_net)
        if critic:
            s.critic = self._net(pol.lstm_critic, pol.vf_net, pol.value_net)
        st = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.load().salp_lstm_policy_step(ctypes.byref(s), st))
        return (self.action if actor else None, self.log_prob if actor else None, value if critic else None)


class RecurrentPPO(PPO):
    """sb3-contrib ``RecurrentPPO`` on a :class:`~grasp_lab_salp_amd.vec_env.SalpVecEnv`
    (see the module docstring for the semantics).  ``batch_size`` counts
    env-steps and must be a multiple of ``seq_len``.

    ``fused_step`` (default off; needs a GPU, ``lstm_hidden_size=256`` and
    ``net_arch=(64, 64)``): every policy step of the collection, of
    :meth:`evaluate` and of :meth:`predict` is one ``salp_lstm_policy_step``
    call (two launches) instead of the torch ops' 57.  It pays where the step
    is launch-bound: at the reference's 4 envs the collection took a third
    less time; at 32 768 envs it was 14 % SLOWER than the library GEMMs
    (measured on one MI355X), so it is off unless asked for."""

    def __init__(self, policy, env, learning_rate=3e-4, n_steps=2048, batch_size=64, n_epochs=10, gamma=0.99,
                 gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                 normalize_advantage=True, seed=0, device=None, verbose=0, reset_nonfinite=True,
                 policy_kwargs=None, seq_len=16, use_graphs=None, fused_step=False, tensorboard_log=None,
                 episode_log=0):
        if episode_log:
            raise ValueError("RecurrentPPO collects in lock-step (callbacks see every env-step's tensors): "
                             "episode_log must be 0")
        sim = getattr(env, "sim", env)
        if device == "auto":    # sb3's default: here the simulator's device
            device = None
        self.tensorboard_log = tensorboard_log   # accepted and unused: `history` holds the rows a logger would get
        kw = dict(policy_kwargs or {})
        for k, want in (("n_lstm_layers", 1), ("enable_critic_lstm", True), ("shared_lstm", False)):
            if kw.pop(k, want) != want:
                raise ValueError(f"policy_kwargs {k}={want} is the supported configuration")
        if policy == "MlpLstmPolicy":
            torch.manual_seed(int(seed))
            policy = RecurrentActorCritic(sim.obs_dim, 3, lstm_hidden_size=kw.pop("lstm_hidden_size", 256),
                                          net_arch=tuple(kw.pop("net_arch", (64, 64))))
        elif not isinstance(policy, RecurrentActorCritic):
            raise ValueError("policy must be 'MlpLstmPolicy' or a RecurrentActorCritic")
        if kw:
            raise ValueError(f"unsupported policy_kwargs: {sorted(kw)}")
        if n_steps % seq_len or batch_size % seq_len:
            raise ValueError("n_steps and batch_size must be multiples of seq_len")
        if fused_step:
            _check_fused_step(policy, sim.device if device is None else device)
        super().__init__(policy, env, learning_rate=learning_rate, n_steps=n_steps, batch_size=batch_size,
                         n_epochs=n_epochs, gamma=gamma, gae_lambda=gae_lambda, clip_range=clip_range,
                         ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm,
                         normalize_advantage=normalize_advantage, seed=seed, device=device, verbose=verbose,
                         reset_nonfinite=reset_nonfinite, use_graphs=use_graphs, fused_loss=False,
                         collect="lockstep", fused_update=False)
        self.seq_len = int(seq_len)
        self.n_seq = self.n_steps // self.seq_len
        self._lstm_state = self.policy.initial_state(self.n_envs, self.device)
        # recurrent state at the first step of every sequence [n_seq, 4, n, H]
        self.seq_states = torch.zeros(self.n_seq, 4, self.n_envs, self.policy.hidden, device=self.device)
        self.learning_rate, self.seed = float(learning_rate), int(seed)
        self.fused = self.device.type == "cuda"   # the metrics / evaluation bookkeeping kernels (callbacks.py)
        self.fused_step = bool(fused_step)
        self._steps = {}                # FusedPolicyStep per row count
        self._state_bufs = None         # the collection's two state buffers, used in turn
        self.last_eval = None           # the per-episode results of the last evaluate()
        self.predict_only = False       # RecurrentPPO.load(path, env=None): no env to learn on

    def _need_env(self, what):
        if self.predict_only:
            raise RuntimeError(f"{what}: this model was loaded without an env (RecurrentPPO.load(path, env=None)): "
                               "it can only predict; load it with env=... to train or evaluate")

    def _fused(self, rows):
        if rows not in self._steps:
            self._steps[rows] = FusedPolicyStep(self.policy, rows, self.device)
        return self._steps[rows]

    # -------------------------------------------- collection hooks (PPO)
    def _act(self, t, obs):
        if t % self.seq_len == 0:
            self.seq_states[t // self.seq_len].copy_(self._lstm_state)
        if self.fused_step:
            # the kernel spreads a row's units over workgroups: it never steps in place
            if self._state_bufs is None:
                self._state_bufs = [self._lstm_state, torch.empty_like(self._lstm_state)]
            bufs = self._state_bufs
            new = bufs[1] if self._lstm_state.data_ptr() == bufs[0].data_ptr() else bufs[0]
            eps = torch.randn((self.n_envs, 3), generator=self.sample_gen, device=self.device, dtype=torch.float32)
            a, lp, v = self._fused(self.n_envs)(obs.contiguous(), 1.0 - self._episode_starts,
                                                self._lstm_state.contiguous(), new, eps)
            self._lstm_state = new
            return a, v, lp
        a, v, lp, self._lstm_state = self.policy.act(obs, self._lstm_state, self._episode_starts,
                                                     generator=self.sample_gen)
        return a, v, lp

    def _terminal_value(self, terminal_obs):
        # the critic state after the step, no reset (the episode ended at it)
        if self.fused_step:
            return self._fused(self.n_envs)(terminal_obs.contiguous(), None, self._lstm_state, actor=False)[2]
        return self.policy.predict_values(terminal_obs, self._lstm_state, torch.zeros_like(self._episode_starts))

    def _last_values(self):
        # (a guard reset ends an episode too: the next step's episode start
        # zeroes that env's state, as for any other episode end)
        if self.fused_step:
            return self._fused(self.n_envs)(self._obs.contiguous(), 1.0 - self._episode_starts, self._lstm_state,
                                            actor=False)[2]
        return self.policy.predict_values(self._obs, self._lstm_state, self._episode_starts)

    # ------------------------------------------------ learn with callbacks
    def learn(self, total_timesteps, callback=None, tb_log_name=None, progress_bar=False, log_interval=1):
        """:meth:`PPO.learn` with sb3-contrib's call shape.  ``callback``: a
        callback of :mod:`grasp_lab_salp_amd.callbacks`, a list of them, or
        None; ``on_training_start`` runs once, ``on_step`` after every
        lock-step env-step, on the collection stream (the update waits for it:
        ``evaluate`` and ``save`` see one consistent policy), and
        ``on_training_end`` at the end.  ``self.locals`` then holds the step's
        device tensors under SAC's names: ``obs`` (after the step),
        ``actions`` (unclipped, as stored), ``rewards``, ``terminated`` and
        ``truncated`` (u8, as the task set them, before the divergence guard
        marks its envs), ``dones``, ``info`` [n, INFO_DIM] and ``diverged``
        (u8: the guard's envs).  ``num_timesteps`` advances by ``n_envs`` per
        env-step.  An ``on_step`` that returns False ends training after that
        env-step, before the update.  ``tb_log_name`` and ``progress_bar`` are
        accepted for sb3's signature and unused."""
        self._need_env("learn")
        cb = self._as_callback(callback)
        if cb is None:
            return self._learn(total_timesteps, log_interval)
        cb.on_training_start({"self": self, "total_timesteps": total_timesteps}, globals())
        self._learn(total_timesteps, log_interval, on_env_step=cb.on_step)
        cb.on_training_end()
        return self

    # ----------------------------------------------- predict and evaluate
    @torch.no_grad()
    def _eval_action(self, obs, state, starts, deterministic=True):
        """(unclipped action [n, 3], new state [4, n, H]) of the actor on
        ``obs`` [n, obs_dim] from ``state`` with episode starts ``starts`` [n]:
        the one action function of :meth:`evaluate` and :meth:`predict`.  The
        critic's half of the state is carried over as it is.  Noise comes from
        ``sample_gen`` only when not deterministic."""
        n = obs.shape[0]
        eps = None if deterministic else torch.randn((n, 3), generator=self.sample_gen, device=self.device,
                                                     dtype=torch.float32)
        if self.fused_step:
            new = state.clone()
            a, _, _ = self._fused(n)(obs.contiguous(), (1.0 - starts).contiguous(), state.contiguous(), new, eps,
                                     critic=False)
            return a.clone(), new
        lat, _, new = self.policy.forward_seq(obs.unsqueeze(0), state, starts.unsqueeze(0), critic=False)
        d = self.policy._dist(lat[0])
        return (d.mean if eps is None else d.mean + d.stddev * eps), new

    @torch.no_grad()
    def predict(self, observation, state=None, episode_start=None, deterministic=True):
        """sb3-contrib ``predict``: (action clipped to the env's Box, state).
        A NumPy observation gives a NumPy action; one observation gives one
        action.  ``state``: this package's [4, n, H] tensor as returned by the
        previous call (None: zeros); ``episode_start`` [n] (None: no reset).
        The caller hands the returned state back on the next call (a viewer
        that discards it gets the policy's answer from a fresh state)."""
        as_numpy = not torch.is_tensor(observation)
        obs = torch.as_tensor(observation, dtype=torch.float32, device=self.device)
        single = obs.dim() == 1
        obs = obs.reshape(-1, self.obs_dim)
        n = obs.shape[0]
        if state is None:
            state = self.policy.initial_state(n, self.device)
        else:
            state = torch.as_tensor(state, dtype=torch.float32, device=self.device).reshape(4, n, self.policy.hidden)
        if episode_start is None:
            starts = torch.zeros(n, dtype=torch.float32, device=self.device)
        else:
            starts = torch.as_tensor(episode_start, device=self.device).to(torch.float32).reshape(n)
        a, new = self._eval_action(obs, state, starts, deterministic)
        a = torch.clamp(a, self.low, self.high)
        a = a[0] if single else a
        return (a.cpu().numpy() if as_numpy else a), new

    @torch.no_grad()
    def evaluate(self, env, n_eval_episodes=10, deterministic=True, return_episode_rewards=False, poll_every=8):
        """:meth:`SAC.evaluate <grasp_lab_salp_amd.sac.SAC.evaluate>` with a
        recurrent state: ``env`` is reset and stepped in lock-step on
        :meth:`_eval_action`'s actions, one LSTM state per evaluation env,
        zeroed where the previous step ended an episode (the episode starts
        begin as all ones, as the collection's).  One ``EvalAccount.push`` per
        step; ``last_eval`` keeps returns, lengths and successes.  Neither the
        training env, nor ``_lstm_state``, nor ``sample_gen`` (when
        deterministic) is touched."""
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
        state = self.policy.initial_state(n, dev)
        starts = torch.ones(n, dtype=torch.float32, device=dev)
        left = acc.n_eval_episodes
        max_steps = acc.max_target * int(sim.params.max_cycles)
        poll_every = max(int(poll_every), 1)
        for t in range(1, max_steps + 1):
            a, state = self._eval_action(obs, state, starts, deterministic)
            r = sim.step(torch.clamp(a, self.low, self.high), auto_reset=True, out=out)
            acc.push(r.info, r.terminated, r.truncated)
            starts = (r.terminated | r.truncated).to(torch.float32)
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
    FORMAT, FORMAT_VERSION = "grasp_lab_salp_amd.RecurrentPPO", 1
    _HYPERPARAMETERS = ("learning_rate", "n_steps", "batch_size", "n_epochs", "gamma", "gae_lambda", "clip_range",
                        "ent_coef", "vf_coef", "max_grad_norm", "normalize_advantage", "reset_nonfinite", "seq_len")

    def save(self, path):
        """Everything a resumed run needs, as a zip of this project's own
        layout (``.zip`` is appended to a ``path`` without a suffix; stored,
        not deflated; sb3-contrib cannot read it): ``data.json`` (format tag
        and version, hyperparameters with ``seq_len``, ``lstm_hidden_size``
        and ``net_arch``, ``num_timesteps``, ``seed``, ``obs_dim``,
        ``fused_step``, ``device_type``), ``policy.pth``,
        ``policy.optimizer.pth`` and ``rng.pth`` (the states of ``sample_gen``
        and of the permutation generator ``gen``).  A ``clip_range`` schedule
        is saved as its current value.  Returns the file's path; synchronises."""
        path = self._zip_path(path)
        cpu = lambda t: t.detach().to("cpu", copy=True)  # noqa: E731
        sd = self.opt.state_dict()
        opt = {"state": {k: {n: (cpu(v) if torch.is_tensor(v) else v) for n, v in st.items()}
                         for k, st in sd["state"].items()}, "param_groups": sd["param_groups"]}
        hp = {k: getattr(self, k) for k in self._HYPERPARAMETERS}
        hp["clip_range"] = self._clip()
        hp["lstm_hidden_size"] = self.policy.hidden
        hp["net_arch"] = [m.out_features for m in self.policy.pi_net if isinstance(m, nn.Linear)]
        data = {"format": self.FORMAT, "version": self.FORMAT_VERSION, "hyperparameters": hp,
                "num_timesteps": int(self.num_timesteps), "seed": self.seed, "obs_dim": self.obs_dim,
                "fused_step": self.fused_step, "device_type": self.device.type}
        files = {"policy.pth": {k: cpu(v) for k, v in self.policy.state_dict().items()},
                 "policy.optimizer.pth": opt,
                 "rng.pth": {"sample_gen": self.sample_gen.get_state().clone(), "gen": self.gen.get_state().clone()}}
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
        ``kwargs`` override the saved hyperparameters.  Tensors are read with
        ``torch.load(weights_only=True)``; the parameters are copied into the
        new learner's own tensors, in place (kept graphs and the kernels' raw
        pointers stay valid), and the optimiser keeps this learner's own
        ``param_groups``.  ``fused_step`` is turned off where there is no GPU.
        ``env=None`` gives a predict-only model on ``device`` (``"cpu"`` too;
        ``"auto"``: the GPU if there is one): ``predict`` works; ``learn`` and
        ``evaluate`` raise RuntimeError.  A file of another format or version
        raises ValueError."""
        path = cls._zip_path(path)
        with zipfile.ZipFile(path) as z:
            data = json.loads(z.read("data.json"))
            if data.get("format") != cls.FORMAT or data.get("version") != cls.FORMAT_VERSION:
                raise ValueError(f"{path}: not a {cls.FORMAT} file of version {cls.FORMAT_VERSION} "
                                 f"(format {data.get('format')!r}, version {data.get('version')!r})")
            blobs = {n: torch.load(io.BytesIO(z.read(n)), map_location="cpu", weights_only=True)
                     for n in ("policy.pth", "policy.optimizer.pth", "rng.pth")}
        hp = dict(data["hyperparameters"])
        predict_only = env is None
        if predict_only:
            if device in (None, "auto"):
                device = "cuda" if torch.cuda.is_available() else "cpu"
            env = _NoEnv(data["obs_dim"], device)
            device = None
        dev_type = torch.device(getattr(env, "sim", env).device).type
        hp["fused_step"] = bool(data["fused_step"]) and dev_type == "cuda"   # the HIP kernels need a GPU
        hp["seed"] = data["seed"]
        hp["policy_kwargs"] = {"lstm_hidden_size": hp.pop("lstm_hidden_size"), "net_arch": hp.pop("net_arch")}
        hp.update(kwargs)
        m = cls("MlpLstmPolicy", env, device=device, **hp)
        if m.obs_dim != data["obs_dim"]:
            raise ValueError(f"{path}: saved with obs_dim {data['obs_dim']}, the env has {m.obs_dim}")
        m.predict_only = predict_only
        if predict_only:
            m.env = None
        m.policy.load_state_dict(blobs["policy.pth"], strict=True)      # copy_ into the parameters: in place
        if blobs["policy.optimizer.pth"]["state"]:
            groups = m.opt.state_dict()["param_groups"]   # this learner's own settings (lr may be overridden)
            m.opt.load_state_dict({"state": blobs["policy.optimizer.pth"]["state"], "param_groups": groups})
        m.num_timesteps = int(data["num_timesteps"])
        if data.get("device_type") == m.device.type:         # a generator's state is its device type's own
            m.sample_gen.set_state(blobs["rng.pth"]["sample_gen"])
            m.gen.set_state(blobs["rng.pth"]["gen"])
        return m

    # ------------------------------------------------------------ update
    def _seq_minibatch(self, ids, acc):
        """One PPO gradient step on sequences `ids` (sequence k of env e is
        id k * n_envs + e)."""
        b, pol = self.buf, self.policy
        n, T = self.n_envs, self.seq_len
        k, e = ids // n, ids % n
        t = k.unsqueeze(0) * T + torch.arange(T, device=self.device).unsqueeze(1)   # [T, m]
        ee = e.unsqueeze(0).expand_as(t)
        obs, act = b.obs[t, ee], b.actions[t, ee]
        old_lp, adv, ret, starts = b.log_probs[t, ee], b.advantages[t, ee], b.returns[t, ee], b.episode_starts[t, ee]
        state = self.seq_states[k, :, e].transpose(0, 1)                             # [4, m, H]
        old_lp, adv, ret = (x.reshape(-1) for x in (old_lp, adv, ret))
        norm = self.normalize_advantage and adv.numel() > 1
        cr = self._clip()
        if obs.is_cuda:
            # the loss head as the fused HIP kernels of salp_ppo_loss (the MLP
            # PPO's, ppo.ppo_loss): one launch each way instead of ~25
            lat_pi, lat_vf, _ = pol.forward_seq(obs, state, starts)
            mean = pol.action_net(pol.pi_net(lat_pi.reshape(-1, lat_pi.shape[-1])))
            value = pol.value_net(pol.vf_net(lat_vf.reshape(-1, lat_vf.shape[-1]))).reshape(-1)
            loss, stats = ppo_loss(mean, pol.log_std, value, act.reshape(-1, act.shape[-1]), old_lp, adv, ret, cr,
                                   self.ent_coef, self.vf_coef, norm)
        else:
            v, lp, ent = pol.evaluate(obs, act, state, starts)
            v, lp, ent = (x.reshape(-1) for x in (v, lp, ent))
            if norm:
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            ratio = torch.exp(lp - old_lp)
            pg = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - cr, 1 + cr)).mean()
            vf = torch.nn.functional.mse_loss(ret, v)
            ent_loss = -ent.mean()
            loss = pg + self.ent_coef * ent_loss + self.vf_coef * vf
            clip = ((ratio - 1).abs() > cr).float().mean()
            stats = torch.stack([pg.detach(), vf.detach(), -ent_loss.detach(), clip.detach()])
        self.opt.zero_grad(set_to_none=False)
        loss.backward()
        allreduce_gradients(list(pol.parameters()))
        nn.utils.clip_grad_norm_(pol.parameters(), self.max_grad_norm)
        self.opt.step()
        acc += stats

    def _minibatch(self, idx, acc):
        # PPO._graphed_minibatch captures / replays this with `idx` = sequence ids
        self._seq_minibatch(idx, acc)

    def train(self):
        """n_epochs passes over the rollout's sequences in random minibatches of
        batch_size // seq_len sequences.  On one GPU the minibatch step (the
        BPTT over seq_len steps: ~1 000 small kernels) runs as a HIP graph
        captured in the first update and kept (PPO._graphed_minibatch; the
        collection runs on its own stream, PPO.learn); a ragged last
        minibatch runs eagerly."""
        total = self.n_seq * self.n_envs
        per = self.batch_size // self.seq_len
        if total % per:
            self._graph, self._graph_warm = None, 0
        acc = torch.zeros(4, device=self.device)
        steps = 0
        for _ in range(self.n_epochs):
            perm = torch.randperm(total, generator=self.gen, device=self.device)
            for s in range(0, total, per):
                ids = perm[s:s + per]
                if self.use_graphs and ids.numel() == per:
                    self._graphed_minibatch(ids)
                else:
                    self._seq_minibatch(ids, acc)
                steps += 1
        if self.use_graphs and self._graph_warm > 0:
            acc = acc + self._g_acc
            self._g_acc.zero_()
        vals = (acc / max(steps, 1)).tolist()
        return dict(zip(("pg_loss", "vf_loss", "entropy", "clip_frac"), vals))
