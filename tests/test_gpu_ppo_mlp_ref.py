"""The fused PPO minibatch step (csrc/salp_ppo_mlp.hip: salp_ppo_mlp_grads,
salp_ppo_mlp_adv_partials, salp_ppo_mlp_apply) against float64 references, at
the shapes the product runs and the ones around them.

The row kernel gives a block more than one 64-row tile only above 16 384 rows
(256 blocks at most), which tests/test_gpu_ppo_mlp.py never reaches with a
second implementation beside it.  Here the C ABI is driven directly on tensors
the tests allocate (no PPO object, no env), so the batch and obs_dim are free:

* the gradient reference is ActorCritic(D, 3).double() with torch_ppo_loss
  under autograd, on the same float32 parameters and inputs cast up;
* the Adam reference is torch.optim.Adam's formula (after clip_grad_norm_'s)
  in float64;
* every comparison also runs the float32 torch path on the same inputs and
  reports its error against float64 beside the kernel's: that is the yardstick
  for the bounds (DESIGN.md section 4 lists the measured figures).

Inputs come from seeded CPU generators, so every run sees the same numbers.
Lines starting with "[ppo_mlp_ref]" (pytest -s) print the measured errors."""
import copy
import ctypes
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from grasp_lab_salp_amd import _lib
from grasp_lab_salp_amd.ppo import ActorCritic, torch_ppo_loss

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_BUF = 8192                 # buffer rows the gather draws from (idx repeats rows)
TR, NB_MAX = 64, 256         # salp_ppo_mlp.hip: rows per tile, row blocks at most
CLIP, ENT, VFC = 0.2, 0.01, 0.5
MARGIN = 1 << 16             # canary bytes on either side of a guarded buffer (test_gpu_bounds.py)
NAMES = ["pi_w1", "pi_b1", "pi_w2", "pi_b2", "act_w", "act_b", "log_std", "vf_w1", "vf_b1", "vf_w2", "vf_b2",
         "val_w", "val_b"]
ACTOR = NAMES[:6]

# The multi-tile shapes (B, D): what the launcher's row_blocks() makes of them
#   16 385  257 tiles, 2 per block: 129 blocks carry rows, the last one 1 row, 127 blocks are empty
#   24 000  the last used block has 1 tile, the others 2
#   32 768  the product's minibatch: 2 full tiles everywhere
#   32 833  3 tiles per block (the index prefetch two tiles ahead is live), last block 1 row
#   49 217  4 tiles per block (pipeline steady state), last block a full tile and a 1-row tile
MULTI_TILE = [(16385, 14), (24000, 10), (32768, 10), (32833, 14), (49217, 10), (49217, 1)]


def _order(pol):
    """The policy's tensors in include/salp.h's SalpMlpTensor order."""
    return [pol.pi_net[0].weight, pol.pi_net[0].bias, pol.pi_net[2].weight, pol.pi_net[2].bias,
            pol.action_net.weight, pol.action_net.bias, pol.log_std,
            pol.vf_net[0].weight, pol.vf_net[0].bias, pol.vf_net[2].weight, pol.vf_net[2].bias,
            pol.value_net.weight, pol.value_net.bias]


@functools.lru_cache(maxsize=None)
def _policies(D):
    """(float32, float64) ActorCritic twins holding the same float32 values: the
    orthogonal init moved by 0.05 N(0, 1) (action_net is not near zero).  Shared
    between tests and never modified (a test that changes parameters copies)."""
    with torch.random.fork_rng(devices=[]):
        torch.default_generator.manual_seed(1000 + D)
        p32 = ActorCritic(D, 3)
        with torch.no_grad():
            for p in p32.parameters():
                p.add_(torch.randn(p.shape) * 0.05)
    return p32.to(DEV), copy.deepcopy(p32).double().to(DEV)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


@torch.no_grad()
def _forward64(p64, obs, act):
    """log-prob and value of every buffer row in float64."""
    o = obs.double()
    return p64.dist(o).log_prob(act.double()).sum(-1), p64.value(o)


def _rows(D, n, seed, obs_scale=1.0):
    """n buffer rows: observations N(0, 1) (times obs_scale), actions 0.7 N(0, 1), and the CPU generator."""
    g = torch.Generator().manual_seed(seed)
    obs = (_randn(g, n, D) * obs_scale).to(DEV)
    act = (_randn(g, n, 3) * 0.7).to(DEV)
    return obs, act, g


def _ordinary(D, p64, seed, n=N_BUF, obs_scale=1.0):
    """The distributions of test_gpu_ppo_mlp._fill: old log-probs 0.2 N(0, 1)
    around the policy's own, advantages 3 N(0, 1) + 0.5, returns 5 N(0, 1)."""
    obs, act, g = _rows(D, n, seed, obs_scale)
    lp, _ = _forward64(p64, obs, act)
    return SimpleNamespace(obs=obs, act=act, olp=(lp + 0.2 * _randn(g, n).to(DEV)).float(),
                           adv=(_randn(g, n) * 3 + 0.5).to(DEV), ret=(_randn(g, n) * 5).to(DEV), g=g)


def _idx(g, B, n=N_BUF):
    return torch.randint(0, n, (B,), generator=g).to(DEV)


def _torch_path(pol, c, idx, norm):
    """Gradient (SalpMlpTensor order, float64 copies) and statistics of
    torch_ppo_loss under autograd in the dtype of `pol`."""
    dt = pol.log_std.dtype
    obs, act = c.obs[idx].to(dt), c.act[idx].to(dt)
    pol.zero_grad(set_to_none=True)
    loss, stats = torch_ppo_loss(pol.action_net(pol.pi_net(obs)), pol.log_std, pol.value(obs), act, c.olp[idx].to(dt),
                                 c.adv[idx].to(dt), c.ret[idx].to(dt), CLIP, ENT, VFC, norm and idx.numel() > 1)
    loss.backward()
    grads = [p.grad.detach().double().clone() for p in _order(pol)]
    pol.zero_grad(set_to_none=True)
    return grads, stats.double()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _kernel(p32, c, idx, norm, grads=None, ws=None, adv_part=None):
    """salp_ppo_mlp_grads on rows idx of c: (flat gradient, stats [4])."""
    L = _lib.load()
    B, D = idx.numel(), c.obs.shape[1]
    if grads is None:
        grads = torch.full((L.salp_ppo_mlp_num_params(D),), float("nan"), device=DEV)
    if ws is None:
        ws = torch.empty(L.salp_ppo_mlp_workspace_doubles(B, D), dtype=torch.float64, device=DEV)
    stats = torch.zeros(4, device=DEV)
    m = _lib.SalpPpoMinibatch(batch=B, obs_dim=D, normalize_advantage=int(norm), idx=idx.data_ptr(),
                              obs=c.obs.data_ptr(), actions=c.act.data_ptr(), old_log_prob=c.olp.data_ptr(),
                              advantages=c.adv.data_ptr(), returns=c.ret.data_ptr(), grads=grads.data_ptr(),
                              clip_range=CLIP, ent_coef=ENT, vf_coef=VFC, workspace=ws.data_ptr(),
                              stats=stats.data_ptr(), adv_part=adv_part)
    params = _order(p32)
    for i, t in enumerate(params):
        assert t.is_contiguous() and t.dtype == torch.float32 and t.is_cuda
        m.params[i] = t.data_ptr()
    _lib.check(L.salp_ppo_mlp_grads(ctypes.byref(m), _stream()))
    torch.cuda.synchronize()
    return grads, stats


def _errs(flat, ref, D):
    """Per tensor: largest error of the flat gradient against ref, over ref's largest entry."""
    L = _lib.load()
    out = {}
    for i, (n, r) in enumerate(zip(NAMES, ref)):
        o0, o1 = L.salp_ppo_mlp_offset(D, i), L.salp_ppo_mlp_offset(D, i + 1)
        assert o1 - o0 == r.numel(), n
        out[n] = float((flat[o0:o1].double() - r.reshape(-1)).abs().max()) / (float(r.abs().max()) + 1e-300)
    return out


def _check_grads(tag, flat, g64, g32, D, tol, names=NAMES):
    """The kernel's gradient within tol of every tensor's largest float64 entry;
    the float32 torch path's error beside it in the message.  Returns both worst errors."""
    ek, et = _errs(flat, g64, D), _errs(torch.cat([g.reshape(-1) for g in g32]), g64, D)
    wk, wt = max(ek[n] for n in names), max(et[n] for n in names)
    print(f"[ppo_mlp_ref] {tag}: gradient vs fp64 / largest entry: kernel {wk:.3g}, float32 torch {wt:.3g}")
    bad = {n: (ek[n], et[n]) for n in names if not ek[n] <= tol}
    assert not bad, f"{tag}: tensor: (kernel, float32 torch) error vs fp64, bound {tol}: {bad}"
    return wk, wt


def _check_stats(tag, sk, s64, s32, which=(0, 1, 2, 3)):
    """The project's bound: 1e-5 of max(1, |reference|) per statistic."""
    sk, s64, s32 = sk.tolist(), s64.tolist(), s32.tolist()
    for k in which:
        lim = 1e-5 * max(1.0, abs(s64[k]))
        print(f"[ppo_mlp_ref] {tag}: stat {k}: kernel {abs(sk[k] - s64[k]):.3g}, float32 torch "
              f"{abs(s32[k] - s64[k]):.3g}, bound {lim:.3g}")
        assert abs(sk[k] - s64[k]) <= lim, (tag, k, sk, s64, s32)


class _Guarded:
    """n bytes of 0xFF (NaN as float32 and as float64) between canary margins."""

    def __init__(self, n):
        self.raw = torch.full((MARGIN + n + MARGIN,), 0xA5, dtype=torch.uint8, device=DEV)
        self.raw[MARGIN:MARGIN + n] = 0xFF
        self.n = n

    def view(self, dtype):
        return self.raw[MARGIN:MARGIN + self.n].view(dtype)

    def intact(self):
        return bool((self.raw[:MARGIN] == 0xA5).all()) and bool((self.raw[-MARGIN:] == 0xA5).all())


# ------------------------------------------------------------------ 1. spikes
def _geometry(B):
    """salp_ppo_mlp_grads' split (csrc/salp_ppo_mlp.hip): (blocks, rows per block, blocks that carry rows)."""
    tiles = -(-B // TR)
    nb = min(tiles, NB_MAX)
    rpb = -(-tiles // nb) * TR
    return nb, rpb, -(-B // rpb)


def _spike_positions(B):
    """First and last row of every tile of the first, the middle and the last block that carries rows."""
    _, rpb, used = _geometry(B)
    pos = set()
    for blk in {0, used // 2, used - 1}:
        r0, r1 = blk * rpb, min((blk + 1) * rpb, B)
        for t0 in range(r0, r1, TR):
            pos.update((t0, min(t0 + TR, r1) - 1))
    return sorted(pos)


def test_spike_geometry_restates_the_launcher():
    """The shapes the cases below claim, from the same arithmetic as row_blocks(); the
    workspace size pins the block count (512 advantage partials, 6 statistics and P
    float32 partials per block)."""
    L = _lib.load()
    want = {16385: (256, 128, 129, 9), 24000: (256, 128, 188, 10), 32768: (256, 128, 256, 12),
            32833: (256, 192, 172, 13), 49217: (256, 256, 193, 19)}
    for B, (nb, rpb, used, spikes) in want.items():
        assert _geometry(B) == (nb, rpb, used)
        assert len(_spike_positions(B)) == spikes
        P = L.salp_ppo_mlp_num_params(10)
        assert L.salp_ppo_mlp_workspace_doubles(B, 10) == 512 + nb * 6 + (nb * P + 1) // 2


@pytest.mark.parametrize("B,D", MULTI_TILE)
def test_every_row_of_a_multi_tile_block_reaches_the_gradient(B, D):
    """Background rows carry next to no gradient (advantages and value errors
    1e-3 N(0, 1)); 9 to 19 spike rows at tile and block boundaries carry
    advantages and value errors of +-(1 .. 2).  Each spike has a buffer row of
    its own, so a spike that is dropped, doubled or paired with another row's
    observation moves every tensor but log_std by >= 3.4e-2 of its largest entry
    (CPU runs on these inputs, one spike dropped at a time); the float32 torch
    path is <= 5e-5 from float64.  Bound 1e-3 (never above 1e-2); pg_loss and vf_loss within 1e-5
    relative.  The workspace starts as NaN bytes between canaries: blocks
    without rows (127 of 256 at B = 16 385) must write their zero partials, and
    nothing past salp_ppo_mlp_workspace_doubles may be written."""
    L = _lib.load()
    p32, p64 = _policies(D)
    pos = _spike_positions(B)
    ns = len(pos)
    assert 9 <= ns <= 19
    obs, act, g = _rows(D, N_BUF + ns, seed=B + D)
    lp, v = _forward64(p64, obs, act)
    n = N_BUF + ns
    adv = _randn(g, n) * 1e-3
    dret = _randn(g, n) * 1e-3
    dlp = _randn(g, n) * 0.05
    sign = lambda: torch.randint(0, 2, (ns,), generator=g) * 2.0 - 1.0   # noqa: E731
    adv[N_BUF:] = sign() * (1 + torch.rand(ns, generator=g))
    dret[N_BUF:] = sign() * (1 + torch.rand(ns, generator=g))
    c = SimpleNamespace(obs=obs, act=act, olp=(lp + dlp.to(DEV)).float(), adv=adv.to(DEV),
                        ret=(v + dret.to(DEV)).float())
    idx = _idx(g, B)
    idx[torch.tensor(pos, device=DEV)] = N_BUF + torch.arange(ns, device=DEV)

    g64, s64 = _torch_path(p64, c, idx, False)
    g32, s32 = _torch_path(p32, c, idx, False)
    n_ws = L.salp_ppo_mlp_workspace_doubles(B, D)
    ws, gr = _Guarded(8 * n_ws), _Guarded(4 * L.salp_ppo_mlp_num_params(D))
    flat, sk = _kernel(p32, c, idx, False, grads=gr.view(torch.float32), ws=ws.view(torch.float64))
    assert ws.intact() and gr.intact(), "writes outside the workspace or the gradient"
    assert bool(torch.isfinite(flat).all()), "a partial of a block without rows was never written"
    tol = 1e-3
    assert tol <= 1e-2
    _, wt = _check_grads(f"spikes B={B} D={D}", flat, g64, g32, D, tol)
    assert wt <= 2.5e-4, f"float32 torch is {wt} from fp64 on these inputs: change this case's seed, not the bound"
    for k in (0, 1):
        ek, et = abs(float(sk[k]) - float(s64[k])), abs(float(s32[k]) - float(s64[k]))
        print(f"[ppo_mlp_ref] spikes B={B} D={D}: stat {k} relative: kernel {ek / abs(float(s64[k])):.3g}, "
              f"float32 torch {et / abs(float(s64[k])):.3g}")
        assert ek <= 1e-5 * abs(float(s64[k])), (k, sk.tolist(), s64.tolist(), s32.tolist())


# ------------------------------------------------------- 2. exact row counts
@pytest.mark.parametrize("B,D", MULTI_TILE)
def test_clip_fraction_counts_every_row_once(B, D):
    """old_log_prob = lp - s with s = +-0.5 (ratio 1.65 / 0.61: clipped) or
    U(-0.05, 0.05) (ratio within 0.05 of 1: inside), at least 0.15 from the
    clip edge, so float32 cannot move a row across it: round(stats[3] B) equals
    the float64 count exactly, all rows clipped give exactly 1.0 and none
    exactly 0.0.  A row that is lost or counted twice changes the count by one."""
    p32, p64 = _policies(D)
    c = _ordinary(D, p64, seed=7 * B + D)
    g = c.g
    lp, _ = _forward64(p64, c.obs, c.act)
    idx = _idx(g, B)
    big = (torch.randint(0, 2, (N_BUF,), generator=g) - 0.5).to(DEV)        # +-0.5
    small = ((torch.rand(N_BUF, generator=g) - 0.5) * 0.1).to(DEV)
    pick = (torch.rand(N_BUF, generator=g) < 0.4).to(DEV)
    for mode, s in (("mixed", torch.where(pick, big, small)), ("all", big), ("none", small)):
        c.olp = (lp - s.double()).float()
        ratio = torch.exp(lp[idx] - c.olp[idx].double())
        assert float(((ratio - 1).abs() - CLIP).abs().min()) > 0.14
        want = int(((ratio - 1).abs() > CLIP).sum())
        _, sk = _kernel(p32, c, idx, False)
        got = float(sk[3])
        assert round(got * B) == want, (mode, got * B, want)
        if mode == "all":
            assert want == B and got == 1.0
        if mode == "none":
            assert want == 0 and got == 0.0
        if mode == "mixed":
            assert 0.3 * B < want < 0.5 * B


# ------------------------------------- 3. ordinary inputs at the same shapes
@pytest.mark.parametrize("B", [16385, 32768, 49217])
def test_multi_tile_gradient_equals_fp64_autograd(B):
    """The inputs of test_gpu_ppo_mlp (advantages 3 N + 0.5, normalised) at
    multi-tile sizes, D = 10: every tensor within 1e-4 of its largest float64
    entry, the statistics within 1e-5."""
    D = 10
    p32, p64 = _policies(D)
    c = _ordinary(D, p64, seed=3 * B)
    idx = _idx(c.g, B)
    g64, s64 = _torch_path(p64, c, idx, True)
    g32, s32 = _torch_path(p32, c, idx, True)
    flat, sk = _kernel(p32, c, idx, True)
    _check_grads(f"ordinary B={B}", flat, g64, g32, D, 1e-4)
    _check_stats(f"ordinary B={B}", sk, s64, s32)


# ------------------------------------------------------------ 4. obs_dim sweep
@pytest.mark.parametrize("B", [200, 16400])
def test_obs_dim_sweep(B):
    """D = 1, 2, 6, 13, 14 (SALP_OBS_DIM_MAX): the k < D and (l & 15) < D masks at
    both ends, with 4 blocks and a ragged last tile (B = 200) and on the multi-tile
    path (B = 16 400).  One gradient buffer serves the sweep, NaN before every
    call: grads is overwritten, so a parameter the kernels skipped stays NaN, and
    so must everything past the D's parameter count."""
    L = _lib.load()
    grads = torch.empty(L.salp_ppo_mlp_num_params(14) + 64, device=DEV)
    for D in (1, 2, 6, 13, 14):
        p32, p64 = _policies(D)
        c = _ordinary(D, p64, seed=100 * B + D)
        idx = _idx(c.g, B)
        g64, s64 = _torch_path(p64, c, idx, True)
        g32, s32 = _torch_path(p32, c, idx, True)
        grads.fill_(float("nan"))
        _, sk = _kernel(p32, c, idx, True, grads=grads)
        P = L.salp_ppo_mlp_num_params(D)
        assert P == sum(t.numel() for t in _order(p32))
        assert bool(torch.isfinite(grads[:P]).all()), f"D={D}: a parameter's gradient was not written"
        assert bool(torch.isnan(grads[P:]).all()), f"D={D}: written past the {P} parameters"
        _check_grads(f"obs_dim D={D} B={B}", grads[:P], g64, g32, D, 1e-4)
        _check_stats(f"obs_dim D={D} B={B}", sk, s64, s32)


# ------------------------------------------------- 5. saturated / edge values
def test_saturated_hidden_units():
    """Observations times 8: first-layer pre-activations reach |z| ~ 30, so
    salp_tanhf runs both of its branches and full saturation (1 - h^2 = 0).
    Bound of the ordinary case; no NaN or Inf anywhere.
    (A ratio exactly on the clip edge, 1 +- 0.2f, is not constructible: exp of a
    float32 difference does not land on it.  Not tested.)"""
    B, D = 1000, 10
    p32, p64 = _policies(D)
    c = _ordinary(D, p64, seed=51, obs_scale=8.0)
    with torch.no_grad():
        z = p32.pi_net[0](c.obs)
    assert float(z.abs().max()) > 15 and float(z.abs().min()) < 0.05
    idx = _idx(c.g, B)
    g64, s64 = _torch_path(p64, c, idx, True)
    g32, s32 = _torch_path(p32, c, idx, True)
    flat, sk = _kernel(p32, c, idx, True)
    assert bool(torch.isfinite(flat).all()) and bool(torch.isfinite(sk).all())
    _check_grads("obs x 8", flat, g64, g32, D, 1e-4)
    _check_stats("obs x 8", sk, s64, s32)


def test_wide_and_narrow_log_std():
    """log_std = (-2, 0, 1.5): standard deviations 0.14 to 4.5 in one policy."""
    B, D = 1000, 10
    p32, p64 = (copy.deepcopy(p) for p in _policies(D))
    with torch.no_grad():
        p32.log_std.copy_(torch.tensor([-2.0, 0.0, 1.5]))
        p64.log_std.copy_(p32.log_std.double())
    c = _ordinary(D, p64, seed=52)
    idx = _idx(c.g, B)
    g64, s64 = _torch_path(p64, c, idx, True)
    g32, s32 = _torch_path(p32, c, idx, True)
    flat, sk = _kernel(p32, c, idx, True)
    _check_grads("log_std (-2, 0, 1.5)", flat, g64, g32, D, 1e-4)
    _check_stats("log_std (-2, 0, 1.5)", sk, s64, s32)


def test_one_row_ignores_normalisation():
    """B = 1 with normalize_advantage = 1: there is no standard deviation of one
    value; the kernel leaves the advantage as it is, like torch_ppo_loss."""
    D = 10
    p32, p64 = _policies(D)
    c = _ordinary(D, p64, seed=53)
    idx = _idx(c.g, 1)
    g64, s64 = _torch_path(p64, c, idx, True)
    g32, s32 = _torch_path(p32, c, idx, True)
    flat, sk = _kernel(p32, c, idx, True)
    _check_grads("B=1", flat, g64, g32, D, 1e-4)
    _check_stats("B=1", sk, s64, s32)


def test_equal_advantages_leave_no_policy_gradient():
    """Every advantage 3.7, normalised: (adv - mean) is exactly 0 in the kernel
    (fp64 sums of equal float32 values are exact), so the actor's six tensors get
    exactly 0 and log_std exactly -ent_coef; the critic meets float64 as usual.
    The float64 reference's own actor gradient is 0 up to the rounding of its
    mean: |adv - mean| <= one float64 ulp of 3.7 (4.4e-16), over the 1e-8 in the
    denominator <= 4.4e-8 per row, times O(1) row factors: below 1e-6."""
    L = _lib.load()
    B, D = 1000, 10
    p32, p64 = _policies(D)
    c = _ordinary(D, p64, seed=54)
    c.adv = torch.full_like(c.adv, 3.7)
    idx = _idx(c.g, B)
    g64, s64 = _torch_path(p64, c, idx, True)
    g32, s32 = _torch_path(p32, c, idx, True)
    flat, sk = _kernel(p32, c, idx, True)
    for i, n in enumerate(NAMES):
        o0, o1 = L.salp_ppo_mlp_offset(D, i), L.salp_ppo_mlp_offset(D, i + 1)
        if n in ACTOR:
            assert float(g64[i].abs().max()) <= 1e-6, n
            assert bool((flat[o0:o1] == 0).all()), (n, float(flat[o0:o1].abs().max()))
        if n == "log_std":
            assert torch.equal(flat[o0:o1], torch.full((3,), -ENT, device=DEV)), flat[o0:o1].tolist()
            assert float((g64[i] + ENT).abs().max()) <= 1e-6
    _check_grads("equal advantages", flat, g64, g32, D, 1e-4, names=NAMES[7:])
    _check_stats("equal advantages", sk, s64, s32)


# ------------------------------------------- 6. epoch-wide advantage partials
def test_epoch_advantage_partials_equal_the_minibatch_own():
    """salp_ppo_mlp_adv_partials over 3 minibatches of 1 000 rows in one launch:
    each minibatch's gradient and statistics with its adv_part equal, bit for
    bit, those with adv_part = NULL ("exactly as", include/salp.h), and meet the
    float64 reference."""
    L = _lib.load()
    B, K, D = 1000, 3, 10
    p32, p64 = _policies(D)
    c = _ordinary(D, p64, seed=61)
    idx = _idx(c.g, K * B)
    part = torch.full((K * _lib.ADV_PARTIAL_DOUBLES,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(L.salp_ppo_mlp_adv_partials(B, K, idx.data_ptr(), c.adv.data_ptr(), part.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(part).all())
    for k in range(K):
        ik = idx[k * B:(k + 1) * B]
        own, s_own = _kernel(p32, c, ik, True)
        pre, s_pre = _kernel(p32, c, ik, True, adv_part=part.data_ptr() + 8 * k * _lib.ADV_PARTIAL_DOUBLES)
        assert torch.equal(own, pre) and torch.equal(s_own, s_pre), k
        g64, s64 = _torch_path(p64, c, ik, True)
        g32, s32 = _torch_path(p32, c, ik, True)
        _check_grads(f"adv partials minibatch {k}", pre, g64, g32, D, 1e-4)
        _check_stats(f"adv partials minibatch {k}", s_pre, s64, s32)


# ---------------------------------------------------------------- 7. Adam
B1, B2, EPS = 0.9, 0.999, 1e-5


def _adam_ref(w, g, m, v, step, lr, max_norm):
    """clip_grad_norm_(max_norm) and torch.optim.Adam's update in float64, double betas."""
    norm = float(g.pow(2).sum().sqrt())
    if max_norm > 0:
        g = g * min(1.0, max_norm / (norm + 1e-6))
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    t = step + 1
    w = w - lr / (1 - B1 ** t) * m / (v.sqrt() / math.sqrt(1 - B2 ** t) + EPS)
    return w, m, v, norm, g


def _adam_torch32(params, g, m, v, step, lr, max_norm, offs):
    """The same step by torch.optim.Adam and clip_grad_norm_ in float32: flat (w, m, v)."""
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.Adam(ps, lr=lr, betas=(B1, B2), eps=EPS)
    for i, p in enumerate(ps):
        p.grad = g[offs[i]:offs[i + 1]].view_as(p).clone()
        opt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": m[offs[i]:offs[i + 1]].view_as(p).clone(),
                        "exp_avg_sq": v[offs[i]:offs[i + 1]].view_as(p).clone()}
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
    opt.step()
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])   # noqa: E731
    return (flat(ps), flat([opt.state[p]["exp_avg"] for p in ps]), flat([opt.state[p]["exp_avg_sq"] for p in ps]))


def _ulp32(x):
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


@pytest.mark.parametrize("D", [1, 14])
@pytest.mark.parametrize("blocks", [False, True], ids=["k_mlp_apply", "k_mlp_norm+k_mlp_adam"])
def test_adam_step_equals_fp64_adam(blocks, D):
    """salp_ppo_mlp_apply, one block (workspace NULL) and many (workspace set),
    with P = 8 839 / 10 503 parameters (no multiple of 64 or 256), from step
    0, 1, 999 and 100 000, max_grad_norm 0.5 (clipping by ~10), 1e9 and 0 (off),
    lr 3e-4 and 1e-2.  Moments are zero at step 0, else m = 0.01 N(0, 1) and
    v = m^2 (1 + U(0, 1)); gradients 0.05 N(0, 1) with 1 % exact zeros and 1 %
    at 1e-6 (near eps).  Against float64 Adam:
      weights   |w - w_ref| <= 1e-4 lr + 2 ulp32(w) each (a full step is ~lr)
      exp_avg_sq   1e-5 relative + 1e-12 each
      exp_avg      the same + 6 ulp32 of the larger of |beta1 m| and |(1 - beta1) g|
      step         exact;   grad_norm 2e-7 relative.
    torch.optim.Adam in float32 on the same state is measured beside it; it is
    the reason for exp_avg's last term.  Where the two addends of exp_avg cancel
    (|m_new| < 1e-4 at addends of ~1e-2, ~0.5 % of the entries) no float32
    arithmetic meets 1e-5 of the result: float32 torch misses 1e-5 |m| + 1e-12
    by up to 87x there (MI355X, these inputs; printed with -s), and its error
    reaches 3.2 ulp32 of the larger addend (a CPU run of the same inputs); the
    term is twice that.  Counting roundings gives at most 5.4 (the two products,
    the clipped gradient, the sum, the float32 betas and the clipping
    coefficient's two).  exp_avg_sq has no cancellation and keeps the
    plain bound: float32 torch is at 0.02 of it.  Before 1 - beta was taken in
    double (salp_ppo_mlp.hip) the kernels sat at 1.29 of it without clipping:
    1.0f - (float)0.999 is 1.29e-5 below 0.001."""
    L = _lib.load()
    p32, _ = _policies(D)
    params0 = [t.detach().clone() for t in _order(p32)]
    offs = [L.salp_ppo_mlp_offset(D, t) for t in range(14)]
    P = L.salp_ppo_mlp_num_params(D)
    assert P == offs[13] == sum(t.numel() for t in params0) and P % 64 and P % 256
    g = torch.Generator().manual_seed(70 + D)
    worst = {"w": (0.0, 0.0), "m": (0.0, 0.0), "v": (0.0, 0.0)}   # (kernel, float32 torch), in units of the bound
    bad, plain_m = [], 0.0   # plain_m: float32 torch's exp_avg error over the bound without the addend term
    for step in (0, 1, 999, 100000):
        for max_norm in (0.5, 1e9, 0.0):
            for lr in (3e-4, 1e-2):
                grads = _randn(g, P) * 0.05
                u = torch.rand(P, generator=g)
                grads[u < 0.01] = 0.0
                grads[u > 0.99] = 1e-6
                m0 = _randn(g, P) * 0.01 if step else torch.zeros(P)
                v0 = m0 * m0 * (1 + torch.rand(P, generator=g))
                grads, m0, v0 = grads.to(DEV), m0.to(DEV), v0.to(DEV)
                w0 = torch.cat([t.reshape(-1) for t in params0])
                wr, mr, vr, nr, gc = _adam_ref(w0.double(), grads.double(), m0.double(), v0.double(), step, lr,
                                               max_norm)
                wt, mt, vt = _adam_torch32(params0, grads, m0, v0, step, lr, max_norm, offs)
                # the kernel, on copies of the state
                params = [t.clone() for t in params0]
                mk, vk = m0.clone(), v0.clone()
                st, gn = torch.tensor([float(step)], device=DEV), torch.full((1,), float("nan"), device=DEV)
                ws = torch.zeros(_lib.APPLY_WORKSPACE_DOUBLES, dtype=torch.float64, device=DEV)
                a = _lib.SalpPpoAdam(obs_dim=D, norm_ready=0, grads=grads.data_ptr(), exp_avg=mk.data_ptr(),
                                     exp_avg_sq=vk.data_ptr(), step=st.data_ptr(), grad_norm=gn.data_ptr(), lr=lr,
                                     beta1=B1, beta2=B2, eps=EPS, max_grad_norm=max_norm,
                                     workspace=ws.data_ptr() if blocks else None)
                for i, t in enumerate(params):
                    a.params[i] = t.data_ptr()
                _lib.check(L.salp_ppo_mlp_apply(ctypes.byref(a), _stream()))
                torch.cuda.synchronize()
                wk = torch.cat([t.reshape(-1) for t in params])
                tag = f"step {step} max_norm {max_norm} lr {lr}"
                assert float(st) == step + 1, tag
                assert abs(float(gn) - nr) <= 2e-7 * nr, (tag, float(gn), nr)
                if blocks:
                    assert int(ws.view(torch.int64)[-1]) == 0, "the arrival count is left at zero"
                if max_norm == 0.5:
                    assert nr > 4.0   # clipping is active
                addend = torch.maximum((B1 * m0.double()).abs(), ((1 - B1) * gc).abs())
                lim = {"w": 1e-4 * lr + 2 * _ulp32(wr), "m": 1e-5 * mr.abs() + 1e-12 + 6 * _ulp32(addend),
                       "v": 1e-5 * vr.abs() + 1e-12}
                plain_m = max(plain_m, float(((mt.double() - mr).abs() / (1e-5 * mr.abs() + 1e-12)).max()))
                for key, xk, xt, xr in (("w", wk, wt, wr), ("m", mk, mt, mr), ("v", vk, vt, vr)):
                    ek = float(((xk.double() - xr).abs() / lim[key]).max())
                    et = float(((xt.double() - xr).abs() / lim[key]).max())
                    if ek > worst[key][0]:
                        worst[key] = (ek, et)
                    if not ek <= 1.0:
                        bad.append((tag, key, ek, et))
    for key, (ek, et) in worst.items():
        print(f"[ppo_mlp_ref] adam blocks={blocks} D={D}: {key} worst error / bound: kernel {ek:.3g} "
              f"(float32 torch there {et:.3g})")
    print(f"[ppo_mlp_ref] adam blocks={blocks} D={D}: float32 torch's exp_avg error / (1e-5 |m| + 1e-12): "
          f"{plain_m:.3g}")
    assert not bad, f"(case, tensor, kernel error / bound, float32 torch error / bound): {bad}"
