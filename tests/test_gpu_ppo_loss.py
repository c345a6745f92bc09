"""Fused PPO loss head (salp_ppo_loss) against the torch expression of SB3's
PPO loss (ppo.torch_ppo_loss): loss terms and gradients, float32 tolerance.

Below the first two tests, the C entry point itself against the float64
restatement tests/ppo_loss_ref.py.  out[8], dmu, dvalue and a workspace of
exactly SALP_PPO_WORKSPACE_DOUBLES doubles sit between canary blocks and are
filled with NaN before the call, the workspace too: a partial that is read
without having been written by this call turns the outputs NaN.

Bounds (ppo_loss_ref.bounds, whose docstring counts the roundings one by one;
u = 2^-24, everything from the reference's own intermediates, first order):
  logp      e_lp = u (9 sum_j t_j + 6 sum_j T_j), t = d^2 / (2 var), T = t + |log_std| + 0.92
  ratio     rho = e_lp + u (|logp| + |old_logp|) + 2 u   (relative: the ratio's relative error is the
            absolute error of logp - old_logp, plus expf's 1 ulp)
  A         normalised: e_A = u |mean| / std + |A| (5 u + (D + 3) 2^-53 kappa): the float32 rounding of
            the mean, then the roundings of inv and of the row, then what the one-pass variance
            q - s mean loses in fp64 (D <= 269 additions deep, kappa = sum adv^2 / sum (adv - mean)^2);
            not normalised: 0
  dmu       |d| / var ((e_A r + |dL_dr| r (rho + 3 u)) / B + 8 u |dlogp|), exactly 0 on cut rows
  dvalue    5 u |dvalue|
  dlog_std  the sum of the row bounds e_dlp |z - 1| + |dlogp| (9 u z + 2 u |z - 1|), z = d^2 / var, plus
            u (|S| + |ent_coef| + |S - ent_coef|)
  pg        the mean of e_A R + |A| R (rho + 3 u), R = max(r, clamp(r)), plus u |pg|
  vf        4 u vf;  entropy: three float32 additions;  loss: its terms' bounds + 2 u per coefficient
            and per addition
  clip_fraction  float32(reference) bit for bit, on inputs whose ratios are all further than
            r rho + 4 u (1 + c) from 1 -+ c (asserted on the reference; ppo_loss_ref.settle builds them)
tests/test_ppo_loss_ref_host.py shows on the CPU that float32 arithmetic in the kernel's operation order
stays inside these bounds on every family below.  Lines starting with "[ppo_loss]" (pytest -s) print
worst error / bound per tensor."""
import ctypes

import numpy as np
import pytest
import torch

import ppo_loss_ref as R
from grasp_lab_salp_amd import _lib
from grasp_lab_salp_amd.ppo import ppo_loss, torch_ppo_loss

pytestmark = pytest.mark.gpu


def _case(B, seed, ratio_spread):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    mu = r(B, 3) * 0.5
    log_std = r(3) * 0.3
    value = r(B) * 10
    actions = mu + r(B, 3) * log_std.exp()
    d = torch.distributions.Normal(mu, log_std.exp().expand_as(mu))
    old = d.log_prob(actions).sum(-1) + r(B) * ratio_spread   # ratios around 1, some clipped
    adv = r(B) * 100 + 3
    ret = value + r(B) * 5
    return mu, log_std, value, actions, old, adv, ret


@pytest.mark.parametrize("B,normalize", [(32768, True), (32768, False), (1000, True), (1, True)])
def test_fused_loss_matches_torch(B, normalize):
    args = _case(B, 7, 0.3)
    leaves = [t.clone().requires_grad_(True) for t in args[:3]]
    leaves2 = [t.clone().requires_grad_(True) for t in args[:3]]
    kw = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5, normalize_advantage=normalize)
    loss, st = ppo_loss(*leaves, *args[3:], **kw)
    loss.backward()
    loss_t, st_t = torch_ppo_loss(*leaves2, *args[3:], **kw)
    loss_t.backward()
    assert torch.allclose(st, st_t, rtol=1e-4, atol=1e-5), (st, st_t)
    assert torch.allclose(loss, loss_t, rtol=1e-4, atol=1e-5)
    for a, b in zip(leaves, leaves2):
        scale = b.grad.abs().max().item() + 1e-30
        assert (a.grad - b.grad).abs().max().item() <= 1e-4 * scale + 1e-7, (a.grad, b.grad)


def test_fused_loss_rejects_bad_shapes():
    args = _case(64, 1, 0.1)
    with pytest.raises(ValueError):
        ppo_loss(args[0][:, :2], *args[1:], clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True)


# ------------------------------------------------- the entry point against float64
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 131073)   # 131073: three passes + 1 row
KW = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5)
PAD, SENTINEL = 7, 12345.0


class _Guarded:
    """A NaN-filled tensor between two canary blocks."""

    def __init__(self, *shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, device="cuda", dtype=dtype)
        self.t = self.buf[PAD:PAD + n].view(*shape)
        self.t.fill_(float("nan"))

    def intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[-PAD:] == SENTINEL).all())


def _launch(args, clip_range, ent_coef, vf_coef, normalize):
    """One salp_ppo_loss call on the NumPy float32 inputs: {name: _Guarded}."""
    B = args[2].shape[0]
    dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in args]
    g = {"out": _Guarded(8), "dmu": _Guarded(B, 3), "dvalue": _Guarded(B),
         "workspace": _Guarded(R.WORKSPACE_DOUBLES, dtype=torch.float64)}
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().salp_ppo_loss(B, *(p(t) for t in dev), float(clip_range), float(ent_coef), float(vf_coef),
                                         int(normalize), p(g["workspace"].t), p(g["out"].t), p(g["dmu"].t),
                                         p(g["dvalue"].t), st))
    torch.cuda.synchronize()
    return g


def _run(tag, args, normalize, **kw):
    """Launch twice; written, finite, canaries, equal bits.  The kernel's tensors as R.worst's `got`."""
    g, again = _launch(args, normalize=normalize, **kw), _launch(args, normalize=normalize, **kw)
    for name, t in g.items():
        assert bool(torch.isfinite(t.t).all()), (tag, name)           # every element was written
        assert t.intact() and again[name].intact(), (tag, name)
    for name in ("out", "dmu", "dvalue"):
        bits = torch.int32
        assert torch.equal(g[name].t.view(bits), again[name].t.view(bits)), (tag, name)
    got = R.split_out(g["out"].t.cpu().numpy())
    got["dmu"], got["dvalue"] = g["dmu"].t.cpu().numpy(), g["dvalue"].t.cpu().numpy()
    return got


def _inside_bounds(tag, args, normalize, **kw):
    ref = R.loss(*args, normalize_advantage=normalize, **kw)
    bnd = R.bounds(ref)
    assert R.sides_are_decided(ref, bnd)                  # the precondition of the exact clip_fraction
    got = _run(tag, args, normalize, **kw)
    w = R.worst(got, ref, bnd)
    print(f"[ppo_loss] {tag} norm {int(normalize)}: " + " ".join(f"{k} {v:.3g}" for k, v in w.items()))
    assert max(w.values()) <= 1.0, (tag, w)
    return ref, got


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B", SIZES)
def test_loss_head_equals_fp64(B, normalize):
    """(a) the generic recipe at the block, grid and grid-stride seams."""
    _inside_bounds(f"generic B {B}", R.settle(R.generic(B, 7 + B), 0.2, normalize), normalize, **KW)


@pytest.mark.parametrize("B", [257, 65537])
@pytest.mark.parametrize("kind", ["e3", "e4"])
def test_loss_head_far_advantages(B, kind):
    """(b) advantages 1e3 + randn and 1e4 + 0.1 randn, normalised: the fp64 q - s mean."""
    ref, _ = _inside_bounds(f"far {kind} B {B}", R.settle(R.far_advantages(B, 21 + B, kind), 0.2, True), True, **KW)
    assert abs(ref.mean) / ref.std > 500


@pytest.mark.parametrize("B", [2, 257, 65537])
def test_loss_head_equal_advantages(B):
    """(b) all advantages equal, normalised: A is exactly 0, so the policy
    gradient is exactly zero and d loss / d log_std is -ent_coef in float32."""
    args = R.settle(R.far_advantages(B, 5, "equal"), 0.2, False)
    got = _run(f"equal B {B}", args, True, **KW)
    ref = R.loss(*args, normalize_advantage=False, **KW)          # (for the terms A does not enter)
    assert got["pg"] == 0 and (got["dmu"] == 0).all()
    assert (got["dlog_std"] == -np.float32(KW["ent_coef"])).all()
    assert np.float32(got["clip_fraction"]) == np.float32(ref.clip_fraction)
    bnd = R.bounds(ref)
    assert abs(got["vf"] - ref.vf) <= bnd.vf and (np.abs(got["dvalue"] - ref.dvalue) <= bnd.dvalue).all()
    assert abs(got["entropy"] - ref.entropy) <= bnd.entropy


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B", [257, 65537])
@pytest.mark.parametrize("clip", [0.0, 1e9])
def test_loss_head_clip_extremes(B, normalize, clip):
    """(c) clip_range 0 (every row clipped) and 1e9 (none; 1 - clip negative)."""
    kw = dict(KW, clip_range=clip)
    ref, got = _inside_bounds(f"clip {clip:g} B {B}", R.settle(R.generic(B, 31 + B), clip, normalize), normalize, **kw)
    assert got["clip_fraction"] == ref.clip_fraction == (1.0 if clip == 0.0 else 0.0)
    if clip == 0.0:         # the gradient passes exactly where A and r - 1 have opposite signs
        assert ((got["dmu"] != 0).all(1) == (ref.A * (ref.ratio - 1) < 0)).all()


@pytest.mark.parametrize("B", [256, 65537])
def test_loss_head_subgradient_conventions(B):
    """(d) log_std = 0 and old_logp the kernel's own float32 log-prob: every
    ratio is exactly 1, observable as clip_fraction == 0 at clip_range = 0.
    There min(A r, A clamp(r)) is a tie and r sits on both closed ends of the
    clamp, so d pg / d logp_b = -A_b / B in full (split ties: 0.5 + 0.5; an open
    interval would give half, unsplit ties twice).  Closed forms: dmu = -A d / B,
    dlog_std = sum_b -A (d^2 - 1) / B - ent_coef; exact at B = 256 (A a power
    of two, d on eighths), at 65537 within 3 u (1 / B and two products) per row
    term and 2 u on the float32 sum and the subtraction."""
    args = R.convention_rows(B, 41)
    got = _run(f"conventions B {B}", args, False, clip_range=0.0, ent_coef=0.25, vf_coef=0.5)
    assert got["clip_fraction"] == 0
    mu, _, _, act, _, adv, _ = (a.astype(np.float64) for a in args)
    d, dlp = act - mu, -adv / B
    want_dmu, want_ls = dlp[:, None] * d, (dlp[:, None] * (d * d - 1)).sum(0) - 0.25
    if B == 256:
        assert np.array_equal(got["dmu"], want_dmu) and np.array_equal(got["dlog_std"], want_ls)
    assert (np.abs(got["dmu"] - want_dmu) <= 3 * R.U * np.abs(want_dmu)).all()
    lim = 3 * R.U * np.abs(dlp[:, None] * (d * d - 1)).sum(0) + 2 * R.U * (np.abs(want_ls) + 0.25)
    assert (np.abs(got["dlog_std"] - want_ls) <= lim).all()
    assert got["pg"] == np.float32(-adv.mean())


def test_loss_head_clipped_rows():
    """(e) ratios 1.5 and 0.5 at clip_range 0.2: A > 0, r > 1 + c and A < 0,
    r < 1 - c are exactly +-0 in dmu, as are rows with A == 0; A < 0, r > 1 + c
    and A > 0, r < 1 - c carry the unclipped gradient (within the bound)."""
    args, kind = R.clipped_rows(335, 51)
    ref, got = _inside_bounds("clipped rows", args, False, **KW)
    cut = (kind == 0) | (kind == 1) | (kind == 4)
    assert (ref.passes == ~((kind == 0) | (kind == 1))).all() and (ref.dmu[cut] == 0).all()
    assert (got["dmu"][cut] == 0).all() and (got["dmu"][~cut] != 0).all()
    assert np.float32(got["clip_fraction"]) == 1.0


def test_loss_head_backward_scales_with_the_upstream_gradient():
    """(f) through ppo.ppo_loss: (3 loss).backward() gives three times loss.backward()'s gradients."""
    args = [torch.from_numpy(a).cuda() for a in R.generic(1000, 3)]
    grads = []
    for k in (1.0, 3.0):
        leaves = [t.clone().requires_grad_(True) for t in args[:3]]
        loss, _ = ppo_loss(*leaves, *args[3:], normalize_advantage=True, **KW)
        (k * loss).backward()
        grads.append([t.grad for t in leaves])
    for g1, g3 in zip(*grads):
        assert bool((g1 != 0).any()) and torch.equal(3.0 * g1, g3)
