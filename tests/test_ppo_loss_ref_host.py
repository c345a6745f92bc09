"""The float64 restatement of the PPO loss head (tests/ppo_loss_ref.py) against
``ppo.torch_ppo_loss`` under float64 autograd, and its error bounds against a
NumPy float32 restatement of the kernel's row arithmetic (csrc/salp_ppo.hip:
the same operation order, no contraction, fp64 sums of the float32 row terms):
the bounds tests/test_gpu_ppo_loss.py holds the kernel to can be met.  No GPU.

Lines starting with "[ppo_loss host]" (pytest -s) print worst error / bound."""
import numpy as np
import pytest
import torch

import ppo_loss_ref as R
from grasp_lab_salp_amd.ppo import torch_ppo_loss

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 131073)
KW = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5)


def kernel_f32(mu, log_std, value, actions, old_logp, adv, ret, clip_range, ent_coef, vf_coef, normalize):
    """k_ppo_adv_sums, k_ppo_rows and k_ppo_final in NumPy float32: the names
    of R.worst's `got`."""
    f = np.float32
    mu, ls, value, act, old, adv, ret = (np.asarray(x, f) for x in (mu, log_std, value, actions, old_logp, adv, ret))
    B = value.shape[0]
    amean, ainv = f(0), f(1)
    if normalize and B > 1:
        a64 = adv.astype(np.float64)
        s, q = a64.sum(), (a64 * a64).sum()
        mean = s / B
        var = max(q - s * mean, 0.0) / (B - 1)
        amean, ainv = f(mean), f(1) / (f(np.sqrt(var)) + f(1e-8))
    sd = np.exp(ls)
    var = sd * sd
    d = act - mu
    lp = R.logp_f32(mu, ls, act)
    A = (adv - amean) * ainv if normalize else adv
    r = np.exp(lp - old)
    c = f(clip_range)
    lo, hi = f(1) - c, f(1) + c
    rc = np.minimum(np.maximum(r, lo), hi)
    p1, p2 = A * r, A * rc
    tie = np.where(p1 == p2, f(0.5), f(0))
    g1, g2 = np.where(p1 < p2, f(1), tie), np.where(p2 < p1, f(1), tie)
    inside = (r >= lo) & (r <= hi)
    dL = g1 * A + np.where(inside, g2 * A, f(0))
    invB = f(1) / f(B)
    dlp = -invB * dL * r
    dmu = dlp[:, None] * d / var
    rows_ls = dlp[:, None] * (d * d / var - f(1))
    e = ret - value
    dvalue = f(vf_coef) * (f(-2) * e * invB)
    t = [np.minimum(p1, p2).astype(np.float64).sum(), (e * e).astype(np.float64).sum(),
         float((np.abs(r - f(1)) > c).sum())] + list(rows_ls.astype(np.float64).sum(0))
    assert all(x.dtype == f for x in (lp, A, r, rc, dL, dlp, dmu, rows_ls, dvalue))
    pg, vf = f(-t[0] / B), f(t[1] / B)
    ent = f(0)
    for j in range(3):
        ent = ent + (f(0.5) + f(R.LOG_SQRT_2PI) + ls[j])
    return {"loss": pg - f(ent_coef) * ent + f(vf_coef) * vf, "pg": pg, "vf": vf, "entropy": ent,
            "clip_fraction": f(t[2] / B), "dlog_std": np.array([f(t[3 + j]) - f(ent_coef) for j in range(3)]),
            "dmu": dmu, "dvalue": dvalue}


def _inside_bounds(tag, args, normalize, **kw):
    ref = R.loss(*args, normalize_advantage=normalize, **kw)
    bnd = R.bounds(ref)
    assert R.sides_are_decided(ref, bnd)
    w = R.worst(kernel_f32(*args, normalize=normalize, **kw), ref, bnd)
    print(f"[ppo_loss host] {tag} norm {int(normalize)}: " + " ".join(f"{k} {v:.3g}" for k, v in w.items()))
    assert max(w.values()) <= 1.0, (tag, w)
    return ref, w


@pytest.mark.parametrize("B", [1, 2, 257, 4099])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("clip", [0.2, 0.0, 1e9])
def test_restatement_equals_torch_float64_autograd(B, normalize, clip):
    args = R.settle(R.generic(B, 11 + B), clip, normalize)
    kw = dict(clip_range=clip, ent_coef=0.01, vf_coef=0.5, normalize_advantage=normalize)
    ref = R.loss(*args, **kw)
    t = [torch.from_numpy(a.astype(np.float64)) for a in args]
    leaves = [x.requires_grad_(True) for x in t[:3]]
    lt, st = torch_ppo_loss(*leaves, *t[3:], **kw)
    lt.backward()
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-300)  # noqa: E731
    close(ref.loss, lt.item())
    close([ref.pg, ref.vf, ref.entropy], st.numpy()[:3])
    assert np.float32(ref.clip_fraction) == np.float32(st[3].item())     # (torch takes this mean in float32)
    # (gradients: 1e-12 of the tensor's largest entry, as sums of cancelling terms carry it)
    for got, leaf in ((ref.dmu, leaves[0]), (ref.dlog_std, leaves[1]), (ref.dvalue, leaves[2])):
        g = leaf.grad.numpy()
        assert np.abs(got - g).max() <= 1e-12 * np.abs(g).max(), (np.abs(got - g).max(), np.abs(g).max())
    if clip == 0.2 and B >= 257:
        assert set(np.unique(ref.branch)) == {R.UNCLIPPED, R.CLIPPED, R.TIE} and not ref.passes.all()
        assert (ref.inside == (ref.branch == R.TIE)).all()


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("normalize", [True, False])
def test_float32_row_arithmetic_is_inside_the_bounds_generic(B, normalize):
    _inside_bounds(f"generic B {B}", R.settle(R.generic(B, 7 + B), 0.2, normalize), normalize, **KW)


@pytest.mark.parametrize("B", [257, 65537])
@pytest.mark.parametrize("kind", ["e3", "e4"])
def test_float32_row_arithmetic_is_inside_the_bounds_far_advantages(B, kind):
    ref, _ = _inside_bounds(f"far {kind} B {B}", R.settle(R.far_advantages(B, 21 + B, kind), 0.2, True), True, **KW)
    assert abs(ref.mean) / ref.std > 500


@pytest.mark.parametrize("B", [257, 65537])
def test_float32_row_arithmetic_equal_advantages_give_exact_zeros(B):
    got = kernel_f32(*R.far_advantages(B, 5, "equal"), normalize=True, **KW)
    assert got["pg"] == 0 and (got["dmu"] == 0).all()
    assert (got["dlog_std"] == -np.float32(KW["ent_coef"])).all()


@pytest.mark.parametrize("B", [257, 65537])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("clip", [0.0, 1e9])
def test_float32_row_arithmetic_is_inside_the_bounds_clip_extremes(B, normalize, clip):
    kw = dict(KW, clip_range=clip)
    ref, _ = _inside_bounds(f"clip {clip:g} B {B}", R.settle(R.generic(B, 31 + B), clip, normalize), normalize, **kw)
    assert ref.clip_fraction == (1.0 if clip == 0.0 else 0.0)


@pytest.mark.parametrize("B", [256, 65537])
def test_float32_row_arithmetic_conventions(B):
    """Ratio exactly 1 at clip_range 0: the tie and the closed interval pass the full -A / B."""
    args = R.convention_rows(B, 41)
    got = kernel_f32(*args, 0.0, 0.25, 0.5, False)
    assert got["clip_fraction"] == 0
    mu, _, _, act, _, adv, _ = (a.astype(np.float64) for a in args)
    d = act - mu
    dlp = -adv / B
    want_dmu, want_ls = dlp[:, None] * d, (dlp[:, None] * (d * d - 1)).sum(0) - 0.25
    if B == 256:
        assert np.array_equal(got["dmu"], want_dmu) and np.array_equal(got["dlog_std"], want_ls)
    assert (np.abs(got["dmu"] - want_dmu) <= 3 * R.U * np.abs(want_dmu)).all()
    lim = 3 * R.U * np.abs(dlp[:, None] * (d * d - 1)).sum(0) + 2 * R.U * (np.abs(want_ls) + 0.25)
    assert (np.abs(got["dlog_std"] - want_ls) <= lim).all()


def test_float32_row_arithmetic_clipped_rows():
    args, kind = R.clipped_rows(335, 51)
    ref, _ = _inside_bounds("clipped rows", args, False, **KW)
    got = kernel_f32(*args, normalize=False, **KW)
    cut = (kind == 0) | (kind == 1) | (kind == 4)
    assert (got["dmu"][cut] == 0).all() and (ref.dmu[cut] == 0).all() and (ref.passes == ~((kind == 0) | (kind == 1))).all()
    assert (got["dmu"][~cut] != 0).all()
