"""SAC's networks as HIP kernels (csrc/salp_sac_mlp.hip, include/salp.h
salp_sac_net_*) on the GPU, and the learner with ``fused_mlp=True``.

The reference is always the same nn.Module as a float64 copy under autograd on
the same float32 values; the plain float32 torch path (rocBLAS GEMMs) runs
beside every comparison as the yardstick.  The bound is the project's own
(tests/test_gpu_sac.py, test_gpu_ppo_mlp_ref._check_grads): per tensor, the
error against float64 over the tensor's largest float64 entry is at most 4 x
the float32 torch path's plus a floor of 4 u, u = 2^-24.  Lines starting with
"[sac_mlp]" (pytest -s) print both errors per tensor.

Inputs come from seeded CPU generators.  TR = salp_sac_net_tile_rows() rows
make a tile; the backward runs at most MAXB = salp_sac_net_max_blocks() row
blocks per network, block bx taking tiles bx, bx + MAXB, ..."""
import copy
import ctypes

import pytest
import torch

from grasp_lab_salp_amd import _lib, sac

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
MARGIN = 4096
HID = (256, 256)


def _geometry():
    L = _lib.load()
    return L.salp_sac_net_tile_rows(), L.salp_sac_net_max_blocks()


TR, MAXB = 32, 64     # asserted against the library in test_geometry_is_the_library_s
BATCHES = [1, TR - 1, TR, TR + 1, 257]
DIMS = [6, 10, 14]


def test_geometry_is_the_library_s():
    assert _geometry() == (TR, MAXB)


class _Guarded:
    """n bytes of 0xFF (NaN as float32) between canary margins (tests/test_gpu_bounds.py)."""

    def __init__(self, n):
        self.raw = torch.full((MARGIN + n + MARGIN,), 0xA5, dtype=torch.uint8, device=DEV)
        self.raw[MARGIN:MARGIN + n] = 0xFF
        self.n = n

    def f32(self, *shape):
        return self.raw[MARGIN:MARGIN + self.n].view(torch.float32).view(*shape)

    def intact(self):
        return bool((self.raw[:MARGIN] == 0xA5).all()) and bool((self.raw[-MARGIN:] == 0xA5).all())

    def untouched(self):
        return self.intact() and bool((self.raw[MARGIN:MARGIN + self.n] == 0xFF).all())


class _Net:
    """One network: the module it lives in, its parameters in the kernel's
    flat order and how the module evaluates (out, h1, h2)."""

    def __init__(self, mod, kind):
        self.mod, self.kind = mod, kind
        self.out_dim = 6 if kind == "actor" else 1

    def params(self, mod=None):
        mod = self.mod if mod is None else mod
        return mod.net_params() if self.kind == "actor" else list(mod.parameters())

    def run(self, mod, x0, x1):
        if self.kind == "actor":
            h1 = mod.latent_pi[:2](x0)
            h2 = mod.latent_pi[2:](h1)
            return torch.cat([mod.mu(h2), mod.log_std(h2)], dim=1), h1, h2
        h1 = mod[:2](torch.cat([x0, x1], dim=1))
        h2 = mod[2:4](h1)
        return mod[4](h2), h1, h2

    def grads6(self, mod):
        """The six kernel tensors' gradients of `mod`, flat, float64."""
        g = [p.grad.detach().double().reshape(-1) for p in self.params(mod)]
        return g if self.kind != "actor" else g[:4] + [torch.cat(g[4:6]), torch.cat(g[6:8])]


NAMES6 = ("W1", "b1", "W2", "b2", "W3", "b3")
_nets = {}


def _networks(D):
    """An actor and four critic networks (a critic and a target copy's two each) of obs_dim D on the GPU."""
    if D not in _nets:
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(900 + D)
            actor = sac._Actor(D, 3, HID).to(DEV).flatten_()
            c1, c2 = sac._Critic(D, 3, HID).to(DEV).flatten_(), sac._Critic(D, 3, HID).to(DEV).flatten_()
        assert actor.is_flat() and c1.is_flat() and c2.is_flat()
        _nets[D] = (_Net(actor, "actor"), [_Net(q, "critic") for q in (c1.qf0, c1.qf1, c2.qf0, c2.qf1)])
    return _nets[D]


def _inputs(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, generator=g).to(DEV), (torch.rand(B, 3, generator=g) * 2 - 1).to(DEV)


def _fill(arr, tensors):
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr() if t is not None else None


def _kernel_forward(nets, x0, x1, keep):
    """salp_sac_net_forward into guarded buffers: ([out], [h1], [h2]) per network (h: None if not kept)."""
    n, B, od = len(nets), x0.shape[0], nets[0].out_dim
    d1 = 0 if x1 is None else x1.shape[1]
    gs = {"out": [_Guarded(B * od * 4) for _ in nets]}
    for k in ("h1", "h2"):
        gs[k] = [_Guarded(B * 256 * 4) for _ in nets] if keep else None
    f = _lib.SalpSacNetForward(batch=B, d0=x0.shape[1], d1=d1, out_dim=od, n_nets=n)
    _fill(f.params, [net.params()[0] for net in nets])
    _fill(f.x0, [x0] * n)
    _fill(f.x1, [x1] * n)
    _fill(f.out, [g.f32(B, od) for g in gs["out"]])
    if keep:
        _fill(f.h1, [g.f32(B, 256) for g in gs["h1"]])
        _fill(f.h2, [g.f32(B, 256) for g in gs["h2"]])
    _lib.check(_lib.load().salp_sac_net_forward(ctypes.byref(f), None))
    torch.cuda.synchronize()
    for k, lst in gs.items():
        assert lst is None or all(g.intact() for g in lst), f"{k}: a canary beside the buffer was overwritten"
    shape = {"out": (B, od), "h1": (B, 256), "h2": (B, 256)}
    return tuple(None if gs[k] is None else [g.f32(*shape[k]) for g in gs[k]] for k in ("out", "h1", "h2"))


def _kernel_backward(nets, x0, x1, h1, h2, dout, want_p=True, want_dx=True):
    """salp_sac_net_backward with a NaN-filled guarded workspace and outputs: (gflat [n, P] guarded, dx1)."""
    L = _lib.load()
    n, B, od = len(nets), x0.shape[0], nets[0].out_dim
    d0, d1 = x0.shape[1], 0 if x1 is None else x1.shape[1]
    P = L.salp_sac_net_num_params(d0 + d1, od)
    ws = _Guarded(4 * L.salp_sac_net_workspace_floats(B, d0, d1, od, n))
    gp = _Guarded(4 * n * P)
    gx = _Guarded(4 * B * d1) if want_dx else None
    b = _lib.SalpSacNetBackward(batch=B, d0=d0, d1=d1, out_dim=od, n_nets=n,
                                dx1=gx.f32(B, d1).data_ptr() if want_dx else None,
                                workspace=ws.f32(ws.n // 4).data_ptr())
    _fill(b.params, [net.params()[0] for net in nets])
    _fill(b.x0, [x0] * n)
    _fill(b.x1, [x1] * n)
    _fill(b.h1, h1)
    _fill(b.h2, h2)
    _fill(b.dout, dout)
    if want_p:
        _fill(b.dparams, [gp.f32(n, P)[i] for i in range(n)])
    _lib.check(L.salp_sac_net_backward(ctypes.byref(b), None))
    torch.cuda.synchronize()
    assert ws.intact() and gp.intact() and (gx is None or gx.intact()), "a canary beside a buffer was overwritten"
    return gp, (gx.f32(B, d1) if want_dx else None)


def _bound(tag, got, ref, plain, bad):
    """Append (tag, kernel error, float32 torch error) to `bad` if `got` misses the bound; print both."""
    ref = ref.double()
    top = float(ref.abs().max())
    if top == 0.0:
        ek = et = 0.0
        ok = bool((got == 0).all())
    else:
        ek = float((got.double() - ref).abs().max()) / top
        et = float((plain.double() - ref).abs().max()) / top
        ok = ek <= 4 * et + 4 * U
    print(f"[sac_mlp] {tag}: kernel {ek:.3g}, float32 torch {et:.3g}")
    if not ok:
        bad.append((tag, ek, et))
    return 4 * et + 4 * U


def _torch_pass(nets, x0, x1, dout, dtype):
    """The modules' own forward and backward in `dtype` (float64: on copies): per network (out, h1, h2, grads6), and x1.grad."""
    x0, x1 = x0.to(dtype), None if x1 is None else x1.to(dtype).requires_grad_(dout is not None)
    res, outs = [], []
    mods = [net.mod if dtype == torch.float32 else copy.deepcopy(net.mod).double() for net in nets]
    for net, mod in zip(nets, mods):
        for p in mod.parameters():
            p.grad = None
        outs.append(net.run(mod, x0, x1))
    if dout is not None:
        torch.autograd.backward([o[0] for o in outs], [d.to(dtype) for d in dout])
    for net, mod, o in zip(nets, mods, outs):
        res.append(tuple(t.detach() for t in o) + (net.grads6(mod) if dout is not None else None,))
        for p in mod.parameters():
            p.grad = None
    return res, (x1.grad.detach() if dout is not None and x1 is not None else None)


def _groups(D):
    actor, critics = _networks(D)
    return [("actor", [actor], False), ("critics", critics[:2], True), ("four", critics, True)]


# ------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("B", BATCHES)
def test_forward_equals_fp64(B, D):
    """The actor, two critics in one launch and four networks in one launch:
    out and the kept h1, h2 against float64; a pass that keeps nothing gives
    the same out bit for bit; canaries beside every output buffer survive."""
    x0, xa = _inputs(B, D, 1000 + 17 * B + D)
    bad = []
    for name, nets, with_x1 in _groups(D):
        x1 = xa if with_x1 else None
        out, h1, h2 = _kernel_forward(nets, x0, x1, keep=True)
        lean, _, _ = _kernel_forward(nets, x0, x1, keep=False)
        assert all(torch.equal(a, b) for a, b in zip(out, lean)), name
        r64, _ = _torch_pass(nets, x0, x1, None, torch.float64)
        r32, _ = _torch_pass(nets, x0, x1, None, torch.float32)
        for i in range(len(nets)):
            for k, got in enumerate((out[i], h1[i], h2[i])):
                assert bool(torch.isfinite(got).all())
                _bound(f"forward B={B} D={D} {name}[{i}] {('out', 'h1', 'h2')[k]}", got, r64[i][k], r32[i][k], bad)
    assert not bad, f"(tensor, kernel error, float32 torch error) against fp64: {bad}"


# ----------------------------------------------------------------- 2. backward
def _check_backward(tag, nets, x0, x1, dout, bad):
    """Kernel forward (kept) + backward against the float64 and float32 module passes; returns
    (gflat [n, P], dx1, the references) for further checks."""
    n = len(nets)
    _, h1, h2 = _kernel_forward(nets, x0, x1, keep=True)
    gp, dx = _kernel_backward(nets, x0, x1, h1, h2, dout, want_dx=x1 is not None)
    P = gp.n // 4 // n
    g = gp.f32(n, P)
    assert bool(torch.isfinite(g).all()) and (dx is None or bool(torch.isfinite(dx).all())), tag
    r64, dx64 = _torch_pass(nets, x0, x1, dout, torch.float64)
    r32, dx32 = _torch_pass(nets, x0, x1, dout, torch.float32)
    L = _lib.load()
    off = [L.salp_sac_net_offset(x0.shape[1] + (0 if x1 is None else x1.shape[1]), nets[0].out_dim, t) for t in range(7)]
    bounds = {}
    for i in range(n):
        for t, name in enumerate(NAMES6):
            bounds[(i, name)] = _bound(f"{tag} net {i} d{name}", g[i, off[t]:off[t + 1]], r64[i][3][t], r32[i][3][t], bad)
    if dx is not None:
        _bound(f"{tag} dx1", dx, dx64, dx32, bad)
    return g, dx, r64, dx64, off, bounds


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("B", BATCHES)
def test_backward_equals_fp64_and_is_deterministic(B, D):
    """All six parameter-gradient tensors per network, and dx1 summed over the
    two critics, against float64 from random dout.  The workspace and the
    outputs start as NaN between canaries; results are finite and equal a
    second run's bit for bit; with dparams = NULL the same dx1 comes out bit
    for bit and the flat gradient buffer stays untouched."""
    x0, xa = _inputs(B, D, 2000 + 17 * B + D)
    g = torch.Generator().manual_seed(2500 + 17 * B + D)
    bad = []
    for name, nets, with_x1 in _groups(D)[:2]:
        x1 = xa if with_x1 else None
        dout = [torch.randn(B, nets[0].out_dim, generator=g).to(DEV) for _ in nets]
        gk, dx, *_ = _check_backward(f"backward B={B} D={D} {name}", nets, x0, x1, dout, bad)
        _, h1, h2 = _kernel_forward(nets, x0, x1, keep=True)
        gp2, dx2 = _kernel_backward(nets, x0, x1, h1, h2, dout, want_dx=with_x1)
        assert torch.equal(gp2.f32(*gk.shape), gk), name
        if with_x1:
            assert torch.equal(dx2, dx), name
            gp3, dx3 = _kernel_backward(nets, x0, x1, h1, h2, dout, want_p=False)
            assert torch.equal(dx3, dx) and gp3.untouched(), name
    assert not bad, f"(tensor, kernel error, float32 torch error) against fp64: {bad}"


# ------------------------------------------------------ 3. tile and block seams
def test_rows_at_tile_and_block_seams():
    """B = TR MAXB + 1: block 0 runs a second tile, of one ragged row.  dout is
    zero except on rows {0, TR - 1, TR, TR MAXB - 1, TR MAXB}: the two ends of
    the first tile, the first row of the second block, the last row of the last
    block and the row of block 0's second tile.  Each has an input of its own.
    First, on the CPU in float64 from the five rows alone (the others have no
    gradient): leaving any one of them out moves every weight-gradient tensor
    by at least 100 x the bound."""
    D = 10
    B = TR * MAXB + 1
    rows = [0, TR - 1, TR, TR * MAXB - 1, TR * MAXB]
    x0, xa = _inputs(B, D, 3000)
    g = torch.Generator().manual_seed(3001)
    _, critics = _networks(D)
    nets = critics[:2]
    dout = []
    for _ in nets:
        d = torch.zeros(B, 1)
        # magnitudes in 1 .. 2, one negative: the sum (db3) cannot cancel below 2
        d[rows] = (1.0 + torch.rand(len(rows), 1, generator=g)) * torch.tensor([[1.0], [1.0], [-1.0], [1.0], [1.0]])
        dout.append(d.to(DEV))
    bad = []
    gk, dx, r64, dx64, off, bounds = _check_backward(f"seams B={B}", nets, x0, xa, dout, bad)
    assert not bad, f"(tensor, kernel error, float32 torch error) against fp64: {bad}"
    # the CPU check of the test's own power, with the bounds the comparison just used
    for i, net in enumerate(nets):
        mod = copy.deepcopy(net.mod).double().cpu()
        per_row = []
        for r in rows:
            for p in mod.parameters():
                p.grad = None
            out, _, _ = net.run(mod, x0[r:r + 1].double().cpu(), xa[r:r + 1].double().cpu())
            out.backward(dout[i][r:r + 1].double().cpu())
            per_row.append(net.grads6(mod))
        for t, name in enumerate(NAMES6):
            total = sum(pr[t] for pr in per_row)
            top = float(total.abs().max())
            assert float((total - r64[i][3][t].cpu()).abs().max()) <= 1e-12 * top     # the five rows are the gradient
            for k, r in enumerate(rows):
                moved = float(per_row[k][t].abs().max()) / top
                assert moved >= 100 * bounds[(i, name)], (i, name, r, moved, bounds[(i, name)])
    assert bool((dx[[r for r in range(B) if r not in rows][:64]] == 0).all())


# ------------------------------------------------- 4. dead and exactly-zero units
def test_dead_and_exactly_zero_units():
    """Hidden unit 5 of layer 1 has its W1 row and b1 zeroed (pre-activation
    exactly 0), unit 77 a bias of -1e3 (dead); units 9 and 130 of layer 2 the
    same.  Their gradients are exactly 0 on the kernel path, as torch's
    threshold_backward gives, and so is the column of dW2 / dW3 their zero
    activation multiplies; the other tensors stay within the bound."""
    D, B = 10, TR + 1
    x0, xa = _inputs(B, D, 4000)
    g = torch.Generator().manual_seed(4001)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(4002)
        actor = sac._Actor(D, 3, HID).to(DEV).flatten_()
        critic = sac._Critic(D, 3, HID).to(DEV).flatten_()
    groups = [("actor", [_Net(actor, "actor")], None), ("critics", [_Net(critic.qf0, "critic"),
                                                                     _Net(critic.qf1, "critic")], xa)]
    Z1, N1, Z2, N2 = 5, 77, 9, 130
    bad = []
    for name, nets, x1 in groups:
        for net in nets:
            W1, b1, W2, b2 = net.params()[:4]
            with torch.no_grad():
                W1[Z1] = 0.0
                b1[Z1] = 0.0
                b1[N1] = -1e3
                W2[Z2] = 0.0
                b2[Z2] = 0.0
                b2[N2] = -1e3
        dout = [torch.randn(B, nets[0].out_dim, generator=g).to(DEV) for _ in nets]
        gk, dx, r64, dx64, off, _ = _check_backward(f"dead units {name}", nets, x0, x1, dout, bad)
        _, h1, h2 = _kernel_forward(nets, x0, x1, keep=True)
        d_in = off[1] // 256
        for i in range(len(nets)):
            assert bool((h1[i][:, [Z1, N1]] == 0).all()) and bool((h2[i][:, [Z2, N2]] == 0).all())
            t = {n: gk[i, off[k]:off[k + 1]] for k, n in enumerate(NAMES6)}
            ref = {n: r64[i][3][k] for k, n in enumerate(NAMES6)}
            w1, w2, w3 = t["W1"].view(256, d_in), t["W2"].view(256, 256), t["W3"].view(-1, 256)
            zero = [w1[[Z1, N1]], t["b1"][[Z1, N1]], w2[:, [Z1, N1]], w2[[Z2, N2]], t["b2"][[Z2, N2]], w3[:, [Z2, N2]]]
            assert all(bool((z == 0).all()) for z in zero), (name, i)
            r1, r2 = ref["W1"].view(256, d_in), ref["W2"].view(256, 256)
            assert bool((r1[[Z1, N1]] == 0).all()) and bool((r2[:, [Z1, N1]] == 0).all()) \
                and bool((r2[[Z2, N2]] == 0).all())
            assert float(w1.abs().max()) > 0 and float(w2.abs().max()) > 0
    assert not bad, f"(tensor, kernel error, float32 torch error) against fp64: {bad}"


# ----------------------------------------------------------- 5. the gradient step
def _make_learner(**kw):
    """tests/test_gpu_sac.py's `learner` recipe: 64 envs, batch 64, three collected env-steps."""
    from grasp_lab_salp_amd.vec_env import SalpVecEnv
    m = sac.SAC("MlpPolicy", SalpVecEnv(64, seed=3), learning_starts=128, batch_size=64, buffer_size=512, seed=1, **kw)
    for _ in range(3):
        m.collect_step()
    torch.cuda.synchronize()
    return m


def _step(pol, la, batch, eps, fused, fused_mlp):
    from test_gpu_sac import _grads_of
    for p in list(pol.parameters()) + [la]:
        p.grad = None
    st = sac.critic_phase(pol, la, batch, eps[0], eps[1], 0.99, -3.0, fused, fused_mlp=fused_mlp)
    actor_loss = sac.actor_phase(pol, st, fused, fused_mlp=fused_mlp)
    losses = {"critic_loss": st["critic_loss"], "ent_coef_loss": st["ent_coef_loss"], "actor_loss": actor_loss}
    return {k: float(v) for k, v in losses.items()}, _grads_of(pol, la)


def test_one_gradient_step_equals_fp64():
    """critic_phase + actor_phase of one sampled batch three ways: fused_mlp,
    fused alone (torch's GEMMs) and plain torch on a float64 copy.  The three
    losses, every actor / critic gradient and log_alpha.grad within the bound.
    The fused_mlp actor pass leaves the critics' gradients as the critic pass
    made them (it computes none)."""
    m = _make_learner()
    assert m.fused and not m.fused_mlp and m.n_updates == 0
    batch = m.replay.sample(64, m._update)
    g = torch.Generator().manual_seed(7)
    eps = [torch.randn(64, 3, generator=g).to(DEV) for _ in range(2)]
    la = torch.full((1,), -0.7, device=DEV, requires_grad=True)
    pol64 = copy.deepcopy(m.policy).double()
    la64 = la.detach().double().requires_grad_(True)
    l_k, g_k = _step(m.policy, la, batch, eps, True, True)
    l_p, g_p = _step(m.policy, la, batch, eps, True, False)
    l_d, g_d = _step(pol64, la64, tuple(t.double() for t in batch), [e.double() for e in eps], False, False)
    for p in m.policy.parameters():
        p.grad = None
    bad = []
    for k in l_d:
        ek, ep = abs(l_k[k] - l_d[k]) / abs(l_d[k]), abs(l_p[k] - l_d[k]) / abs(l_d[k])
        print(f"[sac_mlp] gradient step: {k} {l_d[k]:.6g}: fused_mlp {ek:.3g}, fused {ep:.3g}")
        if not ek <= 4 * ep + 4 * U:
            bad.append((k, ek, ep))
    assert set(g_k) == set(g_d)
    for k, ref in g_d.items():
        assert float(ref.abs().max()) > 0, k
        _bound(f"gradient step: {k}", g_k[k], ref, g_p[k], bad)
    assert not bad, f"(tensor, fused_mlp error, fused error) against fp64: {bad}"


def test_short_run_with_fused_mlp():
    """42 env-steps of SAC(fused_mlp=True).learn, a gradient step after each from the third on."""
    from grasp_lab_salp_amd.vec_env import SalpVecEnv
    m = sac.SAC("MlpPolicy", SalpVecEnv(64, seed=3), learning_starts=128, batch_size=64, buffer_size=512, seed=1,
                fused_mlp=True)
    assert m.fused and m.fused_mlp
    pol = m.policy
    actor0, target0 = pol.actor.flat.clone(), pol.critic_target.flat.clone()
    m.learn(42 * 64)
    torch.cuda.synchronize()
    assert m.num_timesteps == 42 * 64 and m.n_updates == 40 and int(m._update) == 40
    assert all(bool(torch.isfinite(p).all()) for p in pol.parameters()) and bool(torch.isfinite(m.log_ent_coef))
    assert float(m.log_ent_coef.detach()) != 0.0
    assert pol.critic.is_flat() and pol.critic_target.is_flat() and pol.actor.is_flat()
    assert not torch.equal(pol.critic_target.flat, target0) and not torch.equal(pol.critic_target.flat, pol.critic.flat)
    assert not torch.equal(pol.actor.flat, actor0)
    assert m.history and m.history[-1]["n_updates"] == 40 and m.timing["update_s"] > 0
