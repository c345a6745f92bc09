"""The LSTM cell kernels k_lstm_fwd / k_lstm_bwd (csrc/salp_lstm.hip) through
their four C entry points, salp_lstm_cell_forward / _backward and
salp_lstm_step_forward / _backward, called directly with every output between
canary blocks and filled with NaN before the call.

Reference: the equations of the file header in float64 on the CPU,
    i, f, o = sigmoid, g = tanh of the gate pre-activations G (+ GX),
    c = f (c_prev keep) + i g,  h = o tanh(c),  hk_next = h keep_next,
backward by float64 autograd of these with respect to the gates and c_prev
given dh = d_out (+ dhk_next keep_next) and dc.  The backward kernels get the
forward kernel's own act and c, as the learner passes them.

Bound: per tensor, the largest error over the reference's
largest magnitude is at most 4 x the same figure of the float32 torch path (the
CPU branch of recurrent_ppo.lstm_cell, run on the GPU under autograd) plus 4 u,
u = 2^-24.  Shapes (rows, H): 255 elements (one short of a 256-thread block),
256 exactly, one unit per row, the learner's default H = 256 below and over a
block edge, and the old test's (300, 64).  Lines starting with "[lstm_cell]"
(pytest -s) print the figures."""
import ctypes

import pytest
import torch

from grasp_lab_salp_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAD, SENTINEL = 7, 12345.0
EINVAL = -1                      # include/salp.h SALP_EINVAL
SHAPES = [(1, 1), (1, 64), (5, 51), (4, 64), (257, 1), (3, 256), (33, 256), (300, 64)]
CASES = [(m, H, "mixed") for m, H in SHAPES] + [(33, 256, "zeros"), (33, 256, "ones")]


class _Guarded:
    """A NaN-filled float32 tensor between two canary blocks."""

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


def _p(t):
    return ctypes.c_void_p(0 if t is None else (t.t if isinstance(t, _Guarded) else t).data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _written(out):
    for name, g in out.items():
        assert g.intact(), name
        assert bool(torch.isfinite(g.t).all()), name            # every element was written
    return {k: g.t for k, g in out.items()}


def _forward(G, c_prev, keep, gx=None, keep_next=None, step=True, rc=0):
    m, H = c_prev.shape
    out = {"h": _Guarded(m, H), "c": _Guarded(m, H), "act": _Guarded(m, 4 * H)}
    lib = _lib.load()
    if step:
        if keep_next is not None:
            out["hk"] = _Guarded(m, H)
        got = lib.salp_lstm_step_forward(m, H, _p(G), _p(gx), _p(c_prev), _p(keep), _p(keep_next), _p(out["h"]),
                                         _p(out["c"]), _p(out["act"]), _p(out.get("hk")), _stream())
    else:
        assert gx is None and keep_next is None
        got = lib.salp_lstm_cell_forward(m, H, _p(G), _p(c_prev), _p(keep), _p(out["h"]), _p(out["c"]),
                                         _p(out["act"]), _stream())
    torch.cuda.synchronize()
    assert got == rc
    return _written(out)


def _backward(fwd, c_prev, keep, d_out, dc=None, dhk_next=None, keep_next=None, step=True):
    m, H = c_prev.shape
    out = {"dG": _Guarded(m, 4 * H), "dc_prev": _Guarded(m, H)}
    lib = _lib.load()
    if step:
        got = lib.salp_lstm_step_backward(m, H, _p(fwd["act"]), _p(c_prev), _p(keep), _p(fwd["c"]), _p(d_out),
                                          _p(dhk_next), _p(keep_next), _p(dc), _p(out["dG"]), _p(out["dc_prev"]),
                                          _stream())
    else:
        assert dhk_next is None and keep_next is None
        got = lib.salp_lstm_cell_backward(m, H, _p(fwd["act"]), _p(c_prev), _p(keep), _p(fwd["c"]), _p(d_out), _p(dc),
                                          _p(out["dG"]), _p(out["dc_prev"]), _stream())
    torch.cuda.synchronize()
    assert got == 0
    return _written(out)


def _equations(x, gx, dc, dhk_next, dtype, device):
    """The header's equations under autograd in `dtype` on `device`: h, c, act, hk, dG, dc_prev."""
    t = lambda a: a.to(device=device, dtype=dtype)  # noqa: E731
    g = (t(x["G"]) + t(x["GX"]) if gx else t(x["G"])).requires_grad_(True)
    cp = t(x["c_prev"]).requires_grad_(True)
    i, f, gg, o = g.chunk(4, 1)
    c = torch.sigmoid(f) * (cp * t(x["keep"]).unsqueeze(1)) + torch.sigmoid(i) * torch.tanh(gg)
    h = torch.sigmoid(o) * torch.tanh(c)
    dh = t(x["d_out"])
    if dhk_next:
        dh = dh + t(x["dhk_next"]) * t(x["keep_next"]).unsqueeze(1)
    dcn = t(x["dc"]) if dc else torch.zeros_like(c)
    dG, dcp = torch.autograd.grad((h * dh).sum() + (c * dcn).sum(), (g, cp))
    act = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)], 1)
    out = {"h": h, "c": c, "act": act, "dG": dG, "dc_prev": dcp}
    if "keep_next" in x:
        out["hk"] = h * t(x["keep_next"]).unsqueeze(1)
    return {k: v.detach() for k, v in out.items()}


def _inputs(m, H, keep_mode):
    g = torch.Generator().manual_seed(1000 * m + H)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    keeps = {"mixed": lambda: (torch.rand(m, generator=g) < 0.5).float(), "zeros": lambda: torch.zeros(m),
             "ones": lambda: torch.ones(m)}
    return {"G": 1.5 * r(m, 4 * H), "GX": r(m, 4 * H), "c_prev": r(m, H), "keep": keeps[keep_mode](),
            "keep_next": (torch.rand(m, generator=g) < 0.5).float(), "d_out": r(m, H), "dhk_next": r(m, H),
            "dc": r(m, H)}


def _rel(x, ref64):
    scale = float(ref64.abs().max())
    if scale == 0.0:                      # (dc_prev with keep all 0): nothing but exact zeros will do
        return 0.0 if bool((x == 0).all()) else float("inf")
    return float((x.double().cpu() - ref64).abs().max()) / scale


def _check(tag, x, got, names, **variant):
    ref = _equations(x, dtype=torch.float64, device="cpu", **variant)
    t32 = _equations(x, dtype=torch.float32, device="cuda", **variant)
    for name in names:
        e_k, e_t = _rel(got[name], ref[name]), _rel(t32[name], ref[name])
        print(f"[lstm_cell] {tag} {name}: kernel {e_k:.3e} torch f32 {e_t:.3e} (bound {4 * e_t + 4 * U:.3e})")
        assert e_k <= 4 * e_t + 4 * U, (tag, name, e_k, e_t)


def _same_bits(a, b, names):
    for name in names:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name


FWD, BWD = ("h", "c", "act"), ("dG", "dc_prev")


@pytest.mark.parametrize("m,H,keep_mode", CASES)
def test_cell_and_step_equal_fp64(m, H, keep_mode):
    x = _inputs(m, H, keep_mode)
    d = {k: v.cuda() for k, v in x.items()}
    tag = f"({m}, {H}) keep {keep_mode}"
    G, GX, cp, keep, kn = d["G"], d["GX"], d["c_prev"], d["keep"], d["keep_next"]
    off = keep == 0

    # ---- forward: the cell, and the step with each option absent and present
    cell = _forward(G, cp, keep, step=False)
    _check(tag + " cell", x, cell, FWD, gx=False, dc=True, dhk_next=False)
    _same_bits(cell, _forward(G, cp, keep), FWD)                       # the step without options is the cell
    step = _forward(G, cp, keep, gx=GX, keep_next=kn)
    _check(tag + " step gx keep_next", x, step, FWD + ("hk",), gx=True, dc=True, dhk_next=False)
    _same_bits(step, _forward(G, cp, keep, gx=GX), FWD)
    only_kn = _forward(G, cp, keep, keep_next=kn)
    _same_bits(only_kn, cell, FWD)
    assert torch.equal(only_kn["hk"], cell["h"] * kn[:, None]) and torch.equal(step["hk"], step["h"] * kn[:, None])
    for f in (cell, step):
        i, _, g, _ = f["act"].chunk(4, 1)
        assert torch.equal(f["c"][off], (i * g)[off])                  # keep == 0: c is i g to the bit

    # ---- backward on the forward kernel's own act and c
    zeros = torch.zeros_like(cp)
    for name, f, step_args, variant in (
            ("cell", cell, {}, dict(gx=False, dhk_next=False)),
            ("step gx keep_next", step, dict(dhk_next=d["dhk_next"], keep_next=kn), dict(gx=True, dhk_next=True))):
        is_step = bool(step_args)
        with_dc = _backward(f, cp, keep, d["d_out"], dc=d["dc"], step=is_step, **step_args)
        _check(f"{tag} {name} dc", x, with_dc, BWD, dc=True, **variant)
        no_dc = _backward(f, cp, keep, d["d_out"], dc=None, step=is_step, **step_args)
        _check(f"{tag} {name} dc NULL", x, no_dc, BWD, dc=False, **variant)
        _same_bits(no_dc, _backward(f, cp, keep, d["d_out"], dc=zeros, step=is_step, **step_args), BWD)
        for b in (with_dc, no_dc):                                     # keep == 0: nothing reaches c_prev or f
            assert bool((b["dc_prev"][off] == 0).all()) and bool((b["dG"][:, H:2 * H][off] == 0).all())
            assert bool((b["dG"][:, :H] != 0).any())
    # the step without options is the cell; with dhk_next alone it is the step on the cell's act
    _same_bits(_backward(cell, cp, keep, d["d_out"], dc=d["dc"]), _backward(cell, cp, keep, d["d_out"], dc=d["dc"],
                                                                           step=False), BWD)
    plain = _backward(cell, cp, keep, d["d_out"], dc=d["dc"], dhk_next=d["dhk_next"], keep_next=kn)
    _check(tag + " cell act, dhk_next", x, plain, BWD, gx=False, dc=True, dhk_next=True)


def test_saturated_gates():
    """Gate columns at +-20, +-88, +-100 and +-1e4 (row r holds value r in gate
    u % 4 of unit u, generic values elsewhere): everything finite; at +-1e4 the
    activation is exactly 0 or 1 (-1 or 1 for g) and its dG exactly 0."""
    vals = [20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4]
    m, H = len(vals), 8
    g = torch.Generator().manual_seed(9)
    G = torch.randn(m, 4 * H, generator=g)
    sat = torch.zeros(m, 4 * H, dtype=torch.bool)
    for r, v in enumerate(vals):
        for u in range(H):
            G[r, (u % 4) * H + u] = v
            sat[r, (u % 4) * H + u] = True
    G, sat = G.cuda(), sat.cuda()
    cp, dh, dc = (torch.randn(m, H, generator=g).cuda() for _ in range(3))
    keep = torch.ones(m, device="cuda")
    f = _forward(G, cp, keep, step=False)                     # (_written: finite)
    b = _backward(f, cp, keep, dh, dc=dc, step=False)
    is_g = torch.zeros(4 * H, dtype=torch.bool, device="cuda")
    is_g[2 * H:3 * H] = True
    for r in (6, 7):
        a, s = f["act"][r], sat[r]
        want = torch.where(is_g, torch.full_like(a, -1.0 if r == 7 else 1.0), torch.full_like(a, 0.0 if r == 7 else 1.0))
        assert torch.equal(a[s], want[s])
        assert bool((b["dG"][r][s] == 0).all())
    assert bool((b["dG"][~sat] != 0).any())


def test_rejections_launch_nothing():
    """SALP_EINVAL, and no output written: keep_next without hk_next, hk_next
    without keep_next, dhk_next without keep_next, hidden = 0 in all four."""
    m, H = 4, 8
    lib = _lib.load()
    t = lambda *s: torch.randn(*s, device="cuda")  # noqa: E731
    G, cp, keep, kn, act, c, dh = t(m, 4 * H), t(m, H), torch.ones(m, device="cuda"), torch.ones(m, device="cuda"), \
        t(m, 4 * H), t(m, H), t(m, H)
    o = {k: _Guarded(m, H) for k in ("h", "c", "hk", "dc_prev")}
    o["act"], o["dG"] = _Guarded(m, 4 * H), _Guarded(m, 4 * H)
    st = _stream()
    fwd_out = (_p(o["h"]), _p(o["c"]), _p(o["act"]))
    calls = [
        lib.salp_lstm_step_forward(m, H, _p(G), None, _p(cp), _p(keep), _p(kn), *fwd_out, None, st),
        lib.salp_lstm_step_forward(m, H, _p(G), None, _p(cp), _p(keep), None, *fwd_out, _p(o["hk"]), st),
        lib.salp_lstm_step_backward(m, H, _p(act), _p(cp), _p(keep), _p(c), _p(dh), _p(dh), None, None, _p(o["dG"]),
                                    _p(o["dc_prev"]), st),
        lib.salp_lstm_cell_forward(m, 0, _p(G), _p(cp), _p(keep), *fwd_out, st),
        lib.salp_lstm_step_forward(m, 0, _p(G), None, _p(cp), _p(keep), _p(kn), *fwd_out, _p(o["hk"]), st),
        lib.salp_lstm_cell_backward(m, 0, _p(act), _p(cp), _p(keep), _p(c), _p(dh), None, _p(o["dG"]),
                                    _p(o["dc_prev"]), st),
        lib.salp_lstm_step_backward(m, 0, _p(act), _p(cp), _p(keep), _p(c), _p(dh), None, None, None, _p(o["dG"]),
                                    _p(o["dc_prev"]), st),
    ]
    torch.cuda.synchronize()
    assert calls == [EINVAL] * len(calls)
    assert all(g.untouched() for g in o.values())
