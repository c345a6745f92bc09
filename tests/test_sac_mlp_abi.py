"""The fused SAC networks' part of the C ABI (include/salp.h "SAC",
salp_sac_net_*, added under ABI 14): the ctypes mirrors against the header's
field order and gcc's layout, the flat parameter layout, argument checks that
return before any launch, the actor's flat parameters and the keyword's
refusals.  No GPU needed."""
import copy
import ctypes
import os
import re
import subprocess

import pytest
import torch

from grasp_lab_salp_amd import _abi, _lib, sac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "salp.h")
STRUCTS = [("SalpSacNetForward", _lib.SalpSacNetForward), ("SalpSacNetBackward", _lib.SalpSacNetBackward)]
FUNCTIONS = ["salp_sac_net_num_params", "salp_sac_net_offset", "salp_sac_net_workspace_floats",
             "salp_sac_net_tile_rows", "salp_sac_net_max_blocks", "salp_sac_net_forward", "salp_sac_net_backward"]


@pytest.fixture(scope="module")
def lib():
    from grasp_lab_salp_amd import build
    build.build()
    return _lib.load()


def _header_fields(name):
    """(field, array length or None) in the header's order (the method of test_sac_abi.py, with array fields)."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", text, flags=re.S).group(1)
    out = []
    for d in body.split(";"):
        if d.strip():
            f, n = re.findall(r"(\w+)\s*(?:\[(\d+)\])?\s*$", d.strip())[0]
            out.append((f, int(n) if n else None))
    return out


@pytest.mark.parametrize("name,cls", STRUCTS)
def test_struct_mirrors_match_header_and_compiler(name, cls, tmp_path):
    fields = [f for f, _ in cls._fields_]
    hdr = _header_fields(name)
    assert [f for f, _ in hdr] == fields
    for (f, n), (_, ct) in zip(hdr, cls._fields_):
        assert (n is None) == (not issubclass(ct, ctypes.Array)), f
        if n:
            assert ct._length_ == n == _lib.SAC_NET_MAX_NETS, f
    src = tmp_path / "o.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "salp.h"\nint main(void) {\n'
                   + f'    printf("%zu\\n", sizeof({name}));\n'
                   + "".join(f'    printf("%zu\\n", offsetof({name}, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "o"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields], name


def test_constants_match_header():
    text = open(HEADER).read()
    for macro, value in (("SALP_SAC_HIDDEN", _lib.SAC_HIDDEN), ("SALP_SAC_NET_IN_MAX", _lib.SAC_NET_IN_MAX),
                         ("SALP_SAC_NET_OUT_MAX", _lib.SAC_NET_OUT_MAX),
                         ("SALP_SAC_NET_MAX_NETS", _lib.SAC_NET_MAX_NETS)):
        assert f"#define {macro} {value}\n" in text, macro
    enum = re.search(r"typedef enum SalpSacNetTensor\s*\{(.*?)\}", re.sub(r"/\*.*?\*/", "", text, flags=re.S),
                     flags=re.S).group(1)
    names = [e.split("=")[0].strip() for e in enum.split(",") if e.strip()]
    assert names.index("SALP_SAC_NET_N_TENSORS") == _lib.SAC_NET_N_TENSORS == 6


def test_abi_is_still_14(lib):
    assert _abi.ABI_VERSION == 14 and lib.salp_abi_version() == 14
    assert "#define SALP_ABI_VERSION 14" in open(HEADER).read()


@pytest.mark.parametrize("d_in,d_out", [(6, 6), (14, 6), (9, 1), (17, 1)])
def test_flat_layout_is_the_torch_linear_sizes_back_to_back(lib, d_in, d_out):
    sizes = [256 * d_in, 256, 256 * 256, 256, d_out * 256, d_out]
    offs = [lib.salp_sac_net_offset(d_in, d_out, t) for t in range(7)]
    assert offs == [sum(sizes[:t]) for t in range(7)]
    assert lib.salp_sac_net_num_params(d_in, d_out) == sum(sizes)
    net = torch.nn.Sequential(torch.nn.Linear(d_in, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(),
                              torch.nn.Linear(256, d_out))
    assert [p.numel() for p in net.parameters()] == sizes


def test_layout_and_geometry_queries_reject_bad_arguments(lib):
    assert lib.salp_sac_net_num_params(18, 1) == -1 and lib.salp_sac_net_offset(18, 1, 0) == -1
    assert b"salp_sac_net_offset" in lib.salp_last_error(None)
    assert lib.salp_sac_net_num_params(0, 1) == -1 and lib.salp_sac_net_num_params(9, 7) == -1
    assert lib.salp_sac_net_num_params(9, 0) == -1 and lib.salp_sac_net_offset(9, 1, 7) == -1
    assert lib.salp_sac_net_offset(9, 1, -1) == -1
    tr, mb = lib.salp_sac_net_tile_rows(), lib.salp_sac_net_max_blocks()
    assert tr > 0 and 0 < mb <= 64
    P = lib.salp_sac_net_num_params(13, 1)
    # one partial per block and network, then the networks' dx1: blocks = min(tiles, max_blocks)
    for B in (1, tr, tr + 1, tr * mb, tr * mb + 1, 100 * tr * mb):
        nb = min(-(-B // tr), mb)
        assert lib.salp_sac_net_workspace_floats(B, 10, 3, 1, 2) == 2 * nb * P + 2 * B * 3, B
    assert lib.salp_sac_net_workspace_floats(64, 10, 0, 6, 1) == 2 * lib.salp_sac_net_num_params(10, 6)
    assert nb * P <= 64 * 70_000      # the partial traffic per network is bounded
    for bad in ((0, 10, 3, 1, 2), (64, 15, 3, 1, 2), (64, 10, 3, 1, 5), (64, 10, 3, 1, 0), (64, 0, 3, 1, 1),
                (64, 10, -1, 1, 1), (64, 10, 3, 7, 1)):
        assert lib.salp_sac_net_workspace_floats(*bad) == -1, bad
    assert b"salp_sac_net_workspace_floats" in lib.salp_last_error(None)


def _fwd(**kw):
    """A forward argument block whose pointers are all non-NULL (never dereferenced: the checks come first)."""
    f = _lib.SalpSacNetForward(batch=64, d0=10, d1=3, out_dim=1, n_nets=2)
    for name in ("params", "x0", "x1", "out", "h1", "h2"):
        for i in range(4):
            getattr(f, name)[i] = 4096
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(f, k)[v[0]] = v[1]
        else:
            setattr(f, k, v)
    return f


def _bwd(**kw):
    b = _lib.SalpSacNetBackward(batch=64, d0=10, d1=3, out_dim=1, n_nets=2, dx1=4096, workspace=4096)
    for name in ("params", "x0", "x1", "h1", "h2", "dout", "dparams"):
        for i in range(4):
            getattr(b, name)[i] = 4096
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(b, k)[v[0]] = v[1]
        else:
            setattr(b, k, v)
    return b


def test_entry_points_are_bound_and_reject_bad_arguments(lib):
    for f in FUNCTIONS:
        assert f in _lib.SIGNATURES and hasattr(lib, f), f
    assert lib.salp_sac_net_forward(None, None) == -1
    assert b"salp_sac_net_forward" in lib.salp_last_error(None)
    for kw in (dict(batch=0), dict(batch=-3), dict(batch=1 << 31), dict(n_nets=5), dict(n_nets=0), dict(d0=0),
               dict(d0=15), dict(d1=-1), dict(out_dim=0), dict(out_dim=7), dict(params=(1, None)),
               dict(x0=(0, None)), dict(x1=(1, None)), dict(out=(1, None)), dict(h1=(0, None)), dict(h2=(1, None))):
        lib.salp_sac_polyak(0, None, None, 0.5, None)       # another function's message in between
        assert lib.salp_sac_net_forward(ctypes.byref(_fwd(**kw)), None) == -1, kw
        assert b"salp_sac_net_forward" in lib.salp_last_error(None), kw
    assert lib.salp_sac_net_backward(None, None) == -1
    assert b"salp_sac_net_backward" in lib.salp_last_error(None)
    for kw in (dict(batch=0), dict(n_nets=5), dict(d0=15), dict(out_dim=7), dict(params=(0, None)),
               dict(x0=(1, None)), dict(x1=(0, None)), dict(h1=(1, None)), dict(h2=(0, None)), dict(dout=(1, None)),
               dict(dparams=(1, None)), dict(dparams=(0, None)), dict(workspace=None),
               dict(d0=13, d1=0)):                         # dx1 without action columns
        lib.salp_sac_polyak(0, None, None, 0.5, None)
        assert lib.salp_sac_net_backward(ctypes.byref(_bwd(**kw)), None) == -1, kw
        assert b"salp_sac_net_backward" in lib.salp_last_error(None), kw
    nothing = _bwd(dx1=None)
    for i in range(4):
        nothing.dparams[i] = None
    assert lib.salp_sac_net_backward(ctypes.byref(nothing), None) == -1
    assert b"neither" in lib.salp_last_error(None)


@pytest.mark.parametrize("obs_dim", [6, 14])
def test_actor_flatten(lib, obs_dim):
    torch.manual_seed(obs_dim)
    actor = sac._Actor(obs_dim, 3, (256, 256))
    before = {k: v.clone() for k, v in actor.state_dict().items()}
    x = torch.randn(5, obs_dim)
    y0 = [t.clone() for t in actor(x)]
    assert not actor.is_flat()
    assert actor.flatten_() is actor and actor.is_flat()
    assert all(torch.equal(v, before[k]) for k, v in actor.state_dict().items()) and len(before) == 8
    assert all(torch.equal(a, b) for a, b in zip(actor(x), y0))
    off = [lib.salp_sac_net_offset(obs_dim, 6, t) for t in range(7)]
    assert actor.flat.numel() == off[6]
    head = actor.flat[off[4]:off[5]].view(6, 256)
    assert torch.equal(head[:3], actor.mu.weight) and torch.equal(head[3:], actor.log_std.weight)
    assert head.data_ptr() == actor.mu.weight.data_ptr()
    bias = actor.flat[off[5]:off[6]]
    assert torch.equal(bias[:3], actor.mu.bias) and torch.equal(bias[3:], actor.log_std.bias)
    assert torch.equal(actor.flat[:off[1]].view(256, obs_dim), actor.latent_pi[0].weight)
    assert torch.equal(actor.flat[off[2]:off[3]].view(256, 256), actor.latent_pi[2].weight)
    # the parameters are the buffer: a step on one shows in the other
    with torch.no_grad():
        actor.log_std.bias += 1.0
    assert torch.equal(actor.flat[off[5] + 3:], before["log_std.bias"] + 1.0)
    d = copy.deepcopy(actor).double()
    mu, ls = d(x.double())
    assert mu.dtype == torch.float64 and mu.shape == ls.shape == (5, 3)
    assert torch.allclose(mu.float(), y0[0], atol=1e-5)
    moved = copy.deepcopy(actor)
    assert moved.flatten_().is_flat() and torch.equal(moved.flat, actor.flat)


def test_policy_flattens_the_actor_and_keeps_its_sizes():
    pol = sac.SACPolicy(10)
    assert pol.actor.is_flat() and pol.critic.is_flat() and pol.critic_target.is_flat()
    assert pol.hidden == (256, 256)
    assert [p.data_ptr() for net in pol.critic.net_params() for p in net] == \
        [p.data_ptr() for p in pol.critic.parameters()]


class _CpuSim:
    device, n_envs, obs_dim = "cpu", 4, 10


def test_fused_mlp_refusals():
    with pytest.raises(ValueError, match="GPU"):
        sac.SAC("MlpPolicy", _CpuSim(), fused_mlp=True)
    assert sac.SAC("MlpPolicy", _CpuSim()).fused_mlp is False
    pol = sac.SACPolicy(10)
    small = sac.SACPolicy(10, hidden=(64, 64))
    with pytest.raises(ValueError, match="fused=True"):
        sac._check_fused_mlp(pol, False, "cuda")
    with pytest.raises(ValueError, match="GPU"):
        sac._check_fused_mlp(pol, True, "cpu")
    with pytest.raises(ValueError, match="256"):
        sac._check_fused_mlp(small, True, "cuda")
    sac._check_fused_mlp(pol, True, "cuda")
    batch = (torch.zeros(4, 10), torch.zeros(4, 3), torch.zeros(4, 10), torch.zeros(4), torch.zeros(4))
    la = torch.zeros(1, requires_grad=True)
    with pytest.raises(ValueError):
        sac.critic_phase(pol, la, batch, torch.zeros(4, 3), torch.zeros(4, 3), 0.99, -3.0, False, fused_mlp=True)
    with pytest.raises(ValueError):
        sac.actor_phase(pol, {"obs": batch[0]}, False, fused_mlp=True)
