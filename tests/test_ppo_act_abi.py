"""salp_ppo_mlp_act's C boundary without a GPU: the struct's layout in the
header, the ctypes mirror and gcc agree, and every documented rejection is
SALP_EINVAL with a message before anything is launched."""
import ctypes
import os
import subprocess

import pytest

from grasp_lab_salp_amd import _abi, _lib
from test_abi import HEADER, ROOT, _header_struct_fields

ACTOR = range(0, 7)      # SALP_MLP_PI_W1 .. SALP_MLP_LOG_STD
CRITIC = range(7, 13)    # SALP_MLP_VF_W1 .. SALP_MLP_VAL_B


@pytest.fixture(scope="module")
def lib():
    from grasp_lab_salp_amd import build
    build.build()
    return _lib.load()


def test_struct_fields_match_header():
    assert _header_struct_fields("SalpPpoMlpAct") == [f for f, _ in _lib.SalpPpoMlpAct._fields_]


def test_struct_offsets_match_the_c_compiler(tmp_path):
    cls, name = _lib.SalpPpoMlpAct, "SalpPpoMlpAct"
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / "o.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "salp.h"\nint main(void) {\n'
                   + f'    printf("%zu\\n", sizeof({name}));\n'
                   + "".join(f'    printf("%zu\\n", offsetof({name}, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "o"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    assert _lib.N_MLP_TENSORS == len(ACTOR) + len(CRITIC)


def _args(**kw):
    """A call that passes validation (the pointers are never dereferenced on
    the host, and a rejected or zero-row call launches nothing)."""
    a = _lib.SalpPpoMlpAct(rows=8, obs_dim=10, obs=0x1000, eps=0x1000, action=0x1000, log_prob=0x1000, value=0x1000)
    for t in range(_lib.N_MLP_TENSORS):
        a.params[t] = 0x1000
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rejected(lib, a, word):
    rc = lib.salp_ppo_mlp_act(ctypes.byref(a) if a is not None else None, None)
    msg = lib.salp_last_error(None) or b""
    return rc == -1 and msg.startswith(b"salp_ppo_mlp_act: ") and word in msg, (rc, msg)


def test_rejections_before_any_launch(lib):
    ok, got = _rejected(lib, None, b"null")
    assert ok, got
    for kw, word in (({"rows": -1}, b"rows"), ({"obs_dim": 0}, b"obs_dim"), ({"obs_dim": 15}, b"obs_dim"),
                     ({"obs": None}, b"obs"), ({"action": None, "log_prob": None, "eps": None, "value": None}, b"absent"),
                     ({"action": None, "eps": None}, b"log_prob"), ({"action": None, "log_prob": None}, b"eps")):
        ok, got = _rejected(lib, _args(**kw), word)
        assert ok, (kw, got)
    for t in range(_lib.N_MLP_TENSORS):
        a = _args()
        a.params[t] = None
        ok, got = _rejected(lib, a, b"actor" if t in ACTOR else b"critic")
        assert ok, (t, got)
    # a tensor of an absent network is not needed: these pass validation and, with no rows, launch nothing
    a = _args(rows=0, action=None, log_prob=None, eps=None)
    for t in ACTOR:
        a.params[t] = None
    assert lib.salp_ppo_mlp_act(ctypes.byref(a), None) == 0
    a = _args(rows=0, value=None)
    for t in CRITIC:
        a.params[t] = None
    assert lib.salp_ppo_mlp_act(ctypes.byref(a), None) == 0


def test_zero_rows_is_ok(lib):
    assert lib.salp_ppo_mlp_act(ctypes.byref(_args(rows=0)), None) == 0
    assert lib.salp_ppo_mlp_act(ctypes.byref(_args(rows=0, eps=None, log_prob=None)), None) == 0


def test_abi_is_still_14(lib):
    assert lib.salp_abi_version() == 14 == _abi.ABI_VERSION
    assert "#define SALP_ABI_VERSION 14" in open(HEADER).read()
    assert _abi.OBS_DIM_MAX == 14     # the bound of obs_dim above
