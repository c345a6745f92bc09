"""The SAC part of the C ABI (include/salp.h "SAC", ABI 14): the ctypes
mirrors of its structs against the header's field order and gcc's layout, the
version in the three places that state it, and argument checks that return
before any launch (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import pytest

from grasp_lab_salp_amd import _abi, _lib, sac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "salp.h")
STRUCTS = [("SalpReplay", _lib.SalpReplay), ("SalpReplayAdd", _lib.SalpReplayAdd),
           ("SalpReplaySample", _lib.SalpReplaySample), ("SalpSacTd", _lib.SalpSacTd), ("SalpSacPi", _lib.SalpSacPi)]
FUNCTIONS = ["salp_replay_add", "salp_replay_sample", "salp_sac_actor_head_forward", "salp_sac_actor_head_backward",
             "salp_sac_td_head", "salp_sac_pi_head", "salp_sac_polyak"]


@pytest.fixture(scope="module")
def lib():
    from grasp_lab_salp_amd import build
    build.build()
    return _lib.load()


def _header_fields(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", text, flags=re.S).group(1)
    return [re.findall(r"(\w+)\s*$", d.strip())[0] for d in body.split(";") if d.strip()]


@pytest.mark.parametrize("name,cls", STRUCTS)
def test_struct_mirrors_match_header_and_compiler(name, cls, tmp_path):
    fields = [f for f, _ in cls._fields_]
    assert _header_fields(name) == fields
    src = tmp_path / "o.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "salp.h"\nint main(void) {\n'
                   + f'    printf("%zu\\n", sizeof({name}));\n'
                   + "".join(f'    printf("%zu\\n", offsetof({name}, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "o"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields], name


def test_abi_is_14_everywhere(lib):
    assert _abi.ABI_VERSION == 14
    assert "#define SALP_ABI_VERSION 14" in open(HEADER).read()
    assert lib.salp_abi_version() == 14


def test_constants_match_header():
    text = open(HEADER).read()
    assert f"#define SALP_SAC_WORKSPACE_DOUBLES {_lib.SAC_WORKSPACE_DOUBLES}" in text
    assert f"0x{sac.REPLAY_STREAM:08X}" in text


def test_entry_points_are_bound_and_reject_bad_arguments(lib):
    for f in FUNCTIONS:
        assert f in _lib.SIGNATURES and hasattr(lib, f), f
    rb = _lib.SalpReplay()   # all zero
    assert lib.salp_replay_add(ctypes.byref(rb), None, None) == -1
    assert b"salp_replay_add" in lib.salp_last_error(None)
    assert lib.salp_replay_sample(None, None, None) == -1
    assert lib.salp_sac_actor_head_forward(0, None, None, None, None, None, None) == -1
    assert lib.salp_sac_actor_head_backward(4, None, None, None, None, None, None, None, None) == -1
    assert lib.salp_sac_td_head(None, None) == -1
    assert lib.salp_sac_pi_head(ctypes.byref(_lib.SalpSacPi(batch=4)), None) == -1
    assert lib.salp_sac_polyak(0, None, None, 0.005, None) == -1
