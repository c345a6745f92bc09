"""The episode-metrics part of the C ABI (include/salp.h "Episode metrics and
evaluation"): the ctypes mirrors of its structs against the header's field
order and gcc's layout, its constants, and argument checks that return before
any launch (no GPU needed).  The ABI number does not move for these entry
points: they are recognised by their symbols."""
import ctypes
import os
import re
import subprocess

import pytest

from grasp_lab_salp_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "salp.h")
STRUCTS = [("SalpEpisodeWindow", _lib.SalpEpisodeWindow), ("SalpEpisodePush", _lib.SalpEpisodePush),
           ("SalpEvalState", _lib.SalpEvalState)]
FUNCTIONS = ["salp_episode_window_push", "salp_episode_window_summary", "salp_eval_account"]


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


def test_constants_match_header(tmp_path):
    assert (_lib.EPWIN_COLS, _lib.EPWIN_MAX_WINDOW, _lib.EPSUM_DIM) == (20, 1024, 84)
    text = open(HEADER).read()
    assert "#define SALP_EPWIN_COLS 20" in text and "#define SALP_EPWIN_MAX_WINDOW 1024" in text
    assert "#define SALP_EPSUM_DIM 84" in text
    # the row's info columns are the header's enum range, and Python's names for it
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include "salp.h"\nint main(void) {\n    printf("%d %d %d %d\\n", '
                   "(int)SALP_INFO_PATH_LENGTH, (int)SALP_INFO_AVG_R_OBSTACLE, (int)SALP_INFO_EP_RETURN, "
                   "(int)SALP_INFO_EP_LEN);\n    return 0;\n}\n")
    exe = tmp_path / "c"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [_abi.INFO["path_length"], _abi.INFO["avg_rewards_obstacle"], _abi.INFO["ep_return"],
                   _abi.INFO["ep_len"]]
    assert got[1] - got[0] + 1 + 4 == _lib.EPWIN_COLS


def test_abi_number_did_not_move(lib):
    assert _abi.ABI_VERSION == 14 and lib.salp_abi_version() == 14


def _good():
    """Structs whose pointers are non-NULL (never dereferenced: each call below fails a check first)."""
    p = ctypes.c_void_p(64)
    win = _lib.SalpEpisodeWindow(100, 0, p, p)
    push = _lib.SalpEpisodePush(8, p, p, p, None)
    st = _lib.SalpEvalState(8, p, p, p, p, p, p, p)
    return win, push, st


def test_entry_points_are_bound_and_reject_bad_arguments(lib):
    for f in FUNCTIONS:
        assert f in _lib.SIGNATURES and hasattr(lib, f), f
    B = ctypes.byref
    out = ctypes.c_void_p(64)

    def bad(rc, name):
        assert rc == -1 and name.encode() in lib.salp_last_error(None), name

    win, push, st = _good()
    bad(lib.salp_episode_window_push(None, B(push), None), "salp_episode_window_push")
    bad(lib.salp_episode_window_push(B(win), None, None), "salp_episode_window_push")
    bad(lib.salp_episode_window_summary(None, out, None), "salp_episode_window_summary")
    bad(lib.salp_episode_window_summary(B(win), None, None), "salp_episode_window_summary")
    bad(lib.salp_eval_account(None, B(push), None), "salp_eval_account")
    bad(lib.salp_eval_account(B(st), None, None), "salp_eval_account")
    for w in (0, -1, 1025):
        win, push, _ = _good()
        win.window = w
        bad(lib.salp_episode_window_push(B(win), B(push), None), "salp_episode_window_push")
        bad(lib.salp_episode_window_summary(B(win), out, None), "salp_episode_window_summary")
    for field in ("rows", "count"):
        win, push, _ = _good()
        setattr(win, field, None)
        bad(lib.salp_episode_window_push(B(win), B(push), None), "salp_episode_window_push")
        bad(lib.salp_episode_window_summary(B(win), out, None), "salp_episode_window_summary")
    for n in (0, -3):
        win, push, st = _good()
        push.n_envs = n
        bad(lib.salp_episode_window_push(B(win), B(push), None), "salp_episode_window_push")
        bad(lib.salp_eval_account(B(st), B(push), None), "salp_eval_account")
        st.n_envs = n
        bad(lib.salp_eval_account(B(st), B(push), None), "salp_eval_account")
    for field in ("info", "terminated", "truncated"):
        win, push, st = _good()
        setattr(push, field, None)
        bad(lib.salp_episode_window_push(B(win), B(push), None), "salp_episode_window_push")
        bad(lib.salp_eval_account(B(st), B(push), None), "salp_eval_account")
    for field in ("target", "offset", "done_count", "ep_return", "ep_len", "success", "remaining"):
        win, push, st = _good()
        setattr(st, field, None)
        bad(lib.salp_eval_account(B(st), B(push), None), "salp_eval_account")
    win, push, st = _good()
    push.n_envs = 9                      # a step of another size than the state
    bad(lib.salp_eval_account(B(st), B(push), None), "salp_eval_account")
