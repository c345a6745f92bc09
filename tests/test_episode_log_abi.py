"""salp_collect_episodes and salp_episode_window_push_log at the C boundary
without a GPU: the struct's layout in the header, the ctypes mirror and gcc
agree, and every rejection the header lists is SALP_EINVAL with a message
before anything is launched."""
import ctypes
import os
import subprocess

import pytest

from grasp_lab_salp_amd import _abi, _lib
from test_abi import HEADER, ROOT, _header_struct_fields

P = 0x1000   # a pointer that passes validation; a rejected call never dereferences it


@pytest.fixture(scope="module")
def lib():
    from grasp_lab_salp_amd import build
    build.build()
    return _lib.load()


def test_struct_fields_match_header():
    assert _header_struct_fields("SalpEpisodeLog") == [f for f, _ in _lib.SalpEpisodeLog._fields_]


def test_struct_offsets_match_the_c_compiler(tmp_path):
    cls, name = _lib.SalpEpisodeLog, "SalpEpisodeLog"
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / "o.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "salp.h"\nint main(void) {\n'
                   + f'    printf("%zu\\n", sizeof({name}));\n'
                   + "".join(f'    printf("%zu\\n", offsetof({name}, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "o"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]


def _window(**kw):
    w = _lib.SalpEpisodeWindow(window=100, reserved=0, rows=P, count=P)
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def _log(**kw):
    log = _lib.SalpEpisodeLog(per_env=2, rows=P, step=P, count=P)
    for k, v in kw.items():
        setattr(log, k, v)
    return log


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def test_push_log_rejections_before_any_launch(lib):
    name = b"salp_episode_window_push_log: "
    cases = [(None, _log(), 8, P), (_window(window=0), _log(), 8, P),
             (_window(window=_lib.EPWIN_MAX_WINDOW + 1), _log(), 8, P), (_window(rows=None), _log(), 8, P),
             (_window(count=None), _log(), 8, P), (_window(), None, 8, P), (_window(), _log(per_env=0), 8, P),
             (_window(), _log(per_env=-3), 8, P), (_window(), _log(), 0, P), (_window(), _log(), -1, P),
             (_window(), _log(rows=None), 8, P), (_window(), _log(step=None), 8, P),
             (_window(), _log(count=None), 8, P), (_window(), _log(), 8, None)]
    for k, (w, log, n, lost) in enumerate(cases):
        rc = lib.salp_episode_window_push_log(_ref(w), _ref(log), n, lost, None)
        msg = lib.salp_last_error(None) or b""
        assert rc == -1 and msg.startswith(name), (k, rc, msg)


def test_collect_episodes_rejects_a_null_handle(lib):
    """The log's own checks need a handle (a GPU): tests/test_gpu_episode_log.py
    runs them.  Without one the call is refused like salp_collect."""
    r = _lib.SalpPolicyRollout()
    assert lib.salp_collect_episodes(None, ctypes.byref(r), _ref(_log()), None) == -1
    assert b"null handle" in lib.salp_last_error(None)
    assert lib.salp_collect_episodes(None, None, None, None) == -1


def test_abi_is_still_14(lib):
    assert lib.salp_abi_version() == 14 == _abi.ABI_VERSION
    assert "#define SALP_ABI_VERSION 14" in open(HEADER).read()
    assert f"#define SALP_EPWIN_COLS {_lib.EPWIN_COLS}" in open(HEADER).read()
