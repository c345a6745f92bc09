"""The kernel fingerprint covers the device functions the kernel calls
(grasp_lab_salp_amd/_codeobj.py): k_rollout's tick loops are a separate
function (wave_ticks), so a fingerprint of the kernel symbol alone would not
move when they change.  On a copy of the built library: an edited byte of the
callee moves the fingerprint; the callee moved to another address of the code
object (symbol and the caller's PC-relative literals updated) does not; a
kernel that calls nothing hashes as before.  CPU only."""
import struct

import pytest

from grasp_lab_salp_amd import _codeobj

CALLEE = "wave_ticksILb0E"


@pytest.fixture(scope="module")
def lib():
    from grasp_lab_salp_amd import build
    return build.build()


def _rollout_object(lib):
    """(library bytes, offset of k_rollout<false, false>'s code object in them, the code object)."""
    blob = open(lib, "rb").read()
    for _ident, co in _codeobj._code_objects(blob):
        if any(_codeobj.ROLLOUT_KERNEL in n for n in _codeobj._symbols(co)):
            return bytearray(blob), blob.index(co), co
    raise AssertionError("k_rollout<false, false> not found")


def _by_name(co, fragment):
    hits = [(addr, off, size) for addr, (n, off, size) in _codeobj._functions(co).items() if fragment in n]
    assert len(hits) == 1, (fragment, hits)
    return hits[0]


def test_kernel_calls_the_tick_function(lib):
    _blob, _base, co = _rollout_object(lib)
    funcs = _codeobj._functions(co)
    k_addr, _off, _size = _by_name(co, _codeobj.ROLLOUT_KERNEL)
    names = [n for n, _o, _s in _codeobj._callees(co, k_addr, funcs)]
    assert any(CALLEE in n for n in names), names
    # the split collection kernel calls nothing: its fingerprint is the kernel symbol's alone
    s_addr, _off, _size = _by_name(co, _codeobj.SPLIT_COLLECT_KERNEL)
    assert _codeobj._callees(co, s_addr, funcs) == []


def test_editing_the_callee_moves_the_fingerprint(lib, tmp_path):
    blob, base, co = _rollout_object(lib)
    before = _codeobj.kernel_sha(lib, _codeobj.ROLLOUT_KERNEL)
    split = _codeobj.kernel_sha(lib, _codeobj.SPLIT_COLLECT_KERNEL)
    _addr, off, size = _by_name(co, CALLEE)
    blob[base + off + size // 2] ^= 0x01   # one bit in the middle of the callee, outside the kernel symbol
    edited = tmp_path / "libsalp_edited.so"
    edited.write_bytes(bytes(blob))
    assert _codeobj.kernel_sha(str(edited), _codeobj.ROLLOUT_KERNEL) not in (None, before)
    assert _codeobj.kernel_sha(str(edited), _codeobj.SPLIT_COLLECT_KERNEL) == split


def _symtab_value_offset(co, address, size):
    """File offset (in the code object) of st_value of the function symbol at `address`."""
    shoff, = struct.unpack_from("<Q", co, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", co, 0x3A)
    for k in range(shnum):
        (_n, sh_type, _f, _a, off, ssize, _l, _i, _al, entsize) = struct.unpack_from("<IIQQQQIIQQ", co,
                                                                                      shoff + k * shentsize)
        if sh_type != 2:
            continue
        for j in range(ssize // entsize):
            _st_name, info, _o, _shndx, value, sz = struct.unpack_from("<IBBHQQ", co, off + j * entsize)
            if (info & 0xF) == 2 and value == address and sz == size:
                return off + j * entsize + 8
    raise AssertionError("symbol not found")


def test_moving_the_callee_keeps_the_fingerprint(lib, tmp_path):
    blob, base, co = _rollout_object(lib)
    before = _codeobj.kernel_sha(lib, _codeobj.ROLLOUT_KERNEL)
    funcs = _codeobj._functions(co)
    k_addr, k_off, k_size = _by_name(co, _codeobj.ROLLOUT_KERNEL)
    c_addr, c_off, c_size = _by_name(co, CALLEE)
    reach = {o for _n, o, _s in _codeobj._callees(co, k_addr, funcs)} | {k_off}
    # a function outside the kernel's call graph, large enough to hold the callee: its bytes are the new home
    victims = [(a, o, s) for a, (_n, o, s) in funcs.items() if o not in reach and s >= c_size]
    assert victims, "no function large enough to take the callee"
    v_addr, v_off, v_size = min(victims, key=lambda x: x[2])
    delta = v_addr - c_addr
    struct.pack_into("<Q", blob, base + _symtab_value_offset(co, v_addr, v_size), c_addr)   # the two swap addresses
    blob[base + v_off:base + v_off + c_size] = co[c_off:c_off + c_size]
    blob[base + c_off:base + c_off + c_size] = bytes(c_size)   # nothing is left at the old address
    struct.pack_into("<Q", blob, base + _symtab_value_offset(co, c_addr, c_size), v_addr)
    # the kernel's calls: s_getpc_b64, s_add_u32 lo-literal, s_addc_u32 hi-literal
    code = co[k_off:k_off + k_size]
    w = struct.unpack("<%dI" % (k_size // 4), code)
    patched = 0
    for i in range(len(w)):
        if (w[i] & 0xFF80FFFF) != 0xBE801C00:
            continue
        pc = k_addr + 4 * (i + 1)
        j = next(j for j in range(i + 1, i + 5) if (w[j] & 0xFF800000) == 0x80000000)
        jc = next(j2 for j2 in range(j + 2, j + 8) if (w[j2] & 0xFF800000) == 0x82000000)
        lit = (w[jc + 1] << 32 | w[j + 1])
        lit = lit - (1 << 64) if lit >> 63 else lit
        if pc + lit != c_addr:
            continue
        new = (lit + delta) & ((1 << 64) - 1)
        struct.pack_into("<I", blob, base + k_off + 4 * (j + 1), new & 0xFFFFFFFF)
        struct.pack_into("<I", blob, base + k_off + 4 * (jc + 1), new >> 32)
        patched += 1
    assert patched >= 1
    moved = tmp_path / "libsalp_moved.so"
    moved.write_bytes(bytes(blob))
    _blob2, _base2, co2 = _rollout_object(str(moved))
    assert _by_name(co2, CALLEE)[0] == v_addr
    assert any(CALLEE in n for n, _o, _s in _codeobj._callees(co2, k_addr, _codeobj._functions(co2)))
    assert _codeobj.kernel_sha(str(moved), _codeobj.ROLLOUT_KERNEL) == before
