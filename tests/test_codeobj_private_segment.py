"""The plain k_rollout kernels call wave_ticks without register saves.

wave_ticks<false> (csrc/salp_kernels.hip) has local linkage and is marked
[[clang::not_tail_called]], so LLVM's interprocedural register allocation
leaves out every callee save in it.  If a call site gets the IR `tail` marker
again, the function saves 132 registers per call and the kernels' private
segment grows by its 528-byte save area (72 / 88 B become 596 / 612 B).  The
kernel descriptor's private_segment_fixed_size says which of the two was
built; the bound of 128 B leaves room for compiler drift and cannot admit the
save area.  One integer from the code object's metadata; CPU only."""
import pytest

from grasp_lab_salp_amd import _codeobj

PLAIN_COLLECT_KERNEL = "k_rolloutILb0ELb1EE"   # k_rollout<RAND = false, POL = true>
BOUND = 128


@pytest.fixture(scope="module")
def lib():
    from grasp_lab_salp_amd import build
    return build.build()


@pytest.mark.parametrize("symbol", [_codeobj.ROLLOUT_KERNEL, PLAIN_COLLECT_KERNEL])
def test_plain_rollout_kernels_hold_no_save_area(lib, symbol):
    size = _codeobj.private_segment_size(lib, symbol)
    print(symbol, "private_segment_fixed_size", size)
    assert size is not None, f"{symbol}: kernel not found in {lib}"
    assert size <= BOUND, f"{symbol}: {size} B of private memory per lane (wave_ticks saves registers again?)"


def test_reader_reads_the_descriptor_word(lib):
    """A kernel known to spill (the randomised k_rollout keeps its boundary's
    frame in private memory) reads as more than the bound, an unknown or
    ambiguous name as None: the reader does not return 0 for everything."""
    assert _codeobj.private_segment_size(lib, "k_rolloutILb1ELb0EE") > BOUND
    assert _codeobj.private_segment_size(lib, "no_such_kernel") is None
    assert _codeobj.private_segment_size(lib, "k_rollout") is None
