"""The bzip2 decoder's host twin (up_bz_decode_host: csrc/bz_block.h, serial
along the chain) against Python's bz2 module on the case list of
tests/bz_cases.py.  No device is opened."""
import bz2

import pytest

from tests import bz_cases
from unipeak_amd import capi


@pytest.fixture(scope="module")
def lib():
    try:
        return capi.load_library()
    except OSError as e:
        pytest.fail(f"library not built: {e}")


@pytest.mark.parametrize("name", bz_cases.VALID_NAMES)
def test_host_decodes(lib, name):
    plain, z = bz_cases.valid_cases()[name]
    assert bz2.decompress(z) == plain  # the independent decoder agrees with the case itself
    got, info = capi.bunzip_host(z)
    assert got == plain
    scan = bz_cases.bit_scan(z)
    assert info.blocks == sum(1 for _, k in scan if k == 0)
    assert info.streams == sum(1 for _, k in scan if k == 1)
    assert info.reason == capi.BZ_OK


def test_alignments_covered():
    """the committed seeds' files start a block at every one of the eight bit alignments"""
    seen = set()
    for s in bz_cases.ALIGN_SEEDS:
        z = bz_cases.valid_cases()[f"align_seed{s}"][1]
        seen |= {b % 8 for b, k in bz_cases.bit_scan(z) if k == 0}
    assert seen == set(range(8))


@pytest.mark.parametrize("name", bz_cases.CORRUPT_NAMES)
def test_host_refuses(lib, name):
    z, reason = bz_cases.corrupt_cases()[name]
    with pytest.raises(capi.BzError) as e:
        capi.bunzip_host(z)
    assert e.value.reason != capi.BZ_OK and e.value.reason != capi.BZ_NOSPACE
    if reason is not None:
        assert e.value.reason == reason, (name, str(e.value))


def test_host_reports_size_before_it_writes(lib):
    """a destination that is too small: UP_E_ARG, reason NOSPACE, the full size in *n_out and
    nothing written past cap"""
    import ctypes

    import numpy as np
    plain, z = bz_cases.valid_cases()["a100000"]
    src = np.frombuffer(z, np.uint8)
    dst = np.full(1000 + 8, 0xEE, np.uint8)
    n, info = ctypes.c_uint64(0), capi.BzInfo()
    rc = lib.up_bz_decode_host(src.ctypes.data, len(src), dst.ctypes.data, 1000, ctypes.byref(n), ctypes.byref(info))
    assert rc == -1 and info.reason == capi.BZ_NOSPACE and n.value == len(plain)
    assert dst[:1000].tobytes() == plain[:1000] and (dst[1000:] == 0xEE).all()
