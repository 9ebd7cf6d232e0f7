"""The bzip2 decoder on the device (capi.Bunzip: csrc/bzip2.hip) on the case
list of tests/bz_cases.py: byte-identical to Python's bz2 module, the block
and candidate counts against a plain bit scan of the file, and every corrupt
file refused with its reason and no output.  The corrupt files went through
tools/bz_check (the same block decoder under ASan and UBSan on the host)
before they went to a device."""
import bz2

import pytest

from tests import bz_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bz(gpu_lib):
    with gpu_lib.Bunzip(0) as h:
        yield h


@pytest.mark.parametrize("name", bz_cases.VALID_NAMES)
def test_device_decodes(bz, name):
    plain, z = bz_cases.valid_cases()[name]
    assert bz2.decompress(z) == plain
    got, info = bz.decode(z)
    assert len(got) == len(plain)
    assert got == plain
    scan = bz_cases.bit_scan(z)
    assert info.blocks == sum(1 for _, k in scan if k == 0)
    assert info.streams == sum(1 for _, k in scan if k == 1)
    assert info.dropped == 0 and info.reason == 0


@pytest.mark.parametrize("name", ["empty", "one_byte", "wiggle_level1", "three_streams", "align_seed1",
                                  "align_seed3", "align_seed5", "align_seed10"])
def test_scan_matches_bit_scan(bz, name):
    z = bz_cases.valid_cases()[name][1]
    bits, kinds = bz.scan(z)
    want = bz_cases.bit_scan(z)
    assert list(zip(bits.tolist(), kinds.tolist())) == want


def test_scan_finds_magics_at_every_alignment_and_at_the_edges(bz):
    """synthetic bytes: both magics at each of the eight alignments, one flush with the start and
    one flush with the end of the buffer, none where the last bits are missing"""
    nbits = 8 * 300
    v = 0
    places = [(0, 0)] + [(200 + 100 * s + s, s % 2) for s in range(8)] + [(nbits - 48, 1)]
    for bit, kind in places:
        magic = bz_cases.END_MAGIC if kind else bz_cases.BLOCK_MAGIC
        v |= magic << (nbits - bit - 48)
    data = v.to_bytes(nbits // 8, "big")
    assert bz_cases.bit_scan(data) == sorted(places)
    bits, kinds = bz.scan(data)
    assert list(zip(bits.tolist(), kinds.tolist())) == sorted(places)
    bits, kinds = bz.scan(data[:-1])  # the last magic loses its tail
    assert list(zip(bits.tolist(), kinds.tolist())) == sorted(places)[:-1]


@pytest.mark.parametrize("name", bz_cases.CORRUPT_NAMES)
def test_device_refuses(bz, gpu_lib, name):
    z, reason = bz_cases.corrupt_cases()[name]
    with pytest.raises(gpu_lib.BzError) as e:
        bz.decode(z)
    assert e.value.reason not in (gpu_lib.BZ_OK, gpu_lib.BZ_NOSPACE)
    if reason is not None:
        assert e.value.reason == reason, (name, str(e.value))


def test_handle_survives_a_corrupt_file(bz):
    """an error leaves no state behind: a valid file decodes right after a corrupt one"""
    plain, z = bz_cases.valid_cases()["wiggle_level9"]
    with pytest.raises(ValueError):
        bz.decode(bz_cases.corrupt_cases()["cut_in_symbols"][0])
    assert bz.decode(z)[0] == plain
    t = bz.timings()
    assert t[7] >= 1 and t[1] > 0
