"""The device's DEFLATE encoder (csrc/deflate.hip) through capi.Deflate.  The checker
is Python's zlib: every output must inflate to its input, with the right CRC-32 or
Adler-32; nothing is compared with zlib's own compressed bytes."""
import struct
import zlib

import numpy as np
import pytest

from unipeak_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dfl(gpu_lib):
    with gpu_lib.Deflate() as d:
        yield d


def profile_text(n_bytes, seed=7):
    """lines like a -w density profile: position, tab, a %g score"""
    rng = np.random.default_rng(seed)
    out, pos, size = [], 10_000, 0
    score = 0.01
    while size < n_bytes:
        pos += 1 if rng.random() < 0.9 else int(rng.integers(2, 3000))
        score = max(1e-5, score * float(np.exp(rng.normal(0, 0.05))))
        line = f"{pos}\t{score:.6g}\n"
        out.append(line)
        size += len(line)
    return "".join(out).encode()[:n_bytes]


def section(n_items, seed):
    """a bigWig data section: the 24-byte header and (start, float) items"""
    rng = np.random.default_rng(seed)
    starts = 5000 + np.cumsum(rng.integers(1, 4, n_items)).astype("<u4")
    vals = np.round(np.abs(np.cumsum(rng.normal(0, 0.01, n_items))) + 0.001, 4).astype("<f4")
    items = np.zeros(n_items, capi.BW_ITEM_DTYPE)
    items["start"], items["value"] = starts, vals
    end = int(starts[-1]) + 1 if n_items else 0
    head = struct.pack("<IIIIIBBH", 3, int(starts[0]) if n_items else 0, end, 0, 1, 2, 0, n_items)
    return head + items.tobytes()


def no_repeat_block(n, seed=3):
    """n bytes over 24 values in which no 3-gram occurs twice, so no match exists and
    the block still compresses (4.6 bits of entropy per byte): a random walk that only
    takes a byte whose 3-gram is new"""
    rng = np.random.default_rng(seed)
    out, seen = [0, 1], set()
    while len(out) < n:
        for b in rng.permutation(24):
            g = (out[-2], out[-1], int(b))
            if g not in seen:
                seen.add(g)
                out.append(int(b))
                break
        else:
            raise AssertionError("walk stuck")
    data = bytes(x + 97 for x in out)
    grams = [data[i:i + 3] for i in range(len(data) - 2)]
    assert len(set(grams)) == len(grams)
    return data


def fibonacci_bytes(seed=11):
    f = [1, 1]
    while len(f) < 24:
        f.append(f[-1] + f[-2])
    data = np.repeat(np.arange(24, dtype=np.uint8) + 65, f)  # 121,392 bytes
    np.random.default_rng(seed).shuffle(data)
    return data.tobytes()


def inflate_raw(out):
    return zlib.decompress(out + b"\x03\x00", wbits=-15)


def stream_inputs():
    blk = capi.dfl_block()
    rng = np.random.default_rng(5)
    text = profile_text(3 * blk + 17)
    r32 = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    r40 = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    p258 = rng.integers(0, 256, 258, dtype=np.uint8).tobytes()
    return {
        "empty": b"",
        "one": b"x",
        "text_B-1": text[:blk - 1],
        "text_B": text[:blk],
        "text_B+1": text[:blk + 1],
        "text_3B+17": text,
        "zeros": bytes(200_000),
        "random_B": rng.integers(0, 256, blk, dtype=np.uint8).tobytes(),
        "no_match": no_repeat_block(3000),
        "dist_32768": r32 + r32,
        "dist_40000": r40 + r40,
        "fibonacci": fibonacci_bytes(),
        "period_3": b"abc" * 7000,
        "period_258": p258 * 300,
    }


@pytest.fixture(scope="module")
def inputs(gpu_lib):
    return stream_inputs()


NAMES = ["empty", "one", "text_B-1", "text_B", "text_B+1", "text_3B+17", "zeros", "random_B", "no_match",
         "dist_32768", "dist_40000", "fibonacci", "period_3", "period_258"]


@pytest.mark.parametrize("name", NAMES)
def test_stream_roundtrip(dfl, inputs, name):
    data = inputs[name]
    out, crc = dfl.stream(data)
    print(name, len(data), "->", len(out))
    assert len(out) <= capi.dfl_bound(len(data))
    assert crc == zlib.crc32(data)
    assert inflate_raw(out) == data
    if not data:
        assert out == b""
    # as a gzip member and as a zlib stream
    gz = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + out + b"\x03\x00" + struct.pack("<II", crc, len(data))
    assert zlib.decompress(gz, wbits=31) == data
    zs = b"\x78\x9c" + out + b"\x03\x00" + struct.pack(">I", zlib.adler32(data))
    assert zlib.decompress(zs) == data


def test_stream_stored_path(dfl, inputs):
    """random bytes do not compress: the block goes out stored, within the bound"""
    data = inputs["random_B"]
    blk = capi.dfl_block()
    assert len(data) == blk == 65536
    out, _ = dfl.stream(data)
    assert len(out) <= capi.dfl_bound(len(data)) == blk + 10
    # a 65,536-byte block is two stored blocks: 65,535 bytes and 1 byte
    assert out[0] == 0 and struct.unpack_from("<HH", out, 1) == (0xFFFF, 0x0000)
    assert out[5:5 + 65535] == data[:65535]
    at = 5 + 65535
    assert out[at] == 0 and struct.unpack_from("<HH", out, at + 1) == (1, 0xFFFE)
    assert out[at + 5:] == data[65535:]


def test_stream_compresses(dfl, inputs):
    """sizes that only a working matcher reaches"""
    zeros, _ = dfl.stream(inputs["zeros"])
    assert len(zeros) < 200_000 // 100  # 258-byte matches at distance 1
    twice, _ = dfl.stream(inputs["dist_32768"])
    # the first half is literals at about 8 bits; the second is matches at distance 32,768
    # wherever the hash table still holds the first occurrence.  Without them the block
    # is stored: 65,546 bytes
    assert len(twice) < 49152
    nomatch, _ = dfl.stream(inputs["no_match"])
    assert nomatch[0] & 7 == 4 and len(nomatch) < 3000 * 0.75  # one dynamic block, not final
    p3, _ = dfl.stream(inputs["period_3"])
    assert len(p3) < 21000 // 20
    p258, _ = dfl.stream(inputs["period_258"])
    assert len(p258) < 258 * 300 // 10
    fibo, _ = dfl.stream(inputs["fibonacci"])
    assert len(fibo) < len(inputs["fibonacci"]) * 0.45  # entropy is 2.6 bits per byte


def test_stream_deterministic(dfl, inputs):
    blk = capi.dfl_block()
    data = profile_text(4 * blk, seed=21)
    a, crc_a = dfl.stream(data)
    b, crc_b = dfl.stream(data)
    assert a == b and crc_a == crc_b
    # a block compresses the same wherever it sits: blocks [1, 3) alone
    first, _ = dfl.stream(data[:blk])
    mid, _ = dfl.stream(data[blk:3 * blk])
    last, _ = dfl.stream(data[3 * blk:])
    assert a == first + mid + last
    with capi.Deflate() as other:  # and in another handle
        assert other.stream(data)[0] == a


def seg_case(lengths_or_bytes):
    segs = list(lengths_or_bytes)
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
    return b"".join(segs), off, segs


def check_segments(dfl, segs):
    data, off, segs = seg_case(segs)
    got = dfl.segments(data, off)
    assert len(got) == len(segs)
    for i, (z, s) in enumerate(zip(got, segs)):
        assert zlib.decompress(z) == s, i  # header, final block and Adler-32
    return got


def test_segments_sections(dfl):
    rng = np.random.default_rng(9)
    segs = [b"", b"\x07", section(1, 1), section(1023, 2), section(1024, 3),
            profile_text(32768, seed=4), profile_text(65536, seed=5),
            rng.integers(0, 256, 65536, dtype=np.uint8).tobytes(),  # stored, two blocks, the last final
            bytes(65536), b"", rng.integers(0, 256, 100, dtype=np.uint8).tobytes()]
    got = check_segments(dfl, segs)
    assert got[0] == got[9]
    assert len(got[8]) < 700
    # the same segments in another order give the same streams
    again = check_segments(dfl, segs[::-1])
    assert again[::-1] == got


def test_segments_mixed_300(dfl):
    rng = np.random.default_rng(31)
    segs = []
    for i in range(300):
        kind = i % 5
        n = int(rng.integers(0, 1025))
        if kind == 0:
            segs.append(section(max(n, 1), 100 + i))
        elif kind == 1:
            segs.append(profile_text(int(rng.integers(0, 9000)), seed=i))
        elif kind == 2:
            segs.append(rng.integers(0, 256, int(rng.integers(0, 3000)), dtype=np.uint8).tobytes())
        elif kind == 3:
            segs.append(bytes([i & 255]) * int(rng.integers(0, 5000)))
        else:
            segs.append(b"" if i % 10 == 4 else b"ab"[:1 + (i & 1)])
    check_segments(dfl, segs)


def test_segments_too_long(dfl):
    data = bytes(65537)
    with pytest.raises(capi.UpError) as e:
        dfl.segments(data, [0, 65537])
    assert e.value.code == -1  # UP_E_ARG
    with pytest.raises(capi.UpError):
        dfl.segments(data, [0, 10, 5])  # offsets that go backwards


def huffman_only(data, wbits):
    c = zlib.compressobj(6, zlib.DEFLATED, wbits, 8, zlib.Z_HUFFMAN_ONLY)
    return c.compress(data) + c.flush()


def test_lz_stage_is_alive(dfl):
    """a cap, not a measurement: literals-only coding cannot get below zlib's
    Z_HUFFMAN_ONLY on the same blocks"""
    blk = capi.dfl_block()
    text = profile_text(4 * blk, seed=77)
    out, _ = dfl.stream(text)
    cap = sum(len(huffman_only(text[i:i + blk], -15)) for i in range(0, len(text), blk))
    print("text", len(text), "device", len(out), "huffman-only", cap)
    assert len(out) < cap
    segs = [section(1024, 500 + i) for i in range(64)]
    data, off, _ = seg_case(segs)
    got = dfl.segments(data, off)
    dev = sum(len(z) for z in got)
    cap = sum(len(huffman_only(s, 15)) for s in segs)
    print("sections", len(data), "device", dev, "huffman-only", cap)
    assert dev < cap
