"""Inputs for the bzip2 decoder's tests (test_bz_host.py, test_gpu_bz.py): the
valid and the corrupt files, made with Python's bz2 module -- the independent
encoder and decoder, never the code under test -- and a plain bit scan for the
two 48-bit magics, the reference for up_bz_scan and for the block counts."""
import bz2
import functools

import numpy as np

from unipeak_amd import capi

BLOCK_MAGIC = 0x314159265359
END_MAGIC = 0x177245385090


def bit_scan(data):
    """[(bit offset, kind)] ascending: kind 0 = block magic, 1 = end-of-stream magic, at any of
    the eight bit alignments"""
    a = np.frombuffer(bytes(data) + b"\0", np.uint8).astype(np.uint16)
    hits = []
    for s in range(8):
        sh = (((a[:-1] << s) | (a[1:] >> (8 - s))) & 0xFF).astype(np.uint8).tobytes()
        for magic, kind in ((BLOCK_MAGIC, 0), (END_MAGIC, 1)):
            pat, at = magic.to_bytes(6, "big"), 0
            while True:
                at = sh.find(pat, at)
                if at < 0:
                    break
                if 8 * at + s + 48 <= 8 * len(data):
                    hits.append((8 * at + s, kind))
                at += 1
    return sorted(hits)


def get_bits(data, bit, k):
    v = int.from_bytes(data, "big")
    return (v >> (8 * len(data) - bit - k)) & ((1 << k) - 1)


def set_bits(data, bit, k, value):
    v = int.from_bytes(data, "big")
    sh = 8 * len(data) - bit - k
    v = (v & ~(((1 << k) - 1) << sh)) | ((value & ((1 << k) - 1)) << sh)
    return v.to_bytes(len(data), "big")


def wiggle_text(n, seed=11):
    """n bytes of variableStep wiggle text"""
    rng = np.random.default_rng(seed)
    out, size, pos = [], 0, 1
    while size < n:
        if len(out) % 5000 == 0:
            out.append(f"variableStep chrom=chr{1 + len(out) // 5000} span=1\n")
            pos = 1
        else:
            pos += int(rng.integers(1, 40))
            out.append(f"{pos}\t{int(rng.integers(1, 30))}\n")
        size += len(out[-1])
    return "".join(out).encode()[:n]


def align_text(seed):
    """the text of the block-alignment files: three level-1 blocks of wiggle text"""
    return wiggle_text(250_000, seed=1000 + seed)


# seeds of align_text whose files' block starts cover all eight bit alignments (found by
# running bit_scan over seeds 0, 1, 2, ... on the CPU; test_alignments_covered asserts it)
ALIGN_SEEDS = (1, 3, 5, 10)


@functools.lru_cache(maxsize=None)
def valid_cases():
    """{name: (plain bytes, .bz2 bytes)}"""
    rng = np.random.default_rng(5)
    rnd = rng.integers(0, 256, 350_000, dtype=np.uint8).tobytes()
    wig = wiggle_text(350_000)
    c = bz2.compress
    plain = {
        "empty": b"",
        "one_byte": b"x",
        "a3": b"a" * 3, "a4": b"a" * 4, "a5": b"a" * 5, "a259": b"a" * 259, "a260": b"a" * 260,
        "a100000": b"a" * 100_000,
        # count byte 4 after a run of byte 4; count byte 97 after a run of 'a'; count byte 97 after
        # a run of 'b' with 'a's next; a run that ends the block
        "count_is_run_byte": b"\x04" * 8 + b"z" + b"a" * 101 + b"y" + b"b" * 101 + b"a" * 9 + b"\x04" * 4,
        "count_is_next_byte": b"b" * 101 + b"a" * 3 + b"c" * 8 + b"\x04" * 5 + b"\x01" * 3 + b"q" * 4,
        "ab": b"ab" * 50_000,
        "abc": b"abc" * 40_000,
        "all_bytes": bytes(range(256)) * 3,
    }
    cases = {k: (v, c(v)) for k, v in plain.items()}
    cases["random_level1"] = (rnd, c(rnd, 1))
    cases["wiggle_level1"] = (wig, c(wig, 1))
    cases["wiggle_level9"] = (wig, c(wig, 9))
    parts = [wig[:150_000], rnd[:30_000], b"a" * 1000]
    cases["three_streams"] = (b"".join(parts), c(parts[0], 1) + c(parts[1], 5) + c(parts[2], 9))
    cases["empty_stream_between"] = (parts[2] + parts[1], c(parts[2]) + c(b"") + c(parts[1], 2))
    for s in ALIGN_SEEDS:
        t = align_text(s)
        cases[f"align_seed{s}"] = (t, c(t, 1))
    return cases


VALID_NAMES = ("empty", "one_byte", "a3", "a4", "a5", "a259", "a260", "a100000", "count_is_run_byte",
               "count_is_next_byte", "ab", "abc", "all_bytes", "random_level1", "wiggle_level1", "wiggle_level9",
               "three_streams", "empty_stream_between") + tuple(f"align_seed{s}" for s in ALIGN_SEEDS)


@functools.lru_cache(maxsize=None)
def corrupt_cases():
    """{name: (.bz2 bytes, expected UP_BZ_* reason or None for "any error")}.  The base file is
    one level-9 block; its header fields stand at fixed bits after the stream header (32) and
    the block magic (48): CRC 80, randomised 112, origPtr 113, symbol map 137."""
    text = wiggle_text(20_000)
    z = bz2.compress(text)
    used16 = get_bits(z, 137, 16)
    n_groups_at = 153 + 16 * bin(used16).count("1")
    assert 2 <= get_bits(z, n_groups_at, 3) <= 6
    end = [b for b, k in bit_scan(z) if k == 1]
    assert len(end) == 1
    return {
        "plain_text": (text, capi.BZ_NOT_BZIP2),
        "level_0": (z[:3] + b"0" + z[4:], capi.BZ_BAD_LEVEL),
        "cut_in_header": (z[:18], capi.BZ_TRUNCATED),
        "cut_in_symbols": (z[:len(z) // 2], capi.BZ_TRUNCATED),
        "cut_before_stream_crc": (z[:-4], capi.BZ_TRUNCATED),
        "origptr_ffffff": (set_bits(z, 113, 24, 0xFFFFFF), capi.BZ_ORIGPTR),
        "randomised": (set_bits(z, 112, 1, 1), capi.BZ_RANDOMISED),
        "ngroups_7": (set_bits(z, n_groups_at, 3, 7), capi.BZ_NGROUPS),
        "flipped_symbol_bit": (set_bits(z, 4 * len(z), 1, 1 - get_bits(z, 4 * len(z), 1)), None),
        "wrong_stream_crc": (set_bits(z, end[0] + 48, 32, get_bits(z, end[0] + 48, 32) ^ 1), capi.BZ_STREAM_CRC),
        "trailing_garbage": (z + b"garbage", capi.BZ_TRAILING),
    }


CORRUPT_NAMES = ("plain_text", "level_0", "cut_in_header", "cut_in_symbols", "cut_before_stream_crc",
                 "origptr_ffffff", "randomised", "ngroups_7", "flipped_symbol_bit", "wrong_stream_crc",
                 "trailing_garbage")
