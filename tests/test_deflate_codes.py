"""The DEFLATE encoder's length-limited Huffman code lengths (csrc/dfl_codes.h),
through the host twin up_dfl_code_lengths: no GPU needed.

Every histogram runs at max_len 15 and 7.  A prefix code of depth L has at most
2^L codewords, so 286 used symbols have no code of depth 7: there the routine must
refuse (UP_E_ARG), and the equal-frequency case runs at 128 symbols, the most that
fit, beside the 286 at depth 15.
"""
import heapq
from fractions import Fraction

import numpy as np
import pytest

from unipeak_amd import capi


def fib(n):
    a, b, out = 1, 1, []
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def huffman_cost(freq):
    """sum freq * depth of an unlimited Huffman code, and its greatest depth"""
    used = [f for f in freq if f]
    if len(used) < 2:
        return sum(used), 1 if used else 0
    heap = [(f, 0) for f in used]  # (weight, height)
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return cost, heap[0][1]


def sparse_random():
    rng = np.random.default_rng(20260)
    f = np.zeros(286, np.int64)
    idx = rng.choice(286, 60, replace=False)
    f[idx] = rng.integers(1, 5000, 60)
    f[idx[:5]] = 1  # ties at the bottom
    return f.tolist()


HISTOGRAMS = {
    "fibonacci24": fib(24),                       # unlimited depth 23
    "equal128": [7] * 128,
    "none": [0] * 30,
    "one": [0] * 9 + [5] + [0] * 20,
    "two": [0, 3, 0, 0, 9] + [0] * 25,
    "sparse": sparse_random(),
}


def check(freq, max_len):
    freq = list(freq)
    lens = capi.dfl_code_lengths(freq, max_len).tolist()
    assert len(lens) == len(freq)
    used = [i for i, f in enumerate(freq) if f]
    for i, f in enumerate(freq):
        if f == 0:
            assert lens[i] == 0, i
        else:
            assert 1 <= lens[i] <= max_len, (i, lens[i])
    if len(used) >= 2:
        assert sum(Fraction(1, 2 ** lens[i]) for i in used) == 1
    if len(used) == 1:
        assert lens[used[0]] == 1
    for i in used:
        for j in used:
            if freq[i] > freq[j]:
                assert lens[i] <= lens[j], (i, j)
    cost, depth = huffman_cost(freq)
    got = sum(freq[i] * lens[i] for i in used)
    if depth <= max_len:
        assert got == cost
    else:
        assert got >= cost
    return lens


@pytest.mark.parametrize("max_len", [15, 7])
@pytest.mark.parametrize("name", sorted(HISTOGRAMS))
def test_code_lengths(name, max_len):
    check(HISTOGRAMS[name], max_len)


def test_fibonacci_is_really_limited():
    """the limiter runs: the unlimited code is 23 deep"""
    assert huffman_cost(fib(24))[1] == 23
    for max_len in (15, 7):
        assert max(check(fib(24), max_len)) == max_len


def test_equal_286():
    lens = check([3] * 286, 15)
    assert sorted(set(lens)) == [8, 9]  # 226 codes of 8 bits and 60 of 9
    with pytest.raises(capi.UpError):  # 286 codewords do not fit in depth 7
        capi.dfl_code_lengths([3] * 286, 7)
    assert set(check([3] * 128, 7)) == {7}


def test_arguments():
    for bad in ([1] * 289, ):
        with pytest.raises(capi.UpError):
            capi.dfl_code_lengths(bad, 15)
    with pytest.raises(capi.UpError):
        capi.dfl_code_lengths([1, 2, 3], 16)
    with pytest.raises(capi.UpError):
        capi.dfl_code_lengths([1, 2, 3], 1)  # three symbols, depth 1
    with pytest.raises(capi.UpError):
        capi.dfl_code_lengths([2 ** 31, 2 ** 31], 15)  # the tree's weights would wrap
