"""The Huffman encode inputs of tests/huffman_inputs.py (CPU).

1. Every named input has the property its name claims -- code lengths, sizes, first positions, equal
   counts -- so a wrong generator cannot turn a test of tests/test_gpu_huffman_encode_paths.py into
   a no-op.
2. The oracle agrees with the plain references on them: its histogram with histogram(), its encode
   of single-value strings with the 3-byte dictionary, its decode of its own encode with the input.
3. The kernel constants the inputs are laid out around are the sources'.
"""
import os
import re

import numpy as np
import pytest

from tests import huffman_inputs as HI
from tests import oracle_lib as O

CSRC = os.path.join(O.ROOT, "imageencoder_amd", "csrc")


def _roundtrip(data: bytes):
    o = O.load()
    dec = o.huffman_decode(o.huffman_encode(data))
    assert dec is not None
    out, passthrough = dec
    assert passthrough or out[: len(data)] == data
    return passthrough


# ------------------------------------------------------------------ the references themselves
def test_pack_bits_is_the_per_bit_packer():
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, 999, dtype=np.uint8)
    code, length = HI.ragged_table(32, 2, zeros=9)
    ref = []
    for b in data:
        l = int(length[b])
        ref.extend((int(code[b]) >> (l - 1 - k)) & 1 for k in range(l))
    bits, end = HI.pack_bits(data, code, length, 77)
    assert end == 77 + len(ref) and np.array_equal(bits, np.array(ref, np.uint8))
    bits, end = HI.pack_bits(data, code, np.zeros(256, np.uint8), 5)
    assert bits.size == 0 and end == 5
    bits, end = HI.pack_bits(np.zeros(0, np.uint8), code, length, 9)
    assert bits.size == 0 and end == 9


def test_histogram_small():
    hist, first = HI.histogram(bytes([7, 7, 3, 255, 3, 0]))
    assert hist[7] == 2 and hist[3] == 2 and hist[255] == 1 and hist[0] == 1 and hist.sum() == 6
    assert (first[7], first[3], first[255], first[0]) == (0, 2, 3, 5)
    assert first[1] == HI.NOPOS and np.count_nonzero(first != HI.NOPOS) == 4
    hist, first = HI.histogram(b"")
    assert not hist.any() and (first == HI.NOPOS).all()


def test_code_lengths_small():
    assert HI.code_lengths([5]) == [0]
    assert HI.code_lengths([1, 1]) == [1, 1]
    assert HI.code_lengths([1, 1, 2, 4]) == [1, 2, 3, 3]
    assert HI.code_lengths([0, 3, 0, 3, 3, 3]) == [2, 2, 2, 2]


# ------------------------------------------------------------------ Fibonacci alphabets
@pytest.mark.parametrize("nsym", [16, 17, 18])
@pytest.mark.parametrize("order", HI.ORDERS)
def test_fib_strings(nsym, order):
    data = HI.fib_string(nsym, order)
    assert len(data) == HI.FIB_SIZES[nsym]
    hist, first = HI.histogram(data)
    assert list(hist[:nsym]) == HI.fib_counts(nsym) and not hist[nsym:].any()
    assert max(HI.code_lengths(hist)) == nsym - 1
    eh, ef = O.load().histogram(data)
    assert np.array_equal(eh, hist) and np.array_equal(ef, first)
    if nsym - 1 <= 15:
        assert not _roundtrip(data)
    else:
        O.load().huffman_encode(data)  # (a 16- or 17-bit length does not fit the dictionary's 4 bits: no round trip)


def test_fib_orders_differ_in_first_occurrence():
    for nsym in (16, 17, 18):
        firsts = [tuple(np.argsort(HI.histogram(HI.fib_string(nsym, o))[1][:nsym], kind="stable")) for o in HI.ORDERS]
        assert len(set(firsts)) == 3
        assert firsts[0] == tuple(range(nsym)) and firsts[1] == tuple(range(nsym - 1, -1, -1))


def test_fib_scaled_is_five_long_code_tiles():
    data = HI.fib_string(18, "shuffled", scale=3)
    assert len(data) == 3 * 6764 and (len(data) + 4095) // 4096 == 5
    assert max(HI.code_lengths(HI.histogram(data)[0])) == 17


# ------------------------------------------------------------------ single values: zero-bit codes
@pytest.mark.parametrize("value", HI.SINGLE_VALUES)
@pytest.mark.parametrize("n", HI.SINGLE_N)
def test_single_value_file(value, n):
    data = HI.single_value(value, n)
    assert len(data) == n and set(data) == {value}
    assert HI.code_lengths(HI.histogram(data)[0]) == [0]
    assert O.load().huffman_encode(data) == HI.single_value_file(value)


def test_single_value_file_of_42():
    assert HI.single_value_file(42) == bytes.fromhex("8102a0")
    assert HI.single_value_file(0) == bytes.fromhex("810000")


# ------------------------------------------------------------------ equal counts
@pytest.mark.parametrize("k", HI.EQUAL_K)
def test_equal_count_alphabets(k):
    o = O.load()
    seen = set()
    for order in HI.ORDERS:
        vals = HI.equal_count_values(k, order)
        assert len(set(vals.tolist())) == k
        for layout in HI.LAYOUTS:
            data = HI.equal_count(k, order, layout)
            hist, first = HI.histogram(data)
            assert len(data) == k * HI.EQUAL_M
            assert set(hist[hist != 0].tolist()) == {HI.EQUAL_M} and np.count_nonzero(hist) == k
            # the values first occur in the order the name says
            assert [int(v) for v in np.argsort(first, kind="stable")[:k]] == vals.tolist()
            step = HI.EQUAL_M if layout == "blocked" else 1
            assert [int(first[v]) for v in vals] == [i * step for i in range(k)]
            eh, ef = o.histogram(data)
            assert np.array_equal(eh, hist) and np.array_equal(ef, first)
            lens = HI.code_lengths(hist)
            if max(lens) <= 15:
                passthrough = _roundtrip(data)
                assert passthrough == (k >= 255)  # 255 and 256 values of 8-bit codes: no gain, '0' + input
            seen.add(data)
    assert len(seen) == (6 if k > 2 else 4)  # (two values: shuffled is one of the other two orders)


# ------------------------------------------------------------------ placed first occurrences
def _check_places(data: bytes, places):
    hist, first = HI.histogram(data)
    for v, at in places:
        assert int(first[v]) == at, (v, at)
    eh, ef = O.load().histogram(data)
    assert np.array_equal(eh, hist) and np.array_equal(ef, first)
    return hist, first


@pytest.mark.parametrize("n", HI.EDGE_N)
def test_edge_strings(n):
    data = HI.edge_string(n)
    assert len(data) == n
    places = HI.edge_places(n)
    assert [at for _, at in places] == [at for at in HI.EDGE_AT if at < n]
    hist, first = _check_places(data, places)
    # nothing else is late: every other value is within the first chunk
    others = [v for v in range(256) if hist[v] and v not in {p[0] for p in places}]
    assert all(int(first[v]) < 4096 for v in others)
    # (no decode round trip here: a value seen once among 16 384 bytes may get a code of more than
    # 15 bits, which the dictionary's 4-bit length field does not hold)


def test_edge_set_covers_the_issue():
    assert {15, 16, 17, 4096, 16_384, 16_385} <= set(HI.EDGE_N)
    assert set(HI.EDGE_AT) == {4095, 4096, 16_383, 16_384, 16_385, 262_143, 262_144}
    assert max(HI.EDGE_N) > max(HI.EDGE_AT)
    assert 4 * 4096 in HI.EDGE_N  # (ch + Q) * kHistTile == n: the scan's break with equality


def test_all_values_early():
    data = HI.all_values_early()
    hist, first = _check_places(data, ())
    assert len(data) == 300_000 and np.count_nonzero(hist) == 16
    assert int(first[first != HI.NOPOS].max()) == 15
    assert not _roundtrip(data)


def test_late_last_byte():
    data = HI.late_last_byte()
    hist, first = _check_places(data, ((250, len(data) - 1),))
    assert hist[250] == 1 and len(data) > 64 * 4096
    late = [v for v in range(256) if hist[v] and int(first[v]) >= 64 * 4096]
    assert late == [250]


def test_six_strings():
    six = dict(HI.six_strings())
    assert list(six) == ["no_gain", "empty", "single_value", "short", "one_tile", "one_tile_plus_one"]
    assert [len(d) for d in six.values()] == [3000, 0, 1000, 37, 16384, 16385]
    assert max(len(d) for d in six.values()) <= HI.SIX_PITCH and HI.SIX_PITCH % 2 == 1
    # strings 1 .. 5 start at five different offsets within a 16-byte line, none of them 0
    offs = [(k * HI.SIX_PITCH) % 16 for k in range(1, 6)]
    assert 0 not in offs and len(set(offs)) == 5
    o = O.load()
    assert len(o.huffman_encode(six["no_gain"])) == 3001
    assert o.huffman_encode(six["single_value"]) == HI.single_value_file(42)
    for name in ("short", "one_tile", "one_tile_plus_one"):
        assert len(o.huffman_encode(six[name])) < len(six[name])
        assert not _roundtrip(six[name])


def test_batch256():
    strings = HI.batch256()
    assert len(strings) == 256
    assert all(1 <= len(s) <= 200 for s in strings[:255]) and max(len(s) for s in strings[:255]) <= HI.BATCH256_PITCH
    last = strings[-1]
    assert len(last) == 400_003
    run_v, run_at, run_len = HI.BATCH256_RUN
    hist, first = _check_places(last, HI.BATCH256_PLACES + ((run_v, run_at),))
    assert [at for _, at in HI.BATCH256_PLACES] == [262_143, 262_144, 330_000, 400_002]
    assert hist[run_v] == run_len == 16 and run_at == 390_000 and last[run_at:run_at + 16] == bytes([run_v]) * 16
    # (values seen once among 400 003 bytes: codes of more than 15 bits, so no decode round trip)
    o = O.load()
    assert len(o.huffman_encode(last)) < len(last)
    gains = sum(len(o.huffman_encode(s)) <= len(s) for s in strings[:255])
    assert 20 < gains < 235  # both the dictionary path and the no-gain path among the short ones
    for s in strings[:8]:
        eh, ef = o.histogram(s)
        h, f = HI.histogram(s)
        assert np.array_equal(eh, h) and np.array_equal(ef, f)


def test_big_hist_input_places():
    """(The 34 MB string itself is only made on the GPU machine; here its layout.)"""
    assert HI.BIG_N == 2048 * 16384 + 16384 + 5
    ats = [at for _, at in HI.BIG_PLACES]
    assert all(HI.BIG_STRIDE <= at < HI.BIG_N for at in ats)
    assert ats[0] == HI.BIG_STRIDE and ats[-1] == HI.BIG_N - 1
    assert HI.BIG_N - HI.BIG_STRIDE - 16384 == 5  # workgroup 1's second step is a 5-byte tail


def test_tables():
    for L in (1, 7, 8, 15, 16, 17, 31, 32):
        code, length = HI.full_table(L, 50 + L)
        assert (length == L).all() and int(code.max()) < (1 << L) and len(set(code.tolist())) > (1 if L > 1 else 0)
    for maxlen, zeros in ((9, 0), (20, 0), (15, 6), (16, 6)):
        code, length = HI.ragged_table(maxlen, 60 + maxlen, zeros=zeros)
        assert int(length.max()) == maxlen and np.count_nonzero(length == 0) == zeros
        assert all(int(c) < (1 << int(l)) for c, l in zip(code, length))


# ------------------------------------------------------------------ the sources' constants
def test_kernel_constants():
    src = open(os.path.join(CSRC, "ie_huffman.hip")).read()
    common = open(os.path.join(CSRC, "ie_device.h")).read()
    tpb = int(re.search(r"constexpr int kTPB = (\d+);", common).group(1))
    assert re.search(r"constexpr int kHistTile = kTPB \* 16;", src) and tpb * 16 == 4096
    assert int(re.search(r"constexpr int kHistLoads = (\d+);", src).group(1)) * 4096 == 16384
    assert int(re.search(r"constexpr int kFirstScanChunks = (\d+);", src).group(1)) == 64
    assert int(re.search(r"#define IE_FIRST_Q (\d+)", src).group(1)) == 4
    assert int(re.search(r"#define IE_PACK_BPT (\d+)", src).group(1)) * tpb == 16384
    assert re.search(r"return maxlen <= 16 \? kTPB \* IE_PACK_BPT : kTPB \* 16;", src)
