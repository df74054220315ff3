"""Inputs for the Huffman ENCODE side (ie_huffman.hip, ie_capi_huffman.cpp, host/huffman.cpp) and the
plain references they are checked against.  No GPU and no oracle in this file: numpy only.

References
  pack_bits     the per-bit MSB-first packer (what pack_kernel must write)
  histogram     np.bincount plus the first index of every value (what hist / first_scan / first_full
                must return)
  code_lengths  a heap Huffman returning the multiset of code lengths -- for max-length claims only,
                where tie-breaking cannot matter

Inputs: every one is seeded and deterministic; tests/test_huffman_inputs.py holds each to the
property its name claims, so that tests/test_gpu_huffman_encode_paths.py reaches what it says.
"""
import heapq

import numpy as np

NOPOS = np.uint64(2**64 - 1)  # first position of a value that does not occur


# ------------------------------------------------------------------ plain references
def pack_bits(data, code, length, start=0):
    """The code words of ``data``'s bytes, MSB first, one after another: (bits, end) with bits a
    uint8 array of 0/1 and end = start + bits.size, the stream bit after the last one.  Bit k of
    symbol b's word is (code[b] >> (length[b] - 1 - k)) & 1, k = 0 .. length[b] - 1."""
    data = np.asarray(data, dtype=np.uint8).ravel()
    code = np.asarray(code).astype(np.uint64)
    lens = np.asarray(length).astype(np.int64)[data]
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, np.uint8), start
    first = np.cumsum(lens) - lens                   # the stream bit (from 0) of every symbol's word
    sym = np.repeat(np.arange(data.size), lens)      # per output bit: its symbol ...
    k = np.arange(total, dtype=np.int64) - first[sym]  # ... and its place in the word, 0 = MSB
    shift = (lens[sym] - 1 - k).astype(np.uint64)
    bits = ((code[data][sym] >> shift) & np.uint64(1)).astype(np.uint8)
    return bits, start + total


def histogram(data):
    """(hist uint32[256], first uint64[256]): the count of every byte value and the index of its
    first occurrence (NOPOS where it does not occur)."""
    a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data.ravel()
    hist = np.bincount(a, minlength=256).astype(np.uint32)
    first = np.full(256, NOPOS, dtype=np.uint64)
    vals, idx = np.unique(a, return_index=True)
    first[vals] = idx.astype(np.uint64)
    return hist, first


def code_lengths(counts):
    """The sorted code lengths of a Huffman code for the non-zero ``counts`` (a lone symbol: [0]).
    Equal weights are merged in heap order, so only tie-independent facts (the longest code of a
    Fibonacci alphabet) may be read off the result."""
    heap = [(int(c), i, (i,)) for i, c in enumerate(c for c in counts if c)]
    depth = [0] * len(heap)
    heapq.heapify(heap)
    nxt = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for leaf in a[2] + b[2]:
            depth[leaf] += 1
        heapq.heappush(heap, (a[0] + b[0], nxt, a[2] + b[2]))
        nxt += 1
    return sorted(depth)


# ------------------------------------------------------------------ named inputs
ORDERS = ("ascending", "descending", "shuffled")


def fib_counts(nsym):
    f = [1, 1]
    while len(f) < nsym:
        f.append(f[-1] + f[-2])
    return f[:nsym]


def fib_string(nsym, order, scale=1):
    """Byte value i occurs scale * Fibonacci(i) times (1, 1, 2, 3, 5, ...): the longest code is
    nsym - 1 bits whatever the tie-breaking.  order: bytes sorted ascending, descending, or a seeded
    shuffle -- the first-occurrence order of the values differs between the three."""
    a = np.repeat(np.arange(nsym, dtype=np.uint8), np.array(fib_counts(nsym)) * scale)
    if order == "descending":
        a = a[::-1].copy()
    elif order == "shuffled":
        np.random.default_rng(1000 + nsym).shuffle(a)
    else:
        assert order == "ascending"
    return a.tobytes()


FIB_SIZES = {16: 2583, 17: 4180, 18: 6764}  # bytes; longest codes 15, 16 and 17 bits


def single_value(value, n):
    return bytes([value]) * n


SINGLE_N = (3, 4, 1000, 16384, 2 * 16384 + 5)
SINGLE_VALUES = (42, 0)


def single_value_file(value):
    """What the reference writes for n >= 3 copies of one value: {1, count 1, length 0}, the key,
    no code bits, the stop bit -- 21 bits -- and no data bits."""
    return bytes([0x81, value >> 4, (value & 0xF) << 4])


EQUAL_K = (2, 3, 5, 16, 17, 64, 100, 255, 256)
EQUAL_M = 40
LAYOUTS = ("blocked", "interleaved")


def equal_count_values(k, order):
    vals = np.arange(k, dtype=np.int64) * (256 // k)
    if order == "descending":
        vals = vals[::-1]
    elif order == "shuffled":
        vals = np.random.default_rng(2000 + k).permutation(vals)
    return vals.astype(np.uint8)


def equal_count(k, order, layout, m=EQUAL_M):
    """k distinct values, m of each, first seen in ``order``; blocked: all of one value, then all of
    the next; interleaved: round-robin."""
    vals = equal_count_values(k, order)
    a = np.repeat(vals, m) if layout == "blocked" else np.tile(vals, m)
    assert layout in LAYOUTS
    return a.tobytes()


def skewed(n, seed, p=0.08):
    return np.minimum(np.random.default_rng(seed).geometric(p, n), 255).astype(np.uint8).tobytes()


def uniform(n, seed, hi=256):
    return np.random.default_rng(seed).integers(0, hi, n, dtype=np.uint8).tobytes()


def placed(n, places, seed, base_hi=200, runs=()):
    """n bytes random in [0, base_hi) with value v written at index at for (v, at) in places and
    value v over [at, at + length) for (v, at, length) in runs.  Placed values are >= base_hi, so
    each first occurs exactly where it is put."""
    a = np.random.default_rng(seed).integers(0, base_hi, n, dtype=np.uint8)
    for v, at in places:
        assert v >= base_hi and at < n
        a[at] = v
    for v, at, length in runs:
        assert v >= base_hi and at + length <= n
        a[at:at + length] = v
    return a


# (a) the six strings of the odd-pitch batch, by name
SIX_PITCH = 20011


def six_strings():
    return [
        ("no_gain", uniform(3000, 11)),
        ("empty", b""),
        ("single_value", single_value(42, 1000)),
        ("short", skewed(37, 12, p=0.4)),
        ("one_tile", skewed(16384, 13, p=0.2)),
        ("one_tile_plus_one", skewed(16385, 14, p=0.2)),
    ]


# (e) the batch of 256 strings at pitch 256 whose last string runs past the pitch
BATCH256_PITCH = 256
BATCH256_LAST_N = 400_003
BATCH256_PLACES = ((230, 262_143), (231, 262_144), (232, 330_000), (233, 400_002))
BATCH256_RUN = (240, 390_000, 16)


def batch256():
    """255 strings of 1 .. 200 bytes (even ones uniform, odd ones skewed) and a last one of
    400 003 bytes with values first seen at BATCH256_PLACES and a 16-byte run of 240 at 390 000."""
    rng = np.random.default_rng(31)
    lens = rng.integers(1, 201, 255)
    out = [uniform(int(n), 3000 + k) if k % 2 == 0 else skewed(int(n), 3000 + k, p=0.5) for k, n in enumerate(lens)]
    out.append(placed(BATCH256_LAST_N, BATCH256_PLACES, 32, runs=(BATCH256_RUN,)).tobytes())
    return out


# (e) the one large input: the histogram's second grid stride for a single string
BIG_STRIDE = 2048 * 16384
BIG_N = BIG_STRIDE + 16384 + 5
BIG_PLACES = ((200, BIG_STRIDE), (201, BIG_STRIDE + 8191), (202, BIG_STRIDE + 16383), (203, BIG_N - 1))


def big_hist_input():
    return placed(BIG_N, BIG_PLACES, 33)


# (f) first-occurrence edges of a single string
EDGE_AT = (4095, 4096, 16_383, 16_384, 16_385, 262_143, 262_144)
EDGE_N = (15, 16, 17, 4096, 16_384, 16_385, 262_144, 262_145, 270_001)


def edge_string(n):
    """n bytes random in [0, 200) with a fresh value (201, 202, ...) at every index of EDGE_AT
    below n."""
    places = tuple((201 + i, at) for i, at in enumerate(EDGE_AT) if at < n)
    return placed(n, places, 4000 + n).tobytes()


def edge_places(n):
    return tuple((201 + i, at) for i, at in enumerate(EDGE_AT) if at < n)


EARLY_N = 300_000


def all_values_early():
    """300 000 bytes over 16 values, all of them among the first 16 bytes: the first-occurrence
    scan is complete after its first round."""
    a = np.random.default_rng(41).integers(0, 16, EARLY_N, dtype=np.uint8)
    a[:16] = np.arange(16, dtype=np.uint8)[::-1]
    return a.tobytes()


LATE_LAST_N = 300_001


def late_last_byte():
    """Random in [0, 200) -- every such value seen within the first chunks -- and 250 as the very
    last byte: the only value the scan leaves to the full pass."""
    return placed(LATE_LAST_N, ((250, LATE_LAST_N - 1),), 42).tobytes()


# code tables for the pack tests
def full_table(L, seed):
    """Every one of the 256 codes L bits long, random below 2**L."""
    rng = np.random.default_rng(seed)
    length = np.full(256, L, dtype=np.uint8)
    code = rng.integers(0, 1 << L, 256, dtype=np.uint64).astype(np.uint32)
    return code, length


def ragged_table(maxlen, seed, zeros=0):
    """Random lengths in 1 .. maxlen with at least four codes of exactly maxlen bits and ``zeros``
    symbols of length 0 (the symbols stay in the data: they contribute no bits)."""
    rng = np.random.default_rng(seed)
    length = rng.integers(1, maxlen + 1, 256).astype(np.uint8)
    pick = rng.permutation(256)
    length[pick[:4]] = maxlen
    length[pick[4:4 + zeros]] = 0
    code = np.array([int(rng.integers(0, 1 << int(l))) if l else 0 for l in length], np.uint64).astype(np.uint32)
    return code, length
