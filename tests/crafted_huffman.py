"""Constructed Huffman streams: valid files of the format that no encoder here writes.

One named, seeded table (entries()), shared by the CPU tests (tests/test_crafted_huffman.py), the
golden generator (tests/golden/make_golden_crafted_huffman.py: the reference's own decode of the
wrapped image files, pinned by md5 in manifest_crafted_huffman.json) and the GPU tests
(tests/test_gpu_huffman_crafted.py).  Only the table is committed: huffman_craft.pack rebuilds every
file, and every entry records the symbols the builder put in.

The device decode (ie_huffman_decode.hip) cuts the code stream into chunks of CHUNK bits and walks
each from its 15 possible entry offsets; TC chunks share a table workgroup, TPB an emit workgroup,
G a composition group.  The families are sized against those constants.

Families
  fixed           every code L bits long, L = 1, 2, 6, 8, 11, 12, 15: the 15 entry walks of a chunk
                  never merge, min(L, 15) of them survive.  L <= 8 uses all 2^L code words (L = 8: a
                  permutation of the bytes).  For L > 8 a code of 256 words cannot be complete, and
                  a walk that meets no code slides onto the true path; so the code words are the
                  L-bit strings whose ones lie at least d + 1 apart (d the smallest that leaves at
                  most 256 of them: 233 at L = 11, 129 at L = 12, 181 at L = 15; the all-zero word
                  among them), topped up to 256 with scattered other words, and the stream is a
                  sequence with that spacing: every window of it, at every phase, is a code word.
  long_short      a 1-bit code beside 200 or 255 codes of 15 bits, the 15-bit groups listed first;
                  incomplete (14 of a chunk's 15 entry walks meet no code and slide); the 15-bit
                  codes straddle chunk ends and chunk middles at every offset 1..14
  l1_edge         codes of 10, 11 and 12 bits, two 12-bit siblings on an 11-bit prefix next to an
                  11-bit code (the first-level table holds 11 bits); and the unary comb 1, 01, 001,
                  ... down to two 15-bit leaves
  sizes           code streams of less than a chunk, of exactly 3 chunks ending on a byte (no
                  padding) and one code less or more, of 64, 65, 256 and 257 chunks
  emit_threshold  an emit workgroup of exactly IE_HUF_EMIT_LDS symbols (6- and 7-bit codes, 6 6 6 7 7:
                  160 a chunk), of one more, far fewer (L = 8) and far more (L = 1)
  dup             two code words for every byte value
  invalid         members of the families above with one position that no code prefixes: in the
                  first chunk, in the second half of a chunk, in the last chunk, past the 256th
                  chunk, and in the padding (zero bits that walk to no leaf)

Left out, because the reference leaves them undefined: a dictionary entry of 0 bits (treeAddLeaf
shifts by len - 1, Huffman.cpp:155), and a code word that is a prefix of another (the longer one's
leaf hangs below a node that already is one; which of the two the walk finds depends on the order
the nodes were made in).
"""
from __future__ import annotations

import zlib

import numpy as np

from tests import huffman_craft as H

CHUNK, TC, TPB, G, SYNC, L1, EMIT_LDS = 1024, 64, 256, 256, 64, 11, 40960
FAMILIES = ("fixed", "long_short", "l1_edge", "sizes", "emit_threshold", "dup", "invalid")
FIXED_L = (1, 2, 6, 8, 11, 12, 15)
# the entry of every family whose dictionary also codes a whole image file (every byte has a code)
WRAPPED = {"fixed": "fixed_8", "long_short": "long_short_255", "l1_edge": "l1_10_11_12", "sizes": "sizes_257_chunks",
           "emit_threshold": "emit_below", "dup": "dup_9"}


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ------------------------------------------------------------------------------ dictionaries
def spaced_words(L: int, d: int) -> list[int]:
    """The L-bit words whose ones lie at least d + 1 positions apart."""
    out = []
    for w in range(1 << L):
        ones = [i for i in range(L) if (w >> i) & 1]
        if all(b - a > d for a, b in zip(ones, ones[1:])):
            out.append(w)
    return out


def fixed_spacing(L: int) -> int:
    d = 0
    while len(spaced_words(L, d)) > 256:
        d += 1
    return d


def fixed_dict(L: int, rng):
    """(groups, d): see the module docstring."""
    d = fixed_spacing(L)
    words = spaced_words(L, d)
    if L > 8:
        have = set(words)
        while len(words) < 256:
            w = int(rng.integers(1, 1 << L))
            if w not in have:
                have.add(w)
                words.append(w)
    keys = rng.permutation(256)[: len(words)]
    entries = [(int(k), int(w)) for k, w in zip(keys, words)]
    order = rng.permutation(len(entries))
    return H.split_groups(L, [entries[i] for i in order]), d


def spaced_stream(rng, nbits: int, d: int) -> np.ndarray:
    """nbits random bits whose ones lie at least d + 1 apart."""
    if d == 0:
        return rng.integers(0, 2, size=nbits).astype(np.uint8)
    out = np.zeros(nbits, dtype=np.uint8)
    draw = rng.random(nbits) < 0.4
    last = -d - 1
    for i in np.flatnonzero(draw):
        if i - last > d:
            out[i] = 1
            last = i
    return out


def long_short_dict(rng, nlong: int):
    """'0' in one bit; nlong scattered 15-bit words that begin with 1; the 15-bit groups first."""
    words = rng.choice(1 << 14, size=nlong, replace=False) + (1 << 14)
    keys = rng.permutation(256)
    longs = [(int(k), int(w)) for k, w in zip(keys[1: nlong + 1], words)]
    return H.split_groups(15, longs) + [(1, [(int(keys[0]), 0)])]


def l1_dict(rng):
    """64 scattered slots of 8/4096 of the code space (slot 0 among them), each holding an 11-bit
    code, the two 12-bit codes on the next 11-bit prefix, and a 10-bit code."""
    slots = [0] + [int(s) for s in rng.choice(np.arange(1, 512), size=63, replace=False)]
    keys = [int(k) for k in rng.permutation(256)]
    c10, c11, c12 = [], [], []
    for i, s in enumerate(slots):
        base = s << 3  # in 12-bit units
        c11.append((keys[4 * i], base >> 1))
        c12.append((keys[4 * i + 1], base + 2))
        c12.append((keys[4 * i + 2], base + 3))
        c10.append((keys[4 * i + 3], (base + 4) >> 2))
    return H.split_groups(12, c12, [127, 1]) + H.split_groups(10, c10) + H.split_groups(11, c11)


def comb_dict(rng):
    """1, 01, 001, ... 0^13 1, then the two 15-bit leaves 0^14 1 and 0^15: complete, depth 15."""
    keys = [int(k) for k in rng.permutation(256)[:16]]
    groups = [(b, [(keys[b - 1], 1)]) for b in range(1, 15)]
    groups.append((15, [(keys[14], 1), (keys[15], 0)]))
    return [groups[i] for i in rng.permutation(len(groups))]


def sizes_dict(rng):
    """63 codes of 7 bits, 63 of 8 and 130 of 9, laid side by side from code word 0 (incomplete: the
    last 4/512 of the code space are free), written in 5 groups so that the dictionary and its stop
    bit fill whole bytes: the code stream begins on a byte."""
    keys = [int(k) for k in rng.permutation(256)]
    c7 = [(keys[i], i) for i in range(63)]
    c8 = [(keys[63 + i], 126 + i) for i in range(63)]
    c9 = [(keys[126 + i], 378 + i) for i in range(130)]
    return H.split_groups(9, c9, [100, 29, 1]) + H.split_groups(7, c7) + H.split_groups(8, c8)


def emit_dict(rng):
    """31 codes of 6 bits and 63 of 7 (incomplete), in 3 groups: the code stream begins on a byte."""
    keys = [int(k) for k in rng.permutation(256)]
    c6 = [(keys[i], i) for i in range(31)]
    c7 = [(keys[31 + i], 64 + i) for i in range(63)]
    return H.split_groups(7, c7, [40, 23]) + H.split_groups(6, c6)


def dup_dict(rng):
    """All 512 words of 9 bits: byte perm[w & 255] has the code words w and w ^ 256."""
    perm = rng.permutation(256)
    entries = [(int(perm[w & 255]), w) for w in rng.permutation(512)]
    return H.split_groups(9, entries, [127, 127, 127, 127, 4])


def tiny_dict(rng):
    """10 and 11 alone: nothing begins with 0, so zero padding walks to no leaf."""
    return [(2, [(7, 2), (8, 3)])]


# ------------------------------------------------------------------------------ streams
def _random_codes(rng, groups, count: int):
    """`count` code words drawn uniformly from the dictionary: (codes [count, 2], symbols)."""
    flat = [(key, code, bits) for bits, entries in groups for key, code in entries]
    pick = rng.integers(0, len(flat), size=count)
    arr = np.asarray(flat, dtype=np.int64)[pick]
    return arr[:, 1:3], arr[:, 0].astype(np.uint8)


def _codes_to_bits(rng, groups, nbits: int, exact_lengths=(7, 8, 9)):
    """Random code words filling exactly nbits (the tail chosen among `exact_lengths`, which the
    dictionary must hold and which must reach every length from 3 * min on)."""
    by_len = {}
    for bits, entries in groups:
        by_len.setdefault(bits, []).extend(entries)
    lo, hi = min(exact_lengths), max(exact_lengths)
    codes, syms = _random_codes(rng, groups, nbits // min(by_len) + 1)  # more than fit
    keep = int(np.searchsorted(np.cumsum(codes[:, 1]), nbits - 3 * hi, side="right"))  # (3 * hi bits or more stay free)
    codes, syms = codes[:keep], syms[:keep]
    rem = nbits - int(codes[:, 1].sum())
    k = -(-rem // hi)
    assert lo * k <= rem, (rem, exact_lengths)
    lens = [lo] * k
    i = 0
    while sum(lens) < rem:
        if lens[i % k] < hi and lens[i % k] + 1 in exact_lengths:
            lens[i % k] += 1
        i += 1
    tail, tsym = [], []
    for ln in lens:
        key, code = by_len[ln][int(rng.integers(0, len(by_len[ln])))]
        tail.append((code, ln))
        tsym.append(key)
    codes = np.concatenate([codes.reshape(-1, 2), np.asarray(tail, dtype=np.int64).reshape(-1, 2)])
    return codes, np.concatenate([syms, np.asarray(tsym, dtype=np.uint8)])


def _long_short_codes(rng, groups, nchunks: int):
    """'0's and 15-bit codes; a 15-bit code starts off(j) = 1 + (j // 2) % 14 bits before the j-th
    half-chunk boundary, so that chunk ends (even j) and middles (odd j) both see every offset."""
    longs = [e for bits, entries in groups if bits == 15 for e in entries]
    short_key = next(entries[0][0] for bits, entries in groups if bits == 1)
    codes, syms, p = [], [], 0

    def put_long():
        key, code = longs[int(rng.integers(0, len(longs)))]
        codes.append((code, 15))
        syms.append(key)

    for j in range(1, 2 * nchunks):
        target = j * (CHUNK // 2) - (1 + (j // 2) % 14)
        while p < target:
            if target - p >= 15 and rng.random() < 0.12:
                put_long()
                p += 15
            else:
                codes.append((0, 1))
                syms.append(short_key)
                p += 1
        put_long()
        p += 15
    for _ in range(int(rng.integers(20, 200))):
        codes.append((0, 1))
        syms.append(short_key)
    return np.asarray(codes, dtype=np.int64), np.asarray(syms, dtype=np.uint8)


class Entry:
    """name, family, groups (the dictionary), the file, the code stream's first and end bit, and
    `symbols`: the symbols the builder coded (None for an invalid entry).  The decode yields these
    followed by whatever the padding bits decode to."""

    def __init__(self, family, name, build):
        self.family, self.name, self._build = family, name, build
        self._made = None

    def _make(self):
        if self._made is None:
            groups, stream, symbols = self._build(_rng(self.name))
            data, start, end = H.pack(groups, stream)
            self._made = (groups, data, start, end, None if symbols is None else bytes(bytearray(symbols)))
        return self._made

    groups = property(lambda self: self._make()[0])
    data = property(lambda self: self._make()[1])
    code_start = property(lambda self: self._make()[2])
    end_bit = property(lambda self: self._make()[3])
    symbols = property(lambda self: self._make()[4])

    @property
    def valid(self) -> bool:
        return self.family != "invalid"

    @property
    def lut(self) -> np.ndarray:
        if not hasattr(self, "_lut"):
            self._lut = H.prefix_table(self.groups)
            self._lut.setflags(write=False)
        return self._lut

    @property
    def model(self) -> H.Model:
        if not hasattr(self, "_model"):
            self._model = H.Model(self.data, self.lut, self.code_start)
        return self._model

    @property
    def chunks(self) -> int:
        return self.model.nchunks(CHUNK)


# ------------------------------------------------------------------------------ the families
def _fixed(L, nchunks):
    def build(rng):
        groups, d = fixed_dict(L, rng)
        nsym = (nchunks * CHUNK - int(rng.integers(0, 600))) // L
        bits = spaced_stream(rng, nsym * L, d)
        word = {code: key for _, entries in groups for key, code in entries}
        vals = bits.reshape(nsym, L).astype(np.int64) @ (1 << np.arange(L - 1, -1, -1, dtype=np.int64))
        return groups, bits, [word[int(v)] for v in vals]
    return build


def _long_short(nlong, nchunks):
    def build(rng):
        groups = long_short_dict(rng, nlong)
        codes, syms = _long_short_codes(rng, groups, nchunks)
        return groups, codes, syms
    return build


def _drawn(make_dict, nbits_of):
    """Uniform draws over the dictionary's code words, about nbits_of(rng) bits of them."""
    def build(rng):
        groups = make_dict(rng)
        flat = [bits for bits, entries in groups for _ in entries]
        codes, syms = _random_codes(rng, groups, int(nbits_of(rng) * len(flat) / sum(flat)))
        return groups, codes, syms
    return build


def _sized(nbits_of, trim=0):
    """The sizes dictionary and a code stream of exactly nbits_of(code_start) bits; trim = -1 drops
    its last code, +1 appends one."""
    def build(rng):
        groups = sizes_dict(rng)
        start = int(H.dictionary_bits(groups).size)
        codes, syms = _codes_to_bits(rng, groups, nbits_of(start))
        if trim < 0:
            codes, syms = codes[:-1], syms[:-1]
        if trim > 0:
            c, s = _random_codes(rng, groups, 1)
            codes, syms = np.concatenate([codes, c]), np.concatenate([syms, s])
        return groups, codes, syms
    return build


def _emit_pattern(extra: bool):
    """TPB chunks of 6 6 6 7 7; with `extra`, three periods somewhere are sixteen 6-bit codes (the
    same 96 bits, one symbol more)."""
    def build(rng):
        groups = emit_dict(rng)
        by_len = {bits: entries for bits, entries in groups if bits == 6}
        by_len[7] = [e for bits, entries in groups if bits == 7 for e in entries]
        periods = TPB * CHUNK // 32
        at = int(rng.integers(periods // 4, periods // 2)) if extra else -1
        lens = []
        k = 0
        while k < periods:
            if k == at:
                lens += [6] * 16
                k += 3
            else:
                lens += [6, 6, 6, 7, 7]
                k += 1
        codes, syms = [], []
        for ln in lens:
            key, code = by_len[ln][int(rng.integers(0, len(by_len[ln])))]
            codes.append((code, ln))
            syms.append(key)
        return groups, np.asarray(codes, dtype=np.int64), syms
    return build


def _with_hole(base, where):
    """The valid build `base` with 15 bits no code prefixes put between two codes: `where` maps
    (rng, code starts relative to the stream, total bits) to the index of the code they go before."""
    def build(rng):
        groups, codes, _ = base(rng)
        bits = H.code_bits(codes) if np.asarray(codes).ndim == 2 else np.asarray(codes)
        lut = H.prefix_table(groups)
        starts = np.asarray(H.Model(np.packbits(bits).tobytes(), lut, 0).path(), dtype=np.int64)
        starts = starts[starts < bits.size]
        at = int(starts[where(rng, starts, int(bits.size))])
        hole = H._field([H.no_code_word(lut)], 15)
        return groups, np.concatenate([bits[:at], hole, bits[at:]]), None
    return build


def _padding_hole(rng):
    groups = tiny_dict(rng)
    start = int(H.dictionary_bits(groups).size)
    n = 40
    while (start + 2 * n) % 8 == 0:
        n += 1
    codes = [(int(c), 2) for c in rng.integers(2, 4, size=n)]
    return groups, np.asarray(codes, dtype=np.int64), None


def _first_in(lo, hi):
    """The first code at or after bit `lo` (negative: from the end) that starts before `hi`."""
    def where(rng, starts, total):
        a = lo if lo >= 0 else total + lo
        i = int(np.searchsorted(starts, a))
        assert i < starts.size and (hi is None or starts[i] < (hi if hi >= 0 else total + hi)), (a, hi)
        return i
    return where


_ENTRIES = None


def entries() -> list[Entry]:
    global _ENTRIES
    if _ENTRIES is not None:
        return _ENTRIES
    out = []

    def add(family, name, build):
        out.append(Entry(family, name, build))

    for L in FIXED_L:
        add("fixed", f"fixed_{L}", _fixed(L, TC + 3))
    add("long_short", "long_short_200", _long_short(200, 70))
    add("long_short", "long_short_255", _long_short(255, 30))
    add("l1_edge", "l1_10_11_12", _drawn(l1_dict, lambda rng: 66 * CHUNK + int(rng.integers(0, CHUNK))))
    add("l1_edge", "l1_comb", _drawn(comb_dict, lambda rng: 66 * CHUNK + int(rng.integers(0, CHUNK))))
    add("sizes", "sizes_short", _sized(lambda s: 301))
    add("sizes", "sizes_3_chunks_exact", _sized(lambda s: 3 * CHUNK))
    add("sizes", "sizes_3_chunks_minus", _sized(lambda s: 3 * CHUNK, trim=-1))
    add("sizes", "sizes_3_chunks_plus", _sized(lambda s: 3 * CHUNK, trim=1))
    for n in (TC, TC + 1, TPB, TPB + 1):
        add("sizes", f"sizes_{n}_chunks", _sized(lambda s, n=n: n * CHUNK - 8 * (13 + n % 7) - 3))
    add("emit_threshold", "emit_exact", _emit_pattern(False))
    add("emit_threshold", "emit_plus_one", _emit_pattern(True))
    add("emit_threshold", "emit_below", _fixed(8, TPB + 2))
    add("emit_threshold", "emit_above", _fixed(1, TPB + 2))
    add("dup", "dup_9", _drawn(dup_dict, lambda rng: 40 * CHUNK + int(rng.integers(0, CHUNK))))
    add("invalid", "invalid_first_chunk", _with_hole(_long_short(200, 5), _first_in(100, 400)))
    add("invalid", "invalid_second_half", _with_hole(_drawn(l1_dict, lambda rng: 5 * CHUNK + 77),
                                                      _first_in(2 * CHUNK + 600, 2 * CHUNK + 700)))
    add("invalid", "invalid_last_chunk", _with_hole(_sized(lambda s: 7 * CHUNK - 100), _first_in(-400, None)))
    add("invalid", "invalid_past_256", _with_hole(_drawn(emit_dict, lambda rng: (TPB + 3) * CHUNK - 50), _first_in(-300, None)))
    add("invalid", "invalid_padding", _padding_hole)
    assert len({e.name for e in out}) == len(out)
    _ENTRIES = out
    return out


def by_family(family: str) -> list[Entry]:
    return [e for e in entries() if e.family == family]


def by_name(name: str) -> Entry:
    return next(e for e in entries() if e.name == name)


def valid_entries() -> list[Entry]:
    return [e for e in entries() if e.valid]


# ------------------------------------------------------------------------------ whole image files
WRAP_DIMS = {"sizes": (256, 256)}  # the other families: 64 x 32
WRAP_GEN = {"fixed": ("M", 31), "long_short": ("U", 32), "l1_edge": ("M", 33), "sizes": ("U", 34),
            "emit_threshold": ("U", 35), "dup": ("M", 36)}
_WRAPPED = {}


def wrap_dims(family: str):
    return WRAP_DIMS.get(family, (64, 32))


def wrapped(family: str):
    """(name, file, plain): an image file whose Huffman pass uses the dictionary of WRAPPED[family].
    `plain` is what the pass coded: the oracle's 4x4 encode of a seeded picture without its
    passthrough bit (a Huffman-coded file decodes to the settings header from bit 0)."""
    if family not in _WRAPPED:
        from imageencoder_amd import synth
        from tests import oracle_lib as O
        e = by_name(WRAPPED[family])
        rng = _rng("wrap_" + e.name)
        w, h = wrap_dims(family)
        gen, seed = WRAP_GEN[family]
        y = synth.frame(gen, w, h, seed=seed)
        enc = O.load().encode_image(y, 4, O.read_matrix("matrix.txt", 4), rle=True, huffman=False)
        bits = np.unpackbits(np.frombuffer(enc, dtype=np.uint8))
        assert bits[0] == 0
        plain = np.packbits(bits[1:])
        cm = H.code_map(e.groups)
        assert set(cm) == set(range(256)), "every byte value needs a code"
        which = rng.integers(0, 1 << 30, size=plain.size)
        codes = np.asarray([cm[int(b)][int(r) % len(cm[int(b)])] for b, r in zip(plain, which)], dtype=np.int64)
        data, _, _ = H.pack(e.groups, codes)
        _WRAPPED[family] = (e.name, data, plain.tobytes())
    return _WRAPPED[family]
