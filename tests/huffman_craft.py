"""A builder for Huffman-coded streams, and a serial model of their decode, for tests.

Plain Python and numpy -- no GPU, no library code -- so a test can hand the Huffman decoders any
stream the format allows, not only what the encoder's tree builder writes.  The layout restated here
(Huffman.cpp:120-173, 354-402):

  file    groups ... '0' codes ... zero bits to the next byte
  group   '1' count:7 bits:4, then count entries  key:8 code:bits   (MSB first)

A dictionary is a list of groups (bits, [(key, code word), ...]) of at most 127 entries each, in
the order they are written.  A stream is the dictionary plus a list of (code word, bits) pairs, or
raw bits where a test wants a position no code prefixes.

The decode walks the code stream bit by bit from the first bit after the stop bit to the end of the
last byte; a code that begins inside the padding runs on into zero bits until it completes.
Model.decode() is that walk; the other methods restate what the device passes derive from it for a
chunk length C: every chunk's true entry offset, the boundaries its 15 entry walks stand on after
`sync` bits (a position no code prefixes slides one bit), and the symbols per chunk and per half.
"""
from __future__ import annotations

import numpy as np

MAX_GROUP = 127
MAX_BITS = 15


def _field(vals, width: int) -> np.ndarray:
    """The low `width` bits of every value, MSB first, as a flat 0/1 array."""
    v = np.asarray(vals, dtype=np.int64).reshape(-1, 1)
    if width == 0 or v.size == 0:
        return np.zeros(0, dtype=np.uint8)
    return ((v >> np.arange(width - 1, -1, -1, dtype=np.int64)) & 1).astype(np.uint8).ravel()


def split_groups(bits: int, entries, sizes=None):
    """`entries` of one code length as groups of at most 127 (or of the given sizes)."""
    entries = list(entries)
    if sizes is None:
        sizes = [MAX_GROUP] * (len(entries) // MAX_GROUP) + ([len(entries) % MAX_GROUP] if len(entries) % MAX_GROUP else [])
    assert sum(sizes) == len(entries) and all(0 < s <= MAX_GROUP for s in sizes)
    out, at = [], 0
    for s in sizes:
        out.append((bits, entries[at: at + s]))
        at += s
    return out


def dictionary_bits(groups) -> np.ndarray:
    """The dictionary and its stop bit."""
    parts = []
    for bits, entries in groups:
        assert 1 <= bits <= MAX_BITS and 1 <= len(entries) <= MAX_GROUP
        parts += [_field([1], 1), _field([len(entries)], 7), _field([bits], 4)]
        rows = np.zeros((len(entries), 8 + bits), dtype=np.uint8)
        for i, (key, code) in enumerate(entries):
            assert 0 <= key < 256 and 0 <= code < (1 << bits)
            rows[i, :8] = _field([key], 8)
            rows[i, 8:] = _field([code], bits)
        parts.append(rows.ravel())
    parts.append(_field([0], 1))
    return np.concatenate(parts)


def code_bits(codes) -> np.ndarray:
    """The bits of a list of (code word, length) pairs, lengths mixed."""
    codes = np.asarray(codes, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(int(codes[:, 1].sum()), dtype=np.uint8)
    ends = np.cumsum(codes[:, 1])
    starts = ends - codes[:, 1]
    for ln in np.unique(codes[:, 1]):
        sel = codes[:, 1] == ln
        idx = starts[sel].reshape(-1, 1) + np.arange(ln, dtype=np.int64)
        out[idx.ravel()] = _field(codes[sel, 0], int(ln))
    return out


def pack(groups, stream) -> tuple[bytes, int, int]:
    """The file of a dictionary and a code stream (an array of bits, or (code word, length) pairs):
    (bytes, the code stream's first bit, its end bit before the padding)."""
    d = dictionary_bits(groups)
    s = np.asarray(stream)
    s = s.astype(np.uint8) if s.ndim == 1 else code_bits(s)
    return np.packbits(np.concatenate([d, s])).tobytes(), int(d.size), int(d.size + s.size)


def prefix_table(groups) -> np.ndarray:
    """sym | len << 8 for every 15-bit prefix; 0 where no code word is a prefix.  A code word that
    is a prefix of another is left to the caller to avoid (the reference leaves it undefined)."""
    lut = np.zeros(1 << MAX_BITS, dtype=np.uint16)
    for bits, entries in groups:
        for key, code in entries:
            lo = code << (MAX_BITS - bits)
            assert not lut[lo: lo + (1 << (MAX_BITS - bits))].any(), "code words overlap"
            lut[lo: lo + (1 << (MAX_BITS - bits))] = key | (bits << 8)
    return lut


def code_map(groups) -> dict:
    """key -> [(code word, length), ...] in dictionary order."""
    m = {}
    for bits, entries in groups:
        for key, code in entries:
            m.setdefault(key, []).append((code, bits))
    return m


def no_code_word(lut: np.ndarray) -> int:
    """The smallest 15-bit string no code prefixes."""
    free = np.flatnonzero(lut == 0)
    assert free.size, "the code is complete"
    return int(free[0])


class Model:
    """The serial decode of one file: positions are file bits."""

    def __init__(self, data: bytes, lut: np.ndarray, code_start: int):
        self.data, self.lut, self.start = data, lut, code_start
        self.nbits = 8 * len(data)
        bits = np.concatenate([np.unpackbits(np.frombuffer(data, dtype=np.uint8)), np.zeros(MAX_BITS, dtype=np.uint8)])
        win = np.zeros(self.nbits, dtype=np.int64)  # the 15 bits from every position, zeros past the end
        for k in range(MAX_BITS):
            win = (win << 1) | bits[k: k + self.nbits]
        e = lut[win]
        self.len_at = (e >> 8).astype(np.int64)
        self.sym_at = (e & 0xFF).astype(np.uint8)
        self._path = None

    def path(self):
        """The positions of the true path's codes, or None when it meets a position no code
        prefixes (the oracle's None)."""
        if self._path is None:
            pos, p, ln = [], self.start, self.len_at
            while p < self.nbits:
                if ln[p] == 0:
                    pos = None
                    break
                pos.append(p)
                p += int(ln[p])
            self._path = (pos,)
        return self._path[0]

    def decode(self):
        """The symbols of the per-bit walk, the padding's included; None for an invalid stream."""
        pos = self.path()
        return None if pos is None else self.sym_at[np.asarray(pos, dtype=np.int64)].tobytes()

    def nchunks(self, C: int) -> int:
        return (self.nbits - self.start + C - 1) // C

    def chunk_entries(self, C: int) -> list[int]:
        """Every chunk's true entry offset: the first code of the true path at or after its first bit."""
        pos = np.asarray(self.path(), dtype=np.int64)
        out = []
        for k in range(self.nchunks(C)):
            cs = self.start + k * C
            i = int(np.searchsorted(pos, cs, side="left"))
            nxt = int(pos[i]) if i < pos.size else int(pos[-1] + self.len_at[pos[-1]])
            out.append(nxt - cs)
        return out

    def chunk_counts(self, C: int):
        """(symbols whose code starts in each chunk, of those the ones before the first boundary at
        or past the chunk's middle)."""
        pos = np.asarray(self.path(), dtype=np.int64) - self.start
        n = self.nchunks(C)
        whole = np.bincount(pos // C, minlength=n)
        first = np.zeros(n, dtype=np.int64)
        for k in range(n):
            first[k] = np.searchsorted(pos, k * C + C // 2, side="left") - np.searchsorted(pos, k * C, side="left")
        return whole, first

    def survivors(self, C: int, sync: int) -> list[int]:
        """Per chunk: the distinct boundaries inside it that its 15 entry walks stand on once they
        have passed `sync` bits (no code at a position: one bit on; past the stream: the chunk's end)."""
        out = []
        for k in range(self.nchunks(C)):
            cs = self.start + k * C
            ce = cs + C
            stop = min(cs + sync, ce)
            seen = set()
            for d in range(MAX_BITS):
                p = cs + d
                while p < stop:
                    p = ce if p >= self.nbits else p + (int(self.len_at[p]) or 1)
                p = min(p, ce)
                if p < ce:
                    seen.add(p)
            out.append(len(seen))
        return out

    def sliding_entries(self, C: int, sync: int) -> list[int]:
        """Per chunk: how many of its 15 entry walks meet a position no code prefixes within
        `sync` bits."""
        out = []
        for k in range(self.nchunks(C)):
            cs = self.start + k * C
            stop = min(cs + sync, cs + C, self.nbits)
            n = 0
            for d in range(MAX_BITS):
                p = cs + d
                while p < stop and self.len_at[p]:
                    p += int(self.len_at[p])
                n += p < stop
            out.append(n)
        return out

    def long_codes(self, C: int, lo: int = 12) -> np.ndarray:
        """Per chunk: the true path's codes of at least `lo` bits that start in it."""
        pos = np.asarray(self.path(), dtype=np.int64)
        sel = pos[self.len_at[pos] >= lo] - self.start
        return np.bincount(sel // C, minlength=self.nchunks(C))

    def straddles(self, C: int, bits: int = MAX_BITS):
        """(offsets at chunk ends, offsets at chunk middles): for every code of `bits` bits on the
        true path that begins before such a boundary and ends after it, the bits before it."""
        pos = np.asarray(self.path(), dtype=np.int64)
        pos = pos[self.len_at[pos] == bits] - self.start
        ends, mids = set(), set()
        for p in pos:
            b = (int(p) // (C // 2) + 1) * (C // 2)  # the next half-chunk boundary after p
            if p < b < p + bits and int(p) % (C // 2):
                (mids if (b // (C // 2)) % 2 else ends).add(b - int(p))
        return ends, mids
