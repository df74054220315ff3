"""A stream builder for tests: image and video files written record by record.

Plain Python and numpy -- no GPU, no library code -- so a test can hand the decoders any stream the
format allows, not only what an encoder writes.  The layout restated here:

  file    [0 passthrough bit] qb:5  q[N*N] each qb wide  rle:1  W:15  H:15
          (video: frames:15 gop:15 merange:15)  records ...  zero bits to the next byte
  record  bl:4, then with RLE lw in bl bits, then lw (RLE) or N*N (no RLE) values, each bl bits
          wide, two's complement, MSB first.  bl = 0 is a 4-bit record of no values: get(0) reads 0.

A record is the tuple (bl, lw, values); without RLE lw is N*N.  Values are given signed; only their
low bl bits are stored.
"""
from __future__ import annotations

import numpy as np


def _field(vals, width: int) -> np.ndarray:
    """The low `width` bits of every value, MSB first, as a flat 0/1 array."""
    v = np.asarray(vals, dtype=np.int64).reshape(-1, 1)
    if width == 0 or v.size == 0:
        return np.zeros(0, dtype=np.uint8)
    return ((v >> np.arange(width - 1, -1, -1, dtype=np.int64)) & 1).astype(np.uint8).ravel()


def bits_of(value: int, width: int) -> np.ndarray:
    return _field([value], width)


def matrix_bits(q) -> int:
    """The width the matrix is stored with: the bit length of its largest entry."""
    return max(1, int(max(int(v) for v in q)).bit_length())


def header_bits(n: int, q, rle, w: int, h: int, video=None) -> np.ndarray:
    """Passthrough bit, 5-bit matrix width, matrix, rle, 15-bit W and H; video = (frames, gop,
    merange) appends three 15-bit fields."""
    q = [int(v) for v in np.asarray(q).ravel()]
    assert len(q) == n * n
    qb = matrix_bits(q)
    parts = [bits_of(0, 1), bits_of(qb, 5), _field(q, qb), bits_of(1 if rle else 0, 1), bits_of(w, 15), bits_of(h, 15)]
    if video is not None:
        parts += [bits_of(int(x), 15) for x in video]
    return np.concatenate(parts)


def record_bits(rec, n: int, rle) -> np.ndarray:
    bl, lw, vals = rec
    assert 0 <= bl <= 15
    if rle:
        assert 0 <= lw < (1 << bl) and lw <= n * n, (bl, lw)  # (bl = 0: no count bits, lw = 0)
    else:
        assert lw == n * n
    assert len(vals) == lw
    parts = [bits_of(bl, 4)]
    if rle:
        parts.append(bits_of(lw, bl))
    parts.append(_field(vals, bl))
    return np.concatenate(parts)


def record_len(rec, rle) -> int:
    bl, lw, _ = rec
    return 4 + bl * (lw + (1 if rle else 0))


def _finish(parts) -> bytes:
    bits = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return np.packbits(bits).tobytes()  # (zero bits to the next byte)


def pack(records, n: int, q, rle, w: int, h: int):
    """An image file of `records` (one per block, (w / n) * (h / n) of them).  Returns (bytes,
    positions): the file and the bit position of every record, plus the end bit as last entry."""
    assert w % n == 0 and h % n == 0 and len(records) == (w // n) * (h // n)
    parts = [header_bits(n, q, rle, w, h)]
    pos = [int(parts[0].size)]
    for r in records:
        b = record_bits(r, n, rle)
        parts.append(b)
        pos.append(pos[-1] + int(b.size))
    return _finish(parts), pos


def mvec_bits(merange: int) -> int:
    """The width of a motion vector component: the signed value `merange`'s (1 bit for 0)."""
    return int(merange).bit_length() + 1


def pack_video(frames, n: int, q, rle, w: int, h: int, gop: int, merange: int, positions: bool = False):
    """A video file.  frames: one (mvecs, records) per frame; mvecs is None for an I-frame, else
    one (vx, vy) per 16x16 macroblock, each stored in the bit length of merange plus a sign bit
    as the encoder sizes it (the width of the signed value `merange`): any value of that field is
    valid, not only those inside [-merange, merange].

    With positions the result is (bytes, pos): pos[f] = dict(start = the frame's first bit, vec =
    the first bit of every macroblock's vector pair ([] for an I-frame), rec = the first bit of
    every record, end = the frame's end bit, which is the next frame's first)."""
    mv = mvec_bits(merange)
    lo, hi = -(1 << (mv - 1)), (1 << (mv - 1)) - 1
    parts = [header_bits(n, q, rle, w, h, video=(len(frames), gop, merange))]
    at = int(parts[0].size)
    pos = []
    for f, (mvecs, records) in enumerate(frames):
        assert (mvecs is None) == (f % gop == 0)
        assert len(records) == (w // n) * (h // n)
        fp = dict(start=at, vec=[], rec=[])
        if mvecs is not None:
            assert len(mvecs) == (w // 16) * (h // 16)
            v = np.asarray(mvecs, dtype=np.int64).reshape(-1, 2)
            assert v.size == 0 or (lo <= v.min() and v.max() <= hi), (f, mv)
            parts.append(_field(v.ravel(), mv))
            fp["vec"] = [at + 2 * mv * k for k in range(len(mvecs))]
            at += 2 * mv * len(mvecs)
        for r in records:
            b = record_bits(r, n, rle)
            parts.append(b)
            fp["rec"].append(at)
            at += int(b.size)
        fp["end"] = at
        pos.append(fp)
    return (_finish(parts), pos) if positions else _finish(parts)


class _Reader:
    def __init__(self, data: bytes):
        self.bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8))
        self.pos = 0

    def get(self, width: int) -> int:
        return int(self.fields(1, width)[0]) if width else 0

    def fields(self, count: int, width: int) -> np.ndarray:
        """`count` unsigned fields of `width` bits; bits past the end read 0."""
        need = count * width
        if need == 0:
            return np.zeros(count, dtype=np.int64)
        b = self.bits[self.pos: self.pos + need]
        if b.size < need:
            b = np.concatenate([b, np.zeros(need - b.size, dtype=np.uint8)])
        self.pos += need
        return b.reshape(count, width).astype(np.int64) @ (1 << np.arange(width - 1, -1, -1, dtype=np.int64))


def _signed(v: np.ndarray, width: int) -> np.ndarray:
    return np.where(v >= (1 << (width - 1)), v - (1 << width), v) if width else v


def parse(data: bytes, n: int):
    """The serial parse of an image file written without the Huffman pass.  Returns (records, q,
    rle, w, h, positions), records and positions as pack takes and returns them."""
    rd = _Reader(data)
    assert rd.get(1) == 0, "Huffman-coded file"
    qb = rd.get(5)
    q = rd.fields(n * n, qb)
    rle = bool(rd.get(1))
    w, h = rd.get(15), rd.get(15)
    records, pos = [], [rd.pos]
    for _ in range((w // n) * (h // n)):
        bl = rd.get(4)
        lw = rd.get(bl) if rle else n * n
        assert lw <= n * n, "value count beyond the block"
        vals = _signed(rd.fields(lw, bl), bl)
        records.append((bl, lw, [int(v) for v in vals]))
        pos.append(rd.pos)
    return records, q.astype(np.uint16), rle, w, h, pos


def parse_video(data: bytes, n: int):
    """The serial parse of a video file written without the Huffman pass, the twin of pack_video.
    Returns (frames, q, rle, w, h, gop, merange, positions), frames and positions as pack_video
    takes and returns them."""
    rd = _Reader(data)
    assert rd.get(1) == 0, "Huffman-coded file"
    qb = rd.get(5)
    q = rd.fields(n * n, qb)
    rle = bool(rd.get(1))
    w, h = rd.get(15), rd.get(15)
    nframes, gop, merange = rd.get(15), max(1, rd.get(15)), rd.get(15)
    mv = mvec_bits(merange)
    nmb = (w // 16) * (h // 16)
    frames, pos = [], []
    for f in range(nframes):
        fp = dict(start=rd.pos, vec=[], rec=[])
        mvecs = None
        if f % gop:
            fp["vec"] = [rd.pos + 2 * mv * k for k in range(nmb)]
            v = _signed(rd.fields(2 * nmb, mv), mv).reshape(nmb, 2)
            mvecs = [(int(a), int(b)) for a, b in v]
        records = []
        for _ in range((w // n) * (h // n)):
            fp["rec"].append(rd.pos)
            bl = rd.get(4)
            lw = rd.get(bl) if rle else n * n
            assert lw <= n * n, "value count beyond the block"
            records.append((bl, lw, [int(x) for x in _signed(rd.fields(lw, bl), bl)]))
        fp["end"] = rd.pos
        frames.append((mvecs, records))
        pos.append(fp)
    return frames, q.astype(np.uint16), rle, w, h, gop, merange, pos
