"""Constructed streams: valid files of the format that no encoder here writes.

One named, seeded table (entries()), shared by the CPU tests (tests/test_crafted_streams.py), the
golden generator (tests/golden/make_golden_crafted.py: the reference's own decode of every entry,
pinned by md5 in manifest_crafted.json) and the GPU tests (tests/test_gpu_decode_crafted.py).
Only the table is committed: stream_craft.pack rebuilds every file.

Families
  width        every field width bl = 1..15 in one image, value counts 0, 1, N*N-1, N*N and random,
               values at both ends of the range; RLE on and off; the reference matrix, all ones
               and all 65535 (+-16384 x 65535 saturates far beyond the clamp)
  zero_width   bl = 0 records (4 bits, a block of zeros: get(0) reads 0): a whole image of them,
               alternating with long records, in runs that cross chunk boundaries, first and last
  lengths      at bl = 1, 5, 12 every value count the count field can hold up to N*N; value lists
               that end in zeros; widths wider than the values need
  boundary     images of longest records (bl = 15, N*N values: D bits) behind a lead record whose
               size sweeps the chunk boundaries over the offsets inside a record
  format_fuzz  uniform draws over bl, the value count and the values
  ties         blocks whose exact inverse transform is an integer (or an integer + k/4) at every
               pixel, around 0 and 255: the output is a truncation, so these must come out exact
  big          256x256 4x4 images with more than 256 records in a chunk (the decode walks again)
"""
from __future__ import annotations

import zlib
from fractions import Fraction

import numpy as np

from tests import matrix_sweep, oracle_lib as O
from tests import stream_craft as S

FAMILIES = ("width", "zero_width", "lengths", "boundary", "format_fuzz", "ties", "big")


# ------------------------------------------------------------------------------ shared pieces
def matrix(n: int, name: str) -> np.ndarray:
    if name == "ref":
        return O.read_matrix("matrix.txt" if n == 4 else "matrix8_1.txt", n)
    if name == "ones":
        return np.ones(n * n, dtype=np.uint16)
    if name == "max":
        return np.full(n * n, 65535, dtype=np.uint16)
    return matrix_sweep.by_name(n, name)


def zigzag(n: int) -> list[int]:
    """Natural index of every zig-zag rank (algo.cpp:33-37, 68-87)."""
    def key(i):
        x, y = i % n, i // n
        return (x + y, y if (x - y) & 1 else x)
    return sorted(range(n * n), key=key)


def entry_span(n: int) -> int:
    """D: the longest record, 4 + 15 (N*N + 1) bits."""
    return 4 + 15 * (n * n + 1)


def planned_chunk_bits(n: int, span: int, nblocks: int) -> int:
    """The chunk length the library plans for a record span (ie_capi_decode.cpp plan_chunks): about
    24 (4x4) / 28 (8x8) records per chunk, a multiple of 32 within [256, 2^15]."""
    recs = 24 if n == 4 else 28
    want = max((nblocks + recs - 1) // recs, 1)
    c = (span + want - 1) // want
    return min(max((c + 31) // 32 * 32, 256), 1 << 15)


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _full(rng, bl: int, count: int) -> list[int]:
    """`count` values uniform over the whole range of a bl-bit field."""
    if bl == 0:
        return [0] * count
    return [int(v) for v in rng.integers(-(1 << (bl - 1)), 1 << (bl - 1), size=count)]


def _edges(bl: int) -> list[int]:
    lo, hi = -(1 << (bl - 1)), (1 << (bl - 1)) - 1
    return [v for v in (lo, hi, -1, 0, 1) if lo <= v <= hi]  # (a 1-bit field holds -1 and 0)


def _fit(n: int, rle, bl: int, lw: int) -> int:
    """The value count nearest lw that a record of width bl can state."""
    return min(lw, n * n, (1 << bl) - 1) if rle else n * n


def _rec(rng, n, rle, bl, lw, edges_at=None):
    lw = _fit(n, rle, bl, lw)
    vals = _full(rng, bl, lw)
    if edges_at is not None and bl:
        ed = _edges(bl)
        for k in range(min(lw, len(ed))):  # (fewer values than edges: the edges in turn over the records)
            vals[(edges_at + k) % lw] = ed[(edges_at // 15 + k) % len(ed)]
    return (bl, lw, vals)


def _longest(rng, n):
    return (15, n * n, _full(rng, 15, n * n))


class Entry:
    def __init__(self, family, name, n, rle, w, h, mat, build):
        self.family, self.name, self.n, self.rle, self.w, self.h, self.mat = family, name, n, bool(rle), w, h, mat
        self._build = build
        self._file = None

    @property
    def nblocks(self) -> int:
        return (self.w // self.n) * (self.h // self.n)

    @property
    def q(self) -> np.ndarray:
        return matrix(self.n, self.mat)

    def records(self):
        return self._build(_rng(self.name), self)

    def file(self):
        """(bytes, positions) of stream_craft.pack, built once."""
        if self._file is None:
            self._file = S.pack(self.records(), self.n, self.q, self.rle, self.w, self.h)
        return self._file

    @property
    def data(self) -> bytes:
        return self.file()[0]

    def chunk_entries(self):
        """(C, [d_k]): the planned chunk length for the whole file and every chunk's true entry
        offset -- the first record start (or the end of the records) at or after its first bit."""
        data, pos = self.file()
        hb = pos[0]
        C = planned_chunk_bits(self.n, 8 * len(data) - hb, self.nblocks)
        starts = np.asarray(pos, dtype=np.int64) - hb
        nch = max((8 * len(data) - hb + C - 1) // C, 1)
        ds = []
        for k in range(nch):
            i = int(np.searchsorted(starts, k * C, side="left"))
            if i < len(starts) - 1:  # (the last entry of pos is the end bit, not a record)
                ds.append(int(starts[i]) - k * C)
        return C, ds

    def chunk_record_counts(self):
        data, pos = self.file()
        hb = pos[0]
        C = planned_chunk_bits(self.n, 8 * len(data) - hb, self.nblocks)
        starts = (np.asarray(pos[:-1], dtype=np.int64) - hb) // C
        return C, np.bincount(starts)


# ------------------------------------------------------------------------------ the families
def _width(rng, e):
    nn = e.n * e.n
    recs = []
    for i in range(e.nblocks):
        bl = 1 + i % 15
        lw = [0, 1, nn - 1, nn, int(rng.integers(0, nn + 1))][(i // 15) % 5]
        recs.append(_rec(rng, e.n, e.rle, bl, lw, edges_at=i))
    return recs


def _zero(e):
    return (0, 0 if e.rle else e.n * e.n, [0] * (0 if e.rle else e.n * e.n))


ZERO_RUN = {4: 100, 8: 16}  # records per run of _zero_runs


def _zero_all(rng, e):
    return [_zero(e)] * e.nblocks


def _zero_alternate(rng, e):
    return [_zero(e) if i % 2 == 0 else _rec(rng, e.n, e.rle, 12 + (i // 2) % 4, e.n * e.n) for i in range(e.nblocks)]


def _zero_runs(rng, e):
    """Runs of bl = 0 records (4 bits each, with or without RLE) between pairs of long records,
    sized so that planned chunk boundaries fall inside the runs (tests/test_crafted_streams.py
    checks that they do)."""
    run = ZERO_RUN[e.n]
    recs = []
    while len(recs) < e.nblocks:
        recs += [_zero(e)] * run
        recs += [_rec(rng, e.n, e.rle, 15, e.n * e.n), _rec(rng, e.n, e.rle, 9, e.n * e.n)]
    return recs[: e.nblocks]


def _zero_first_last(rng, e):
    recs = [_rec(rng, e.n, e.rle, int(rng.integers(1, 13)), int(rng.integers(0, e.n * e.n + 1))) for _ in range(e.nblocks)]
    recs[0] = _zero(e)
    recs[-1] = _zero(e)
    return recs


def lengths_table(n: int) -> list[tuple[int, int]]:
    return [(bl, lw) for bl in (1, 5, 12) for lw in range(min(n * n, (1 << bl) - 1) + 1)]


def _lengths(part):
    def build(rng, e):
        tab = lengths_table(e.n)
        recs = []
        for i in range(e.nblocks):
            bl, lw = tab[(part * e.nblocks + i) % len(tab)]
            kind = i % 3
            if kind == 0:    # the whole range of the field
                vals = _full(rng, bl, lw)
            elif kind == 1:  # a width wider than the values need: -1, 0, 1 (and -2 .. 1 from bl = 5 on)
                vals = [int(v) for v in rng.integers(-1 if bl < 5 else -2, 2 if bl > 1 else 1, size=lw)]
            else:            # a list that ends in zeros (the encoder drops those)
                vals = _full(rng, bl, lw)
                for k in range(max(0, lw - 1 - lw // 3), lw):
                    vals[k] = 0
            recs.append((bl, lw, vals))
        return recs
    return build


# first records of the boundary sweep: (bl, lw, matrix); chosen (tests/test_crafted_streams.py
# checks the outcome) so that the chunks' true entry offsets reach 0, D - 1 and every 64-wide band
BOUNDARY_LEADS = {
    4: [(3, 0, "ref"), (1, 1, "ref"), (0, 0, "ones"), (1, 0, "max"), (2, 1, "ref"), (2, 2, "ones"), (3, 3, "max"),
        (2, 3, "ref"), (3, 2, "ones"), (5, 0, "max"), (5, 1, "ref"), (6, 13, "ones"), (6, 14, "max"), (6, 16, "ref"),
        (1, 0, "ones"), (0, 0, "max")],
    8: [(6, 35, "ref"), (5, 9, "ref"), (0, 0, "ref"), (1, 0, "ones"), (1, 1, "max"), (2, 1, "ref"), (2, 2, "ones"),
        (2, 3, "max"), (3, 0, "ref"), (3, 2, "ones"), (3, 3, "max"), (3, 4, "ref"), (3, 5, "ones"), (3, 6, "max"),
        (3, 7, "ref"), (4, 3, "ones")],
}
BOUNDARY_DIMS = {4: (128, 64), 8: (128, 128)}


def _boundary(lead):
    def build(rng, e):
        bl, lw = lead
        first = (bl, lw, _full(rng, bl, lw))
        return [first] + [_longest(rng, e.n) for _ in range(e.nblocks - 1)]
    return build


def _fuzz(rng, e):
    recs = []
    for _ in range(e.nblocks):
        bl = int(rng.integers(0, 16))
        recs.append(_rec(rng, e.n, e.rle, bl, int(rng.integers(0, e.n * e.n + 1))))
    return recs


def tie_positions(n: int) -> list[int]:
    """Natural indices of (0,0), (N/2,0), (0,N/2), (N/2,N/2): with the reference's C(0) = 1/2,
    C(u > 0) = sqrt(1/2) and cos((2i+1) pi / 4) = +-sqrt(1/2) every term is +-Y q / 4 on paper
    (for 4x4 blocks these are (2,0), (0,2), (2,2))."""
    h = n // 2
    return [0, h * n, h, h * n + h]


def _bits_for(v: int) -> int:
    b = 1
    while not -(1 << (b - 1)) <= v < (1 << (b - 1)):
        b += 1
    return b


def _ties(rng, e):
    n, q = e.n, [int(v) for v in e.q]
    zz = zigzag(n)
    rank = {nat: k for k, nat in enumerate(zz)}
    tp = tie_positions(n)
    recs = []
    for i in range(e.nblocks):
        kind = i % 4
        if kind == 0:
            # DC only: pixel = Y q / 4 + 128.  Around 0 (Y q near -512), around 255 (near 508) and
            # mid-range, every residue of Y q mod 4 the quantiser allows
            target = (-512, 508, 0)[(i // 4) % 3]
            y = int(np.floor(target / q[0])) + (i // 12) % 6 - 2
            y = max(-16384, min(16383, y))
            bl = min(15, _bits_for(y) + ((i // 4) % 2) * int(rng.integers(0, 4)))
            recs.append((bl, 1, [y]) if e.rle else (bl, n * n, [y] + [0] * (n * n - 1)))
            continue
        # the four positions, every pixel an integer: the structural products even, the sum of
        # all four a multiple of 4 (a sign flip of a term changes a pixel by half its product);
        # products of a size that leaves pixels inside [0, 255]
        for _ in range(1000):
            ys = []
            for k, p in enumerate(tp):
                y = int(rng.integers(-600 if k == 0 else -240, 601 if k == 0 else 241)) // q[p]
                ys.append(y + (y & 1 if (q[p] & 1 and k) else 0))
            a, b, c, d = [y * q[p] for y, p in zip(ys, tp)]
            pix4 = [512 + a + si * b + sj * c + si * sj * d for si in (1, -1) for sj in (1, -1)]  # 4 x pixel
            if b % 2 == 0 and c % 2 == 0 and d % 2 == 0 and (a + b + c + d) % 4 == 0 and any(ys[1:]) and \
                    any(0 <= x <= 1020 for x in pix4):
                break
        else:
            ys = [0, 0, 0, 0]
        vals = [0] * (n * n)
        for y, p in zip(ys, tp):
            vals[rank[p]] = y
        lw = max(rank[p] for p in tp) + 1 if e.rle else n * n
        bl = min(15, max(max(_bits_for(v) for v in ys), _bits_for(lw) - 1 if e.rle else 1) + (kind == 3) * 3)
        recs.append((bl, lw, vals[:lw]))
    return recs


def exact_pixels(n: int, q, rec) -> list[Fraction]:
    """The pixels t + 128 of a ties record in exact rational arithmetic: only the four positions
    of tie_positions may be non-zero, whose factors C(u) cos(...) are 1/2 (u = 0) and +-1/2
    (u = N/2, signs + - - + along the axis)."""
    zz = zigzag(n)
    h = n // 2
    half = Fraction(1, 2)
    s = [1, -1, -1, 1] * (n // 4)
    a = {0: [half] * n, h: [half * x for x in s]}
    bl, lw, vals = rec
    pix = [Fraction(128)] * (n * n)
    for k, v in enumerate(vals[:lw]):
        if v == 0:
            continue
        u, vv = divmod(zz[k], n)
        assert u in a and vv in a, "not a ties block"
        y = v * int(q[zz[k]])
        for i in range(n):
            for j in range(n):
                pix[i * n + j] += y * a[u][i] * a[vv][j]
    return pix


def _big_zero(rng, e):
    """2048 bl = 0 records in a row between long ones: about 780 records in each of the chunks they fill."""
    half = e.nblocks // 4
    return ([_longest(rng, e.n) for _ in range(half)] + [_zero(e)] * (2 * half) +
            [_longest(rng, e.n) for _ in range(e.nblocks - 3 * half)])


def _big_width(rng, e):
    """The same with bl = 1 (5 and 6 bits) and bl = 2 records in place of the bl = 0 ones."""
    half = e.nblocks // 4
    small = [_rec(rng, e.n, True, 1 + (i % 7 == 0), i % 3, edges_at=i) for i in range(2 * half)]
    return ([_rec(rng, e.n, True, 13 + i % 3, e.n * e.n, edges_at=i) for i in range(half)] + small +
            [_rec(rng, e.n, True, 13 + i % 3, e.n * e.n, edges_at=i) for i in range(e.nblocks - 3 * half)])


_ENTRIES = None


def entries() -> list[Entry]:
    global _ENTRIES
    if _ENTRIES is not None:
        return _ENTRIES
    out = []

    def add(family, name, n, rle, w, h, mat, build):
        out.append(Entry(family, name, n, rle, w, h, mat, build))

    for n in (4, 8):
        for rle in (1, 0):
            rs = "rle" if rle else "norle"
            for mat in ("ref", "ones", "max"):
                add("width", f"width_{n}_{rs}_{mat}", n, rle, 64, 64, mat, _width)
            for form, fn in (("all", _zero_all), ("alternate", _zero_alternate), ("runs", _zero_runs),
                             ("first_last", _zero_first_last)):
                add("zero_width", f"zero_{form}_{n}_{rs}", n, rle, 64, 64, "ref", fn)
            for i in range(16):
                add("format_fuzz", f"fuzz_{n}_{rs}_{i}", n, rle, 64, 64, ("ref", "ones", "max", "primes")[i % 4], _fuzz)
        parts = -(-len(lengths_table(n)) // ((64 // n) ** 2))
        for part in range(parts):
            add("lengths", f"lengths_{n}_{part}", n, 1, 64, 64, "ref", _lengths(part))
        w, h = BOUNDARY_DIMS[n]
        for i, (bl, lw, mat) in enumerate(BOUNDARY_LEADS[n]):
            add("boundary", f"boundary_{n}_{i}", n, 1, w, h, mat, _boundary((bl, lw)))
        for mat in ("ref", "ones", "primes", "jpeg_like" if n == 4 else "annex_k", "ref_dc3"):
            add("ties", f"ties_{n}_{mat}", n, 1, 64, 64, mat, _ties)
    add("ties", "ties_4_norle_ones", 4, 0, 64, 64, "ones", _ties)
    add("big", "big_zero_width", 4, 1, 256, 256, "ref", _big_zero)
    add("big", "big_width", 4, 1, 256, 256, "ref", _big_width)
    assert len({e.name for e in out}) == len(out)
    _ENTRIES = out
    return out


def by_family(family: str) -> list[Entry]:
    return [e for e in entries() if e.family == family]


def by_name(name: str) -> Entry:
    return next(e for e in entries() if e.name == name)
