"""Constructed videos: valid P-frame files of the format that no encoder here writes.

One named, seeded table (entries()), shared by the CPU tests (tests/test_crafted_videos.py), the
golden generator (tests/golden/make_golden_crafted_video.py: the reference's own decode of every
entry with motion compensation on and off, pinned by md5 in manifest_crafted_video.json) and the
GPU tests (tests/test_gpu_crafted_videos.py).  Only the table is committed:
stream_craft.pack_video rebuilds every file.  All entries use 4x4 blocks (the reference's decoder
is built for them), W and H multiples of 16, nothing larger than 256x144x5.

A vector component is stored in mv = bits_needed(merange) bits, so every value of that field is
valid, not only [-merange, merange]; the decoder clamps the block position into the frame through
int16 (a sum beyond 32767 turns negative and clamps to 0).  A P-frame's decoded error is the
inverse transform + 128, so a bl = 0 record ADDS 128 to the copied pixels: records that keep the
picture carry a DC near -512 / q[0] (`_pf_record`).

Families
  vec_extremes  64x48, merange 8: every component from {lo, lo+1, -merange-1, -1, 0, 1, merange+1,
                hi-1, hi} (lo, hi: the limits of the field) over an I-frame of per-pixel noise
  vec_widths    merange 0, 1, 2, 3, 15, 16, 255, 256, 16383, 16384, 32767: field widths 1 .. 16,
                vectors uniform over the whole field; the 16-bit entries hold macroblocks with
                mx + vx > 32767 and my + vy > 32767
  vec_phase     merange 32767 (the widest vector window, 7 + 32 bits) and merange 1 (2 + 2 bits):
                the I-frame's first record moves the first vector of the P-frames over all 8 bit
                phases; vectors half small (the low bits of the field decide the pixels), half
                uniform over the field (the high bits do)
  dense         256x144, I P P: P-frames of bl = 0 records (4 bits each), alone or with a bl = 15
                record every 37th block, with and without RLE: chunks of exactly 256 records (the
                position list's capacity) and of more (the decode walks again)
  long          every record bl = 15 with 16 values: 259 bits (RLE) / 244 bits across chunk ends
  saturate      I-frames that decode to flat 0, flat 255 and a 0 / 255 checker of blocks, then four
                P-frames of DC-only errors that land far outside [0, 255], at -2 .. 2 and at
                253 .. 257 (halves included): clamped reconstructions feed the next frame
  groups        32x32, 5 frames, gop 2, 3, 5 and 9 (I P I P I, a ragged last group, one group, a
                gop beyond the frame count)
  geometry      16x16 (one macroblock; its last P-frame is vectors + 16 four-bit records: the
                vector window nearest the end of a stream), 64x16 and 16x64
  gop_case      I P P with bl = 0 and bl = 15 records in every frame, vectors inside the search range
"""
from __future__ import annotations

import numpy as np

from tests import crafted_streams as CS
from tests import stream_craft as S

N = 4
NN = 16
FAMILIES = ("vec_extremes", "vec_widths", "vec_phase", "dense", "long", "saturate", "groups", "geometry", "gop_case")
WIDTH_MERANGES = (0, 1, 2, 3, 15, 16, 255, 256, 16383, 16384, 32767)
DENSE_EVERY = 37  # dense (b), (c): a bl = 15 record at every block index that is a multiple of this
ZZ = CS.zigzag(N)


# ------------------------------------------------------------------------------ shared pieces
def field_limits(merange: int) -> tuple[int, int]:
    mv = S.mvec_bits(merange)
    return -(1 << (mv - 1)), (1 << (mv - 1)) - 1


def extreme_components(merange: int) -> list[int]:
    lo, hi = field_limits(merange)
    return sorted({v for v in (lo, lo + 1, -merange - 1, -1, 0, 1, merange + 1, hi - 1, hi) if lo <= v <= hi})


REC_POS_CAP = 256  # record positions kept per chunk (kRecPosCap, ie_device.h)


def planned_chunk_bits(e) -> tuple[int, int]:
    """(C, chunks per frame) of a P-frame video, the library's plan restated (plan_chunks over the
    frame's bound of 4 + 16 (N*N + 1) bits per block, about 24 records per chunk, a multiple of 32;
    ie_decode_gop and ie_vdec cap it at REC_POS_CAP x the shortest record an encoder writes: 4 bits
    with RLE, 4 + N*N without)."""
    bound = e.nblocks * (4 + 16 * (NN + 1))
    want = max((e.nblocks + 23) // 24, 1)
    c = (bound + want - 1) // want
    c = min(max((c + 31) // 32 * 32, 256), REC_POS_CAP * (4 if e.rle else 4 + NN))
    return c, max((bound + c - 1) // c, 1)


def _zero(rle):
    return (0, 0 if rle else NN, [0] * (0 if rle else NN))


def _sized(vals, rle, widen=0):
    """The record of `vals` (zig-zag order, trailing zeros dropped with RLE) in the narrowest field
    that holds them, `widen` bits wider (15 at most)."""
    vals = [int(v) for v in vals]
    if rle:
        while vals and vals[-1] == 0:
            vals.pop()
    else:
        vals = vals + [0] * (NN - len(vals))
    lw = len(vals)
    bl = max([CS._bits_for(v) for v in vals] + [CS._bits_for(lw) - 1 if rle else 1, 1])
    return (min(15, bl + widen), lw, vals)


def _noise_record(rng, e, centre=0):
    """An I-frame block of per-pixel noise: every coefficient about +-100 / q, the mean near 128 + centre."""
    q = e.q
    vals = [int(round(float(rng.uniform(-100, 100)) / int(q[ZZ[k]]))) for k in range(NN)]
    vals[0] = int(round((4 * centre + float(rng.uniform(-160, 160))) / int(q[0])))
    return _sized(vals, e.rle, int(rng.integers(0, 3)))


def _noise_frame(rng, e, centre=0):
    return [_noise_record(rng, e, centre) for _ in range(e.nblocks)]


def _pf_record(rng, e, widen=None):
    """A P-frame record that keeps the picture: DC near -512 / q[0] (error + 128 near 0), a few
    small values behind it."""
    q0 = int(e.q[0])
    lw = int(rng.integers(1, NN + 1))
    vals = [int(round(-512 / q0)) + int(rng.integers(-12, 13))] + [int(v) for v in rng.integers(-2, 3, size=lw - 1)]
    return _sized(vals, e.rle, int(rng.integers(0, 4)) if widen is None else widen)


def _pf_mixed(rng, e, i):
    """The P-frame records of vec_extremes: picture-keeping ones, every fourth bl = 0 or full range."""
    if i % 8 == 3:
        return _zero(e.rle)
    if i % 8 == 7:
        return CS._rec(rng, N, e.rle, int(rng.integers(1, 16)), int(rng.integers(0, NN + 1)))
    return _pf_record(rng, e)


def _uniform_vectors(rng, e):
    lo, hi = field_limits(e.merange)
    return [(int(a), int(b)) for a, b in rng.integers(lo, hi + 1, size=(e.nmb, 2))]


def _extreme_vectors(rng, e):
    c = extreme_components(e.merange)
    return [(c[int(a)], c[int(b)]) for a, b in rng.integers(0, len(c), size=(e.nmb, 2))]


def _is_i(e, f):
    return f % e.gop == 0


class Entry:
    n = N

    def __init__(self, family, name, w, h, frames, gop, merange, rle, mat, build):
        self.family, self.name, self.w, self.h, self.frames = family, name, w, h, frames
        self.gop, self.merange, self.rle, self.mat = gop, merange, bool(rle), mat
        self._build = build
        self._frames = None
        self._file = None

    @property
    def nblocks(self) -> int:
        return (self.w // N) * (self.h // N)

    @property
    def nmb(self) -> int:
        return (self.w // 16) * (self.h // 16)

    @property
    def mv(self) -> int:
        return S.mvec_bits(self.merange)

    @property
    def q(self) -> np.ndarray:
        return CS.matrix(N, self.mat)

    def frame_list(self):
        """[(vectors or None, records)] per frame, built once."""
        if self._frames is None:
            self._frames = self._build(CS._rng(self.name), self)
            assert len(self._frames) == self.frames
        return self._frames

    def file(self):
        """(bytes, positions) of stream_craft.pack_video, built once."""
        if self._file is None:
            self._file = S.pack_video(self.frame_list(), N, self.q, self.rle, self.w, self.h, self.gop, self.merange,
                                      positions=True)
        return self._file

    @property
    def data(self) -> bytes:
        return self.file()[0]

    @property
    def end_bit(self) -> int:
        return self.file()[1][-1]["end"]

    def settings(self) -> dict:
        return dict(w=self.w, h=self.h, frames=self.frames, gop=self.gop, merange=self.merange, rle=int(self.rle),
                    matrix=self.mat)


# ------------------------------------------------------------------------------ the families
def _vec_extremes(rng, e):
    out = []
    for f in range(e.frames):
        if _is_i(e, f):
            out.append((None, _noise_frame(rng, e)))
        else:
            out.append((_extreme_vectors(rng, e), [_pf_mixed(rng, e, i + f) for i in range(e.nblocks)]))
    return out


def _vec_widths(rng, e):
    out = [(None, _noise_frame(rng, e))]
    for f in range(1, e.frames):
        vec = _uniform_vectors(rng, e)
        lo, hi = field_limits(e.merange)
        vec[f % 2] = (lo, hi) if f % 2 else (hi, lo)  # (the limits themselves, whatever the draw)
        if e.mv == 16:
            # the int16 wrap (48x32: macroblock columns 0, 16, 32, rows 0, 16): the last column and
            # the last row with a vector that takes the position beyond 32767, both in the corner
            mbx = e.w // 16
            vec[mbx - 1] = (32767 - 5 * f, vec[mbx - 1][1])             # mx = 32: 32 + vx > 32767
            vec[mbx] = (vec[mbx][0], 32760 + f)                         # my = 16: 16 + vy > 32767
            vec[e.nmb - 1] = (32740 + f, 32767)
        out.append((vec, [_pf_record(rng, e) for _ in range(e.nblocks)]))
    return out


def _vec_phase(lead_bl):
    def build(rng, e):
        rng = CS._rng(f"vec_phase_{e.merange}")  # (one video per merange: only the lead differs)
        first = _noise_frame(rng, e)
        first[0] = (lead_bl, 0, [])  # 4 + lead_bl bits (RLE: a count of 0): the phase of all that follows
        out = [(None, first)]
        lo, hi = field_limits(e.merange)
        for f in range(1, e.frames):
            vec = _uniform_vectors(rng, e)
            for k in range(0, e.nmb, 2):
                vec[k] = (int(rng.integers(max(lo, -20), min(hi, 20) + 1)), int(rng.integers(max(lo, -20), min(hi, 20) + 1)))
            out.append((vec, [_pf_record(rng, e) for _ in range(e.nblocks)]))
        return out
    return build


def _dense(every):
    def build(rng, e):
        out = [(None, _noise_frame(rng, e, centre=-80))]  # (dark: two P-frames of + 128 leave most of it unclamped)
        for f in range(1, e.frames):
            recs = []
            for i in range(e.nblocks):
                if every and i % every == 0:
                    recs.append(_sized([int(round(-512 / int(e.q[0]))) + int(rng.integers(-12, 13))] +
                                       [int(v) for v in rng.integers(-2, 3, size=NN - 2)] + [1], e.rle, 15))
                else:
                    recs.append(_zero(e.rle))
            out.append((_uniform_vectors(rng, e), recs))
        return out
    return build


def _long(rng, e):
    """bl = 15, 16 values: magnitudes 2^1 .. 2^14 in turn (the last: the whole range); in P-frames
    half of the records keep the picture (a DC near -512 / q[0] in a 15-bit field)."""
    out = []
    for f in range(e.frames):
        recs = []
        for i in range(e.nblocks):
            k = 1 + (i + f) % 14
            vals = [int(v) for v in rng.integers(-(1 << k), 1 << k, size=NN)]
            if not _is_i(e, f) and i % 2:
                vals = [int(round(-512 / int(e.q[0]))) + int(rng.integers(-12, 13))] + [int(v) for v in rng.integers(-2, 3, size=NN - 1)]
            if vals[-1] == 0:
                vals[-1] = 1
            recs.append((15, NN, vals))
        out.append((None if _is_i(e, f) else _extreme_vectors(rng, e), recs))
    return out


# the values saturate's P-frames aim at before the clamp, in halves (q[0] = 2: a DC step is 1/2)
SATURATE_TARGETS2 = [-8000, -600, -4, -3, -2, -1, 0, 1, 2, 3, 4, 200, 256, 400, 506, 507, 508, 509, 510, 511, 512, 513, 514,
                     1200, 9000]


def saturate_dc(q0: int, ref: int, target2: int) -> int:
    """The DC for which ref + error is target2 / 2: error = DC q0 / 4 + 128."""
    assert q0 == 2
    return target2 - 2 * ref - 256


def _saturate(form):
    def build(rng, e):
        q0 = int(e.q[0])
        bx = e.w // N
        first = {"flat0": lambda b: 0, "flat255": lambda b: 255, "checker": lambda b: 255 * ((b % bx + b // bx) & 1)}[form]
        state = [first(b) for b in range(e.nblocks)]  # every block stays flat: DC-only records
        out = [(None, [_sized([saturate_dc(q0, 0, 2 * (v - 128) + 256)], e.rle) for v in state])]
        for f in range(1, e.frames):
            recs = []
            for b in range(e.nblocks):
                t2 = SATURATE_TARGETS2[(b + 7 * f + b // bx) % len(SATURATE_TARGETS2)]
                recs.append(_sized([saturate_dc(q0, state[b], t2)], e.rle, (b + f) % 3))
                state[b] = min(255, max(0, t2 // 2))  # (clamp, then truncate: floor inside [0, 255])
            out.append(([(0, 0)] * e.nmb, recs))
        return out
    return build


def _geometry_one(rng, e):
    out = [(None, _noise_frame(rng, e, centre=-80))]
    for f in range(1, e.frames):
        out.append((_uniform_vectors(rng, e), [_zero(e.rle)] * e.nblocks))
    return out


def _gop_case(rng, e):
    frames = []
    for f in range(e.frames):
        recs = []
        for i in range(e.nblocks):
            k = (i + f) % 4
            if k == 0:
                recs.append((0, 0, []))
            elif k == 1:  # bl = 15 fields holding small values
                lw = int(rng.integers(0, NN + 1))
                recs.append((15, lw, [int(v) for v in rng.integers(-6, 7, size=lw)]))
            elif k == 2:
                recs.append(CS._rec(rng, N, True, 15, int(rng.integers(0, NN + 1)), edges_at=i))
            else:
                recs.append(CS._rec(rng, N, True, int(rng.integers(1, 8)), int(rng.integers(0, NN + 1))))
        mv = None if _is_i(e, f) else [(int(a), int(b)) for a, b in rng.integers(-e.merange, e.merange + 1, size=(e.nmb, 2))]
        frames.append((mv, recs))
    return frames


_ENTRIES = None


def entries() -> list[Entry]:
    global _ENTRIES
    if _ENTRIES is not None:
        return _ENTRIES
    out = []

    def add(family, name, w, h, frames, gop, merange, rle, build, mat="ref"):
        out.append(Entry(family, name, w, h, frames, gop, merange, rle, mat, build))

    add("vec_extremes", "vec_extremes_rle", 64, 48, 5, 5, 8, 1, _vec_extremes)
    add("vec_extremes", "vec_extremes_norle", 64, 48, 5, 5, 8, 0, _vec_extremes)
    for m in WIDTH_MERANGES:
        add("vec_widths", f"vec_widths_{m}", 48, 32, 3, 3, m, 1, _vec_widths)
    for m in (32767, 1):
        for lead in range(8):
            add("vec_phase", f"vec_phase_{m}_{lead}", 48, 32, 3, 3, m, 1, _vec_phase(lead))
    add("dense", "dense_a_rle_zero", 256, 144, 3, 3, 8, 1, _dense(0))
    add("dense", "dense_b_rle_every37", 256, 144, 3, 3, 8, 1, _dense(DENSE_EVERY))
    add("dense", "dense_c_norle_every37", 256, 144, 3, 3, 8, 0, _dense(DENSE_EVERY))
    add("dense", "dense_d_norle_zero", 256, 144, 3, 3, 8, 0, _dense(0))
    add("long", "long_rle", 64, 48, 3, 3, 8, 1, _long)
    add("long", "long_norle", 64, 48, 3, 3, 8, 0, _long)
    for form in ("flat0", "flat255", "checker"):
        add("saturate", f"saturate_{form}", 64, 48, 5, 5, 8, 1, _saturate(form))
    for gop in (2, 3, 5, 9):
        add("groups", f"groups_gop{gop}", 32, 32, 5, gop, 8, 1, _vec_extremes)
    add("geometry", "geometry_16x16_m32767", 16, 16, 3, 3, 32767, 1, _geometry_one)
    add("geometry", "geometry_16x16_m1", 16, 16, 3, 3, 1, 1, _geometry_one)
    add("geometry", "geometry_64x16", 64, 16, 3, 3, 8, 1, _vec_extremes)
    add("geometry", "geometry_16x64", 16, 64, 3, 3, 8, 1, _vec_extremes)
    add("gop_case", "gop_case", 64, 48, 3, 3, 8, 1, _gop_case)
    assert len({e.name for e in out}) == len(out)
    _ENTRIES = out
    return out


def by_family(family: str) -> list[Entry]:
    return [e for e in entries() if e.family == family]


def by_name(name: str) -> Entry:
    return next(e for e in entries() if e.name == name)
