"""The constructed videos (tests/crafted_videos.py) on the CPU.

1. The builder: stream_craft.parse_video(pack_video(x)) gives back the table's vectors, records and
   bit positions.
2. The oracle pinned: oracle.decode_video_gop of every entry, motion compensation on and off, has
   the md5 of the REFERENCE's own decode (manifest_crafted_video.json, written by
   tests/golden/make_golden_crafted_video.py from the reference's decoder).
3. Reach: what every family is there to meet, computed here from the table and the builder's bit
   positions alone -- no library code, so the GPU tests cannot pass by missing their target.

The numbers of the chunk plan restated in 3 (model_chunk_bits): a P-frame video's record chunks are
capped at kRecPosCap x the shortest record (ie_decode_gop in ie_capi_decode.cpp and vd_enqueue in
ie_capi_vdec.cpp: `cmax = kRecPosCap * min_rec`, min_rec = 4 bits with RLE, 4 + N*N = 20 bits
without), kRecPosCap = 256 being the record positions kept per chunk (ie_device.h); a chunk with
more records takes rec_decode_kernel's second walk (ie_decode.hip: `listed = R[j] <= kRecPosCap`).
The chunks of a frame are planned from its bound, nblocks x (4 + 16 (N*N + 1)) bits
(bound_bits_per_block, ie_ctx.hpp; plan_chunks: about 24 records per chunk), and start at the
frame's first bit plus its vector bits.
"""
import hashlib
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import crafted_videos as CV
from tests import oracle_lib as O
from tests import stream_craft as S

MANIFEST = json.load(open(os.path.join(O.GOLDEN, "manifest_crafted_video.json")))

REC_POS_CAP = 256                 # kRecPosCap (ie_device.h)
CHUNK_BITS_RLE = 256 * 4          # kRecPosCap x a bl = 0 record
CHUNK_BITS_NORLE = 256 * 20       # kRecPosCap x a bl = 1 record of 16 values


def _md5(b: bytes) -> str:
    return hashlib.md5(b).hexdigest()


def model_chunk_bits(e) -> tuple[int, int]:
    """(C, chunks per frame) of a P-frame video: the plan restated in tests/crafted_videos.py (plain
    Python, shared with the GPU tests); every entry's frame is large enough for the cap to decide."""
    c, nch = CV.planned_chunk_bits(e)
    assert CV.REC_POS_CAP == REC_POS_CAP and c == (CHUNK_BITS_RLE if e.rle else CHUNK_BITS_NORLE)
    return c, nch


def chunk_counts(e, f) -> np.ndarray:
    """Record starts in every chunk of frame f: chunk k is the C bits from the frame's first record
    (its first bit plus its vector bits) + k C."""
    c, nch = model_chunk_bits(e)
    fp = e.file()[1][f]
    base = fp["start"] + (0 if f % e.gop == 0 else e.nmb * 2 * e.mv)
    assert base == fp["rec"][0]
    k = (np.asarray(fp["rec"], dtype=np.int64) - base) // c
    assert k.max() < nch
    return np.bincount(k)


def crossings(e, f) -> int:
    """Records of frame f that hold a chunk end strictly inside."""
    c, _ = model_chunk_bits(e)
    fp = e.file()[1][f]
    starts = np.asarray(fp["rec"], dtype=np.int64) - fp["rec"][0]
    ends = np.asarray(fp["rec"][1:] + [fp["end"]], dtype=np.int64) - fp["rec"][0]
    return int(((ends - 1) // c > starts // c).sum())


def p_frames(e):
    return [f for f in range(e.frames) if f % e.gop]


def macroblocks(e, f):
    """(mx, my, vx, vy) of every macroblock of P-frame f."""
    mbx = e.w // 16
    return [((k % mbx) * 16, (k // mbx) * 16, vx, vy) for k, (vx, vy) in enumerate(e.frame_list()[f][0])]


def clamp_int(v: int, hi: int) -> int:
    return min(max(v, 0), hi)


def clamp16(v: int, hi: int) -> int:
    """The reference's clamp: the sum goes through int16 first."""
    return clamp_int((v + 32768) % 65536 - 32768, hi)


_DEC = {}


def decoded(oracle, e, mc) -> np.ndarray:
    """[frames][h][w] Y of the oracle's decode, computed once."""
    if (e.name, mc) not in _DEC:
        out = np.frombuffer(oracle.decode_video_gop(e.data, CV.N, bool(mc)), dtype=np.uint8)
        _DEC[e.name, mc] = out.reshape(e.frames, e.w * e.h * 3 // 2)
    return _DEC[e.name, mc][:, : e.w * e.h].reshape(e.frames, e.h, e.w)


# ------------------------------------------------------------------ 1. the builder
def test_table_is_stable_and_named():
    assert [e.name for e in CV.entries()] == [m["name"] for m in MANIFEST]
    assert {e.family for e in CV.entries()} == set(CV.FAMILIES)
    for e in CV.entries():
        assert e.w % 16 == 0 and e.h % 16 == 0 and e.w * e.h * e.frames <= 256 * 144 * 5, e.name
        assert (e.w, e.h) == (256, 144) or e.w * e.h <= 64 * 48, e.name
        assert len(e.data) == (e.end_bit + 7) // 8


@pytest.mark.parametrize("name", [e.name for e in CV.entries()])
def test_parse_video_gives_back_the_table(name):
    e = CV.by_name(name)
    data, pos = e.file()
    frames, q, rle, w, h, gop, merange, pos2 = S.parse_video(data, CV.N)
    assert (rle, w, h, gop, merange, len(frames)) == (e.rle, e.w, e.h, e.gop, e.merange, e.frames)
    assert np.array_equal(q, e.q)
    assert pos2 == pos
    lo, hi = CV.field_limits(e.merange)
    for f, ((vec, recs), (vec2, recs2)) in enumerate(zip(e.frame_list(), frames)):
        assert (vec is None) == (f % e.gop == 0) and vec2 == vec and recs2 == recs, f
        assert vec is None or all(lo <= c <= hi for v in vec for c in v)
        lens = [b - a for a, b in zip(pos[f]["rec"], pos[f]["rec"][1:] + [pos[f]["end"]])]
        assert lens == [S.record_len(r, e.rle) for r in recs]
        assert pos[f]["vec"] == [pos[f]["start"] + 2 * e.mv * k for k in range(0 if vec is None else e.nmb)]


def test_stream_craft_default_return_is_the_file():
    e = CV.by_name("gop_case")
    assert S.pack_video(e.frame_list(), CV.N, e.q, e.rle, e.w, e.h, e.gop, e.merange) == e.data


# ------------------------------------------------------------------ 2. oracle == reference
@pytest.mark.parametrize("mc", [1, 0])
@pytest.mark.parametrize("m", MANIFEST, ids=lambda m: m["name"])
def test_oracle_decodes_crafted_video_as_reference(oracle, m, mc):
    e = CV.by_name(m["name"])
    assert dict(e.settings(), family=e.family) == {k: m[k] for k in list(e.settings()) + ["family"]}
    assert _md5(e.data) == m["md5"], "the table no longer builds the file the reference decoded"
    dec = oracle.decode_video_gop(e.data, CV.N, bool(mc))
    assert len(dec) == e.frames * (e.w * e.h * 3 // 2)
    assert _md5(dec) == m[f"dec{mc}_md5"]


# ------------------------------------------------------------------ 3. what the families reach
@pytest.mark.parametrize("name", [e.name for e in CV.by_family("vec_extremes")])
def test_vec_extremes_reach_every_edge(oracle, name):
    e = CV.by_name(name)
    assert (e.w, e.h, e.merange, e.mv) == (64, 48, 8, 5)
    assert CV.extreme_components(8) == [-16, -15, -9, -1, 0, 1, 9, 14, 15]
    mbs = [m for f in p_frames(e) for m in macroblocks(e, f)]
    assert {c for m in mbs for c in m[2:]} == set(CV.extreme_components(8))
    W16, H16 = e.w - 16, e.h - 16
    assert any(mx + vx < 0 for mx, my, vx, vy in mbs), "left edge"
    assert any(mx + vx > W16 for mx, my, vx, vy in mbs), "right edge"
    assert any(my + vy < 0 for mx, my, vx, vy in mbs), "top edge"
    assert any(my + vy > H16 for mx, my, vx, vy in mbs), "bottom edge"
    assert any(max(abs(vx), abs(vy)) > e.merange and 0 <= mx + vx <= W16 and 0 <= my + vy <= H16 and min(abs(vx), abs(vy)) > 1
               for mx, my, vx, vy in mbs), "a vector beyond merange that lands inside the frame"
    # the content tells a wrong clamp: in the frame the first P-frame copies from, the block at the
    # clamped position differs from the block one pixel further inside, at every clamped macroblock
    ref = decoded(oracle, e, 0)[0]
    for mx, my, vx, vy in macroblocks(e, p_frames(e)[0]):
        cx, cy = clamp_int(mx + vx, W16), clamp_int(my + vy, H16)
        if (cx, cy) != (mx + vx, my + vy):
            ox, oy = (1 if cx == 0 else -1) * (cx != mx + vx), (1 if cy == 0 else -1) * (cy != my + vy)
            assert not np.array_equal(ref[cy: cy + 16, cx: cx + 16], ref[cy + oy: cy + oy + 16, cx + ox: cx + ox + 16])


def test_vec_widths_cover_the_field_widths():
    es = CV.by_family("vec_widths")
    assert [e.merange for e in es] == list(CV.WIDTH_MERANGES)
    assert [e.mv for e in es] == [1, 2, 3, 3, 5, 6, 9, 10, 15, 16, 16]
    for e in es:
        assert (e.w, e.h, e.frames) == (48, 32, 3)
        lo, hi = CV.field_limits(e.merange)
        comps = [c for f in p_frames(e) for m in macroblocks(e, f) for c in m[2:]]
        assert min(comps) <= lo // 2 and max(comps) >= (hi + 1) // 2, e.name  # the whole field, not the search range
        assert {lo, hi} <= set(comps), e.name


@pytest.mark.parametrize("merange", [16384, 32767])
def test_vec_widths_16_bit_entries_wrap(oracle, merange):
    """A macroblock where plain int arithmetic and the int16 arithmetic pick different source
    blocks, in x and in y -- and blocks whose pixels differ in the frame copied from."""
    e = CV.by_name(f"vec_widths_{merange}")
    assert e.mv == 16
    W16, H16 = e.w - 16, e.h - 16
    in_x = in_y = 0
    for f in p_frames(e):
        ref = decoded(oracle, e, 0)[f - 1]
        for mx, my, vx, vy in macroblocks(e, f):
            a, b = (clamp16(mx + vx, W16), clamp16(my + vy, H16)), (clamp_int(mx + vx, W16), clamp_int(my + vy, H16))
            # (from the second P-frame on a frame of clamped copies repeats its corner blocks: only
            # macroblocks whose two candidates differ in content count)
            differ = not np.array_equal(ref[a[1]: a[1] + 16, a[0]: a[0] + 16], ref[b[1]: b[1] + 16, b[0]: b[0] + 16])
            in_x += mx + vx > 32767 and a[0] != b[0] and a[1] == b[1] and differ
            in_y += my + vy > 32767 and a[1] != b[1] and a[0] == b[0] and differ
        assert in_x >= 1 and in_y >= 1, (e.name, f, in_x, in_y)  # (already in the first P-frame, over the noise)


@pytest.mark.parametrize("merange,mv", [(32767, 16), (1, 2)])
def test_vec_phase_covers_all_bit_phases(merange, mv):
    es = [e for e in CV.by_family("vec_phase") if e.merange == merange]
    assert len(es) == 8 and all(e.mv == mv for e in es)
    first = {e.file()[1][p_frames(e)[0]]["vec"][0] % 8: e.name for e in es}
    assert sorted(first) == list(range(8)), first  # (one entry per phase: deleting any loses its phase)
    # and inside a frame the macroblocks' windows start at several phases of their own
    assert all(len({p % 8 for p in e.file()[1][1]["vec"]}) == (1 if mv == 16 else 2) for e in es)
    for e in es:  # small vectors (the low bits decide) next to field-wide ones (the high bits do)
        comps = [abs(c) for f in p_frames(e) for m in macroblocks(e, f) for c in m[2:]]
        assert sum(0 < c <= 20 for c in comps) >= 4
        assert mv == 2 or sum(c > 1000 for c in comps) >= 4


def test_dense_chunks_hold_exactly_and_more_than_a_position_list():
    a, b, c, d = (CV.by_name(n) for n in ("dense_a_rle_zero", "dense_b_rle_every37", "dense_c_norle_every37",
                                          "dense_d_norle_zero"))
    assert [e.name for e in (a, b, c, d)] == [e.name for e in CV.by_family("dense")]
    for e in (a, b, c, d):
        assert (e.w, e.h, e.frames, e.gop, e.nblocks) == (256, 144, 3, 3, 2304)
        assert model_chunk_bits(e)[0] == (CHUNK_BITS_RLE if e.rle else CHUNK_BITS_NORLE)
        assert model_chunk_bits(e)[1] > 1
    for f in p_frames(a):
        counts = chunk_counts(a, f)
        assert len(counts) == 9 and (counts == REC_POS_CAP).all(), counts  # R == kRecPosCap in every chunk
        assert all(r[0] == 0 for r in a.frame_list()[f][1])
    for f in p_frames(b):
        recs = b.frame_list()[f][1]
        assert all((r[0], r[1]) == ((15, 16) if i % CV.DENSE_EVERY == 0 else (0, 0)) for i, r in enumerate(recs))
        assert S.record_len(recs[0], True) == 259  # 4 + 15 (16 + 1): the longest 4x4 record
        counts = chunk_counts(b, f)
        assert counts.max() <= REC_POS_CAP and crossings(b, f) >= 1, counts  # listed chunks, records across their ends
    for f in p_frames(c):
        recs = c.frame_list()[f][1]
        assert all(r[0] == (15 if i % CV.DENSE_EVERY == 0 else 0) for i, r in enumerate(recs))
        assert S.record_len(recs[0], False) == 244 and S.record_len(recs[1], False) == 4
        assert chunk_counts(c, f).max() > REC_POS_CAP
    for f in p_frames(d):
        assert all(r[0] == 0 for r in d.frame_list()[f][1])
        counts = chunk_counts(d, f)
        assert counts.max() == 5 * REC_POS_CAP and counts.sum() == d.nblocks  # 1280 four-bit records in 5120 bits


@pytest.mark.parametrize("name", [e.name for e in CV.by_family("long")])
def test_long_records_cross_chunk_ends(name):
    e = CV.by_name(name)
    assert model_chunk_bits(e)[1] > 1
    for f in range(e.frames):
        recs = e.frame_list()[f][1]
        assert all(r[0] == 15 and r[1] == 16 for r in recs)
        assert {S.record_len(r, e.rle) for r in recs} == {259 if e.rle else 244}
        if f % e.gop:
            assert crossings(e, f) >= (40 if e.rle else 2), (f, crossings(e, f))
    mags = [max(abs(v) for v in r[2]) for f in range(e.frames) for r in e.frame_list()[f][1]]
    assert max(mags) > 16000 and min(mags) < 16  # values across the 15-bit range


@pytest.mark.parametrize("name", [e.name for e in CV.by_family("saturate")])
def test_saturate_reaches_both_bounds(oracle, name):
    """reference + error before the clamp, as an exact fraction: the records are DC-only (the error
    is DC q[0] / 4 + 128 at every pixel of the block) and the vectors zero, so the sum is the
    oracle's previous frame + that; the oracle's frame is its clamp, truncated."""
    e = CV.by_name(name)
    assert (e.w, e.h, e.frames, e.gop) == (64, 48, 5, 5)  # four P-frames in a row
    dec = decoded(oracle, e, 1)
    first = dec[0]
    want = {"saturate_flat0": {0}, "saturate_flat255": {255}, "saturate_checker": {0, 255}}[name]
    assert set(np.unique(first).tolist()) == want
    if name == "saturate_checker":
        assert (first[::4, ::4] != np.roll(first[::4, ::4], 1, axis=1)).all()
    q0 = int(e.q[0])
    bx = e.w // 4
    below = above = at0 = at255 = near = 0
    for f in p_frames(e):
        vec, recs = e.frame_list()[f]
        assert all(v == (0, 0) for v in vec)
        for b, r in enumerate(recs):
            assert r[1] <= 1, "DC only (a DC of 0 is a record of no values)"
            dc = r[2][0] if r[1] else 0
            y, x = 4 * (b // bx), 4 * (b % bx)
            ref = dec[f - 1][y: y + 4, x: x + 4]
            assert (ref == ref[0, 0]).all()
            v = int(ref[0, 0]) + Fraction(dc * q0, 4) + 128
            got = dec[f][y: y + 4, x: x + 4]
            assert (got == int(min(max(v, 0), 255))).all(), (f, b, v)
            below += v < 0
            above += v > 255
            at0 += v == 0
            at255 += v == 255
            near += v in (-2, -1, Fraction(-1, 2), 1, 2, 253, 254, 256, 257, Fraction(511, 2))
    assert below >= 20 and above >= 20 and at0 >= 4 and at255 >= 4 and near >= 40, (below, above, at0, at255, near)
    big = [abs(r[2][0]) for f in p_frames(e) for r in e.frame_list()[f][1] if r[1]]
    assert max(big) > 4000  # errors of large magnitude


def test_groups_and_geometry_shapes():
    assert [(e.gop, e.frames, e.w, e.h) for e in CV.by_family("groups")] == [(g, 5, 32, 32) for g in (2, 3, 5, 9)]
    assert [p_frames(e) for e in CV.by_family("groups")] == [[1, 3], [1, 2, 4], [1, 2, 3, 4], [1, 2, 3, 4]]
    geo = CV.by_family("geometry")
    assert [(e.w, e.h) for e in geo] == [(16, 16), (16, 16), (64, 16), (16, 64)]
    for e in geo[:2]:  # the last P-frame: one vector pair and 16 four-bit records, then the end of the file
        fp = e.file()[1][-1]
        assert e.nmb == 1 and fp["end"] - fp["vec"][0] == 2 * e.mv + 64 and len(e.data) == (fp["end"] + 7) // 8
    assert [e.mv for e in geo[:2]] == [16, 2]
