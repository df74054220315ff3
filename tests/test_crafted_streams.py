"""The stream builder and the constructed families (CPU).

1. tests/stream_craft.py round trips: pack(parse(x)) == x on the reference's own small encodes,
   parse(pack(r)) == r on seeded random record lists.
2. The conditions the families are there to meet, checked on the inputs themselves: every width,
   the longest record, chunk boundaries at every offset band of a record, chunks with more records
   than a position list holds, pixels that are exact integers.
3. The oracle's decode of every entry == the REFERENCE's (manifest_crafted.json, written by
   tests/golden/make_golden_crafted.py from the reference's decoders).
"""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import crafted_streams as CS
from tests import oracle_lib as O
from tests import stream_craft as S


def _md5(b: bytes) -> str:
    return hashlib.md5(b).hexdigest()


MANIFEST = json.load(open(os.path.join(O.GOLDEN, "manifest_crafted.json")))


# ------------------------------------------------------------------ 1. the builder
@pytest.mark.parametrize("name", ["ex0_4x4", "ex0_4x4_norle", "ex0_8x8", "synU4x4px_4x4", "synU200x56_4x4",
                                  "synU200x56_8x8", "synM200x56_4x4"])
def test_pack_parse_golden_encodes(name):
    """pack(parse(x)) == x on files the reference wrote: 4x4 and 8x8, RLE on and off."""
    c = next(c for c in O.manifest() if c["name"] == name)
    x = O.case_expected(c)
    assert x is not None and not c["huffman"]
    recs, q, rle, w, h, pos = S.parse(x, c["n"])
    assert (w, h, int(rle)) == (c["w"], c["h"], c["rle"])
    assert np.array_equal(q, O.read_matrix(c["matrix"], c["n"]))
    assert pos[0] == O.load().header(c["n"], q, c["rle"], w, h)[1]  # ieo_write_header's layout
    y, pos2 = S.pack(recs, c["n"], q, rle, w, h)
    assert y == x and pos2 == pos


@pytest.mark.parametrize("rle", [True, False], ids=["rle", "norle"])
@pytest.mark.parametrize("n", [4, 8])
def test_parse_pack_random_records(n, rle):
    for seed in range(4):
        rng = np.random.default_rng(1000 * n + 10 * seed + rle)
        w, h = n * int(rng.integers(1, 6)), n * int(rng.integers(1, 6))
        recs = []
        for _ in range((w // n) * (h // n)):
            bl = int(rng.integers(0, 16))
            lw = int(rng.integers(0, min(n * n, (1 << bl) - 1) + 1)) if rle else n * n
            recs.append((bl, lw, CS._full(rng, bl, lw)))
        q = rng.integers(1, 65536, size=n * n).astype(np.uint16)
        data, pos = S.pack(recs, n, q, rle, w, h)
        r2, q2, rle2, w2, h2, pos2 = S.parse(data, n)
        assert r2 == recs and np.array_equal(q2, q) and (rle2, w2, h2) == (rle, w, h) and pos2 == pos
        assert [b - a for a, b in zip(pos, pos[1:])] == [S.record_len(r, rle) for r in recs]
        assert len(data) == (pos[-1] + 7) // 8


# ------------------------------------------------------------------ 2. what the families reach
def test_table_is_stable_and_named():
    names = [e.name for e in CS.entries()]
    assert names == [m["name"] for m in MANIFEST]
    assert {e.family for e in CS.entries()} == set(CS.FAMILIES)
    for e in CS.entries():
        assert e.w <= 64 and e.h <= 64 or e.family in ("boundary", "big"), e.name
    assert len(CS.by_family("format_fuzz")) == 4 * 16


def test_width_family_reaches_every_width():
    for n in (4, 8):
        nn = n * n
        for rle in (True, False):
            for e in (e for e in CS.by_family("width") if e.n == n and e.rle == rle):
                recs = e.records()
                assert {r[0] for r in recs} == set(range(1, 16)), e.name
                for bl in range(1, 16):
                    vals = {v for r in recs if r[0] == bl for v in r[2]}
                    want = {-(1 << (bl - 1)), (1 << (bl - 1)) - 1, -1, 0} | ({1} if bl > 1 else set())
                    assert want <= vals, (e.name, bl)
                if rle:
                    for bl in range(1, 16):
                        top = min(nn, (1 << bl) - 1)
                        assert {0, 1, min(nn - 1, top), top} <= {r[1] for r in recs if r[0] == bl}, (e.name, bl)
    # the longest record there is: 8x8, bl = 15, 64 values, 979 bits
    assert any(r[0] == 15 and r[1] == 64 and S.record_len(r, True) == 979 == CS.entry_span(8)
               for e in CS.by_family("width") if e.n == 8 and e.rle for r in e.records())
    assert {e.mat for e in CS.by_family("width")} == {"ref", "ones", "max"}


def test_zero_width_family_forms():
    for e in CS.by_family("zero_width"):
        recs, (data, pos) = e.records(), e.file()
        zero = [r[0] == 0 for r in recs]
        assert all(S.record_len(r, e.rle) == 4 for r, z in zip(recs, zero) if z)
        if "_all_" in e.name:
            assert all(zero) and pos[-1] - pos[0] == 4 * e.nblocks
        elif "_alternate_" in e.name:
            assert zero == [i % 2 == 0 for i in range(e.nblocks)]
        elif "_first_last_" in e.name:
            assert zero[0] and zero[-1] and not any(zero[1:-1])
        else:  # runs: a planned chunk boundary with bl = 0 records on both sides
            C, _ = e.chunk_entries()
            starts = np.asarray(pos) - pos[0]
            inside = 0
            for k in range(1, (8 * len(data) - pos[0] + C - 1) // C):
                i = int(np.searchsorted(starts, k * C, side="right")) - 1  # the record holding bit k C
                inside += 0 < i < e.nblocks - 1 and zero[i - 1] and zero[i] and zero[i + 1]
            assert inside >= 1, (e.name, C)


def test_lengths_family_reaches_every_count():
    for n in (4, 8):
        got = {(r[0], r[1]) for e in CS.by_family("lengths") if e.n == n for r in e.records()}
        assert got == set(CS.lengths_table(n))
        assert {(12, lw) for lw in range(n * n + 1)} <= got
        recs = [r for e in CS.by_family("lengths") if e.n == n for r in e.records()]
        assert sum(1 for r in recs if r[1] >= 2 and r[2][-1] == 0 and r[2][-2] == 0 and any(r[2])) >= 8  # ends in zeros
        assert sum(1 for r in recs if r[0] == 12 and r[1] and max(abs(v) for v in r[2]) <= 2) >= 8      # wider than needed


@pytest.mark.parametrize("n", [4, 8])
def test_boundary_sweep_reaches_every_entry_offset(n):
    """plan_chunks' C restated (crafted_streams.planned_chunk_bits); every chunk's true entry offset
    d from the builder's record positions.  Over the sweep: d = 0 (at a chunk past the first, whose
    entry is 0 by definition), d = D - 1, and a d in every 64-wide band of [0, D)."""
    D = CS.entry_span(n)
    ds, later = set(), set()
    for e in CS.by_family("boundary"):
        if e.n != n:
            continue
        recs = e.records()
        assert all(r[0] == 15 and r[1] == n * n for r in recs[1:]) and e.nblocks == (512 if n == 4 else 256)
        C, d = e.chunk_entries()
        assert len(d) >= 8 and d[0] == 0 and all(0 <= x < D for x in d)
        ds |= set(d)
        later |= set(d[1:])
    assert 0 in later and D - 1 in ds
    assert {x // 64 for x in ds} == set(range((D + 63) // 64))
    hbs = {e.file()[1][0] % 32 for e in CS.by_family("boundary") if e.n == n}
    assert len(hbs) >= (2 if n == 4 else 1)  # (37 + N*N qb bits: 5 mod 32 for every 8x8 matrix)


def test_big_entries_overflow_a_position_list():
    """More than kRecPosCap = 256 records in a planned chunk: rec_decode_kernel walks again."""
    for e in CS.by_family("big"):
        C, counts = e.chunk_record_counts()
        assert counts.max() > 256 and counts.min() <= 256, (e.name, C, counts.max())
    assert all(r[0] == 0 for r in CS.by_name("big_zero_width").records()[1024:3072])
    assert {r[0] for r in CS.by_name("big_width").records()[1024:3072]} == {1, 2}


def test_fuzz_family_is_uniform_over_the_format():
    for n in (4, 8):
        for rle in (True, False):
            recs = [r for e in CS.by_family("format_fuzz") if e.n == n and e.rle == rle for r in e.records()]
            assert {r[0] for r in recs} == set(range(16))
            if rle:
                assert {r[1] for r in recs} == set(range(n * n + 1))


def test_ties_family_reaches_integer_pixels():
    """The inverse transform of every ties block in exact rational arithmetic (the factors are 1/2
    and +-1/2 on paper): at least half of the blocks have a pixel that is exactly an integer inside
    [0, 255] -- where a result 1 ulp low truncates to the wrong byte -- and the DC-only blocks
    reach every residue of Y q mod 4 their quantiser allows, on both sides of 0 and of 255."""
    for e in CS.by_family("ties"):
        q = e.q
        recs = e.records()
        integer = 0
        low, high, res = set(), set(), set()
        for r in recs:
            pix = CS.exact_pixels(e.n, q, r)
            integer += any(p.denominator == 1 and 0 <= p <= 255 for p in pix)
            if sum(1 for v in r[2] if v) <= 1 and (not r[2] or all(v == 0 for v in r[2][1:])):
                p = pix[0]
                res.add(int(p * 4) % 4)
                low |= {p < 0} if p < 64 else set()
                high |= {p > 255} if p > 192 else set()
        assert 2 * integer >= len(recs), (e.name, integer, len(recs))
        assert low == {True, False} and high == {True, False}, (e.name, low, high)
        assert res == {(y * int(q[0])) % 4 for y in range(4)}, (e.name, res)
    four = [r for e in CS.by_family("ties") for r in e.records() if sum(1 for v in r[2] if v) >= 2]
    assert len(four) >= 500


# ------------------------------------------------------------------ 3. oracle == reference
@pytest.mark.parametrize("m", MANIFEST, ids=lambda m: m["name"])
def test_oracle_decodes_crafted_as_reference(oracle, m):
    e = CS.by_name(m["name"])
    assert (e.n, int(e.rle), e.w, e.h, e.family) == (m["n"], m["rle"], m["w"], m["h"], m["family"])
    assert _md5(e.data) == m["md5"], "the table no longer builds the file the reference decoded"
    px = oracle.decode_image(e.data, e.n)
    assert px.shape == (e.h, e.w)
    assert _md5(px.tobytes()) == m["dec_md5"]


def test_oracle_decodes_gop_case(oracle):
    """The P-frame video of the GPU test (the entry gop_case of tests/crafted_videos.py), pinned: the
    oracle's decode, motion compensation on and off, has the md5 of the REFERENCE's own decode
    (manifest_crafted_video.json)."""
    from tests import crafted_videos as CV
    e = CV.by_name("gop_case")
    m = next(m for m in json.load(open(os.path.join(O.GOLDEN, "manifest_crafted_video.json"))) if m["name"] == e.name)
    assert _md5(e.data) == m["md5"], "the table no longer builds the file the reference decoded"
    for mc in (1, 0):
        out = oracle.decode_video_gop(e.data, e.n, bool(mc))
        assert len(out) == e.frames * (e.w * e.h * 3 // 2)
        assert _md5(out) == m[f"dec{mc}_md5"], mc
