"""The Huffman stream builder and the constructed families (CPU).

1. Every valid entry of tests/crafted_huffman.py: the oracle's decode == the builder's serial model
   == the symbols the builder put in, followed by what the padding decodes to.  Every invalid entry:
   the oracle returns None, and so does the model.
2. ie_huffman_table (host code of libie_hip.so) returns the builder's prefix table and code start.
3. The conditions the families are there to meet, read off the serial model, so that the GPU tests
   (tests/test_gpu_huffman_crafted.py) provably reach what they claim.
4. The constants of the device decode restated in crafted_huffman are the sources'.
5. The wrapped image files are the ones tests/golden/make_golden_crafted_huffman.py pinned, and the
   oracle's Huffman decode and pixels of them are the manifest's (the pixels: the REFERENCE's).
"""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

from tests import crafted_huffman as CH
from tests import huffman_craft as H
from tests import oracle_lib as O

CHUNK, TC, TPB, G, SYNC, L1, EMIT_LDS = CH.CHUNK, CH.TC, CH.TPB, CH.G, CH.SYNC, CH.L1, CH.EMIT_LDS
MANIFEST = json.load(open(os.path.join(O.GOLDEN, "manifest_crafted_huffman.json")))
VALID = [e.name for e in CH.valid_entries()]
INVALID = [e.name for e in CH.by_family("invalid")]
_ORACLE = {}


def _md5(b: bytes) -> str:
    return hashlib.md5(b).hexdigest()


def _oracle(e):
    if e.name not in _ORACLE:
        _ORACLE[e.name] = O.load().huffman_decode(e.data)
    return _ORACLE[e.name]


# ------------------------------------------------------------------ 1. oracle == model == builder
def test_table_is_named_and_complete():
    assert {e.family for e in CH.entries()} == set(CH.FAMILIES)
    assert [e.name for e in CH.by_family("fixed")] == [f"fixed_{L}" for L in (1, 2, 6, 8, 11, 12, 15)]
    assert set(CH.WRAPPED) == set(CH.FAMILIES) - {"invalid"}
    for family, name in CH.WRAPPED.items():
        assert CH.by_name(name).family == family
    assert max(len(e.data) for e in CH.entries()) < 40000
    for e in CH.entries():
        assert all(1 <= len(entries) <= 127 and 1 <= bits <= 15 for bits, entries in e.groups), e.name


@pytest.mark.parametrize("name", VALID)
def test_oracle_model_and_builder_agree(name):
    e = CH.by_name(name)
    exp = _oracle(e)
    assert exp is not None and not exp[1], "the oracle rejects an entry meant as valid"
    got = e.model.decode()
    assert got == exp[0]
    assert got[: len(e.symbols)] == e.symbols
    # what follows is the padding's: fewer than 8 bits, a code at least one bit long
    pad = 8 * len(e.data) - e.end_bit
    assert 0 <= pad < 8 and len(got) - len(e.symbols) <= pad
    assert (pad == 0) == (len(got) == len(e.symbols))  # (every dictionary here has an all-zero code word)


@pytest.mark.parametrize("name", INVALID)
def test_oracle_rejects_invalid(name):
    e = CH.by_name(name)
    assert _oracle(e) is None
    assert e.model.decode() is None and e.symbols is None


# ------------------------------------------------------------------ 2. the host parse
@pytest.mark.parametrize("name", [e.name for e in CH.entries()])
def test_ie_huffman_table_returns_the_builders_table(name):
    from imageencoder_amd import IE_OK, load_library
    L = load_library()
    e = CH.by_name(name)
    src = np.frombuffer(e.data, dtype=np.uint8)
    lut = np.full(32768, 0xFFFF, dtype=np.uint16)
    start = C.c_uint64(0)
    r = L.ie_huffman_table(C.c_void_p(src.ctypes.data), C.c_size_t(src.size), C.c_uint64(0), C.c_void_p(lut.ctypes.data),
                           C.byref(start))
    assert r == IE_OK
    assert int(start.value) == e.code_start
    assert np.array_equal(lut, e.lut)


def test_group_order_does_not_matter():
    """The same code words in another group order and split: another file, the same table."""
    e = CH.by_name("long_short_200")
    flat = [(bits, ent) for bits, entries in e.groups for ent in entries]
    regrouped = [(bits, [ent]) for bits, ent in reversed(flat)]
    assert np.array_equal(H.prefix_table(regrouped), e.lut)
    assert [bits for bits, _ in e.groups][:2] == [15, 15] and e.groups[-1][0] == 1  # longest first


# ------------------------------------------------------------------ 3. what the families reach
@pytest.mark.parametrize("L", CH.FIXED_L)
def test_fixed_survivors(L):
    e = CH.by_name(f"fixed_{L}")
    assert {bits for bits, _ in e.groups} == {L}
    assert sum(len(entries) for _, entries in e.groups) == min(1 << L, 256)
    if L == 8:
        assert sorted(key for _, entries in e.groups for key, _ in entries) == list(range(256))
    if L > 8:
        assert any(code == 0 for _, entries in e.groups for _, code in entries)
    assert e.chunks >= TC + 1  # two table workgroups
    sv = e.model.survivors(CHUNK, SYNC)
    assert sv[:-1] == [min(L, 15)] * (e.chunks - 1)  # (the last chunk ends inside the stream's last bits)
    if L == 15:
        assert sum(sv[:TC]) == 15 * TC > 3 * TPB  # several rounds of the survivors' loop, R[] nearly full
        assert sum(sv[:TC]) <= TC * 16


def test_long_short_straddles_and_slides():
    for e in CH.by_family("long_short"):
        lens = sorted(bits for bits, entries in e.groups for _ in entries)
        assert lens[0] == 1 and lens[1] == 15 and len(lens) in (201, 256)
        assert int((e.lut == 0).sum()) > 0  # incomplete
        ends, mids = e.model.straddles(CHUNK)
        assert ends == set(range(1, 15)) and mids == set(range(1, 15)), e.name
        assert e.model.long_codes(CHUNK).min() >= 1
        # wrong-phase entries slide: a 15-bit code lies across every chunk's first bit, and the
        # entries inside it meet no code; somewhere all 14 wrong entries do
        sl = e.model.sliding_entries(CHUNK, SYNC)
        assert min(sl[1:-1]) >= 1 and max(sl) == 14, (e.name, sl)
    assert CH.by_name("long_short_200").chunks >= TC + 1


def test_l1_edge_reaches_the_second_level():
    e = CH.by_name("l1_10_11_12")
    by = {}
    for bits, entries in e.groups:
        by.setdefault(bits, []).extend(code for _, code in entries)
    assert sorted(by) == [10, 11, 12] and sum(len(v) for v in by.values()) == 256
    # 12-bit siblings on the 11-bit prefix next to an 11-bit code
    for c in by[11]:
        assert 2 * (c + 1) in by[12] and 2 * (c + 1) + 1 in by[12]
    comb = CH.by_name("l1_comb")
    lens = sorted(bits for bits, entries in comb.groups for _ in entries)
    assert lens == list(range(1, 15)) + [15, 15] and int((comb.lut == 0).sum()) == 0  # complete, depth 15
    for x in (e, comb):
        assert x.model.long_codes(CHUNK, lo=L1 + 1)[:-1].min() >= 1, x.name
        assert x.chunks >= TC + 1


def test_sizes_reach_the_chunk_thresholds():
    s = {e.name: e for e in CH.by_family("sizes")}
    assert all(e.code_start % 8 == 0 for e in s.values())
    assert s["sizes_short"].chunks == 1 and s["sizes_short"].end_bit - s["sizes_short"].code_start < CHUNK
    ex = s["sizes_3_chunks_exact"]
    assert ex.end_bit - ex.code_start == 3 * CHUNK and ex.end_bit == 8 * len(ex.data) and ex.chunks == 3
    assert len(ex.model.decode()) == len(ex.symbols)  # no padding, no padding symbol
    mi, pl = s["sizes_3_chunks_minus"], s["sizes_3_chunks_plus"]
    assert 0 < 3 * CHUNK - (mi.end_bit - mi.code_start) <= 9 and mi.chunks == 3
    assert 0 < (pl.end_bit - pl.code_start) - 3 * CHUNK <= 9 and pl.chunks == 4
    for n in (TC, TC + 1, TPB, TPB + 1):
        assert s[f"sizes_{n}_chunks"].chunks == n
    assert TPB + 1 > G  # 257 chunks: a second composition level as well as a second emit workgroup


def test_emit_threshold_counts():
    ex, p1 = CH.by_name("emit_exact"), CH.by_name("emit_plus_one")
    for e, tot in ((ex, EMIT_LDS), (p1, EMIT_LDS + 1)):
        assert e.chunks == TPB and e.end_bit == 8 * len(e.data)
        whole, first = e.model.chunk_counts(CHUNK)
        assert int(whole.sum()) == tot == len(e.model.decode())
        assert e.model.chunk_entries(CHUNK)[0] == 0
    whole, first = ex.model.chunk_counts(CHUNK)
    assert (whole == 160).all() and (first == 80).all() and set(ex.model.chunk_entries(CHUNK)) == {0}
    lo, hi = CH.by_name("emit_below"), CH.by_name("emit_above")
    assert lo.chunks > TPB and hi.chunks > TPB
    assert int(lo.model.chunk_counts(CHUNK)[0][:TPB].sum()) == TPB * CHUNK // 8 < EMIT_LDS
    assert int(hi.model.chunk_counts(CHUNK)[0][:TPB].sum()) == TPB * CHUNK > EMIT_LDS
    # both emit paths occur among the entries' first workgroups, and both sides of the threshold
    sums = {e.name: int(e.model.chunk_counts(CHUNK)[0][:TPB].sum()) for e in CH.valid_entries()}
    assert min(sums.values()) < EMIT_LDS < max(sums.values()) and EMIT_LDS in sums.values() and EMIT_LDS + 1 in sums.values()


def test_dup_has_two_code_words_per_byte():
    e = CH.by_name("dup_9")
    cm = H.code_map(e.groups)
    assert sorted(cm) == list(range(256)) and all(len(v) == 2 and v[0] != v[1] for v in cm.values())
    # both code words of a byte occur in the stream
    pos = np.asarray(e.model.path(), dtype=np.int64)
    bits = np.unpackbits(np.frombuffer(e.data, dtype=np.uint8))
    tops = {(int(e.model.sym_at[p]), int(bits[p])) for p in pos[:-1]}
    assert any((s, 0) in tops and (s, 1) in tops for s in range(256))


def test_invalid_positions():
    """The one position no code prefixes lies where the entry's name says; before it the true path
    is a valid one."""
    def hole(e):
        m = e.model
        p = e.code_start
        while m.len_at[p]:
            p += int(m.len_at[p])
        return p - e.code_start, p
    k, _ = divmod(hole(CH.by_name("invalid_first_chunk"))[0], CHUNK)
    assert k == 0
    off = hole(CH.by_name("invalid_second_half"))[0]
    assert off % CHUNK >= CHUNK // 2 + 15 and 0 < off // CHUNK < CH.by_name("invalid_second_half").chunks - 1
    e = CH.by_name("invalid_last_chunk")
    assert hole(e)[0] // CHUNK == e.chunks - 1 and e.chunks > 1
    e = CH.by_name("invalid_past_256")
    assert hole(e)[0] // CHUNK >= TPB
    e = CH.by_name("invalid_padding")
    assert e.end_bit <= hole(e)[1] < 8 * len(e.data)  # in the padding: zero bits that walk to no leaf


# ------------------------------------------------------------------ 4. the constants
def test_constants_are_the_sources():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "imageencoder_amd", "csrc")
    hip = open(os.path.join(csrc, "ie_huffman_decode.hip")).read()
    device = open(os.path.join(csrc, "ie_device.h")).read()
    capi = open(os.path.join(csrc, "ie_capi_huffman.cpp")).read()

    def one(pattern, src):
        m = re.findall(pattern, src, flags=re.M)
        assert len(m) == 1, (pattern, m)
        return int(m[0])

    assert one(r"^constexpr int kHufL1 = (\d+);", hip) == L1
    assert one(r"^constexpr int kHufD = (\d+);", hip) == H.MAX_BITS
    assert one(r"^#define IE_HUF_G (\d+)$", hip) == G
    assert one(r"^#define IE_HUF_SYNC (\d+)$", hip) == SYNC
    assert one(r"^#define IE_HUF_TC (\d+)$", hip) == TC
    assert one(r"^#define IE_HUF_EMIT_LDS (\d+)$", hip) == EMIT_LDS
    assert one(r"^constexpr int kTPB = (\d+);", device) == TPB
    assert one(r'getenv\("IE_HUF_CHUNK"\) \? strtoull\(getenv\("IE_HUF_CHUNK"\), nullptr, 10\) : (\d+);', capi) == CHUNK
    assert "kHufEmitT = 2 * kTPB" in hip  # two emit lanes per chunk: its halves


# ------------------------------------------------------------------ 5. the wrapped files
def test_manifest_covers_exactly_the_wrapped_entries():
    assert [m["name"] for m in MANIFEST] == list(CH.WRAPPED.values())
    assert [m["family"] for m in MANIFEST] == list(CH.WRAPPED)


@pytest.mark.parametrize("family", list(CH.WRAPPED))
def test_wrapped_file_is_the_pinned_one(family):
    m = next(m for m in MANIFEST if m["family"] == family)
    name, data, plain = CH.wrapped(family)
    assert name == m["name"] and (m["w"], m["h"]) == CH.wrap_dims(family)
    assert _md5(data) == m["md5"]
    e = CH.by_name(name)
    assert data[: e.code_start // 8] == e.data[: e.code_start // 8]  # the entry's dictionary
    huf = O.load().huffman_decode(data)
    assert huf is not None and not huf[1] and _md5(huf[0]) == m["huf_md5"]
    assert huf[0][: len(plain)] == plain and len(huf[0]) - len(plain) < 8
    assert H.Model(data, e.lut, e.code_start).decode() == huf[0]
    px = np.asarray(O.load().decode_image(data, 4))
    assert px.shape == (m["h"], m["w"]) and _md5(px.tobytes()) == m["dec_md5"]  # the oracle's pixels == the reference's
