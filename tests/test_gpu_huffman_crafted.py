"""The device Huffman decoders on valid streams that no encoder here writes (tests/crafted_huffman.py).

Every valid entry of the table goes through
  * Codec.huffman_decode (host stream, host output),
  * ie_huffman_decode with the stream read in place and a device table, into device memory filled
    with 0xA5: with out_cap = the symbol count (the bytes after it untouched) and with one less
    (IE_ECAP, the first out_cap symbols there, nothing at or past out_cap) -- on the staged emit
    path and on the direct one, whichever the entry takes,
  * ie_huffman_decode_batch in batches that mix the families (the dictionaries differ in length, so
    every image has its own start-bit phase), longest first and longest last, with device, host and
    misaligned device buffers,
and must equal the oracle's per-bit walk byte for byte, the symbols of the padding bits included.
Every invalid entry must come back as IE_EFORMAT, alone and among valid neighbours.  The image files
wrapped in the families' dictionaries go through decode_image_file and decode_image_files against
the oracle's pixels and the md5 of the REFERENCE's decode (manifest_crafted_huffman.json).

tests/test_crafted_huffman.py shows on the CPU what the entries reach inside the kernels.  The
entries, their oracle decodes and their single-stream device decodes are made once per module.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from imageencoder_amd import IE_ECAP, IE_EFORMAT, IEError
from tests import crafted_huffman as CH
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

GUARD = 0xA5
U64MAX = (1 << 64) - 1
NBATCH = 5
MANIFEST = {m["family"]: m for m in json.load(open(os.path.join(O.GOLDEN, "manifest_crafted_huffman.json")))}
VALID = [e.name for e in CH.valid_entries()]
INVALID = [e.name for e in CH.by_family("invalid")]
_STATE = {}


def _codec():
    if "codec" not in _STATE:
        from imageencoder_amd import Codec
        _STATE["codec"] = Codec(0)
    return _STATE["codec"]


class Item:
    """One entry: its file, the builder's table and code start, the oracle's decode (the reference:
    computed once, never changed) and, once test_device_exact_capacity has run or on first use, the
    single-stream device decode."""

    def __init__(self, e):
        self.e, self.name, self.enc, self.len, self.lut, self.sb = e, e.name, e.data, len(e.data), np.array(e.lut), e.code_start
        exp = O.load().huffman_decode(e.data)
        self.exp = None if exp is None else exp[0]
        assert (self.exp is not None) == e.valid
        self._single = None

    def device_stream(self):
        import torch
        return torch.from_numpy(np.frombuffer(self.enc + b"\0" * (-self.len % 4), np.uint8).copy()).cuda()

    def decode_device(self, cap: int, room: int = 64):
        """ie_huffman_decode, stream and table on the device, into the first `cap` bytes of a
        buffer of cap + room guard bytes: (count or the IEError, the whole buffer)."""
        import torch
        buf = torch.full((cap + room,), GUARD, dtype=torch.uint8, device="cuda")
        d = self.device_stream()
        assert d.data_ptr() % 4 == 0
        try:
            res = _codec().huffman_decode_device(d, self.len, torch.from_numpy(self.lut).cuda(), self.sb, buf[:cap])
        except IEError as err:
            res = err
        return res, buf.cpu().numpy()

    @property
    def single(self) -> bytes:
        if self._single is None:
            n, buf = self.decode_device(len(self.exp))
            assert n == len(self.exp)
            self._single = buf[:n].tobytes()
        return self._single


def _item(name) -> Item:
    if name not in _STATE:
        _STATE[name] = Item(CH.by_name(name))
    return _STATE[name]


def _first_diff(got: bytes, exp: bytes) -> str:
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(exp, np.uint8)
    n = min(a.size, b.size)
    bad = np.flatnonzero(a[:n] != b[:n])
    return f"{a.size} symbols against {b.size}, first difference at {int(bad[0]) if bad.size else n} ({bad.size} differ)"


# ------------------------------------------------------------------ 1. single streams
@pytest.mark.parametrize("name", VALID)
def test_host_decode(name):
    it = _item(name)
    got, passthrough = _codec().huffman_decode(it.enc)
    assert not passthrough
    assert got == it.exp, _first_diff(got, it.exp)


@pytest.mark.parametrize("name", VALID)
def test_device_exact_capacity(name):
    it = _item(name)
    n = len(it.exp)
    res, buf = it.decode_device(n)
    assert not isinstance(res, IEError), res
    assert res == n
    assert buf[:n].tobytes() == it.exp, _first_diff(buf[:n].tobytes(), it.exp)
    assert np.all(buf[n:] == GUARD)
    it._single = buf[:n].tobytes()


@pytest.mark.parametrize("name", VALID)
def test_device_one_byte_short(name):
    it = _item(name)
    n = len(it.exp)
    res, buf = it.decode_device(n - 1)
    assert isinstance(res, IEError) and res.code == IE_ECAP, res
    assert np.all(buf[n - 1:] == GUARD)  # nothing at or past out_cap
    assert buf[: n - 1].tobytes() == it.exp[: n - 1], _first_diff(buf[: n - 1].tobytes(), it.exp[: n - 1])


def test_both_emit_paths_were_taken():
    """Among the entries above, first emit workgroups on each side of IE_HUF_EMIT_LDS and on it (the
    symbol counts are the oracle's)."""
    counts = {n: int(CH.by_name(n).model.chunk_counts(CH.CHUNK)[0][: CH.TPB].sum()) for n in VALID}
    assert counts["emit_exact"] == CH.EMIT_LDS and counts["emit_plus_one"] == CH.EMIT_LDS + 1
    assert len(_item("emit_exact").exp) == CH.EMIT_LDS and len(_item("emit_plus_one").exp) == CH.EMIT_LDS + 1
    assert counts["emit_below"] < CH.EMIT_LDS < counts["emit_above"]


# ------------------------------------------------------------------ 2. batches
def _batches():
    """The valid entries dealt into NBATCH batches: the table is ordered by family, so every batch
    mixes them."""
    return [VALID[i::NBATCH] for i in range(NBATCH)]


def _run(items, where="device", out_pitch=None):
    """One batch call.  where: "device" (in, lut and out on the device, read in place), "host", or
    "offset" (a device `in` one byte off alignment with an odd pitch: the staging path).  Returns
    (counts or the IEError, the output slots, the guard bytes after the last slot)."""
    import torch
    c = _codec()
    count = len(items)
    longest = max(it.len for it in items)
    in_pitch = (longest + 15) // 16 * 16 if where != "offset" else (longest + 16) | 1
    slots = np.zeros(count * in_pitch + 1, dtype=np.uint8)
    off = 1 if where == "offset" else 0
    for k, it in enumerate(items):
        slots[off + k * in_pitch: off + k * in_pitch + it.len] = np.frombuffer(it.enc, np.uint8)
    luts = np.concatenate([it.lut for it in items])
    if out_pitch is None:
        out_pitch = max(len(it.exp or b"") for it in items) + 37
    out = np.full(count * out_pitch + 64, GUARD, dtype=np.uint8)
    lens, start_bits = [it.len for it in items], [it.sb for it in items]
    if where == "host":
        d_in, d_lut, d_out = slots, luts, out
    else:
        d_in, d_lut, d_out = torch.from_numpy(slots).cuda()[off:], torch.from_numpy(luts).cuda(), torch.from_numpy(out).cuda()
    try:
        res = c.huffman_decode_batch(d_in, in_pitch, lens, start_bits, d_lut, d_out, out_pitch)
    except IEError as err:
        res = err
    got = d_out if where == "host" else d_out.cpu().numpy()
    return res, got[: count * out_pitch].reshape(count, out_pitch), got[count * out_pitch:]


def _check_complete(items, counts, slots, skip=()):
    for k, it in enumerate(items):
        if k in skip:
            continue
        n = int(counts[k])
        assert n == len(it.exp), (it.name, n, len(it.exp))
        assert slots[k, :n].tobytes() == it.exp, (it.name, _first_diff(slots[k, :n].tobytes(), it.exp))
        assert slots[k, :n].tobytes() == it.single, it.name
        assert np.all(slots[k, n:] == GUARD), it.name


def test_batches_mix_the_families():
    names = _batches()
    assert sorted(n for b in names for n in b) == sorted(VALID)
    for b in names:
        es = [CH.by_name(n) for n in b]
        assert len({e.family for e in es}) >= 3
        assert len({e.code_start for e in es}) >= 3 and len({e.code_start % 32 for e in es}) >= 2
        assert len({e.chunks for e in es}) >= 3


@pytest.mark.parametrize("where", ["device", "host", "offset"])
@pytest.mark.parametrize("order", ["longest_first", "longest_last"])
@pytest.mark.parametrize("b", range(NBATCH))
def test_batch(b, order, where):
    items = sorted((_item(n) for n in _batches()[b]), key=lambda it: it.len, reverse=(order == "longest_first"))
    counts, slots, tail = _run(items, where=where)
    assert not isinstance(counts, IEError), counts
    _check_complete(items, counts, slots)
    assert np.all(tail == GUARD)


# ------------------------------------------------------------------ 3. invalid streams
@pytest.mark.parametrize("name", INVALID)
def test_invalid_single_stream(name):
    it = _item(name)
    assert it.exp is None
    with pytest.raises(IEError) as err:
        _codec().huffman_decode(it.enc)
    assert err.value.code == IE_EFORMAT, err.value
    res, _ = it.decode_device(8 * it.len + 16)
    assert isinstance(res, IEError) and res.code == IE_EFORMAT, res


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("name", INVALID)
def test_invalid_among_valid_neighbours(name, where):
    items = [_item("sizes_3_chunks_plus"), _item(name), _item("l1_comb")]
    err, slots, tail = _run(items, where=where, out_pitch=8 * max(it.len for it in items) + 16)
    assert isinstance(err, IEError) and err.code == IE_EFORMAT and "image 1" in str(err), err
    assert int(err.counts[1]) == U64MAX
    _check_complete(items, err.counts, slots, skip=(1,))
    assert np.all(tail == GUARD)


@pytest.mark.parametrize("order, code, bad", [(("sizes_short", "dup_9", "invalid_second_half", "invalid_first_chunk"), IE_ECAP, 1),
                                              (("sizes_short", "invalid_last_chunk", "dup_9", "invalid_padding"), IE_EFORMAT, 1)])
def test_lowest_failing_image_decides(order, code, bad):
    items = [_item(n) for n in order]
    pitch = len(_item("dup_9").exp) - 777
    assert pitch > len(_item("sizes_short").exp)
    err, slots, tail = _run(items, out_pitch=pitch)
    assert isinstance(err, IEError) and err.code == code and f"image {bad}" in str(err), err
    k = order.index("dup_9")
    assert int(err.counts[k]) == len(items[k].exp) and slots[k].tobytes() == items[k].exp[:pitch]
    for j, n in enumerate(order):
        if n.startswith("invalid"):
            assert int(err.counts[j]) == U64MAX
    _check_complete(items, err.counts, slots, skip=(1, 2, 3))
    assert np.all(tail == GUARD)


# ------------------------------------------------------------------ 4. whole image files
def _wrapped(family):
    """(file, the oracle's pixels) of a family's wrapped image: once per module."""
    key = ("wrapped", family)
    if key not in _STATE:
        _, data, _ = CH.wrapped(family)
        m = MANIFEST[family]
        px = np.asarray(O.load().decode_image(data, 4)).reshape(m["h"], m["w"])
        px.setflags(write=False)
        _STATE[key] = (data, px)
    return _STATE[key]


def _check_pixels(family, got):
    data, ref = _wrapped(family)
    assert np.array_equal(np.asarray(got), ref), family
    assert hashlib.md5(np.ascontiguousarray(got).tobytes()).hexdigest() == MANIFEST[family]["dec_md5"], (family, "reference md5")


@pytest.mark.parametrize("family", list(CH.WRAPPED))
def test_wrapped_image_file(family):
    data, _ = _wrapped(family)
    assert hashlib.md5(data).hexdigest() == MANIFEST[family]["md5"]
    _check_pixels(family, _codec().decode_image_file(data, 4))


def test_wrapped_image_files_batch():
    """The 64 x 32 files as ONE decode_image_files batch (five dictionaries, five start-bit phases);
    the 256 x 256 one -- more than 256 chunks -- beside the oracle encoder's own file of another
    picture of that size."""
    from imageencoder_amd import synth
    small = [f for f in CH.WRAPPED if CH.wrap_dims(f) == (64, 32)]
    assert len(small) == 5
    got = _codec().decode_image_files([_wrapped(f)[0] for f in small], 4)
    for k, f in enumerate(small):
        _check_pixels(f, got[k])
    data, _ = _wrapped("sizes")
    e = CH.by_name(CH.WRAPPED["sizes"])
    assert (8 * len(data) - e.code_start + CH.CHUNK - 1) // CH.CHUNK > CH.TPB
    o = O.load()
    other = o.encode_image(synth.frame("M", 256, 256, seed=37), 4, O.read_matrix("matrix.txt", 4), rle=True, huffman=True)
    assert _codec().huffman_table(other) is not None
    got = _codec().decode_image_files([other, data], 4)
    _check_pixels("sizes", got[1])
    assert np.array_equal(got[0], np.asarray(o.decode_image(other, 4)).reshape(256, 256))
