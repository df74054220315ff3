"""ie_huffman_decode_batch (Codec.huffman_decode_batch): a batch of Huffman code streams decoded by
one set of launches -- every pass of the exact Huffman parse with the image as its grid's y
dimension, one chunk plan for the batch -- against the CPU oracle's per-bit walk of every stream,
byte for byte including the symbols the padding bits decode to, and against the single-stream
ie_huffman_decode on the same stream.

The streams are the outputs of codec.huffman_encode.  Chunk constants of ie_huffman_decode.hip:
1024-bit chunks, kHufTC = 64 chunks per table workgroup, kTPB = 256 chunks per count / emit workgroup,
kHufG = 256 tables per composition group.

b"\\x07\\x08" gains nothing from the Huffman pass, so its file carries no dictionary (the '0' + the
bytes, Huffman.cpp:329-341): there is no code stream and no prefix table.  It enters the batches as
what it is -- an empty code stream (start_bit = 8 * len), for which the oracle's decode returns no
symbol -- and "short" (the same two bytes, 40 times: a coded stream of about 110 bits) is the coded
stream shorter than one chunk.
"""
import numpy as np
import pytest

from imageencoder_amd import IE_ECAP, IE_EFORMAT, IE_EINVAL, IEError
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

CHUNK, TC, TPB, G = 1024, 64, 256, 256
U64MAX = (1 << 64) - 1
GUARD = 0xA5
_STATE = {}


def _codec():
    if "codec" not in _STATE:
        from imageencoder_amd import Codec
        _STATE["codec"] = Codec(0)
    return _STATE["codec"]


class Stream:
    """One input: its Huffman-coded file, its prefix table and code start, the oracle's decode and
    the single-stream device decode (the references: computed once, never changed)."""

    def __init__(self, enc: bytes, start_bit=None):
        import torch
        c = _codec()
        self.enc = enc
        self.len = len(enc)
        t = c.huffman_table(enc)
        if t is None:  # no dictionary: no code stream
            self.lut, self.sb = np.zeros(32768, dtype=np.uint16), 8 * len(enc)
        else:
            self.lut, self.sb = t
        if start_bit is not None:
            self.sb = start_bit
        self.coded = t is not None and self.sb < 8 * len(enc)
        exp = O.load().huffman_decode(enc)
        self.exp = None if exp is None else (exp[0] if self.coded else b"")
        self.chunks = (8 * self.len - self.sb + CHUNK - 1) // CHUNK
        self.single = None
        if self.exp is not None:
            d = torch.from_numpy(np.frombuffer(enc + b"\0" * (-len(enc) % 4 + 4), np.uint8).copy()).cuda()
            out = torch.zeros(8 * self.len + 16, dtype=torch.uint8, device="cuda")
            n = c.huffman_decode_device(d, self.len, torch.from_numpy(self.lut).cuda(), self.sb, out)
            self.single = out[:n].cpu().numpy().tobytes()


def _encode(data: bytes) -> bytes:
    return _codec().huffman_encode(np.frombuffer(data, np.uint8).copy())


def _streams():
    if "streams" in _STATE:
        return _STATE["streams"]
    rng = np.random.default_rng(5)
    skew = rng.geometric(0.2, size=20000).clip(1, 255).astype(np.uint8)  # long codes (<= 15 bits)
    s = {
        "two_bytes": Stream(_encode(b"\x07\x08")),
        "short": Stream(_encode(b"\x07\x08" * 40)),
        "two_symbols": Stream(_encode(bytes(rng.integers(0, 2, size=3001, dtype=np.uint8) * 0xFF))),
        "skewed": Stream(_encode(skew.tobytes())),
    }
    size = 150000
    while True:  # more than kTPB chunks: two emit workgroups, a second composition level
        big = rng.geometric(0.25, size=size).clip(1, 24).astype(np.uint8)
        s["big"] = Stream(_encode(big.tobytes()))
        if s["big"].chunks > max(TPB, G):
            break
        size *= 2
    # the crafted stream of test_huffman_decode_rejects_invalid: codes 00 and 01, so 1x is no code
    bw = "1" + format(2, "07b") + format(2, "04b") + format(1, "08b") + "00" + format(2, "08b") + "01" + "0"
    bw += "00" * 8 + "1"
    bw += "0" * (-len(bw) % 8)
    s["invalid"] = Stream(int(bw, 2).to_bytes(len(bw) // 8, "big"))
    _STATE["streams"] = s
    return s


def _pick(*names):
    s = _streams()
    return [s[n] for n in names]


def _run(streams, where="device", out_pitch=None, lens=None, start_bits=None, in_pitch=None):
    """One batch call.  where: "device" (in, lut and out on the device, read in place), "host", or
    "offset" (a device `in` one byte off alignment with an odd pitch: the staging path).  Returns
    (counts or the IEError, the output slots with the guard fill where nothing was written, and the
    guard bytes after the last slot)."""
    import torch
    c = _codec()
    count = len(streams)
    longest = max(s.len for s in streams)
    if in_pitch is None:
        in_pitch = (longest + 15) // 16 * 16 if where != "offset" else (longest + 16) | 1
    slots = np.zeros(count * in_pitch + 1, dtype=np.uint8)
    off = 1 if where == "offset" else 0
    for k, s in enumerate(streams):
        slots[off + k * in_pitch: off + k * in_pitch + s.len] = np.frombuffer(s.enc, np.uint8)
    luts = np.concatenate([s.lut for s in streams])
    if out_pitch is None:
        out_pitch = max(len(s.exp or b"") for s in streams) + 37
    out = np.full(count * out_pitch + 64, GUARD, dtype=np.uint8)
    lens = [s.len for s in streams] if lens is None else lens
    start_bits = [s.sb for s in streams] if start_bits is None else start_bits
    if where == "host":
        d_in, d_lut, d_out = slots, luts, out
    else:
        d_in, d_lut, d_out = torch.from_numpy(slots).cuda()[off:], torch.from_numpy(luts).cuda(), torch.from_numpy(out).cuda()
    try:
        res = c.huffman_decode_batch(d_in, in_pitch, lens, start_bits, d_lut, d_out, out_pitch)
    except IEError as e:
        res = e
    got = d_out if where == "host" else d_out.cpu().numpy()
    return res, got[: count * out_pitch].reshape(count, out_pitch), got[count * out_pitch:]


def _check_complete(streams, counts, slots, skip=()):
    for k, s in enumerate(streams):
        if k in skip:
            continue
        n = int(counts[k])
        assert n == len(s.exp), (k, n, len(s.exp))
        assert slots[k, :n].tobytes() == s.exp, k
        assert slots[k, :n].tobytes() == s.single, k
        assert np.all(slots[k, n:] == GUARD), k


def test_inputs_cover_the_chunk_thresholds():
    s = _streams()
    assert s["big"].chunks > max(TPB, G)  # (first: the rest of this module relies on it)
    assert not s["two_bytes"].coded and s["two_bytes"].exp == b""
    assert s["short"].coded and s["short"].chunks == 1
    assert s["two_symbols"].coded and 1 < s["two_symbols"].chunks < TC and s["two_symbols"].chunks % TC
    assert TC < s["skewed"].chunks < TPB
    assert s["invalid"].exp is None
    coded = [s[n] for n in ("short", "two_symbols", "skewed", "big")]
    assert len({x.sb for x in coded}) > 1 and len({x.sb % 32 for x in coded}) > 1  # dictionaries differ
    for x in coded:
        assert x.single == x.exp


@pytest.mark.parametrize("order", [("big", "two_bytes", "short", "two_symbols", "skewed"),
                                   ("two_bytes", "skewed", "short", "two_symbols", "big")],
                         ids=["longest_first", "longest_last"])
def test_mixed_lengths(order):
    streams = _pick(*order)
    counts, slots, tail = _run(streams)
    assert not isinstance(counts, IEError), counts
    _check_complete(streams, counts, slots)
    assert np.all(tail == GUARD)


def test_batch_of_one_equals_the_single_call():
    streams = _pick("skewed")
    counts, slots, tail = _run(streams)
    assert not isinstance(counts, IEError), counts
    _check_complete(streams, counts, slots)
    assert np.all(tail == GUARD)


def test_empty_code_stream_among_others():
    s = _streams()
    empty = Stream(s["short"].enc, start_bit=8 * s["short"].len)
    assert empty.exp == b"" and empty.single == b""
    streams = [s["two_symbols"], empty, s["short"]]
    counts, slots, tail = _run(streams)
    assert not isinstance(counts, IEError), counts
    assert int(counts[1]) == 0 and np.all(slots[1] == GUARD)
    _check_complete(streams, counts, slots)


@pytest.mark.parametrize("where", ["device", "host", "offset"])
def test_guard_fill_every_placement(where):
    streams = _pick("short", "skewed", "two_bytes", "two_symbols")
    counts, slots, tail = _run(streams, where=where)
    assert not isinstance(counts, IEError), counts
    _check_complete(streams, counts, slots)
    assert np.all(tail == GUARD)


@pytest.mark.parametrize("where", ["device", "host"])
def test_capacity(where):
    streams = _pick("short", "two_symbols", "skewed")
    pitch = len(streams[2].exp) - 777
    assert pitch > len(streams[1].exp)
    err, slots, tail = _run(streams, where=where, out_pitch=pitch)
    assert isinstance(err, IEError) and err.code == IE_ECAP and "image 2" in str(err), err
    assert int(err.counts[2]) == len(streams[2].exp)
    assert slots[2].tobytes() == streams[2].exp[:pitch]
    assert np.all(tail == GUARD)  # nothing past the slot
    _check_complete(streams, err.counts, slots, skip=(2,))


def test_invalid_code():
    streams = _pick("short", "invalid", "two_symbols")
    err, slots, tail = _run(streams, out_pitch=len(streams[2].exp) + 37)
    assert isinstance(err, IEError) and err.code == IE_EFORMAT and "image 1" in str(err), err
    assert int(err.counts[1]) == U64MAX
    _check_complete(streams, err.counts, slots, skip=(1,))
    assert np.all(tail == GUARD)


@pytest.mark.parametrize("order, code, bad", [(("short", "skewed", "invalid"), IE_ECAP, 1),
                                              (("short", "invalid", "skewed"), IE_EFORMAT, 1)])
def test_lowest_failing_image_decides(order, code, bad):
    streams = _pick(*order)
    pitch = len(_streams()["skewed"].exp) - 777
    err, slots, tail = _run(streams, out_pitch=pitch)
    assert isinstance(err, IEError) and err.code == code and f"image {bad}" in str(err), err
    k = order.index("skewed")
    assert int(err.counts[k]) == len(streams[k].exp) and slots[k].tobytes() == streams[k].exp[:pitch]
    assert int(err.counts[order.index("invalid")]) == U64MAX
    _check_complete(streams, err.counts, slots, skip=(1, 2))


def test_argument_checks():
    streams = _pick("short", "two_symbols")
    err, _, _ = _run(streams, lens=[], start_bits=[])
    assert isinstance(err, IEError) and err.code == IE_EINVAL, err
    pitch = (max(s.len for s in streams) + 15) // 16 * 16
    err, slots, _ = _run(streams, lens=[streams[0].len, pitch + 1], in_pitch=pitch)
    assert isinstance(err, IEError) and err.code == IE_EINVAL and "image 1" in str(err), err
    assert np.all(slots == GUARD)
    err, slots, _ = _run(streams, start_bits=[8 * streams[0].len + 1, streams[1].sb])
    assert isinstance(err, IEError) and err.code == IE_EINVAL and "image 0" in str(err), err
    assert np.all(slots == GUARD)
