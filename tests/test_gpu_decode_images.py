"""ie_decode_images (Codec.decode_images): a batch of independent images decoded by one set of
launches -- every pass of the exact record parse with the image as its grid's y dimension, one chunk
plan for the batch -- against the CPU oracle's decode of every whole file and the single-stream
ie_decode_frames on every slot.  Bit-exact is the bar for every pixel and end bit.

Streams are whole files (settings header + payload, no Huffman pass), so start_bit is the header's
length and the same for every image of a test.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest

from imageencoder_amd import IE_EFORMAT, IE_EINVAL, synth
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

U64MAX = (1 << 64) - 1
_CODECS = {}
_BATCHES = {}


def _q(n):
    return O.read_matrix("matrix.txt" if n == 4 else "matrix8_1.txt", n)


def _codec(n):
    """One context per block size for the whole module."""
    if n not in _CODECS:
        from imageencoder_amd import Codec
        _CODECS[n] = Codec(0, _q(n), n)
    return _CODECS[n]


def _images(w, h, kinds):
    out = []
    for i, k in enumerate(kinds):
        if isinstance(k, int):
            out.append(np.full((h, w), k, dtype=np.uint8))
        else:
            out.append(synth.frame(k, w, h, seed=101 + i))
    return out


class Batch:
    """Files of the oracle's encoder in slots of `pitch` bytes, with the oracle's decode of every
    file and decode_frames' end bit of every slot (the references: computed once, never changed)."""

    def __init__(self, n, rle, w, h, kinds, pitch_mod=(16, 0)):
        o = O.load()
        q = _q(n)
        self.n, self.rle, self.w, self.h = n, rle, w, h
        self.files = [o.encode_image(y, n, q, rle=rle) for y in _images(w, h, kinds)]
        self.hb = o.header(n, q, int(rle), w, h)[1]
        self.ref = [np.asarray(o.decode_image(f, n)).reshape(h, w) for f in self.files]
        self.count = len(self.files)
        longest = max(len(f) for f in self.files)
        self.pitch = self.pitch_for(longest, *pitch_mod)
        self.slots = self.pack(self.pitch)
        self.nbits = np.array([8 * len(f) for f in self.files], dtype=np.uint64)
        c = _codec(n)
        pix = np.zeros((h, w), dtype=np.uint8)
        self.ends = []
        for k, f in enumerate(self.files):
            self.ends.append(c.decode_frames(np.frombuffer(f, np.uint8).copy(), w, h, pix, start_bit=self.hb, rle=rle))
            assert np.array_equal(pix, self.ref[k]), k
        self.ends = np.array(self.ends, dtype=np.uint64)

    @staticmethod
    def pitch_for(longest, mod, rem):
        p = (longest + 8 + mod - 1) // mod * mod
        return p + rem

    def pack(self, pitch, fill=0):
        s = np.full(self.count * pitch, fill, dtype=np.uint8)
        for k, f in enumerate(self.files):
            s[k * pitch: k * pitch + len(f)] = np.frombuffer(f, np.uint8)
        return s


MIXED = [77, "U", "M", 200, "U"]  # constant, noise, mixed, constant, noise


def _batch(n, rle, w=64, h=48, kinds=tuple(MIXED)):
    key = (n, rle, w, h, kinds)
    if key not in _BATCHES:
        _BATCHES[key] = Batch(n, rle, w, h, list(kinds))
    return _BATCHES[key]


def _planned_chunk_bits(n, span, nblocks):
    """The chunk length the library plans for the longest span (ie_capi_decode.cpp plan_chunks): about 24
    (4x4) / 28 (8x8) records per chunk, a multiple of 32 within [256, 2^15]."""
    recs = 24 if n == 4 else 28
    want = max((nblocks + recs - 1) // recs, 1)
    c = (span + want - 1) // want
    return min(max((c + 31) // 32 * 32, 256), 1 << 15)


def _decode(b, streams=None, pitch=None, nbits=None, **kw):
    out = np.zeros((b.count, b.h, b.w), dtype=np.uint8)
    ends = _codec(b.n).decode_images(b.slots if streams is None else streams, b.pitch if pitch is None else pitch,
                                     b.nbits if nbits is None else nbits, b.w, b.h, out, start_bit=b.hb, rle=b.rle,
                                     **kw)
    return out, ends


# ------------------------------------------------------------------ 1. batch against the oracle
@pytest.mark.parametrize("rle", [True, False], ids=["rle", "norle"])
@pytest.mark.parametrize("n", [4, 8])
def test_batch_mixed_content_vs_oracle(n, rle):
    """Five 64x48 images of very different content (constant, noise, mixed) in one batch: every
    image's pixels == the oracle's decode of its file, every end bit == decode_frames' on its slot.
    The constant images' streams are a fraction of the noise images': their trailing chunks hold no
    record.  (A 64x48 image has 192 (4x4) / 48 (8x8) records in all, so no chunk of it can hold
    more than kRecPosCap = 256: the walk-again branch is test_batch_walk_again's.)"""
    b = _batch(n, rle)
    out, ends = _decode(b)
    for k in range(b.count):
        assert np.array_equal(out[k], b.ref[k]), k
    assert np.array_equal(ends, b.ends)
    if rle:  # (without RLE every record holds all its values: the streams differ by bit length only)
        spans = b.nbits - np.uint64(b.hb)
        assert int(spans.min()) * 2 < int(spans.max())  # the shortest stream leaves empty trailing chunks
    assert not _codec(n).last_decode_spec()


@pytest.mark.parametrize("n", [4, 8])
def test_batch_walk_again(n):
    """The same mix at 256x192 (3072 / 768 records per image), RLE on.  One chunk length serves the
    batch, sized by the noise images' streams; checked here on the CPU from the oracle's stream
    lengths: the records of the constant-128 image (all of one length) then number MORE THAN
    kRecPosCap = 256 per chunk of the planned C, so its decode waves take rec_decode_kernel's
    walk-again branch (position lists hold 256), next to the noise images' listed chunks and the
    constant images' empty trailing chunks."""
    w, h = 256, 192
    b = _batch(n, True, w, h, kinds=(128, "U", "M", 77, "U"))
    nblocks = (w // n) * (h // n)
    span = int(b.nbits.max()) - b.hb
    cbits = _planned_chunk_bits(n, span, nblocks)
    # image 0, constant 128: 5-bit records against the noise images' 108 (4x4) / 479 (8x8) bits
    rec_bits = (int(b.ends[0]) - b.hb) // nblocks
    assert (int(b.ends[0]) - b.hb) == rec_bits * nblocks  # every record the same length
    assert min(nblocks, cbits // rec_bits) > 256, (cbits, rec_bits)  # records of its first chunk
    out, ends = _decode(b)
    assert _codec(n).last_decode_info()[0] == (span + cbits - 1) // cbits  # (the plan mirrored above)
    for k in range(b.count):
        assert np.array_equal(out[k], b.ref[k]), k
    assert np.array_equal(ends, b.ends)


# ------------------------------------------------------------------ 2. count = 1
def test_count_one_equals_decode_frames():
    """A golden file with a pinned reference decode (below 1920x1080, no Huffman pass): count = 1
    gives decode_frames' pixels (md5 == the manifest's) and end bit."""
    c = next(c for c in O.manifest() if c.get("dec_md5") and not c["huffman"] and not c["video"] and "file" in c
             and 64 * 48 <= c["w"] * c["h"] < 1920 * 1080)
    n, w, h, rle = c["n"], c["w"], c["h"], bool(c["rle"])
    from imageencoder_amd import Codec
    codec = Codec(0, O.read_matrix(c["matrix"], n), n)
    enc = np.frombuffer(O.case_expected(c), np.uint8).copy()
    hb = O.load().header(n, O.read_matrix(c["matrix"], n), int(rle), w, h)[1]
    one = np.zeros((h, w), dtype=np.uint8)
    end = codec.decode_frames(enc, w, h, one, start_bit=hb, rle=rle)
    got = np.zeros((h, w), dtype=np.uint8)
    ends = codec.decode_images(enc, enc.size, [8 * enc.size], w, h, got, start_bit=hb, rle=rle)
    assert hashlib.md5(one.tobytes()).hexdigest() == c["dec_md5"]
    assert hashlib.md5(got.tobytes()).hexdigest() == c["dec_md5"]
    assert list(ends) == [end]
    codec.close()


# ------------------------------------------------------------------ 3. two composition levels
@pytest.mark.parametrize("n,w,h", [(4, 768, 576), (8, 1928, 1080)])
def test_two_composition_levels(n, w, h):
    """More chunks than G^2 = 1024 (27 648 4x4 blocks: about 1 152 chunks; 32 535 8x8 blocks: about
    1 162): two composition levels per image, three images, each == the single-image decode."""
    import torch
    c = _codec(n)
    o = O.load()
    ys = _images(w, h, ["U", "M", "U"])
    files = [np.frombuffer(o.encode_image(y, n, _q(n), rle=True), np.uint8) for y in ys]
    hb = o.header(n, _q(n), 1, w, h)[1]
    pitch = (max(f.size for f in files) + 31) // 16 * 16
    slots = torch.zeros(3 * pitch, dtype=torch.uint8, device="cuda")
    for k, f in enumerate(files):
        slots[k * pitch: k * pitch + f.size] = torch.from_numpy(f.copy()).cuda()
    out = torch.zeros((3, h, w), dtype=torch.uint8, device="cuda")
    ends = c.decode_images(slots, pitch, [8 * f.size for f in files], w, h, out, start_bit=hb)
    chunks, levels = c.last_decode_info()
    assert levels >= 2 and chunks > 1024, (chunks, levels)
    one = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    for k, f in enumerate(files):
        e = c.decode_frames(slots[k * pitch:], w, h, one, start_bit=hb, length=f.size)
        assert int(ends[k]) == e, k
        assert torch.equal(out[k], one), k


# ------------------------------------------------------------------ 4. slack bits
@pytest.mark.parametrize("n", [4, 8])
def test_slack_bits_ignored(n):
    """nbits[k] = the exact payload end; every byte of a slot past ceil(nbits[k] / 8) is 0xFF and the
    unused low bits of the last byte are ones: pixels and end bits are unchanged."""
    b = _batch(n, True)
    slots = b.pack(b.pitch, fill=0xFF)
    for k in range(b.count):
        end = int(b.ends[k])
        last = k * b.pitch + (end + 7) // 8
        slots[last: (k + 1) * b.pitch] = 0xFF
        if end % 8:
            slots[last - 1] |= 0xFF >> (end % 8)
    for dev in (False, True):
        s = slots
        if dev:
            import torch
            s = torch.from_numpy(slots).cuda()
        out, ends = _decode(b, streams=s, nbits=b.ends)
        for k in range(b.count):
            assert np.array_equal(out[k], b.ref[k]), (dev, k)
        assert np.array_equal(ends, b.ends), dev


# ------------------------------------------------------------------ 5. placement
@pytest.mark.parametrize("n", [4, 8])
def test_input_placement(n):
    """Host input; device input read in place (16-byte aligned, pitch a multiple of 16); device
    input with in_pitch % 16 == 4 and with its base 4 bytes off (both staged): identical pixels."""
    import torch
    b = _batch(n, True)
    ref, ends = _decode(b)  # host input, host output
    assert np.array_equal(ends, b.ends)
    longest = max(len(f) for f in b.files)
    for name, pitch, off in (("in place", b.pitch, 0), ("pitch % 16 == 4", Batch.pitch_for(longest, 16, 4), 0),
                             ("base + 4", b.pitch, 4)):
        assert b.pitch % 16 == 0 and pitch % 16 in (0, 4)
        dev = torch.full((b.count * pitch + 16 + off,), 0xEE, dtype=torch.uint8, device="cuda")
        assert dev.data_ptr() % 16 == 0
        dev[off: off + b.count * pitch] = torch.from_numpy(b.pack(pitch)).cuda()
        out = torch.zeros((b.count, b.h, b.w), dtype=torch.uint8, device="cuda")
        e = _codec(n).decode_images(dev[off:], pitch, b.nbits, b.w, b.h, out, start_bit=b.hb)
        assert np.array_equal(e, b.ends), name
        assert np.array_equal(out.cpu().numpy(), ref), name


@pytest.mark.parametrize("dev_out", [False, True], ids=["host_out", "device_out"])
def test_output_stride_and_pitch(dev_out):
    """stride = w + 24, frame_pitch = stride * h + 40: the bytes between rows and images (0xA5)
    are untouched."""
    b = _batch(4, True)
    stride = b.w + 24
    fp = stride * b.h + 40
    buf = np.full(b.count * fp, 0xA5, dtype=np.uint8)
    dst = buf
    if dev_out:
        import torch
        dst = torch.from_numpy(buf).cuda()
    ends = _codec(4).decode_images(b.slots, b.pitch, b.nbits, b.w, b.h, dst, start_bit=b.hb, stride=stride,
                                   frame_pitch=fp)
    got = dst.cpu().numpy() if dev_out else dst
    assert np.array_equal(ends, b.ends)
    exp = np.full(b.count * fp, 0xA5, dtype=np.uint8)
    for k in range(b.count):
        rows = exp[k * fp: k * fp + stride * b.h].reshape(b.h, stride)
        rows[:, : b.w] = b.ref[k]
    assert np.array_equal(got, exp)


# ------------------------------------------------------------------ 6. one truncated image
@pytest.mark.parametrize("dev_out", [False, True], ids=["host_out", "device_out"])
def test_one_truncated_image(dev_out):
    """Image 2 of four cut in half: IE_EFORMAT naming image 2, end_bits[2] = UINT64_MAX (raw call),
    and images 0, 1 and 3 decoded as in a good batch."""
    from imageencoder_amd import IEError
    b = _batch(4, True, kinds=("U", "M", "U", 77))
    c = _codec(4)
    nbits = b.nbits.copy()
    nbits[2] = np.uint64(b.hb + (int(b.ends[2]) - b.hb) // 2)
    out = np.zeros((b.count, b.h, b.w), dtype=np.uint8)
    dst = out
    if dev_out:
        import torch
        dst = torch.zeros((b.count, b.h, b.w), dtype=torch.uint8, device="cuda")
    with pytest.raises(IEError) as ei:
        c.decode_images(b.slots, b.pitch, nbits, b.w, b.h, dst, start_bit=b.hb)
    assert ei.value.code == IE_EFORMAT
    assert "image 2" in str(ei.value)
    got = dst.cpu().numpy() if dev_out else dst
    for k in (0, 1, 3):
        assert np.array_equal(got[k], b.ref[k]), k
    # the raw call: the end bits of a failed batch
    eb = np.zeros(b.count, dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    ptr = dst.data_ptr() if dev_out else dst.ctypes.data
    r = c.L.ie_decode_images(c.h, b.slots.ctypes.data, b.pitch, nbits.ctypes.data_as(u64p), b.count, b.hb, b.w, b.h, 1,
                             ptr, b.w, b.w * b.h, eb.ctypes.data_as(u64p))
    assert r == IE_EFORMAT
    assert int(eb[2]) == U64MAX
    assert [int(eb[k]) for k in (0, 1, 3)] == [int(b.ends[k]) for k in (0, 1, 3)]
    # the context stays usable
    _, ends = _decode(b)
    assert np.array_equal(ends, b.ends)


# ------------------------------------------------------------------ 7. sub-batches
def test_sub_batches(monkeypatch):
    """Seven images with IE_DEC_BATCH_MAX=2 (sub-batches of 2, 2, 2 and 1 sharing the scratch) ==
    the run without the variable."""
    b = _batch(4, True, kinds=("U", 77, "M", "U", 200, "M", "U"))
    monkeypatch.delenv("IE_DEC_BATCH_MAX", raising=False)
    ref, ends = _decode(b)
    monkeypatch.setenv("IE_DEC_BATCH_MAX", "2")
    out, ends2 = _decode(b)
    assert np.array_equal(ends, b.ends) and np.array_equal(ends2, b.ends)
    assert np.array_equal(out, ref)
    for k in range(b.count):
        assert np.array_equal(out[k], b.ref[k]), k


# ------------------------------------------------------------------ 8. argument errors
def test_argument_errors():
    from imageencoder_amd import IEError
    b = _batch(4, True)
    c = _codec(4)
    out = np.zeros((b.count, b.h, b.w), dtype=np.uint8)
    bad = b.nbits.copy()
    bad[3] = np.uint64(8 * b.pitch + 1)
    with pytest.raises(IEError) as e1:  # nbits[k] > 8 * in_pitch
        c.decode_images(b.slots, b.pitch, bad, b.w, b.h, out, start_bit=b.hb)
    assert e1.value.code == IE_EINVAL
    bad = b.nbits.copy()
    bad[1] = np.uint64(b.hb - 1)
    with pytest.raises(IEError) as e2:  # start_bit > nbits[k]
        c.decode_images(b.slots, b.pitch, bad, b.w, b.h, out, start_bit=b.hb)
    assert e2.value.code == IE_EINVAL
    with pytest.raises(IEError) as e3:  # count = 0
        c.decode_images(b.slots, b.pitch, np.zeros(0, np.uint64), b.w, b.h, out, start_bit=b.hb)
    assert e3.value.code == IE_EINVAL
    assert not out.any()
