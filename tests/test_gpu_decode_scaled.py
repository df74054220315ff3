"""ie_decode_scaled / ie_decode_images_scaled (Codec.decode_scaled, Codec.decode_images_scaled): every
frame or image at 1/2, 1/4 or 1/8 of its size out of the decode pass.  In every case "expected" is
the numpy box mean (tests/scaled_common.py: the mean of the integer pixels, rounded half up) of the
existing full decode's output on the same context (ie_decode_frames / ie_decode_images), and that
full output is itself compared with the oracle's decoded pixels once per stream.  Equality is byte
for byte: pixels, end bits, and every byte of a destination outside the rows.

Streams: the oracle's encode of imageencoder_amd.synth frames (noise "U", mixed "M") and constant
frames -- tests/test_capi_scaled.py checks on the CPU that the noise streams hold exact rounding
ties -- and the valid-but-unwritten streams of tests/crafted_streams.py.
"""
import ctypes as C

import numpy as np
import pytest

from imageencoder_amd import IE_EFORMAT, IE_EINVAL, IE_OK
from tests import crafted_streams as CS
from tests import oracle_lib as O
from tests import scaled_common as SC
from tests.test_gpu_decode_region import CRAFTED

pytestmark = pytest.mark.gpu

U64MAX = (1 << 64) - 1
FILL = 0xA5
_CODECS = {}
_STREAMS = {}
u64p = C.POINTER(C.c_uint64)


def _q(n):
    return O.read_matrix("matrix.txt" if n == 4 else "matrix8_1.txt", n)


def _codec(n):
    """One context per block size for the whole module."""
    if n not in _CODECS:
        from imageencoder_amd import Codec
        _CODECS[n] = Codec(0, _q(n), n)
    return _CODECS[n]


class Stream:
    """`nframes` frames of records from `start_bit` (the oracle's encode), and the full decode on the
    module's context -- compared with the oracle's decoded pixels once, here, then read-only: the
    reference every scaled picture is the box mean of."""

    def __init__(self, n, rle, w, h, kind, nframes, start_bit):
        o, q = O.load(), _q(n)
        self.n, self.rle, self.w, self.h, self.nframes, self.start_bit = n, rle, w, h, nframes, start_bit
        y = SC.frames(kind, w, h, nframes, SC.stream_seed(w, nframes))
        buf, end, _ = o.encode_blocks(y, n, q, rle=rle, start_bit=start_bit)
        self.buf = buf[: (end + 7) // 8 + 3].copy()
        self.end = end
        oracle = np.stack([np.asarray(o.decode_image(o.encode_image(f, n, q, rle=rle), n)).reshape(h, w) for f in y])
        full = np.zeros((nframes, h, w), dtype=np.uint8)
        got_end = _codec(n).decode_frames(self.buf, w, h, full, start_bit=start_bit, nframes=nframes, rle=rle)
        assert got_end == end
        assert np.array_equal(full, oracle)
        full.setflags(write=False)
        self.full = full


def _stream(n, rle, w, h, kind="M", nframes=1, start_bit=0):
    key = (n, rle, w, h, kind, nframes, start_bit)
    if key not in _STREAMS:
        _STREAMS[key] = Stream(*key)
    return _STREAMS[key]


# 4x4 64x32: 128 blocks, a decode wave or two.  4x4 320x240: 4 800 blocks, several count workgroups,
# many decode workgroups, rows of 80 blocks (a wave's lanes straddle block rows).  4x4 200x56: 50
# blocks per row, ow = 50 at s = 4 (no multiple of 4: the one-byte rows of a block row start at every
# alignment).  4x4 52x20: ow = 26 at s = 2 and 13 at s = 4 -- every other row starts at an odd
# address, so the halfword store of s = 2 takes its byte fall-back.  8x8 512x256: 2 048 blocks, more
# than one count workgroup.  8x8 64x64: the small case.
SHAPES = [(4, 64, 32), (4, 320, 240), (4, 200, 56), (4, 52, 20), (8, 512, 256), (8, 64, 64)]
KINDS = ["U", "M", 0, 128, 255]


# ------------------------------------------------------------------ 1. every scale, shape and content
@pytest.mark.parametrize("kind", KINDS, ids=[str(k) for k in KINDS])
@pytest.mark.parametrize("shape", SHAPES, ids=["n{}_{}x{}".format(*s) for s in SHAPES])
def test_every_scale(shape, kind):
    """Noise, mixed content and the constant frames 0, 128 and 255 (the clamps; exact sums)."""
    n, w, h = shape
    s = _stream(n, True, w, h, kind)
    if isinstance(kind, int):
        assert (s.full == kind).all()
    for sc in SC.scales(n):
        out, end = _codec(n).decode_scaled(s.buf, w, h, sc, rle=True)
        assert out.shape == (1, h // sc, w // sc)
        assert np.array_equal(out, SC.box(s.full, sc)), sc
        assert end == s.end


@pytest.mark.parametrize("shape", SHAPES, ids=["n{}_{}x{}".format(*s) for s in SHAPES])
def test_unaligned_device_rows(shape):
    """A device destination that starts at an odd address with an odd stride: word and halfword
    stores take their byte fall-back on some rows and not on others; nothing outside the rows is
    written."""
    import torch
    n, w, h = shape
    s = _stream(n, True, w, h, "U")
    for sc in SC.scales(n):
        ow, oh = w // sc, h // sc
        stride = ow + 3 if (ow + 3) % 2 else ow + 4
        buf = torch.full((1 + stride * oh + 8,), FILL, dtype=torch.uint8, device="cuda:0")
        _, end = _codec(n).decode_scaled(s.buf, w, h, sc, out=buf[1:], stride=stride, frame_pitch=stride * oh)
        exp = np.full(buf.numel(), FILL, dtype=np.uint8)
        box = SC.box(s.full, sc)[0]
        for r in range(oh):
            exp[1 + r * stride: 1 + r * stride + ow] = box[r]
        assert np.array_equal(buf.cpu().numpy(), exp), sc
        assert end == s.end


# ------------------------------------------------------------------ 2. the axes, on the two large shapes
AXES = [(True, 0, 1), (False, 37, 3), (True, 37, 3), (False, 0, 1)]


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("dest", ["host", "device"])
@pytest.mark.parametrize("rle,start_bit,nframes", AXES, ids=["rle_sb0_f1", "norle_sb37_f3", "rle_sb37_f3", "norle_sb0_f1"])
@pytest.mark.parametrize("shape", [(4, 320, 240), (8, 512, 256)], ids=["n4_320x240", "n8_512x256"])
def test_axes(shape, rle, start_bit, nframes, dest, padded):
    """use_rle on and off, start_bit 0 and 37, one and three frames, host and device destinations,
    packed and padded (stride = ow + 5, frame_pitch padded, 0xA5 outside the rows), every scale."""
    import torch
    n, w, h = shape
    s = _stream(n, rle, w, h, "U", nframes, start_bit)
    for sc in SC.scales(n):
        ow, oh = w // sc, h // sc
        stride = ow + 5 if padded else ow
        pitch = stride * oh + (11 if padded else 0)
        if dest == "host":
            buf = np.full(nframes * pitch, FILL, dtype=np.uint8)
        else:
            buf = torch.full((nframes * pitch,), FILL, dtype=torch.uint8, device="cuda:0")
        _, end = _codec(n).decode_scaled(s.buf, w, h, sc, out=buf, start_bit=start_bit, nframes=nframes, rle=rle,
                                         stride=stride, frame_pitch=pitch)
        got = buf if dest == "host" else buf.cpu().numpy()
        assert end == s.end
        box = SC.box(s.full, sc)
        exp = np.full(nframes * pitch, FILL, dtype=np.uint8)
        for f in range(nframes):
            for r in range(oh):
                exp[f * pitch + r * stride: f * pitch + r * stride + ow] = box[f, r]
        assert np.array_equal(got, exp), sc  # the pixels, and 0xA5 everywhere else


@pytest.mark.parametrize("n", [4, 8])
def test_scale_one_equals_decode_frames(n):
    n, w, h = (4, 320, 240) if n == 4 else (8, 512, 256)
    s = _stream(n, False, w, h, "U", 3, 37)
    out, end = _codec(n).decode_scaled(s.buf, w, h, 1, start_bit=37, nframes=3, rle=False)
    assert np.array_equal(out, s.full) and end == s.end


def test_device_stream_read_in_place():
    """A 16-byte aligned device stream is read in place, an unaligned one is staged: same picture."""
    import torch
    n, w, h = 4, 320, 240
    s = _stream(n, True, w, h, "U")
    dev = torch.zeros(s.buf.size + 32, dtype=torch.uint8, device="cuda:0")
    for off in (0, 5):
        dev[off: off + s.buf.size] = torch.from_numpy(s.buf).to("cuda:0")
        for sc in (2, 4):
            out, end = _codec(n).decode_scaled(dev[off: off + s.buf.size], w, h, sc)
            assert np.array_equal(out, SC.box(s.full, sc)) and end == s.end


# ------------------------------------------------------------------ 3. crafted streams
@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_streams(name):
    """Valid streams no encoder here writes: widths wider than needed, trailing zeros, width-0
    records; the two "big" entries put several hundred records into a chunk, so their waves take the
    walk-again branch of the scaled pass on a single stream."""
    e = CS.by_name(name)
    assert e.mat == "ref"
    c = _codec(e.n)
    data = np.frombuffer(e.data, np.uint8).copy()
    hb = e.file()[1][0]
    full = np.zeros((e.h, e.w), dtype=np.uint8)
    end = c.decode_frames(data, e.w, e.h, full, start_bit=hb, rle=e.rle)
    assert np.array_equal(full, np.asarray(O.load().decode_image(e.data, e.n)).reshape(e.h, e.w))
    if e.family == "big":
        assert e.chunk_record_counts()[1].max() > 256
    for sc in SC.scales(e.n):
        out, send = c.decode_scaled(data, e.w, e.h, sc, start_bit=hb, rle=e.rle)
        assert np.array_equal(out[0], SC.box(full, sc)), sc
        assert send == end


# ------------------------------------------------------------------ 4. batches
class Batch:
    """Image files of the oracle's encoder in slots; the full batch decode on the module's context,
    compared with the oracle's decode of every file once."""

    def __init__(self, n, rle, w, h, kinds):
        o, q = O.load(), _q(n)
        self.n, self.rle, self.w, self.h, self.count = n, rle, w, h, len(kinds)
        ys = [SC.frames(k, w, h, 1, seed=31 + i)[0] for i, k in enumerate(kinds)]
        self.files = [o.encode_image(y, n, q, rle=rle) for y in ys]
        self.hb = o.header(n, q, int(rle), w, h)[1]
        self.pitch = (max(len(f) for f in self.files) + 8 + 15) // 16 * 16
        self.slots = np.zeros(self.count * self.pitch, dtype=np.uint8)
        for k, f in enumerate(self.files):
            self.slots[k * self.pitch: k * self.pitch + len(f)] = np.frombuffer(f, np.uint8)
        self.nbits = np.array([8 * len(f) for f in self.files], dtype=np.uint64)
        full = np.zeros((self.count, h, w), dtype=np.uint8)
        self.ends = _codec(n).decode_images(self.slots, self.pitch, self.nbits, w, h, full, start_bit=self.hb, rle=rle).copy()
        for k, f in enumerate(self.files):
            assert np.array_equal(full[k], np.asarray(o.decode_image(f, n)).reshape(h, w)), k
        full.setflags(write=False)
        self.full = full


def test_walk_again_in_a_batch():
    """Two 320x240 4x4 images, RLE on: noise and constant 128.  One chunk plan serves the batch,
    sized from the noise stream, so the constant image's few-bit records number more than
    kRecPosCap = 256 per chunk and its waves walk the chunks again."""
    n, w, h = 4, 320, 240
    b = Batch(n, True, w, h, ["U", 128])
    c = _codec(n)
    nblocks = (w // n) * (h // n)
    for sc in SC.scales(n):
        out, ends = c.decode_images_scaled(b.slots, b.pitch, b.nbits, w, h, sc, start_bit=b.hb, rle=True)
        assert np.array_equal(out, SC.box(b.full, sc)), sc
        assert np.array_equal(ends, b.ends)
    chunks = c.last_decode_info()[0]
    span = int(b.nbits.max()) - b.hb
    cbits = -(-span // chunks)  # the planned chunk is at least this long
    rec_bits = (int(b.ends[1]) - b.hb) // nblocks
    assert (int(b.ends[1]) - b.hb) == rec_bits * nblocks  # every record of the constant image the same length
    assert min(nblocks, cbits // rec_bits) > 256, (chunks, cbits, rec_bits)


def _raw_batch(c, b, nbits, sc, out):
    ends = np.zeros(b.count, dtype=np.uint64)
    ow, oh = b.w // sc, b.h // sc
    r = c.L.ie_decode_images_scaled(c.h, b.slots.ctypes.data, b.pitch, nbits.ctypes.data_as(u64p), b.count, b.hb, b.w,
                                    b.h, int(b.rle), sc, out.ctypes.data, ow, ow * oh, ends.ctypes.data_as(u64p))
    return r, ends, c.L.ie_last_error(c.h).decode()


@pytest.mark.parametrize("n", [4, 8])
def test_batch_with_a_truncated_image(n, monkeypatch):
    """Five 64x32 images of different contents and lengths, image 2 cut mid-stream: IE_EFORMAT names
    it, end_bits[2] = UINT64_MAX, the other four pictures and end bits are the full batch decode's
    -- and the same again in sub-batches of two (IE_DEC_BATCH_MAX, read on every call)."""
    w, h = 64, 32
    b = Batch(n, True, w, h, ["U", "M", "U", 90, "M"])
    c = _codec(n)
    nbits = b.nbits.copy()
    nbits[2] = (b.hb + int(b.nbits[2])) // 2
    keep = [0, 1, 3, 4]
    for sc in SC.scales(n):
        exp = SC.box(b.full, sc)
        results = []
        for batch_max in (None, "2"):
            if batch_max:
                monkeypatch.setenv("IE_DEC_BATCH_MAX", batch_max)
            out = np.full((b.count, h // sc, w // sc), FILL, dtype=np.uint8)
            r, ends, msg = _raw_batch(c, b, nbits, sc, out)
            monkeypatch.delenv("IE_DEC_BATCH_MAX", raising=False)
            assert r == IE_EFORMAT and "image 2" in msg
            assert int(ends[2]) == U64MAX
            assert np.array_equal(out[keep], exp[keep]), sc
            assert np.array_equal(ends[keep], b.ends[keep])
            results.append(ends)
        assert np.array_equal(results[0], results[1])
    # the full batch call reports the same image the same way
    full = np.zeros((b.count, h, w), dtype=np.uint8)
    fe = np.zeros(b.count, dtype=np.uint64)
    r = c.L.ie_decode_images(c.h, b.slots.ctypes.data, b.pitch, nbits.ctypes.data_as(u64p), b.count, b.hb, w, h, 1,
                             full.ctypes.data, w, w * h, fe.ctypes.data_as(u64p))
    assert r == IE_EFORMAT and c.L.ie_last_error(c.h).decode() == msg
    assert np.array_equal(fe, results[0])


# ------------------------------------------------------------------ 5. errors
def _raw(c, s, sc, out, stride, pitch, length=None, nframes=None, w=None, h=None):
    end = C.c_uint64(0)
    nf = s.nframes if nframes is None else nframes
    r = c.L.ie_decode_scaled(c.h, s.buf.ctypes.data, s.buf.size if length is None else length, s.start_bit,
                             s.w if w is None else w, s.h if h is None else h, nf, int(s.rle), sc, out.ctypes.data, stride,
                             pitch, C.byref(end))
    return r, int(end.value), c.L.ie_last_error(c.h).decode()


BAD_SCALES = [(n, s) for n in (4, 8) for s in (0, -1, 3, 16)] + [(4, 8)]  # (8 is legal for 8x8 blocks)


@pytest.mark.parametrize("n,bad", BAD_SCALES, ids=["n{}_s{}".format(*b) for b in BAD_SCALES])
def test_bad_scales(n, bad):
    s = _stream(n, True, 64, 32)
    out = np.full(4096, FILL, dtype=np.uint8)
    r, _, msg = _raw(_codec(n), s, bad, out, 64, 2048)
    assert r == IE_EINVAL and "scale" in msg
    assert (out == FILL).all()


def test_bad_stride_and_pitch():
    n, w, h, sc = 4, 320, 240, 4
    s = _stream(n, True, w, h, "U", 3, 37)
    c = _codec(n)
    ow, oh = w // sc, h // sc
    out = np.full(3 * (ow + 4) * oh, FILL, dtype=np.uint8)
    r, _, msg = _raw(c, s, sc, out, ow - 1, (ow + 4) * oh)
    assert r == IE_EINVAL and "stride" in msg
    stride = ow + 4
    least = (oh - 1) * stride + ow
    r, _, msg = _raw(c, s, sc, out, stride, least - 1)
    assert r == IE_EINVAL and "frame_pitch" in msg
    assert (out == FILL).all()
    r, end, _ = _raw(c, s, sc, out, stride, least)  # the smallest legal pitch
    assert r == IE_OK and end == s.end
    exp = np.full(out.size, FILL, dtype=np.uint8)
    box = SC.box(s.full, sc)
    for f in range(3):
        for row in range(oh):
            exp[f * least + row * stride: f * least + row * stride + ow] = box[f, row]
    assert np.array_equal(out, exp)
    # the dimension checks come before the scale's: a bad frame size names the size
    bad = np.full(64, FILL, dtype=np.uint8)
    r, _, msg = _raw(c, s, 3, bad, 4, 16, nframes=1, w=322)
    assert r == IE_EINVAL and "block size" in msg and "scale" not in msg
    assert (bad == FILL).all()


@pytest.mark.parametrize("n", [4, 8])
def test_truncated_stream(n):
    """The stream is cut in its second half: IE_EFORMAT with the full decode's message, and a host
    destination receives nothing."""
    n, w, h = (4, 320, 240) if n == 4 else (8, 512, 256)
    s = _stream(n, True, w, h)
    c = _codec(n)
    cut = (s.end * 3 // 4) // 8
    full = np.zeros((h, w), dtype=np.uint8)
    end = C.c_uint64(0)
    rf = c.L.ie_decode_frames(c.h, s.buf.ctypes.data, cut, 0, w, h, 1, 1, full.ctypes.data, w, w * h, C.byref(end))
    msg_full = c.L.ie_last_error(c.h).decode()
    assert rf == IE_EFORMAT
    for sc in SC.scales(n):
        ow, oh = w // sc, h // sc
        out = np.full(ow * oh, FILL, dtype=np.uint8)
        r, _, msg = _raw(c, s, sc, out, ow, ow * oh, length=cut)
        assert r == IE_EFORMAT and msg == msg_full
        assert (out == FILL).all()


# ------------------------------------------------------------------ 6. state
@pytest.mark.parametrize("n", [4, 8])
def test_state_after_a_scaled_decode(n):
    n, w, h = (4, 320, 240) if n == 4 else (8, 512, 256)
    s = _stream(n, True, w, h)
    c = _codec(n)
    before = np.zeros((h, w), dtype=np.uint8)
    c.decode_frames(s.buf, w, h, before, rle=True)
    info = c.last_decode_info()
    try:
        c.set_exact_parse(False)
        out, end = c.decode_scaled(s.buf, w, h, 2)
        assert not c.last_decode_spec()
        assert c.last_decode_info() == info  # reported as for the full call
    finally:
        c.set_exact_parse(True)
    assert np.array_equal(out, SC.box(s.full, 2)) and end == s.end
    after = np.zeros((h, w), dtype=np.uint8)
    assert c.decode_frames(s.buf, w, h, after, rle=True) == s.end
    assert np.array_equal(before, after) and np.array_equal(after, s.full[0])
