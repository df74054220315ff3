"""GPU parity of the streamed video decode (ie_vdec_open / next / info / close): for any chunk_frames
and any partition of the video into next calls, the frames handed out in order equal the CPU
oracle's decode (O.load().decode_video_gop of the file O.load().encode_video_gop writes), byte for
byte, and the end bit equals the oracle's encode_gop end -- ie_decode_gop is a second check only.

The payloads are the oracle's (encode_gop from start_bit, a bit pattern in front of it); the frames
come from synth.frames with a fixed seed.  The shapes are the smallest at which each path can go
wrong: one macroblock with a ragged last group, next calls that cross chunk boundaries and chunks
that cross group boundaries, both slots reused three times, the gop = 1 chunk as one parse of
several frames from a device start word, frames of a few bits (chunk boundaries inside one stream
word), a chunk whose first P-frame reads its reference from the other slot, the settings, padded
destinations in pageable, page-locked and device memory, host and device streams, other calls on
the context between two next calls, info(), truncated streams, the argument checks and the
reference's P-frame goldens.
"""
import functools

import numpy as np
import pytest

from imageencoder_amd import IE_EFORMAT, IE_EINVAL, IE_ENOQUANT, IEError, synth
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 23
FILL = 0xA7
U64_MAX = 2 ** 64 - 1


@pytest.fixture(scope="module")
def codec():
    from imageencoder_amd import Codec
    c = Codec(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _matrix(name, n=4):
    if name == "ref":
        return O.read_matrix("matrix.txt" if n == 4 else "matrix8_1.txt", n)
    return O.read_matrix({"second": "matrix4_2.txt" if n == 4 else "matrix8_2.txt"}[name], n)


def _lead(start):
    """The caller's bits before start_bit (a fixed pattern)."""
    return (np.arange(start) * 7 % 3 == 0).astype(np.uint8)


class Case:
    """One video: the oracle's payload behind `start` pattern bits, its end bit and frame bits, and
    the oracle's decoded frames (computed once, never modified)."""

    def __init__(self, kind, w, h, f, n=4, mat="ref", gop=1, merange=0, rle=True, start=0):
        self.w, self.h, self.f, self.n, self.mat, self.gop, self.merange, self.rle, self.start = (
            w, h, f, n, mat, gop, merange, rle, start)
        y = synth.frames(kind, w, h, f, SEED)
        q = _matrix(mat, n)
        o = O.load()
        buf, self.end, fb = o.encode_gop(y, n, q, gop, merange, rle=rle, start_bit=start)
        self.fb = [int(b) for b in fb]
        bits = np.concatenate([_lead(start), np.unpackbits(buf)[start:self.end]])
        self.stream = np.packbits(bits)
        self.stream.setflags(write=False)
        self.file = o.encode_video_gop(synth.yuv420(y), w, h, n, q, rle=rle, gop=gop, merange=merange)
        self._frames = {}

    def frames(self, mc=True):
        if mc not in self._frames:
            dec = np.frombuffer(O.load().decode_video_gop(self.file, self.n, mc), dtype=np.uint8)
            pitch = self.w * self.h * 3 // 2
            assert dec.size == self.f * pitch
            assert (dec.reshape(self.f, pitch)[:, self.w * self.h:] == 0x80).all()
            y = dec.reshape(self.f, pitch)[:, : self.w * self.h].reshape(self.f, self.h, self.w).copy()
            y.setflags(write=False)
            self._frames[mc] = y
        return self._frames[mc]


@functools.lru_cache(maxsize=None)
def _case(*a, **kw):
    return Case(*a, **kw)


def _buffer(codec, nbytes, where):
    if where == "device":
        import torch
        return torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    out = codec.host_array(nbytes) if where == "pinned" else np.empty(nbytes, dtype=np.uint8)
    out[:] = FILL
    return out


def _host(buf):
    return buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()


def _stream_in(codec, c, where, length=None):
    s = np.array(c.stream[:length])
    if where == "host":
        return s
    import torch
    if where == "device":  # (torch allocations are at least 256-byte aligned: read in place)
        return torch.from_numpy(s).cuda()
    return torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), s])).cuda()[1:]  # unaligned: copied


def _run(codec, c, chunk_frames, sizes, mc=True, where="pageable", stride=None, frame_pitch=None, src="host",
         length=None, between=None, after_open=None):
    """Decode case c streamed; next sizes repeat.  Returns (frames (f, h, w), the whole destination,
    the infos after open and after every call, the frames every call returned)."""
    stride = c.w if stride is None else stride
    pitch = stride * c.h if frame_pitch is None else frame_pitch
    codec.set_quant(_matrix(c.mat, c.n), c.n)
    out = _buffer(codec, c.f * pitch, where)
    sin = _stream_in(codec, c, src, length)
    vd = codec.open_video_decode(sin, c.w, c.h, c.f, gop=c.gop, merange=c.merange, start_bit=c.start, rle=c.rle,
                                 motioncomp=mc, chunk_frames=chunk_frames)
    infos, gots = [vd.info()], []
    try:
        if after_open is not None:
            after_open(sin)
        done, i = 0, 0
        while True:
            # (after the last frame the call still gets a buffer: an empty device slice has no address)
            got = vd.next(out[min(done, c.f - 1) * pitch:], sizes[i % len(sizes)], stride=stride, frame_pitch=pitch)
            infos.append(vd.info())
            gots.append(got)
            if got == 0:
                break
            done += got
            i += 1
            if between is not None and i == 1:
                between()
        assert done == c.f
        assert vd.next(out, 1, stride=stride, frame_pitch=pitch) == 0  # after the last frame: nothing, no error
    finally:
        vd.close()
    whole = _host(out)
    rows = np.stack([whole[k * pitch: k * pitch + (c.h - 1) * stride + c.w] for k in range(c.f)])
    frames = np.stack([np.stack([r[j * stride: j * stride + c.w] for j in range(c.h)]) for r in rows])
    return frames, whole, infos, gots


def _check(codec, c, chunk_frames, sizes, mc=True, **kw):
    frames, whole, infos, gots = _run(codec, c, chunk_frames, sizes, mc=mc, **kw)
    assert np.array_equal(frames, c.frames(mc))
    for inf in infos:
        assert inf["chunks_enqueued"] <= inf["chunks_delivered"] + 2, infos
    nchunks = -(-c.f // infos[0]["chunk_frames"])
    assert infos[0]["chunks_enqueued"] == min(2, nchunks) and infos[0]["chunks_delivered"] == 0
    assert infos[-1]["chunks_enqueued"] == infos[-1]["chunks_delivered"] == nchunks
    done = 0
    for got, inf in zip(gots, infos[1:]):  # UINT64_MAX until the last frame is out, then the oracle's
        done += got
        assert inf["end_bit"] == (c.end if done == c.f else U64_MAX), (done, inf)
    return frames, whole, infos


# ------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("size", [1, 2, 5, 100])
@pytest.mark.parametrize("chunk", [1, 2, 3, 4, 7, 9])
def test_ragged_last_group(codec, chunk, size):
    """16x16 (one macroblock), gop 3, 7 frames: groups of 3, 3 and 1; every chunk size against every
    next size, so calls cross chunk boundaries and chunks cross group boundaries (chunk 1: both slots
    are reused three times; 9: one chunk larger than the video)."""
    c = _case("P", 16, 16, 7, gop=3, merange=4, start=13)
    _, _, infos = _check(codec, c, chunk, [size])
    assert infos[0]["chunk_frames"] == chunk


def test_second_check_decode_gop(codec):
    """ie_decode_gop on the same payload gives the same frames and end bit."""
    c = _case("P", 16, 16, 7, gop=3, merange=4, start=13)
    frames, _, _ = _check(codec, c, 2, [3])
    out = np.full(c.f * c.w * c.h, FILL, dtype=np.uint8)
    end = codec.decode_gop(np.array(c.stream), c.w, c.h, out, c.gop, c.merange, c.f, start_bit=c.start)
    assert end == c.end and np.array_equal(out.reshape(frames.shape), frames)


@pytest.mark.parametrize("size", [2, 100])
def test_gop1_chunk_is_one_parse_of_several_frames(codec, size):
    """32x16, gop 1, 7 frames in chunks of 3 (3, 3, 1): each chunk one parse of its frames from the
    device word the chunk before it wrote."""
    _check(codec, _case("P", 32, 16, 7, gop=1, start=5), 3, [size])
    _check(codec, _case("U", 32, 16, 7, gop=1, start=0), 3, [size])


@pytest.mark.parametrize("start", [0, 5])
def test_gop1_frames_of_a_few_bits(codec, start):
    """Flat frames of two blocks: a frame is a few bits, so the chunk boundaries fall inside one
    stream word."""
    c = _case("flat128", 8, 4, 40, gop=1, start=start)
    assert max(c.fb) < 32
    _check(codec, c, 3, [4, 1, 7])


def test_default_chunk_frames(codec, monkeypatch):
    """chunk_frames 0: max(1, target / (w*h)) with IE_CHUNK_MB's target (default 8 MiB)."""
    c = _case("P", 32, 16, 7, gop=1, start=5)
    monkeypatch.delenv("IE_CHUNK_MB", raising=False)
    assert _check(codec, c, 0, [2])[2][0]["chunk_frames"] == (8 << 20) // (32 * 16)
    monkeypatch.setenv("IE_CHUNK_MB", str(2 * 32 * 16 / 1048576.0))
    assert _check(codec, c, 0, [3])[2][0]["chunk_frames"] == 2
    monkeypatch.setenv("IE_CHUNK_MB", "0.0000001")
    assert _check(codec, c, 0, [3])[2][0]["chunk_frames"] == 1


@pytest.mark.parametrize("mc", [True, False], ids=["motioncomp", "no-motioncomp"])
def test_reference_in_the_other_slot(codec, mc):
    """48x32, gop 4, merange 8, 9 frames in chunks of 3: several macroblocks with moving vectors;
    frame 3 (a P-frame) opens chunk 1 and reads frame 2 in the other slot; frame 6 likewise."""
    c = _case("P", 48, 32, 9, gop=4, merange=8, start=7)
    _check(codec, c, 3, [2], mc=mc)
    _check(codec, c, 1, [4], mc=mc)


# ------------------------------------------------------------------------------- settings
def test_rle_off(codec):
    _check(codec, _case("P", 48, 32, 5, gop=3, merange=8, rle=False, start=13), 2, [3])
    _check(codec, _case("P", 32, 16, 5, gop=1, rle=False, start=13), 2, [3])


def test_8x8_blocks(codec):
    """8x8 blocks, every frame an I-frame.  (An 8x8 video with P-frames has no decode to compare
    with: its P-frames carry vectors only, while the reference's decoder -- and the oracle, which
    rejects such a file -- reads a record for every microblock.)"""
    try:
        _check(codec, _case("P", 64, 48, 5, n=8, gop=1, start=7), 2, [3])
        _check(codec, _case("U", 24, 16, 5, n=8, gop=1, start=0), 1, [2])
    finally:
        codec.set_quant(_matrix("ref"), 4)


def test_second_matrices(codec):
    try:
        _check(codec, _case("M", 48, 32, 5, mat="second", gop=3, merange=8, start=5), 2, [3])
        _check(codec, _case("M", 64, 48, 4, n=8, mat="second", gop=1, start=5), 3, [3])
    finally:
        codec.set_quant(_matrix("ref"), 4)


@pytest.mark.parametrize("start", [5, 210])
def test_start_bit_with_a_pattern_in_front(codec, start):
    _check(codec, _case("P", 48, 32, 7, gop=3, merange=8, start=start), 2, [3])
    _check(codec, _case("P", 32, 16, 7, gop=1, start=start), 3, [2])


# ------------------------------------------------------------------------------- destinations
@pytest.mark.parametrize("where", ["pageable", "pinned", "device"])
@pytest.mark.parametrize("gop", [1, 3])
def test_padded_destinations(codec, where, gop):
    """Rows stride = w + 16 apart in frames 1.5 stride h apart: only the w bytes of a row are
    written, the padding and the chroma space keep the caller's bytes."""
    c = _case("P", 48, 32, 7, gop=gop, merange=8 if gop > 1 else 0, start=13)
    stride, pitch = c.w + 16, (c.w + 16) * c.h * 3 // 2
    _, whole, _ = _check(codec, c, 3, [2, 4], where=where, stride=stride, frame_pitch=pitch)
    mask = np.ones(whole.size, dtype=bool)
    for k in range(c.f):
        for r in range(c.h):
            mask[k * pitch + r * stride: k * pitch + r * stride + c.w] = False
    assert (whole[mask] == FILL).all()


@pytest.mark.parametrize("where", ["pageable", "pinned", "device"])
def test_tight_destinations(codec, where):
    _check(codec, _case("P", 48, 32, 7, gop=3, merange=8, start=13), 2, [3], where=where)


# ------------------------------------------------------------------------------- inputs
@pytest.mark.parametrize("gop", [1, 3])
def test_host_stream_overwritten_after_open(codec, gop):
    c = _case("P", 48, 32, 7, gop=gop, merange=8 if gop > 1 else 0, start=13)

    def scribble(sin):
        sin[:] = 0xFF

    _check(codec, c, 2, [3], after_open=scribble)


@pytest.mark.parametrize("src", ["device", "device-unaligned"])
def test_device_stream(codec, src):
    _check(codec, _case("P", 48, 32, 7, gop=3, merange=8, start=13), 2, [3], src=src)
    _check(codec, _case("P", 32, 16, 7, gop=1, start=5), 3, [2], src=src, where="device")


# ------------------------------------------------------------------------------- other calls
@pytest.mark.parametrize("gop", [1, 3])
def test_other_calls_between_two_next_calls(codec, gop):
    """Between two next calls: set_quant with another matrix and a decode_frames of an unrelated,
    larger image (it regrows the context's parse scratch).  That decode is itself correct and the
    remaining frames of the stream are unchanged."""
    c = _case("P", 48, 32, 9, gop=gop, merange=8 if gop > 1 else 0, start=13)
    w2, h2 = 96, 64
    y2 = synth.frames("M", w2, h2, 1, SEED + 1)[0]
    file2 = O.load().encode_image(y2, 4, _matrix("second"))
    want2 = O.load().decode_image(file2, 4)

    def between():  # (decode_image_file: ie_set_quant with the file's matrix, then ie_decode_frames)
        assert np.array_equal(codec.decode_image_file(file2, 4), want2)

    try:
        _check(codec, c, 2, [1, 3], between=between)
    finally:
        codec.set_quant(_matrix("ref"), 4)


# ------------------------------------------------------------------------------- info
def test_info(codec):
    c = _case("P", 16, 16, 7, gop=3, merange=4, start=13)
    _, _, infos = _check(codec, c, 1, [1])
    assert infos[0] == dict(chunk_frames=1, chunks_enqueued=2, chunks_delivered=0, end_bit=U64_MAX)
    for k, inf in enumerate(infos[1: c.f + 1]):  # after frame k: chunk k out, k + 2 in
        assert inf["chunks_delivered"] == k + 1 and inf["chunks_enqueued"] == min(k + 3, c.f)
    assert infos[c.f]["end_bit"] == c.end and infos[c.f - 1]["end_bit"] == U64_MAX


def test_one_open_decoder_per_context(codec):
    c = _case("P", 16, 16, 7, gop=3, merange=4, start=13)
    codec.set_quant(_matrix("ref"), 4)
    s = np.array(c.stream)
    vd = codec.open_video_decode(s, c.w, c.h, c.f, gop=c.gop, merange=c.merange, start_bit=c.start, chunk_frames=2)
    try:
        with pytest.raises(IEError) as e:
            codec.open_video_decode(s, c.w, c.h, c.f, gop=c.gop, merange=c.merange, start_bit=c.start)
        assert e.value.code == IE_EINVAL
    finally:
        vd.close()
    codec.open_video_decode(s, c.w, c.h, c.f, gop=c.gop, merange=c.merange, start_bit=c.start).close()


# ------------------------------------------------------------------------------- truncation
def _cut_bytes(c, frame, where):
    """Bytes to keep so that the stream ends inside `frame` (a P-frame): in its records, or in its
    vectors -- from the oracle's frame bits; the stream is only shortened."""
    mvb = (c.w // 16) * (c.h // 16) * 2 * O.load().bits_needed(c.merange)
    fs = c.start + sum(c.fb[:frame])
    if where == "records":
        nbytes = (fs + mvb + (c.fb[frame] - mvb) // 2) // 8
        assert fs + mvb < 8 * nbytes < fs + c.fb[frame]
    else:
        nbytes = (fs + mvb - 1) // 8
        assert fs <= 8 * nbytes < fs + mvb
    return nbytes


@pytest.mark.parametrize("chunk", [1, 2, 3, 7])
@pytest.mark.parametrize("where,msg", [("records", "stream ends before the last block"),
                                      ("vectors", "stream ends in the motion vectors")])
def test_truncated_stream(codec, where, msg, chunk):
    """The 16x16 gop-3 stream cut inside frame 4: frames 0 to 3 are delivered and equal the
    oracle's, that call returns IE_EFORMAT with got = 4, and every later call IE_EFORMAT with 0."""
    c = _case("P", 16, 16, 7, gop=3, merange=4, start=13)
    nbytes = _cut_bytes(c, 4, where)
    codec.set_quant(_matrix("ref"), 4)
    fb = c.w * c.h
    for sizes in ([100], [4, 1], [3, 3]):
        out = np.full(c.f * fb, FILL, dtype=np.uint8)
        vd = codec.open_video_decode(np.array(c.stream[:nbytes]), c.w, c.h, c.f, gop=c.gop, merange=c.merange,
                                     start_bit=c.start, chunk_frames=chunk)
        try:
            done = 0
            with pytest.raises(IEError, match=msg) as e:
                for size in sizes:
                    try:
                        done += vd.next(out[done * fb:], size)
                    except IEError as err:
                        done += err.got
                        raise
            assert e.value.code == IE_EFORMAT and done == 4
            assert e.value.got == {100: 4, 1: 0, 3: 1}[sizes[-1]]
            assert np.array_equal(out[: 4 * fb].reshape(4, c.h, c.w), c.frames()[:4])
            assert (out[4 * fb:] == FILL).all()
            for _ in range(2):
                with pytest.raises(IEError, match=msg) as e:
                    vd.next(out[4 * fb:], 2)
                assert e.value.code == IE_EFORMAT and e.value.got == 0
            inf = vd.info()
            assert inf["end_bit"] == U64_MAX and inf["chunks_enqueued"] <= inf["chunks_delivered"] + 2
        finally:
            vd.close()
    _check(codec, c, chunk, [3])  # the context decodes the whole stream afterwards


@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_truncated_gop1_stream(codec, chunk):
    """gop 1, cut in the middle of frame 4: a chunk is one parse, its whole frames are the record
    total / blocks per frame."""
    c = _case("U", 32, 16, 7, gop=1, start=0)
    fs = c.start + sum(c.fb[:4])
    nbytes = (fs + c.fb[4] // 2) // 8
    assert fs < 8 * nbytes < fs + c.fb[4] - 300  # (more than one record short of the frame's end)
    codec.set_quant(_matrix("ref"), 4)
    fb = c.w * c.h
    out = np.full(c.f * fb, FILL, dtype=np.uint8)
    vd = codec.open_video_decode(np.array(c.stream[:nbytes]), c.w, c.h, c.f, start_bit=c.start, chunk_frames=chunk)
    try:
        with pytest.raises(IEError, match="stream ends before the last block") as e:
            vd.next(out, 100)
        assert e.value.code == IE_EFORMAT and e.value.got == 4
        assert np.array_equal(out[: 4 * fb].reshape(4, c.h, c.w), c.frames()[:4])
        with pytest.raises(IEError) as e:
            vd.next(out, 1)
        assert e.value.code == IE_EFORMAT and e.value.got == 0
    finally:
        vd.close()


# ------------------------------------------------------------------------------- argument checks
def test_argument_checks(codec):
    """ie_decode_gop's checks with its codes, then the decoder's own."""
    from imageencoder_amd import Codec
    c = _case("P", 48, 32, 7, gop=3, merange=8, start=13)
    s = np.array(c.stream)
    out = np.zeros(c.f * 72 * 48, dtype=np.uint8)

    def code(call):
        with pytest.raises(IEError) as e:
            call()
        return e.value.code

    fresh = Codec(0)
    try:
        assert code(lambda: fresh.open_video_decode(s, c.w, c.h, c.f)) == IE_ENOQUANT
        assert code(lambda: fresh.decode_gop(s, c.w, c.h, out, 1, 0, c.f)) == IE_ENOQUANT
    finally:
        fresh.close()
    codec.set_quant(_matrix("ref"), 4)
    bad = [
        dict(w=50, h=32), dict(w=0, h=32), dict(w=48, h=32, nframes=0),   # dimensions
        dict(w=48, h=32, merange=-1), dict(w=48, h=32, merange=32768),    # merange
        dict(w=72, h=40, gop=2, merange=8), dict(w=64, h=40, gop=2),      # P-frames: W, H multiples of 16
        dict(w=48, h=32, start_bit=8 * s.size + 1),                       # start_bit beyond the stream
    ]
    for kw in bad:
        a = dict(nframes=c.f, gop=3, merange=8, start_bit=c.start)
        a.update(kw)
        got = code(lambda: codec.open_video_decode(s, a["w"], a["h"], a["nframes"], gop=a["gop"], merange=a["merange"],
                                                   start_bit=a["start_bit"]))
        ref = code(lambda: codec.decode_gop(s, a["w"], a["h"], out, a["gop"], a["merange"], a["nframes"],
                                            start_bit=a["start_bit"]))
        assert got == ref == IE_EINVAL, (kw, got, ref)
    # a bad dimension is reported before a bad merange, as by ie_decode_gop
    with pytest.raises(IEError, match="multiples of the block size"):
        codec.open_video_decode(s, 50, 32, c.f, gop=3, merange=-1)
    assert code(lambda: codec.open_video_decode(s, c.w, c.h, c.f, gop=3, merange=8, chunk_frames=-1)) == IE_EINVAL
    _check(codec, _case("P", 40, 24, 3, gop=1), 2, [2])  # (no P-frames: any multiple of the block size)
    codec.set_quant(_matrix("ref"), 4)
    vd = codec.open_video_decode(s, c.w, c.h, c.f, gop=c.gop, merange=c.merange, start_bit=c.start, chunk_frames=2)
    try:
        small = np.zeros(c.w * c.h * 2, dtype=np.uint8)
        assert code(lambda: vd.next(small, 0)) == IE_EINVAL
        assert code(lambda: vd.next(small, -3)) == IE_EINVAL
        assert code(lambda: vd.next(small, 1, stride=c.w - 1)) == IE_EINVAL
        assert code(lambda: vd.next(small, 2, frame_pitch=c.w * c.h - 1)) == IE_EINVAL
        assert vd.next(small, 2) == 2  # the failed calls consumed nothing
        assert np.array_equal(small.reshape(2, c.h, c.w), c.frames()[:2])
    finally:
        vd.close()


# ------------------------------------------------------------------------------- reference goldens
DEC = [c for c in O.manifest_gop() if "dec1_md5" in c]


@pytest.mark.parametrize("mc", [1, 0])
@pytest.mark.parametrize("c", DEC, ids=[c["name"] for c in DEC])
def test_reference_goldens(codec, c, mc):
    """Every P-frame golden tests/test_gop.py decodes, streamed in chunks of 2 frames straight from
    the file bytes behind its header: the oracle's frames (whose md5 is the reference decoder's)."""
    import hashlib
    q = O.read_matrix(c["matrix"], 4)
    codec.set_quant(q, 4)
    try:
        w, h = c["w"], c["h"]
        pitch = w * h * 3 // 2
        f = c["dec1_size"] // pitch
        _, hb = O.load().header(4, q, c["rle"], w, h, video=True, frames=f, gop=c["gop"], merange=c["merange"])
        enc = np.frombuffer(O.case_encoded(c), dtype=np.uint8).copy()
        want = np.frombuffer(O.load().decode_video_gop(enc.tobytes(), 4, bool(mc)), dtype=np.uint8)
        out = np.full(f * pitch, 0x80, dtype=np.uint8)
        vd = codec.open_video_decode(enc, w, h, f, gop=c["gop"], merange=c["merange"], start_bit=hb, rle=bool(c["rle"]),
                                     motioncomp=bool(mc), chunk_frames=2)
        try:
            done = 0
            while done < f:
                done += vd.next(out[done * pitch:], 3, frame_pitch=pitch)
            assert (vd.info()["end_bit"] + 7) // 8 == enc.size
        finally:
            vd.close()
        assert np.array_equal(out, want)
        assert hashlib.md5(out.tobytes()).hexdigest() == c[f"dec{mc}_md5"]
    finally:
        codec.set_quant(_matrix("ref"), 4)
