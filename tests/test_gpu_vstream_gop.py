"""GPU parity of the streamed P-frame video (ie_vstream_open_gop): for any partition of the frames
into pushes the bytes (every pull, then finish's copy; also the device stream after finish), the
end bit and the per-frame bits equal the CPU oracle's (O.load().encode_gop), bit for bit, and -- as
a second check only -- what ie_encode_gop gives on the same input.

The cases are built as tests/test_gpu_gop_groups.py builds them: synth.frames with a fixed seed, a
head with a bit pattern before start_bit, nothing written past the end bit in the device stream.
The shapes are the smallest at which each path can go wrong: one macroblock with a ragged last
group, pushes that cross group and chunk boundaries, chunks of one or two groups (both input slots
reused, a harvest before a slot's third use), frames of a few bits (every chunk boundary inside a
word an earlier chunk wrote and a pull may have returned), two record tiles, an uncovered right
strip, 8x8 blocks, the settings, pinned and pageable frames, stride and frame pitch, another call
on the context between two pushes, the forwarding to the gop = 1 stream, the argument checks and
the reference's P-frame goldens.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from imageencoder_amd import IE_ECAP, IE_EINVAL, MODE_EXACT, MODE_FAST, IEError, synth
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 11


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


@functools.lru_cache(maxsize=None)
def _video(kind, w, h, f):
    y = synth.frames(kind, w, h, f, SEED)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def _expected(kind, w, h, f, n, mat, gop, merange, rle, start):
    """The oracle's payload (computed once per case, never modified)."""
    buf, end, fb = O.load().encode_gop(_video(kind, w, h, f), n, _matrix(mat, n), gop, merange, rle=rle,
                                       start_bit=start)
    buf.setflags(write=False)
    return buf, end, fb


def _lead(start):
    """Caller's bits before start_bit (a fixed pattern), as whole bytes with zero bits after them."""
    bits = (np.arange(start) * 7 % 3 == 0).astype(np.uint8)
    return bits, np.packbits(bits)


def _want(exp, eend, start):
    """The stream from bit 0 to the end bit: the caller's leading bits, then the oracle's payload."""
    bits = np.concatenate([_lead(start)[0], np.unpackbits(exp)[start:eend]])
    return np.packbits(bits)


def _device_bytes(codec, vs):
    out = np.zeros(vs.cap, dtype=np.uint8)
    codec._chk(codec.L.ie_memcpy(codec.h, C.c_void_p(out.ctypes.data), C.c_void_p(vs.device_ptr()), out.size))
    return out


def _stream(codec, y, w, h, f, gop, merange, pushes, rle=True, mode=MODE_FAST, start=0, stride=None, frame_pitch=None,
            pinned=False, between=None, open_kw=None):
    """Push the frames of the flat buffer y as `pushes` says (frames per push, repeated), pulling
    after every push.  Returns (bytes, frame bits, end bit, bytes pulled before finish, device stream)."""
    pitch = frame_pitch if frame_pitch is not None else (stride or w) * h
    y = np.ascontiguousarray(y, dtype=np.uint8).ravel()
    if pinned:
        host = codec.host_array(y.size)
        host[:] = y
        y = host
    kw = dict(gop=gop, merange=merange) if open_kw is None else open_kw
    vs = codec.open_video_stream(w, h, head=_lead(start)[1], start_bit=start, max_frames=f, stride=stride,
                                 frame_pitch=frame_pitch, rle=rle, mode=mode, **kw)
    try:
        out = np.zeros(vs.cap, dtype=np.uint8)
        got, done, i = 0, 0, 0
        while done < f:
            k = min(pushes[i % len(pushes)], f - done)
            vs.push(y[done * pitch:], k)
            done += k
            i += 1
            got += vs.pull(out, got)
            if between is not None and i == 1:
                between()
        pulled = got
        nb, end, fb = vs.finish(out, got)
        got += nb
        assert got == (end + 7) // 8
        return out[:got].tobytes(), [int(b) for b in fb], end, pulled, _device_bytes(codec, vs)
    finally:
        vs.close()


def _check(codec, n, kind, w, h, f, mat, gop, merange, pushes, rle=True, mode=MODE_FAST, start=0, pinned=False,
           second=False):
    exp, eend, efb = _expected(kind, w, h, f, n, mat, gop, merange, rle, start)
    codec.set_quant(_matrix(mat, n), n)
    y = _video(kind, w, h, f)
    got, fb, end, pulled, dev = _stream(codec, y, w, h, f, gop, merange, pushes, rle, mode, start, pinned=pinned)
    assert end == eend and fb == [int(b) for b in efb], (end, eend, fb, list(efb))
    want = _want(exp, eend, start).tobytes()
    assert got == want
    nb = (eend + 7) // 8
    assert dev[:nb].tobytes() == want and not dev[nb:].any()  # the device stream, nothing past the end
    if second:  # the second check: ie_encode_gop on the same input
        import torch
        out = torch.zeros(codec.gop_stream_bound(w, h, f, merange, start), dtype=torch.uint8, device="cuda")
        lead = _lead(start)[1]
        out[: lead.size] = torch.from_numpy(lead).cuda()
        rfb, rend = codec.encode_gop(torch.from_numpy(np.array(y)).cuda(), w, h, out, gop, merange, start_bit=start,
                                     nframes=f, rle=rle, mode=mode)
        assert rend == end and [int(b) for b in rfb] == fb and out[:nb].cpu().numpy().tobytes() == got
    return got, pulled


# ------------------------------------------------------------------------------- shapes
def test_one_macroblock_one_frame_per_push(codec, monkeypatch):
    """16x16, 5 frames, gop 2: groups of 2, 2 and a lone I-frame, one frame per push."""
    monkeypatch.delenv("IE_GOP_BATCH_MAX", raising=False)
    _check(codec, 4, "P", 16, 16, 5, "ref", 2, 4, [1], start=0, second=True)
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "1")
    _check(codec, 4, "P", 16, 16, 5, "ref", 2, 4, [1], start=13)


@pytest.mark.parametrize("batch", [None, 1], ids=["one-chunk", "chunks-of-1"])
@pytest.mark.parametrize("start", [0, 1, 31, 210, 549])
def test_pushes_across_group_boundaries(codec, monkeypatch, start, batch):
    """48x32, 7 frames, gop 3: the partitions [7], [2,4,1] and [1]*7 give identical bytes, the oracle's."""
    if batch:
        monkeypatch.setenv("IE_GOP_BATCH_MAX", str(batch))
    else:
        monkeypatch.delenv("IE_GOP_BATCH_MAX", raising=False)
    a = _check(codec, 4, "P", 48, 32, 7, "ref", 3, 8, [7], start=start, second=(batch is None))[0]
    b = _check(codec, 4, "P", 48, 32, 7, "ref", 3, 8, [2, 4, 1], start=start)[0]
    c = _check(codec, 4, "P", 48, 32, 7, "ref", 3, 8, [1], start=start)[0]
    assert a == b == c


@pytest.mark.parametrize("batch", [1, 2])
def test_several_chunks_reuse_both_slots(codec, monkeypatch, batch):
    """A 5-group video in chunks of 1 or 2 groups: at least three chunks, so both input slots are
    reused and a chunk is harvested before its slot's third use; bytes are pulled while later
    chunks are still to come."""
    monkeypatch.setenv("IE_GOP_BATCH_MAX", str(batch))
    _, pulled = _check(codec, 4, "P", 48, 32, 9, "ref", 2, 8, [1], start=21)
    assert pulled > 0
    _, pulled = _check(codec, 4, "P", 48, 32, 9, "ref", 2, 8, [3, 1], start=21, pinned=True)
    assert pulled > 0


@pytest.mark.parametrize("start", [0, 5])
@pytest.mark.parametrize("w,h", [(4, 4), (8, 12)])
def test_tiny_frames_chunks_share_output_words(codec, monkeypatch, w, h, start):
    """Frames without a macroblock, 40 frames in 14 chunks of one group: a chunk's payload is a few
    bits, so every chunk boundary falls inside a word an earlier chunk wrote and a pull returned."""
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "1")
    _, pulled = _check(codec, 4, "flat128", w, h, 40, "ref", 3, 8, [1], start=start)
    assert pulled > 0
    _check(codec, 4, "U", w, h, 40, "ref", 3, 8, [4, 1, 7], start=start)


def test_two_record_tiles(codec, monkeypatch):
    """96x96 is 576 blocks, two record tiles a frame."""
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "1")
    _check(codec, 4, "P", 96, 96, 6, "ref", 3, 8, [2], start=13)


def test_uncovered_right_strip(codec, monkeypatch):
    """40x16: W % 16 != 0 with H < 32."""
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "1")
    _check(codec, 4, "P", 40, 16, 6, "ref", 2, 8, [1, 3], start=7)


def test_8x8_vectors_only(codec, monkeypatch):
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "1")
    try:
        _check(codec, 8, "P", 64, 48, 5, "ref", 3, 8, [2], start=7, second=True)
    finally:
        codec.set_quant(_matrix("ref"), 4)


# ------------------------------------------------------------------------------- settings
def test_rle_off(codec, monkeypatch):
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "1")
    _check(codec, 4, "P", 48, 32, 5, "ref", 2, 8, [2], rle=False, start=13)


def test_exact_mode(codec, monkeypatch):
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "1")
    _check(codec, 4, "P", 48, 32, 5, "ref", 2, 8, [2], mode=MODE_EXACT, start=13)


def test_second_matrix(codec, monkeypatch):
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "1")
    try:
        _check(codec, 4, "M", 48, 32, 5, "second", 3, 8, [2], start=5)
    finally:
        codec.set_quant(_matrix("ref"), 4)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_pinned_and_pageable_frames(codec, monkeypatch, pinned):
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "2")
    _check(codec, 4, "M", 48, 32, 11, "ref", 2, 8, [3], start=3, pinned=pinned)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("padded", [True, False], ids=["stride", "yuv420"])
def test_stride_and_frame_pitch(codec, monkeypatch, padded, pinned):
    """Rows stride = w + 16 apart in padded frames, and plain YUV420 frames (1.5 w h apart)."""
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "1")
    w, h, f, gop, merange, start = 48, 32, 7, 3, 8, 13
    stride = w + 16 if padded else w
    pitch = stride * h * 3 // 2
    y = _video("P", w, h, f)
    wide = np.full(f * pitch, 0xA7, dtype=np.uint8)
    for k in range(f):
        wide[k * pitch: k * pitch + stride * h].reshape(h, stride)[:, :w] = y[k]
    exp, eend, efb = _expected("P", w, h, f, 4, "ref", gop, merange, True, start)
    codec.set_quant(_matrix("ref"), 4)
    got, fb, end, _, dev = _stream(codec, wide, w, h, f, gop, merange, [2, 1], start=start, stride=stride,
                                   frame_pitch=pitch, pinned=pinned)
    assert end == eend and fb == [int(b) for b in efb]
    assert got == _want(exp, eend, start).tobytes()
    assert not dev[(eend + 7) // 8:].any()


# ------------------------------------------------------------------------------- other calls
@pytest.mark.parametrize("fn", ["encode_gop", "encode_gop_groups"])
def test_a_call_between_pushes(codec, monkeypatch, fn):
    """Another P-frame encode on the same codec between two pushes (it overwrites the context's
    position table; the groups call also regrows the context's group scratch) is itself correct and
    leaves the stream's result unchanged."""
    import torch
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "1")
    codec.set_quant(_matrix("ref"), 4)
    w2, h2, f2, gop2 = 96, 96, 6, 3
    exp2, eend2, efb2 = _expected("P", w2, h2, f2, 4, "ref", gop2, 8, True, 13)

    def between():
        monkeypatch.delenv("IE_GOP_BATCH_MAX")
        out = torch.zeros(codec.gop_stream_bound(w2, h2, f2, 8, 13), dtype=torch.uint8, device="cuda")
        lead = _lead(13)[1]
        out[: lead.size] = torch.from_numpy(lead).cuda()
        fb, end = getattr(codec, fn)(torch.from_numpy(np.array(_video("P", w2, h2, f2))).cuda(), w2, h2, out, gop2, 8,
                                     start_bit=13, nframes=f2)
        assert end == eend2 and list(fb) == list(efb2)
        assert out[: (end + 7) // 8].cpu().numpy().tobytes() == _want(exp2, eend2, 13).tobytes()

    w, h, f, gop, start = 48, 32, 9, 2, 21
    exp, eend, efb = _expected("P", w, h, f, 4, "ref", gop, 8, True, start)
    got, fb, end, _, _ = _stream(codec, _video("P", w, h, f), w, h, f, gop, 8, [3], start=start, between=between)
    assert end == eend and fb == [int(b) for b in efb] and got == _want(exp, eend, start).tobytes()


def test_gop1_forwards_to_the_plain_stream(codec):
    """open_video_stream(gop=1) is the stream opened without the arguments."""
    w, h, f, start = 48, 32, 5, 13
    codec.set_quant(_matrix("ref"), 4)
    y = _video("P", w, h, f)
    a = _stream(codec, y, w, h, f, 1, 0, [2], start=start, open_kw={})
    b = _stream(codec, y, w, h, f, 1, 0, [2], start=start, open_kw=dict(gop=1, merange=8))
    assert a[:3] == b[:3]
    exp, eend, efb = _expected("P", w, h, f, 4, "ref", 1, 8, True, start)
    assert b[2] == eend and b[1] == [int(x) for x in efb] and b[0] == _want(exp, eend, start).tobytes()


# ------------------------------------------------------------------------------- argument checks
def test_errors(codec, monkeypatch):
    import torch
    codec.set_quant(_matrix("ref"), 4)

    def code(call):
        with pytest.raises(IEError) as e:
            call()
        return e.value.code

    assert code(lambda: codec.open_video_stream(64, 48, max_frames=6, gop=2, merange=-1)) == IE_EINVAL
    assert code(lambda: codec.open_video_stream(64, 48, max_frames=6, gop=2, merange=32768)) == IE_EINVAL
    assert code(lambda: codec.open_video_stream(72, 40, max_frames=6, gop=2, merange=8)) == IE_EINVAL  # W % 16, H >= 32
    codec.open_video_stream(72, 40, max_frames=6, gop=1).close()  # (no P-frames: allowed)

    vs = codec.open_video_stream(64, 48, max_frames=2, gop=2, merange=8)
    try:
        y = np.zeros(64 * 48 * 3, dtype=np.uint8)
        assert code(lambda: vs.push(y, 3)) == IE_ECAP  # beyond max_frames
        vs.push(y, 1)
        assert code(lambda: vs.push(y, 2)) == IE_ECAP  # (frames waiting in the slot count)
        assert code(lambda: vs.push(torch.zeros(64 * 48, dtype=torch.uint8, device="cuda"), 1)) == IE_EINVAL
    finally:
        vs.close()


def test_small_pull_buffer_leaves_the_stream_usable(codec, monkeypatch):
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "1")
    w, h, f, gop, start = 48, 32, 9, 2, 21
    exp, eend, efb = _expected("P", w, h, f, 4, "ref", gop, 8, True, start)
    codec.set_quant(_matrix("ref"), 4)
    vs = codec.open_video_stream(w, h, head=_lead(start)[1], start_bit=start, max_frames=f, gop=gop, merange=8)
    try:
        y = np.array(_video("P", w, h, f)).ravel()
        vs.push(y, 6)  # three chunks launched: two of them finished for pull
        with pytest.raises(IEError) as e:
            vs.pull(np.zeros(1, dtype=np.uint8), 0)
        assert e.value.code == IE_ECAP
        out = np.zeros(vs.cap, dtype=np.uint8)
        got = vs.pull(out, 0)
        assert got > 0
        vs.push(y[6 * w * h:], 3)
        got += vs.pull(out, got)
        nb, end, fb = vs.finish(out, got)
        assert end == eend and [int(b) for b in fb] == [int(b) for b in efb]
        assert out[: got + nb].tobytes() == _want(exp, eend, start).tobytes()
    finally:
        vs.close()


# ------------------------------------------------------------------------------- reference goldens
GOLDEN = [c for c in O.manifest_gop() if c["size"] <= 64 * 1024]


@pytest.mark.parametrize("c", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_reference_goldens(codec, monkeypatch, c):
    """Every small P-frame golden (the cases tests/test_gop.py reads), pushed in chunks of one group
    behind the settings header: the stream is the reference's file."""
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "1")
    q = O.read_matrix(c["matrix"], 4)
    codec.set_quant(q, 4)
    try:
        w, h = c["w"], c["h"]
        raw = np.frombuffer(O.case_input(c), dtype=np.uint8)
        pitch = w * h * 3 // 2
        f = raw.size // pitch
        hdr, hb = O.load().header(4, q, c["rle"], w, h, video=True, frames=f, gop=c["gop"], merange=c["merange"])
        vs = codec.open_video_stream(w, h, head=hdr, start_bit=hb, max_frames=f, frame_pitch=pitch, rle=bool(c["rle"]),
                                     gop=c["gop"], merange=c["merange"])
        try:
            out = np.zeros(vs.cap, dtype=np.uint8)
            got = 0
            for f0 in range(0, f, c["gop"]):
                vs.push(raw[f0 * pitch:], min(c["gop"], f - f0))
                got += vs.pull(out, got)
            nb, end, _ = vs.finish(out, got)
        finally:
            vs.close()
        assert out[: got + nb].tobytes() == O.case_encoded(c)
    finally:
        codec.set_quant(_matrix("ref"), 4)
