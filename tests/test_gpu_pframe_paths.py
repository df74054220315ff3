"""GPU parity of the P-frame kernels' less travelled paths (ie_pframe.hip, ie_encode_gop,
ie_decode_gop): ticket-mode emission over several record tiles and over more than 256 of them, SAD
ties and the own-position skip (flat, periodic and static content), candidates clamped at the
frame's edge and wrapped through int16 (merange up to 32767), five-bit records, wide records,
reconstruction clamped at 0 and 255, strips no macroblock covers, row stride and frame pitch, and
the decode of every 4x4 payload among them whose sides are multiples of 16.  Every encode compares stream bytes, per-frame bits and end bit with
the CPU oracle, bit for bit; every decode compares the frames with the oracle's decode of header +
payload.  tests/test_pframe_content.py proves on the CPU that the contents reach these paths.
A record tile is 512 consecutive 4x4 blocks of a frame.
"""
import functools

import numpy as np
import pytest

from imageencoder_amd import MODE_EXACT, MODE_FAST, synth
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

TILE_BLOCKS = 512
SEED = 7


@pytest.fixture(scope="module")
def codec():
    from imageencoder_amd import Codec
    return Codec(0)


@functools.lru_cache(maxsize=None)
def _matrix(name, n=4):
    if name == "ref":
        return O.read_matrix("matrix.txt" if n == 4 else "matrix8_1.txt", n)
    if name == "dc4096":  # no DC of a prediction error survives it: five-bit records on static content
        return O.read_matrix("matrix4_dc4096.txt", 4)
    return np.full(n * n, {"ones": 1, "255": 255, "65535": 65535}[name], dtype=np.uint16)


@functools.lru_cache(maxsize=None)
def _video(kind, w, h, f):
    if kind == "bands":
        # 32-row bands, noise and flat 128 in turn: at 256 px a band is one record tile, so tiles
        # of long records (slow to emit) sit before tiles of short ones that share a word with them
        y = synth.frames("U", w, h, f, SEED).copy()
        y[:, (np.arange(h) // 32) % 2 == 1, :] = 128
        return y
    return synth.frames(kind, w, h, f, SEED)


@functools.lru_cache(maxsize=None)
def _expected(kind, w, h, f, n, mat, gop, merange, rle, start):
    """The oracle's payload (shared by the encode and the decode tests, never modified)."""
    buf, end, fb = O.load().encode_gop(_video(kind, w, h, f), n, _matrix(mat, n), gop, merange, rle=rle,
                                       start_bit=start)
    buf.setflags(write=False)
    return buf, end, fb


def _encode(codec, y, w, h, f, gop, merange, rle, mode, start, dev, stride=None, frame_pitch=None):
    """ie_encode_gop into a host or device stream: (stream bytes to the end bit, frame bits, end)."""
    import torch
    cap = codec.gop_stream_bound(w, h, f, merange, start)
    if dev:
        y = torch.from_numpy(np.ascontiguousarray(y)).cuda()
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    else:
        y = np.ascontiguousarray(y)
        out = np.zeros(cap, dtype=np.uint8)
    fb, end = codec.encode_gop(y, w, h, out, gop, merange, start_bit=start, stride=stride, frame_pitch=frame_pitch,
                               nframes=f, rle=rle, mode=mode)
    host = out.cpu().numpy() if dev else out
    return host[: (end + 7) // 8].tobytes(), fb, end


def _check(codec, n, kind, w, h, f, mat, gop, merange, rle=True, mode=MODE_FAST, start=0, dev=False):
    exp, eend, efb = _expected(kind, w, h, f, n, mat, gop, merange, rle, start)
    codec.set_quant(_matrix(mat, n), n)
    got, fb, end = _encode(codec, _video(kind, w, h, f), w, h, f, gop, merange, rle, mode, start, dev)
    assert end == eend and list(fb) == list(efb), (end, eend, list(fb), list(efb))
    assert got == exp[: (eend + 7) // 8].tobytes()
    return got


# ---------------------------------------------------------------------------- 1. ticket mode
@pytest.fixture(scope="module")
def ticket_codec():
    """A codec of its own created under IE_FORCE_TICKET=1 (ie_create reads the switch): P-frames take
    the tile-sum, tile-scan, emission launches."""
    from imageencoder_amd import Codec
    mp = pytest.MonkeyPatch()
    mp.setenv("IE_FORCE_TICKET", "1")
    try:
        c = Codec(0, _matrix("ref"), 4)
    finally:
        mp.undo()
    yield c
    c.close()


TICKET = [
    # kind, w, h, frames, matrix, gop, rle, start bit, device stream
    ("P", 128, 96, 5, "ref", 5, True, 0, False),       # 2 tiles
    ("U", 128, 96, 5, "ones", 3, True, 13, True),
    ("P", 256, 144, 5, "ref", 5, True, 13, True),      # 5 tiles, the last one partial
    ("U", 256, 144, 5, "ones", 5, False, 0, False),    # (196-bit records: the fullest tile image)
    ("static", 256, 144, 5, "65535", 5, True, 13, False),  # five-bit records: 80-word tiles
    ("P", 528, 16, 5, "ref", 5, True, 0, True),        # 528 blocks: a tile boundary inside a macroblock row
    ("bands", 256, 160, 3, "ones", 3, True, 13, True),   # long-record and short-record tiles in turn
    ("bands", 256, 160, 3, "ones", 3, False, 0, False),
]


@pytest.mark.parametrize("kind,w,h,f,mat,gop,rle,start,dev", TICKET,
                         ids=[f"{c[0]}{c[1]}x{c[2]}_{c[4]}_{'rle' if c[6] else 'norle'}_s{c[7]}" for c in TICKET])
def test_ticket_mode_multi_tile(codec, ticket_codec, kind, w, h, f, mat, gop, rle, start, dev):
    """Several record tiles through pf_tile_sum / pf_tile_scan / pf_emit: equal to the oracle and to
    the look-back codec's stream."""
    assert (w // 4) * (h // 4) > TILE_BLOCKS
    a = _check(ticket_codec, 4, kind, w, h, f, mat, gop, 8, rle=rle, start=start, dev=dev)
    b = _check(codec, 4, kind, w, h, f, mat, gop, 8, rle=rle, start=start, dev=dev)
    assert a == b


@pytest.mark.parametrize("dev,start", [(True, 0), (False, 13)])
def test_ticket_mode_more_than_256_tiles(codec, ticket_codec, dev, start):
    """2048 x 1040 is 260 tiles: the tile scan's second round adds the first round's carry."""
    w, h = 2048, 1040
    assert -(-(w // 4) * (h // 4) // TILE_BLOCKS) == 260
    a = _check(ticket_codec, 4, "M", w, h, 2, "ref", 2, 8, start=start, dev=dev)
    b = _check(codec, 4, "M", w, h, 2, "ref", 2, 8, start=start, dev=dev)
    assert a == b


# ---------------------------------------------------------------------------- 2. content classes
F = 5  # four P-frames in a row where gop >= F
CONTENT = [
    # kind, w, h, matrix, gop, merange, rle, mode, start bit, device stream
    ("static", 64, 48, "dc4096", 2, 8, True, MODE_FAST, 0, False),      # five-bit records, vectors (0, 0)
    ("static", 64, 48, "65535", F, 8, True, MODE_FAST, 13, True),       # reference + 128, clamped at 255
    ("static", 64, 48, "ref", F + 3, 0, True, MODE_EXACT, 0, True),    # no search step
    ("flat128", 64, 48, "ref", F, 8, True, MODE_FAST, 13, False),        # every candidate ties
    ("flat128", 64, 48, "ref", F, 32767, True, MODE_FAST, 0, True),
    ("flat128", 64, 48, "ones", 2, 1, False, MODE_FAST, 13, True),
    ("flat0255", 64, 48, "ones", F, 8, False, MODE_FAST, 0, False),     # 12-bit fields, 0 and 255
    ("flat0255", 64, 48, "255", F + 3, 3, True, MODE_EXACT, 13, True),
    ("flat0255", 64, 48, "ref", F, 20000, True, MODE_FAST, 0, True),
    ("stripesV", 64, 48, "ref", F, 8, True, MODE_FAST, 13, False),
    ("stripesV", 64, 48, "255", 2, 2, False, MODE_FAST, 0, True),
    ("stripesH", 64, 48, "ref", F + 3, 5, True, MODE_EXACT, 13, True),
    ("stripesH", 64, 48, "ones", F, 64, True, MODE_FAST, 0, False),
    ("checker", 64, 48, "ones", F, 8, False, MODE_FAST, 13, True),
    ("checker", 64, 48, "255", F, 3, True, MODE_FAST, 0, True),
    ("checker", 64, 48, "ref", F + 3, 32767, True, MODE_FAST, 13, False),
    ("shiftA", 64, 48, "ref", F, 8, True, MODE_FAST, 0, True),         # true motion found, clamped at the edge
    ("shiftA", 64, 48, "ref", F, 20000, False, MODE_EXACT, 13, True),
    ("shiftB", 64, 48, "ref", F, 40, True, MODE_FAST, 0, False),
    ("shiftB", 64, 48, "255", F + 3, 32767, True, MODE_FAST, 13, True),
    ("U", 64, 48, "ones", F, 8, True, MODE_FAST, 0, True),             # 13 x 16 + 4 bits: the widest RLE records
    ("U", 64, 48, "ones", F, 5, False, MODE_FAST, 13, False),
    ("U", 64, 48, "255", 2, 8, True, MODE_FAST, 0, True),              # coarse error: clamps at 0 and at 255
    # 256 x 144: five tiles in the look-back chain
    ("static", 256, 144, "65535", F, 8, True, MODE_FAST, 13, True),
    ("static", 256, 144, "dc4096", 2, 8, True, MODE_FAST, 0, False),
    ("flat128", 256, 144, "ref", F, 8, True, MODE_FAST, 13, True),
    ("flat0255", 256, 144, "ones", F, 5, False, MODE_FAST, 0, True),
    ("stripesV", 256, 144, "ref", F, 8, True, MODE_EXACT, 13, False),
    ("stripesH", 256, 144, "255", F + 3, 2, True, MODE_FAST, 0, True),
    ("checker", 256, 144, "ones", F, 8, False, MODE_FAST, 13, True),
    ("checker", 256, 144, "ref", 2, 64, True, MODE_FAST, 0, False),
    ("shiftA", 256, 144, "ref", F, 8, True, MODE_FAST, 13, True),
    ("shiftA", 256, 144, "ref", F, 32767, True, MODE_FAST, 0, True),
    ("shiftB", 256, 144, "ref", F, 64, True, MODE_FAST, 13, False),
    ("U", 256, 144, "ones", F, 8, True, MODE_FAST, 0, True),
    ("P", 256, 144, "255", F + 3, 20000, True, MODE_EXACT, 13, True),
    ("bands", 256, 160, "ones", F, 1, True, MODE_FAST, 0, False),
]


def _cid(c):
    return f"{c[0]}{c[1]}x{c[2]}_{c[3]}_g{c[4]}_m{c[5]}{'' if c[6] else '_norle'}{'_exact' if c[7] == MODE_EXACT else ''}"


@pytest.mark.parametrize("c", CONTENT, ids=[_cid(c) for c in CONTENT])
def test_content_classes(codec, c):
    kind, w, h, mat, gop, merange, rle, mode, start, dev = c
    _check(codec, 4, kind, w, h, F, mat, gop, merange, rle=rle, mode=mode, start=start, dev=dev)


# ---------------------------------------------------------------------------- 3. geometry
GEOMETRY = [(16, 16), (32, 16), (16, 32), (72, 28), (48, 12), (12, 28), (64, 40)]
GEOMETRY_SETTINGS = [("ref", F, 8, True), ("ones", 2, 3, False)]  # matrix, gop, merange, rle


@pytest.mark.parametrize("w,h", GEOMETRY)
@pytest.mark.parametrize("kind", ["P", "flat128"])
def test_geometry_4x4(codec, kind, w, h):
    """One macroblock (every candidate clamps to its own position), one macroblock row or column,
    a right and a bottom strip no macroblock covers, and frames without a macroblock."""
    for (mat, gop, merange, rle), start, dev in zip(GEOMETRY_SETTINGS, (13, 0), (True, False)):
        _check(codec, 4, kind, w, h, F, mat, gop, merange, rle=rle, start=start, dev=dev)


def test_geometry_rejected(codec):
    """12 x 48 has no macroblock but W % 16 != 0 with H >= 32: rejected like every such shape."""
    from imageencoder_amd import IEError
    codec.set_quant(_matrix("ref"), 4)
    y = np.zeros((2, 48, 12), dtype=np.uint8)
    out = np.zeros(codec.gop_stream_bound(12, 48, 2, 8), dtype=np.uint8)
    with pytest.raises(IEError):
        codec.encode_gop(y, 12, 48, out, 2, 8, nframes=2)
    with pytest.raises(AssertionError):
        O.load().encode_gop(y, 4, _matrix("ref"), 2, 8)


@pytest.mark.parametrize("w,h", [(72, 24), (64, 48)])
@pytest.mark.parametrize("kind", ["static", "flat128", "flat0255"])
def test_geometry_8x8(codec, kind, w, h):
    """8x8 blocks: vectors only, the frame's own pixels added to the copied block."""
    try:
        _check(codec, 8, kind, w, h, F, "ref", F, 8, start=7, dev=True)
        _check(codec, 8, kind, w, h, F, "ref", 2, 32767, dev=False)
    finally:
        codec.set_quant(_matrix("ref"), 4)


# ---------------------------------------------------------------------------- 4. stride and pitch
STRIDE = [("shiftA", 64, 48, 8), ("P", 256, 144, 16), ("P", 72, 28, 8)]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind,w,h,merange", STRIDE)
def test_stride_and_frame_pitch(codec, kind, w, h, merange, dev):
    """Rows stride = w + 16 apart in YUV-pitched frames: the compact video's stream.  An I-frame
    reference is read at the caller's stride, a reconstructed one at w (four P-frames in a row)."""
    stride = w + 16
    pitch = stride * h * 3 // 2
    y = _video(kind, w, h, F)
    wide = np.full(F * pitch, 0xA7, dtype=np.uint8)
    for f in range(F):
        wide[f * pitch: f * pitch + stride * h].reshape(h, stride)[:, :w] = y[f]
    q = _matrix("ref")
    exp, eend, efb = _expected(kind, w, h, F, 4, "ref", F, merange, True, 13)
    sbuf, send, sfb = O.load().encode_gop(wide, 4, q, F, merange, start_bit=13, stride=stride, frame_pitch=pitch,
                                          dims=(F, h, w))
    assert send == eend and sbuf[: (eend + 7) // 8].tobytes() == exp[: (eend + 7) // 8].tobytes()
    codec.set_quant(q, 4)
    got, fb, end = _encode(codec, wide, w, h, F, F, merange, True, MODE_FAST, 13, dev, stride=stride, frame_pitch=pitch)
    assert end == eend and list(fb) == list(efb)
    assert got == exp[: (eend + 7) // 8].tobytes()


# ---------------------------------------------------------------------------- 5. decode
def _file(kind, w, h, f, mat, gop, merange, rle):
    """Header + payload as the file writer lays them out: (bytes, header bits)."""
    o = O.load()
    hdr, hb = o.header(4, _matrix(mat), rle, w, h, video=True, frames=f, gop=gop, merange=merange)
    buf, end, _ = _expected(kind, w, h, f, 4, mat, gop, merange, rle, hb)
    data = buf[: (end + 7) // 8].copy()
    data[: (hb + 7) // 8] |= hdr[: (hb + 7) // 8]
    return data, hb, end


def _check_decode(codec, kind, w, h, f, mat, gop, merange, rle, outputs=(True, False)):
    import torch
    data, hb, end = _file(kind, w, h, f, mat, gop, merange, rle)
    codec.set_quant(_matrix(mat), 4)
    stride = w + 32
    pitch = stride * h * 3 // 2
    for mc in (True, False):
        exp = np.frombuffer(O.load().decode_video_gop(data.tobytes(), 4, mc), dtype=np.uint8)
        exp = exp.reshape(f, w * h * 3 // 2)[:, : w * h].reshape(f, h, w)
        want = np.full((f, pitch), 0x5A, dtype=np.uint8)
        want[:, : stride * h].reshape(f, h, stride)[:, :, :w] = exp
        for dev in outputs:
            # (device output with a device stream, host output with a host stream)
            out = torch.full((f * pitch,), 0x5A, dtype=torch.uint8, device="cuda") if dev else \
                np.full(f * pitch, 0x5A, dtype=np.uint8)
            src = torch.from_numpy(data.copy()).cuda() if dev else data
            got_end = codec.decode_gop(src, w, h, out, gop, merange, f, start_bit=hb, stride=stride, frame_pitch=pitch,
                                       rle=rle, motioncomp=mc)
            assert got_end == end
            host = out.cpu().numpy() if dev else out
            np.testing.assert_array_equal(host.reshape(f, pitch), want, err_msg=f"mc={mc} dev={dev}")


@pytest.mark.parametrize("c", CONTENT, ids=[_cid(c) for c in CONTENT])
def test_decode_content_classes(codec, c):
    """ie_decode_gop of every content payload, motion compensation on and off, into device and host
    frames with stride w + 32 and a YUV frame pitch: the bytes outside the Y rows stay 0x5A."""
    kind, w, h, mat, gop, merange, rle = c[:7]
    _check_decode(codec, kind, w, h, F, mat, gop, merange, rle)


# the payloads of the ticket, geometry and stride sections whose W and H are multiples of 16:
# (kind, w, h, frames, matrix, gop, merange, rle)
DECODE_OTHER = sorted(set(
    [(c[0], c[1], c[2], c[3], c[4], c[5], 8, c[6]) for c in TICKET] +
    [("M", 2048, 1040, 2, "ref", 2, 8, True)] +
    [(kind, w, h, F) + st for kind in ("P", "flat128") for w, h in GEOMETRY if w % 16 == 0 and h % 16 == 0
     for st in GEOMETRY_SETTINGS] +
    [(kind, w, h, F, "ref", F, merange, True) for kind, w, h, merange in STRIDE if w % 16 == 0 and h % 16 == 0]))


@pytest.mark.parametrize("c", DECODE_OTHER, ids=[f"{c[0]}{c[1]}x{c[2]}x{c[3]}_{c[4]}_g{c[5]}_m{c[6]}"
                                                 f"{'' if c[7] else '_norle'}" for c in DECODE_OTHER])
def test_decode_ticket_geometry_stride_payloads(codec, c):
    """The same decode checks from one macroblock (16 x 16), one macroblock column (16 x 32) and
    one row (32 x 16, 528 x 16) to 8320 macroblocks (2048 x 1040)."""
    kind, w, h, f, mat, gop, merange, rle = c
    _check_decode(codec, kind, w, h, f, mat, gop, merange, rle)


@pytest.mark.parametrize("kind,w,h,mat,gop,rle", [
    ("static", 1024, 256, "65535", 4, True),     # five-bit records: kRecPosCap records in every chunk
    ("static", 1024, 256, "dc4096", 2, True),
    ("checker", 256, 144, "ones", 4, False),     # the longest P-frame records, several chunks
    ("U", 256, 144, "ones", 4, True),
])
def test_decode_many_chunks(codec, kind, w, h, mat, gop, rle):
    _check_decode(codec, kind, w, h, 4, mat, gop, 8, rle)
    assert codec.last_decode_info()[0] > 1


@pytest.mark.parametrize("w,h", [(64, 40), (72, 24)])
def test_decode_rejects_partial_macroblocks(codec, w, h):
    from imageencoder_amd import IE_EINVAL, IEError
    codec.set_quant(_matrix("ref"), 4)
    src = np.zeros(4096, dtype=np.uint8)
    out = np.zeros(2 * w * h, dtype=np.uint8)
    with pytest.raises(IEError) as e:
        codec.decode_gop(src, w, h, out, 2, 8, 2)
    assert e.value.code == IE_EINVAL
