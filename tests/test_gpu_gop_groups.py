"""GPU parity of ie_encode_gop_groups (groups of pictures encoded side by side, then spliced): the
stream bytes, the per-frame bits and the end bit equal the CPU oracle's (O.load().encode_gop), bit
for bit, and -- as a second check only -- what ie_encode_gop gives on the same input.

The shapes are the smallest at which each path can go wrong: one macroblock with a ragged last
group, frames of a few bits (several groups in one output word: the splice's edge ORs), every
class of start bit, two record tiles (the batched scan's per-group tile offsets), an uncovered
right strip, 8x8 blocks (vectors only), waves of groups (IE_GOP_BATCH_MAX), the forwarding paths,
the argument checks, the reference's P-frame goldens and the ticket-mode redo.
"""
import functools

import numpy as np
import pytest

from imageencoder_amd import MODE_EXACT, MODE_FAST, synth
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


def _call(codec, fn, y, w, h, f, gop, merange, rle, mode, start, dev, stride=None, frame_pitch=None):
    """One encode into a stream whose bits before start_bit carry a pattern: (whole buffer, frame bits, end)."""
    import torch
    cap = codec.gop_stream_bound(w, h, f, merange, start)
    head = np.zeros(cap, dtype=np.uint8)
    lead = _lead(start)[1]
    head[: lead.size] = lead
    y = np.array(y, dtype=np.uint8)  # (a writable, contiguous copy: the cached videos are read-only)
    if dev:
        y, out = torch.from_numpy(y).cuda(), torch.from_numpy(head).cuda()
    else:
        out = head
    fb, end = fn(y, w, h, out, gop, merange, start_bit=start, stride=stride, frame_pitch=frame_pitch, nframes=f,
                 rle=rle, mode=mode)
    return (out.cpu().numpy() if dev else out), fb, end


def _want(exp, eend, start):
    """The stream from bit 0 to the end bit: the caller's leading bits, then the oracle's payload."""
    bits = np.concatenate([_lead(start)[0], np.unpackbits(exp)[start:eend]])
    return np.packbits(bits)


def _check(codec, n, kind, w, h, f, mat, gop, merange, rle=True, mode=MODE_FAST, start=0, dev=True, second=True):
    exp, eend, efb = _expected(kind, w, h, f, n, mat, gop, merange, rle, start)
    codec.set_quant(_matrix(mat, n), n)
    y = _video(kind, w, h, f)
    got, fb, end = _call(codec, codec.encode_gop_groups, y, w, h, f, gop, merange, rle, mode, start, dev)
    assert end == eend and list(fb) == list(efb), (end, eend, list(fb), list(efb))
    nb = (eend + 7) // 8
    assert got[:nb].tobytes() == _want(exp, eend, start).tobytes()
    if dev:  # device stream: nothing written past the end
        assert not got[nb:].any()
    if second:  # the second check: ie_encode_gop on the same input
        ref, rfb, rend = _call(codec, codec.encode_gop, y, w, h, f, gop, merange, rle, mode, start, dev)
        assert rend == end and list(rfb) == list(fb) and ref[:nb].tobytes() == got[:nb].tobytes()
    return got[:nb].tobytes()


# ------------------------------------------------------------------------------- shapes
def test_one_macroblock_ragged_last_group(codec):
    """16x16, 5 frames, gop 2: groups of 2, 2 and a lone I-frame."""
    _check(codec, 4, "P", 16, 16, 5, "ref", 2, 4, start=0, dev=True)
    _check(codec, 4, "P", 16, 16, 5, "ref", 2, 4, start=13, dev=False)


@pytest.mark.parametrize("start", [0, 5])
@pytest.mark.parametrize("w,h", [(4, 4), (8, 12)])
def test_tiny_frames_share_output_words(codec, w, h, start):
    """Frames without a macroblock, 40 frames in 14 groups: a group's payload is a few bits, so
    several groups land in one output word and every word is built from the splice's edge ORs."""
    _check(codec, 4, "flat128", w, h, 40, "ref", 3, 8, start=start, dev=True)
    _check(codec, 4, "U", w, h, 40, "ref", 3, 8, start=start, dev=(start == 0))


@pytest.mark.parametrize("start", [0, 1, 31, 210, 549])
def test_start_bit_classes(codec, start):
    """48x32, 7 frames, gop 3: every shift amount class, a start inside a word and inside a byte."""
    _check(codec, 4, "P", 48, 32, 7, "ref", 3, 8, start=start, dev=True)


def test_two_record_tiles(codec):
    """96x96 is 576 blocks, two record tiles a frame: the batched scan with per-group tile offsets."""
    _check(codec, 4, "P", 96, 96, 6, "ref", 3, 8, start=13, dev=True)


def test_uncovered_right_strip(codec):
    """40x16: W % 16 != 0 with H < 32, the strip's workgroups of every group."""
    _check(codec, 4, "P", 40, 16, 6, "ref", 2, 8, start=7, dev=True)


@pytest.mark.parametrize("w,h,gop", [(64, 48, 3), (72, 24, 2)])
def test_8x8_vectors_only(codec, w, h, gop):
    try:
        _check(codec, 8, "P", w, h, 5, "ref", gop, 8, start=7, dev=True)
    finally:
        codec.set_quant(_matrix("ref"), 4)


# ------------------------------------------------------------------------------- settings
def test_rle_off(codec):
    _check(codec, 4, "P", 64, 48, 5, "ref", 2, 8, rle=False, start=13, dev=True)


@pytest.mark.parametrize("merange", [0, 1, 64])
def test_merange(codec, merange):
    _check(codec, 4, "P", 64, 48, 5, "ref", 3, merange, start=3, dev=True)


def test_exact_mode(codec):
    _check(codec, 4, "P", 64, 48, 5, "ref", 2, 8, mode=MODE_EXACT, start=13, dev=True)


def test_second_matrix(codec):
    try:
        _check(codec, 4, "M", 64, 48, 5, "second", 3, 8, start=5, dev=True)
    finally:
        codec.set_quant(_matrix("ref"), 4)


@pytest.mark.parametrize("dev", [True, False], ids=["device", "host"])
def test_stride_and_frame_pitch(codec, dev):
    """Rows stride = w + 16 apart in padded frames; device frames with a device stream, host frames
    with a host stream.  Device stream: the bits before start_bit unchanged, zero past the end."""
    w, h, f, gop, merange, start = 64, 48, 5, 2, 8, 13
    stride = w + 16
    pitch = stride * h * 3 // 2
    y = _video("P", w, h, f)
    wide = np.full(f * pitch, 0xA7, dtype=np.uint8)
    for k in range(f):
        wide[k * pitch: k * pitch + stride * h].reshape(h, stride)[:, :w] = y[k]
    exp, eend, efb = _expected("P", w, h, f, 4, "ref", gop, merange, True, start)
    codec.set_quant(_matrix("ref"), 4)
    got, fb, end = _call(codec, codec.encode_gop_groups, wide, w, h, f, gop, merange, True, MODE_FAST, start, dev,
                         stride=stride, frame_pitch=pitch)
    assert end == eend and list(fb) == list(efb)
    nb = (eend + 7) // 8
    assert got[:nb].tobytes() == _want(exp, eend, start).tobytes()
    if dev:
        assert not got[nb:].any()


@pytest.mark.parametrize("batch", [1, 2])
def test_waves_of_groups(codec, batch, monkeypatch):
    """A 5-group video with IE_GOP_BATCH_MAX = 1 and 2 (waves of 1 or 2 groups sharing the scratch,
    every wave's splice starting at the previous wave's end bit) == the bytes without it."""
    monkeypatch.delenv("IE_GOP_BATCH_MAX", raising=False)
    whole = _check(codec, 4, "P", 48, 32, 9, "ref", 2, 8, start=21, dev=True)
    monkeypatch.setenv("IE_GOP_BATCH_MAX", str(batch))
    assert _check(codec, 4, "P", 48, 32, 9, "ref", 2, 8, start=21, dev=True, second=False) == whole
    assert _check(codec, 4, "P", 48, 32, 9, "ref", 2, 8, start=21, dev=False, second=False) == whole


@pytest.mark.parametrize("gop", [1, 5, 9])
def test_forwarding_paths(codec, gop):
    """gop = 1 and gop >= nframes (one group): the call is ie_encode_gop."""
    _check(codec, 4, "P", 48, 32, 5, "ref", gop, 8, start=13, dev=True)


# ------------------------------------------------------------------------------- argument checks
def test_invalid_arguments_as_encode_gop(codec):
    from imageencoder_amd import IE_ECAP, IE_EINVAL, IEError
    codec.set_quant(_matrix("ref"), 4)

    def code(fn, y, w, h, out, gop, merange, f):
        with pytest.raises(IEError) as e:
            fn(y, w, h, out, gop, merange, nframes=f)
        return e.value.code

    def both(y, w, h, out, gop, merange, f, want):
        a = code(codec.encode_gop_groups, y, w, h, out, gop, merange, f)
        assert a == code(codec.encode_gop, y, w, h, out, gop, merange, f) == want

    y = np.zeros((6, 48, 64), dtype=np.uint8)
    out = np.zeros(codec.gop_stream_bound(64, 48, 6, 8), dtype=np.uint8)
    both(y, 64, 48, out, 2, -1, 6, IE_EINVAL)       # bad merange
    both(y, 64, 48, out, 2, 32768, 6, IE_EINVAL)
    both(y, 64, 48, out[:-1], 2, 8, 6, IE_ECAP)     # capacity one byte short
    y2 = np.zeros((6, 40, 72), dtype=np.uint8)
    out2 = np.zeros(codec.gop_stream_bound(72, 40, 6, 8), dtype=np.uint8)
    both(y2, 72, 40, out2, 2, 8, 6, IE_EINVAL)      # W % 16 with H >= 32
    both(y2, 72, 40, out2[:4], 2, 40000, 6, IE_EINVAL)  # (a bad merange is reported before the shape and the capacity)
    L = codec.L
    for args in ((None, y.ctypes.data, out.ctypes.data), (codec.h, None, out.ctypes.data), (codec.h, y.ctypes.data, None)):
        r = [fn(args[0], args[1], 64, 48, 64, 64 * 48, 6, 2, 8, 1, MODE_FAST, args[2], out.size, 0, None, None)
             for fn in (L.ie_encode_gop_groups, L.ie_encode_gop)]
        assert r[0] == r[1] == IE_EINVAL            # NULL pointers


# ------------------------------------------------------------------------------- reference goldens
GOLDEN = [c for c in O.manifest_gop() if c["size"] <= 64 * 1024]


@pytest.mark.parametrize("c", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_reference_goldens(codec, c):
    """Every small P-frame golden: the header, then the payload through the new call, is the
    reference's file (assembled as tests/test_gop.py::test_oracle_gop_payload_matches_file does)."""
    import torch
    q = O.read_matrix(c["matrix"], 4)
    codec.set_quant(q, 4)
    try:
        w, h = c["w"], c["h"]
        raw = np.frombuffer(O.case_input(c), dtype=np.uint8)
        pitch = w * h * 3 // 2
        f = raw.size // pitch
        hdr, hb = O.load().header(4, q, c["rle"], w, h, video=True, frames=f, gop=c["gop"], merange=c["merange"])
        out = torch.zeros(codec.gop_stream_bound(w, h, f, c["merange"], hb), dtype=torch.uint8, device="cuda")
        _, end = codec.encode_gop_groups(torch.from_numpy(raw.copy()).cuda(), w, h, out, c["gop"], c["merange"],
                                         start_bit=hb, frame_pitch=pitch, nframes=f, rle=bool(c["rle"]))
        bits = np.concatenate([np.unpackbits(hdr)[:hb], np.unpackbits(out.cpu().numpy())[hb:end]]).astype(np.uint8)
        assert np.packbits(bits).tobytes() == O.case_encoded(c)
    finally:
        codec.set_quant(_matrix("ref"), 4)


# ------------------------------------------------------------------------------- ticket-mode redo
def test_timeout_redo_clears_stream(monkeypatch):
    """One reported look-back timeout (IE_FAKE_TIMEOUTS=1, read by ie_create: a codec of its own, as
    in tests/test_gop.py) on a device stream: the stream is cleared from start_bit on, the video is
    redone in ticket mode and equals the oracle's payload, the caller's leading bits kept."""
    from imageencoder_amd import Codec
    monkeypatch.setenv("IE_FAKE_TIMEOUTS", "1")
    monkeypatch.delenv("IE_FORCE_TICKET", raising=False)
    own = Codec(0, _matrix("ref"), 4)
    try:
        _check(own, 4, "P", 64, 48, 7, "ref", 3, 8, start=13, dev=True, second=False)
    finally:
        own.close()
