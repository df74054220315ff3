"""GPU: every matrix of the sweep (tests/matrix_sweep.py) through every path the per-matrix tables
feed, each result against the CPU oracle bit for bit.  The five matrix files of tests/golden hold
powers of two and 255 only and all take the dc_exact branch; these matrices do not.

Encodes run FAST and EXACT, RLE on and off, on uniform noise, 0/255 noise, low-amplitude noise and
a frame whose blocks sit exactly on rounding ties of the DC and the structural coefficients (the
tie count is asserted with the integer rule before anything touches the GPU).  Shapes are the
smallest that reach each kernel: 256 x 48 x 3 is encode4p_kernel on a three-tile chain with a
partial last tile, 200 x 56 the ragged 4 x 4 encode_kernel, 256 x 128 x 2 encode_kernel<8>.
quantize_frames is compared first, so a failure points at a coefficient before it shows as a
stream mismatch."""
import numpy as np
import pytest

from imageencoder_amd import MODE_EXACT, MODE_FAST, stream_bound, synth
from tests import matrix_sweep as MS

pytestmark = pytest.mark.gpu

MIN_TIES = 32


@pytest.fixture(scope="module")
def codec():
    from imageencoder_amd import Codec
    return Codec(0)


def _contents(n, q, w, h, f):
    """(kind, frames) of the four contents; the tie frame's tie count is asserted here."""
    ties = MS.tie_frames(n, q, w, h, f, seed=1)
    counts = MS.tie_counts(ties, n, q)
    for c in range(MS.TIE_COEFS):
        if MS.tie_reachable(n, int(q[MS.tie_index(n, c)])):
            assert counts[c] >= MIN_TIES, (c, counts)
    return [("uniform", MS.noise((f, h, w), 21)), ("0/255", MS.noise_0_255((f, h, w), 22)),
            ("low", MS.low_noise((f, h, w), 23)), ("tie", ties)]


def _expects_requests(n, q):
    """A tie frame asks for FP64 evaluations unless no tie is in reach, or only the DC's with a
    power-of-two quantiser, whose quotient FP32 holds exactly."""
    dc = int(q[0])
    return (any(MS.tie_reachable(n, int(q[k])) for k in MS.structural(n))
            or (MS.tie_reachable(n, dc) and dc & (dc - 1) != 0))


def _sweep_encode(codec, oracle, n, q, w, h, f, start_bit):
    codec.set_quant(q, n)
    for kind, y in _contents(n, q, w, h, f):
        coef = oracle.quantize(y.reshape(f * h, w), n, q)
        for mode in (MODE_FAST, MODE_EXACT):
            got = codec.quantize_frames(y, w, h, nframes=f, mode=mode)
            bad = np.argwhere(got != coef)
            assert bad.size == 0, (kind, mode, "block, coefficient:", bad[:4].tolist())
        for rle in (True, False):
            exp, eend, efb = oracle.encode_blocks(y, n, q, rle, start_bit)
            nb = (eend + 7) // 8
            for mode in (MODE_FAST, MODE_EXACT):
                out = np.zeros(stream_bound(w, h, n, f, start_bit), dtype=np.uint8)
                fb, end = codec.encode_frames(y, w, h, out, start_bit=start_bit, nframes=f, rle=rle, mode=mode)
                req = codec.last_fallbacks()
                assert end == eend and np.array_equal(fb, efb), (kind, rle, mode, end, eend)
                assert out[:nb].tobytes() == exp[:nb].tobytes(), (kind, rle, mode)
                if mode == MODE_FAST and kind == "tie" and _expects_requests(n, q):
                    assert req > 0, (kind, rle)


@pytest.mark.parametrize("name", MS.ids(4))
def test_encode4p_three_tile_chain(codec, oracle, name):
    _sweep_encode(codec, oracle, 4, MS.by_name(4, name), 256, 48, 3, start_bit=165)


@pytest.mark.parametrize("name", MS.ids(4))
def test_encode4_ragged(codec, oracle, name):
    _sweep_encode(codec, oracle, 4, MS.by_name(4, name), 200, 56, 1, start_bit=5)


@pytest.mark.parametrize("name", MS.ids(8))
def test_encode8(codec, oracle, name):
    _sweep_encode(codec, oracle, 8, MS.by_name(8, name), 256, 128, 2, start_bit=5)


def test_set_quant_accepts_every_matrix(codec):
    from imageencoder_amd import IE_OK
    for n in (4, 8):
        for name, q in MS.sweep(n):
            assert codec.L.ie_set_quant(codec.h, q.ctypes.data, n) == IE_OK, (n, name)


def test_counting_instantiation_on_tie_frame(codec, oracle):
    """encode_images_counted on the JPEG-like matrix and the tie frames: streams equal the oracle's
    and the fused byte histogram equals numpy.bincount of the produced stream."""
    import torch
    w, h, f, start_bit = 256, 48, 3, 64
    q = MS.by_name(4, "jpeg_like")
    y = MS.tie_frames(4, q, w, h, f, seed=1)
    codec.set_quant(q, 4)
    pitch = (stream_bound(w, h, 4, 1, start_bit) + 255) // 256 * 256
    out = torch.zeros(pitch * f, dtype=torch.uint8, device="cuda")
    codec.encode_images(torch.from_numpy(y).cuda(), w, h, out, out_pitch=pitch, nframes=f, start_bit=start_bit,
                        count_bytes=True)
    hist, _ = codec.huffman_hist_after_encode(out, pitch, f)
    host = out.cpu().numpy()
    for k in range(f):
        exp, eend, _ = oracle.encode_blocks(y[k:k + 1], 4, q, True, start_bit)
        nb = (eend + 7) // 8
        assert host[k * pitch: k * pitch + nb].tobytes() == exp[:nb].tobytes()
        np.testing.assert_array_equal(hist[k], np.bincount(host[k * pitch: k * pitch + nb], minlength=256))


CASES = [(n, name) for n in (4, 8) for name in MS.ids(n)]


@pytest.mark.parametrize("n,name", CASES, ids=[f"{n}x{n}-{name}" for n, name in CASES])
def test_decode_image_file(codec, oracle, n, name):
    """The noise frame's file decoded on the device == the oracle's decode: large quantisers times
    large coefficients clamp as the reference does."""
    q = MS.by_name(n, name)
    w, h = (200, 56) if n == 4 else (256, 128)
    for y in (MS.noise((h, w), 31), MS.noise_0_255((h, w), 32)):
        enc = oracle.encode_image(y, n, q, rle=True, huffman=True)
        assert codec.encode_image_file(y, w, h, q, n, rle=True, huffman=True) == enc
        assert np.array_equal(codec.decode_image_file(enc, n), oracle.decode_image(enc, n))


@pytest.mark.parametrize("name", ["jpeg_like", "primes", "rand16_0"])
@pytest.mark.parametrize("gen", ["P", "U"])
def test_gop(codec, oracle, name, gen):
    """encode_gop and decode_gop at 64 x 48 x 3, gop 3, merange 8, against the oracle's payload and
    the oracle's decode of the file."""
    import torch
    q = MS.by_name(4, name)
    w, h, f, gop, mer = 64, 48, 3, 3, 8
    codec.set_quant(q, 4)
    y = synth.frames(gen, w, h, f, seed=13)
    hdr, hb = oracle.header(4, q, True, w, h, video=True, frames=f, gop=gop, merange=mer)
    buf, eend, efb = oracle.encode_gop(y, 4, q, gop, mer, start_bit=hb)
    nb = (eend + 7) // 8
    for mode in (MODE_FAST, MODE_EXACT):
        out = torch.zeros(codec.gop_stream_bound(w, h, f, mer, hb), dtype=torch.uint8, device="cuda")
        fb, end = codec.encode_gop(torch.from_numpy(y).cuda(), w, h, out, gop, mer, start_bit=hb, nframes=f, mode=mode)
        assert end == eend and np.array_equal(fb, efb), (mode, end, eend)
        got = out[:nb].cpu().numpy()
        got[: hb // 8] = 0
        exp = buf[:nb].copy()
        exp[: hb // 8] = 0
        mask = np.uint8(0xFF >> (hb % 8))  # the payload's bits of the byte it starts in
        assert (got[hb // 8] & mask) == (exp[hb // 8] & mask)
        assert got[hb // 8 + 1:].tobytes() == exp[hb // 8 + 1:].tobytes(), mode
    bits = np.concatenate([np.unpackbits(hdr)[:hb], np.unpackbits(buf)[hb:eend]]).astype(np.uint8)
    enc = np.packbits(bits)
    pitch = w * h * 3 // 2
    dec = torch.full((f * pitch,), 0x80, dtype=torch.uint8, device="cuda")
    dend = codec.decode_gop(torch.from_numpy(enc.copy()).cuda(), w, h, dec, gop, mer, f, start_bit=hb, frame_pitch=pitch)
    assert (dend + 7) // 8 == enc.size
    assert dec.cpu().numpy().tobytes() == oracle.decode_video_gop(enc.tobytes(), 4)
