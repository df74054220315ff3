"""The context's buffers across calls: a buffer an earlier call sized is regrown by a larger call and
reused by a smaller one, and contexts, pipelines and video streams are torn down in any order.

Every call runs small, large, small on ONE codec (16x16 with 2 frames, 64x48 with 5 frames, 16x16
with 2 frames; P-frames: 32x32 with 4 frames, 64x48 with 7 frames and a short last group, 32x32
again), with host arrays and with device arrays, so the staging buffers, the decoders' scratch and
the streamed pipeline's slots all grow in the middle step and are used below their capacity in the
last.  All results are compared with the CPU oracle, bit for bit.
"""
import functools

import numpy as np
import pytest

from imageencoder_amd import Codec, stream_bound, synth
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

STEPS = [(16, 16, 2), (64, 48, 5), (16, 16, 2)]
GOP_STEPS = [(32, 32, 4, 2, 4), (64, 48, 7, 3, 4), (32, 32, 4, 2, 4)]  # w, h, frames, gop, merange


def _q(n):
    return O.read_matrix("matrix.txt" if n == 4 else "matrix8_1.txt", n)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _buf(size, dev):
    return _dev(np.zeros(size, dtype=np.uint8)) if dev else np.zeros(size, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _case(n, w, h, f):
    """The oracle's results for one shape (computed once, never modified)."""
    o, q = O.load(), _q(n)
    y = synth.frames("M", w, h, f, seed=31)
    chain, end, fb = o.encode_blocks(y, n, q)
    images = [o.encode_blocks(y[k], n, q)[:2] for k in range(f)]
    files = [o.encode_image(y[k], n, q, rle=True) for k in range(f)]
    hb = o.header(n, q, 1, w, h)[1]
    pixels = np.stack([np.asarray(o.decode_image(x, n)).reshape(h, w) for x in files])
    # Huffman: the frames' pixels reduced to eight values (a stream the pass codes with a dictionary)
    sym = [np.ascontiguousarray(y >> 5).ravel(), np.ascontiguousarray(y[0] >> 5).ravel()]
    huf = [o.huffman_encode(s.tobytes()) for s in sym]
    dec = [o.huffman_decode(x)[0] for x in huf]
    for a in (y, chain, pixels, *sym):
        a.setflags(write=False)
    return dict(y=y, chain=chain[: (end + 7) // 8], end=end, fb=[int(b) for b in fb], images=images, files=files,
                hb=hb, file_ends=[hb + o.encode_blocks(y[k], n, q)[1] for k in range(f)], pixels=pixels, sym=sym,
                huf=huf, dec=dec)


def _run_step(codec, n, w, h, f, dev):
    e = _case(n, w, h, f)
    y = _dev(e["y"]) if dev else np.array(e["y"])
    # encode_images: independent streams in slots
    pitch = (stream_bound(w, h, n, 1) + 255) // 256 * 256
    out = _buf(pitch * f, dev)
    ends = codec.encode_images(y, w, h, out, pitch, f)
    got = _host(out)
    for k, (exp, eend) in enumerate(e["images"]):
        nb = (eend + 7) // 8
        assert int(ends[k]) == eend and got[k * pitch: k * pitch + nb].tobytes() == exp[:nb].tobytes(), k
    # encode_frames: one chain
    out = _buf(stream_bound(w, h, n, f), dev)
    fb, end = codec.encode_frames(y, w, h, out, nframes=f)
    assert end == e["end"] and [int(b) for b in fb] == e["fb"]
    assert _host(out)[: len(e["chain"])].tobytes() == e["chain"].tobytes()
    # decode_frames: the chain back (a device stream is read in place: padded for the vector loads)
    src = np.zeros((len(e["chain"]) + 15) // 16 * 16 + 16, dtype=np.uint8)
    src[: len(e["chain"])] = e["chain"]
    pix = _buf(f * w * h, dev)
    assert codec.decode_frames(_dev(src) if dev else src, w, h, pix, nframes=f, length=len(e["chain"])) == e["end"]
    assert np.array_equal(_host(pix).reshape(f, h, w), e["pixels"])
    # decode_images: the files, one slot each
    spitch = (max(len(x) for x in e["files"]) + 8 + 15) // 16 * 16
    slots = np.zeros(f * spitch, dtype=np.uint8)
    for k, x in enumerate(e["files"]):
        slots[k * spitch: k * spitch + len(x)] = np.frombuffer(x, np.uint8)
    pix = _buf(f * w * h, dev)
    ends = codec.decode_images(_dev(slots) if dev else slots, spitch, [8 * len(x) for x in e["files"]], w, h, pix,
                               start_bit=e["hb"])
    assert [int(b) for b in ends] == e["file_ends"]
    assert np.array_equal(_host(pix).reshape(f, h, w), e["pixels"])
    # the Huffman round trip
    luts, sbs = [], []
    for s, enc, dec in zip(e["sym"], e["huf"], e["dec"]):
        assert codec.huffman_encode(_dev(s) if dev else np.array(s)) == enc
        table = codec.huffman_table(enc)
        assert table is not None  # (coded with a dictionary: a property of the input chosen above)
        luts.append(table[0])
        sbs.append(table[1])
        if dev:
            data = np.frombuffer(enc + b"\0" * (-len(enc) % 4 + 4), np.uint8)
            sout = _buf(8 * len(enc) + 16, True)
            cnt = codec.huffman_decode_device(_dev(data), len(enc), _dev(table[0]), table[1], sout)
            assert sout[:cnt].cpu().numpy().tobytes() == dec
        else:
            assert codec.huffman_decode(enc) == (dec, False)
    hpitch = (max(len(x) for x in e["huf"]) + 15) // 16 * 16
    slots = np.zeros(2 * hpitch, dtype=np.uint8)
    for k, x in enumerate(e["huf"]):
        slots[k * hpitch: k * hpitch + len(x)] = np.frombuffer(x, np.uint8)
    opitch = max(len(x) for x in e["dec"]) + 37
    lut = np.concatenate(luts)
    sout = _buf(2 * opitch, dev)
    cnt = codec.huffman_decode_batch(_dev(slots) if dev else slots, hpitch, [len(x) for x in e["huf"]], sbs,
                                     _dev(lut) if dev else lut, sout, opitch)
    for k, dec in enumerate(e["dec"]):
        assert int(cnt[k]) == len(dec) and _host(sout)[k * opitch: k * opitch + len(dec)].tobytes() == dec, k


@pytest.mark.parametrize("n", [4, 8])
def test_regrow_small_large_small(n):
    codec = Codec(0, _q(n), n)
    try:
        for w, h, f in STEPS:
            for dev in (False, True):
                _run_step(codec, n, w, h, f, dev)
    finally:
        codec.close()


@functools.lru_cache(maxsize=None)
def _gop_case(w, h, f, gop, merange):
    o, q = O.load(), _q(4)
    y = synth.frames("P", w, h, f, seed=31)
    buf, end, fb = o.encode_gop(y, 4, q, gop, merange)
    video = np.frombuffer(o.encode_video_gop(synth.yuv420(y), w, h, 4, q, gop=gop, merange=merange), dtype=np.uint8)
    hb = o.header(4, q, 1, w, h, video=True, frames=f, gop=gop, merange=merange)[1]
    pixels = np.frombuffer(o.decode_video_gop(video.tobytes(), 4), dtype=np.uint8)
    pixels = pixels.reshape(f, w * h * 3 // 2)[:, : w * h].reshape(f, h, w)
    y.setflags(write=False)
    return dict(y=y, stream=buf[: (end + 7) // 8], end=end, fb=[int(b) for b in fb], video=video, hb=hb, pixels=pixels)


def test_regrow_pframes():
    codec = Codec(0, _q(4), 4)
    try:
        for w, h, f, gop, merange in GOP_STEPS:
            e = _gop_case(w, h, f, gop, merange)
            for dev in (False, True):
                y = _dev(e["y"]) if dev else np.array(e["y"])
                for call in (codec.encode_gop, codec.encode_gop_groups):
                    out = _buf(codec.gop_stream_bound(w, h, f, merange), dev)
                    fb, end = call(y, w, h, out, gop, merange, nframes=f)
                    assert end == e["end"] and [int(b) for b in fb] == e["fb"], call.__name__
                    got = _host(out)
                    assert got[: len(e["stream"])].tobytes() == e["stream"].tobytes(), call.__name__
                    assert not got[len(e["stream"]):].any()
                pix = _buf(f * w * h, dev)
                src = _dev(e["video"]) if dev else np.array(e["video"])
                end = codec.decode_gop(src, w, h, pix, gop, merange, f, start_bit=e["hb"])
                assert (end + 7) // 8 == e["video"].size
                assert np.array_equal(_host(pix).reshape(f, h, w), e["pixels"])
    finally:
        codec.close()


def test_two_streams_closed_in_reverse_order(monkeypatch):
    """Two video streams open at once on one codec (gop 1 and gop 2, chunks of one group), pushed to
    alternately, finished and closed in the opposite order to opening; and a stream that was opened
    and never pushed to."""
    monkeypatch.setenv("IE_GOP_BATCH_MAX", "1")
    o, q = O.load(), _q(4)
    w, h, f = 48, 32, 6
    ya, yb = synth.frames("M", w, h, f, seed=41), synth.frames("P", w, h, f, seed=43)
    exp_a, end_a, fb_a = o.encode_blocks(ya, 4, q)
    exp_b, end_b, fb_b = o.encode_gop(yb, 4, q, 2, 4)
    codec = Codec(0, q, 4)
    try:
        a = codec.open_video_stream(w, h, max_frames=f)
        b = codec.open_video_stream(w, h, max_frames=f, gop=2, merange=4)
        idle = codec.open_video_stream(w, h, max_frames=f, gop=2, merange=4)
        out_a, out_b = np.zeros(a.cap, dtype=np.uint8), np.zeros(b.cap, dtype=np.uint8)
        got_a = got_b = 0
        for k in range(0, f, 2):
            a.push(ya[k:].ravel(), 2)
            b.push(yb[k:].ravel(), 2)
            got_a += a.pull(out_a, got_a)
            got_b += b.pull(out_b, got_b)
        idle.close()
        nb, end, fb = b.finish(out_b, got_b)
        assert end == end_b and [int(x) for x in fb] == [int(x) for x in fb_b]
        assert out_b[: got_b + nb].tobytes() == exp_b[: (end_b + 7) // 8].tobytes()
        b.close()
        nb, end, fb = a.finish(out_a, got_a)
        assert end == end_a and [int(x) for x in fb] == [int(x) for x in fb_a]
        assert out_a[: got_a + nb].tobytes() == exp_a[: (end_a + 7) // 8].tobytes()
        a.close()
    finally:
        codec.close()


def test_create_encode_close_twenty_times():
    o, q = O.load(), _q(4)
    y = synth.frame("M", 16, 16, seed=5)
    exp, eend, _ = o.encode_blocks(y, 4, q)
    for _ in range(20):
        codec = Codec(0)
        codec.set_quant(q, 4)
        out = np.zeros(stream_bound(16, 16, 4, 1), dtype=np.uint8)
        _, end = codec.encode_frames(y, 16, 16, out)
        codec.close()
    assert end == eend and out[: (eend + 7) // 8].tobytes() == exp[: (eend + 7) // 8].tobytes()
