"""The device P-frame decoders on valid videos that no encoder here writes (tests/crafted_videos.py).

Every entry of the table goes through
  * ie_decode_gop with motion compensation on and off: a host stream to host frames and a device
    stream to device frames, rows W + 32 apart, frames a YUV frame apart, into a destination filled
    with 0x5A -- the Y rows equal the oracle's, every other byte is untouched, the end bit is the
    builder's;
  * the file decoder (Codec.decode_video_file): the oracle's bytes, the header's dimensions and the
    md5 of the REFERENCE's own decode (tests/golden/manifest_crafted_video.json);
and one entry per family through ie_vdec (Codec.open_video_decode) in chunks of 1, 2 and 3 frames (a
P-frame opens a chunk and copies from the other slot) and in one chunk.  Two entries are cut inside
a P-frame's vectors and inside its records: IE_EFORMAT with the message of the place, after which
the same context decodes the whole file.  tests/test_crafted_videos.py shows on the CPU that the
oracle equals the reference on every entry and that the entries reach what they are named for.
The oracle's pixels are computed once per entry and setting, and shared.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import crafted_videos as CV
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

MANIFEST = {m["name"]: m for m in json.load(open(os.path.join(O.GOLDEN, "manifest_crafted_video.json")))}
FILL = 0x5A
NAMES = [e.name for e in CV.entries()]
# one entry per family for the streamed decoder
VDEC = ["vec_extremes_rle", "vec_widths_32767", "vec_phase_32767_7", "dense_c_norle_every37", "long_rle",
        "saturate_checker", "groups_gop3", "geometry_16x16_m1", "gop_case"]
TRUNCATED = ["vec_widths_32767", "dense_c_norle_every37"]
_REF = {}
_GOP = {}


@pytest.fixture(scope="module")
def codec():
    from imageencoder_amd import Codec
    c = Codec(0, CV.entries()[0].q, CV.N)
    yield c
    c.close()


def _ref(e, mc) -> np.ndarray:
    """[frames][h * w * 3 / 2] of the oracle's decode: Y, then the 0x80 fill."""
    if (e.name, mc) not in _REF:
        out = np.frombuffer(O.load().decode_video_gop(e.data, CV.N, bool(mc)), dtype=np.uint8)
        out = out.reshape(e.frames, e.w * e.h * 3 // 2).copy()
        out.setflags(write=False)
        _REF[e.name, mc] = out
    return _REF[e.name, mc]


def _ref_y(e, mc) -> np.ndarray:
    return _ref(e, mc)[:, : e.w * e.h].reshape(e.frames, e.h, e.w)


def _start(e) -> int:
    return e.file()[1][0]["start"]  # the header's length


def _same_frames(e, got, want, route):
    got, want = np.asarray(got).reshape(want.shape), np.asarray(want)
    if not np.array_equal(got, want):
        f = int(np.argmax((got != want).reshape(e.frames, -1).any(axis=1)))
        bad = (got[f] != want[f]).reshape(e.h // 16, 16, e.w // 16, 16).any(axis=(1, 3)).ravel()
        k = int(np.argmax(bad))
        vec = e.frame_list()[f][0]
        raise AssertionError(f"{e.name} [{route}]: frame {f} ({'I' if f % e.gop == 0 else 'P'}), {int(bad.sum())} of "
                             f"{bad.size} macroblocks differ, first {k} (vector {vec[k] if vec else None})")


def _decode_gop(codec, e, mc, data=None):
    """ie_decode_gop into tight host frames: [frames][h][w]."""
    codec.set_quant(e.q, CV.N)
    out = np.full(e.frames * e.w * e.h, FILL, dtype=np.uint8)
    end = codec.decode_gop(np.frombuffer(e.data if data is None else data, dtype=np.uint8).copy(), e.w, e.h, out, e.gop,
                           e.merange, e.frames, start_bit=_start(e), rle=e.rle, motioncomp=bool(mc))
    return out.reshape(e.frames, e.h, e.w), end


# ------------------------------------------------------------------ 1. ie_decode_gop
@pytest.mark.parametrize("mc", [1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_decode_gop(codec, name, mc):
    import torch
    e = CV.by_name(name)
    codec.set_quant(e.q, CV.N)
    want = _ref_y(e, mc)
    stride = e.w + 32
    pitch = stride * e.h * 3 // 2  # a YUV frame of padded rows
    exp = np.full(e.frames * pitch, FILL, dtype=np.uint8)
    for f in range(e.frames):
        exp[f * pitch: f * pitch + stride * e.h].reshape(e.h, stride)[:, : e.w] = want[f]
    src = np.frombuffer(e.data, dtype=np.uint8).copy()
    for route in ("host", "device"):
        if route == "host":
            stream, dst = src, np.full(e.frames * pitch, FILL, dtype=np.uint8)
        else:
            stream = torch.from_numpy(src).cuda()
            dst = torch.full((e.frames * pitch,), FILL, dtype=torch.uint8, device="cuda")
        end = codec.decode_gop(stream, e.w, e.h, dst, e.gop, e.merange, e.frames, start_bit=_start(e), stride=stride,
                               frame_pitch=pitch, rle=e.rle, motioncomp=bool(mc))
        got = dst if route == "host" else dst.cpu().numpy()
        rows = np.stack([got[f * pitch: f * pitch + stride * e.h].reshape(e.h, stride)[:, : e.w] for f in range(e.frames)])
        _same_frames(e, rows, want, f"ie_decode_gop, {route}, motioncomp {mc}")
        assert np.array_equal(got, exp), f"{name} [{route}]: bytes between the rows or frames were written"
        assert end == e.end_bit, (name, route)
        if e.family in ("dense", "long"):  # more than one chunk per frame, as many as the plan restated
            assert codec.last_decode_info()[0] > 1
            assert codec.last_decode_info()[0] == CV.planned_chunk_bits(e)[1]


# ------------------------------------------------------------------ 2. ie_vdec
def _gop_frames(codec, e, mc):
    if (e.name, mc) not in _GOP:
        got, end = _decode_gop(codec, e, mc)
        assert end == e.end_bit
        got.setflags(write=False)
        _GOP[e.name, mc] = got
    return _GOP[e.name, mc]


@pytest.mark.parametrize("mc", [1, 0])
@pytest.mark.parametrize("chunk", [1, 2, 3, 100])
@pytest.mark.parametrize("name", VDEC)
def test_vdec_chunks(codec, name, chunk, mc):
    e = CV.by_name(name)
    want = _gop_frames(codec, e, mc)
    codec.set_quant(e.q, CV.N)
    fb = e.w * e.h
    out = np.full(e.frames * fb, FILL, dtype=np.uint8)
    vd = codec.open_video_decode(np.frombuffer(e.data, dtype=np.uint8).copy(), e.w, e.h, e.frames, gop=e.gop,
                                 merange=e.merange, start_bit=_start(e), rle=e.rle, motioncomp=bool(mc), chunk_frames=chunk)
    try:
        done = 0
        while done < e.frames:
            got = vd.next(out[done * fb:], 2)
            assert got > 0
            done += got
        assert vd.next(out, 1) == 0
        assert vd.info()["end_bit"] == e.end_bit
    finally:
        vd.close()
    _same_frames(e, out, want, f"ie_vdec, chunks of {chunk}, motioncomp {mc}")
    _same_frames(e, out, _ref_y(e, mc), f"ie_vdec against the oracle, chunks of {chunk}, motioncomp {mc}")


def test_vdec_covers_every_family():
    assert {CV.by_name(n).family for n in VDEC} == set(CV.FAMILIES)


# ------------------------------------------------------------------ 3. the file decoder
@pytest.mark.parametrize("name", NAMES)
def test_decode_video_file(codec, name):
    e = CV.by_name(name)
    got, (w, h, f) = codec.decode_video_file(e.data, CV.N)
    assert (w, h, f) == (e.w, e.h, e.frames)
    want = _ref(e, 1)
    _same_frames(e, got.reshape(f, -1)[:, : w * h], _ref_y(e, 1), "decode_video_file")
    assert np.array_equal(got.reshape(f, -1), want)
    assert hashlib.md5(got.tobytes()).hexdigest() == MANIFEST[name]["dec1_md5"], "reference md5"


# ------------------------------------------------------------------ 4. truncation
def _cut(e, f, where) -> int:
    """Bytes to keep so that the stream ends inside P-frame f's vector field / inside its records
    (from the builder's positions; the frame itself starts inside what is kept)."""
    fp = e.file()[1][f]
    nbytes = (fp["vec"][e.nmb // 2] if where == "vectors" else fp["rec"][e.nblocks // 2]) // 8
    assert fp["start"] < 8 * nbytes
    if where == "vectors":
        assert 8 * nbytes < fp["rec"][0]
    else:
        assert fp["rec"][0] < 8 * nbytes < fp["end"] - 8
    return nbytes


@pytest.mark.parametrize("where,msg", [("vectors", "stream ends in the motion vectors"),
                                      ("records", "stream ends before the last block")])
@pytest.mark.parametrize("f", [1, 2])
@pytest.mark.parametrize("name", TRUNCATED)
def test_truncated_decode_gop(codec, name, f, where, msg):
    from imageencoder_amd import IE_EFORMAT, IEError
    e = CV.by_name(name)
    assert f % e.gop
    with pytest.raises(IEError, match=msg) as err:
        _decode_gop(codec, e, 1, e.data[: _cut(e, f, where)])
    assert err.value.code == IE_EFORMAT
    got, end = _decode_gop(codec, e, 1)  # the same context, the whole file
    _same_frames(e, got, _ref_y(e, 1), "ie_decode_gop after a truncated stream")
    assert end == e.end_bit


@pytest.mark.parametrize("where,msg", [("vectors", "stream ends in the motion vectors"),
                                      ("records", "stream ends before the last block")])
@pytest.mark.parametrize("f", [1, 2])
@pytest.mark.parametrize("name", TRUNCATED)
def test_truncated_vdec(codec, name, f, where, msg):
    from imageencoder_amd import IE_EFORMAT, IEError
    e = CV.by_name(name)
    codec.set_quant(e.q, CV.N)
    fb = e.w * e.h
    want = _ref_y(e, 1)

    def run(data):
        out = np.full(e.frames * fb, FILL, dtype=np.uint8)
        vd = codec.open_video_decode(np.frombuffer(data, dtype=np.uint8).copy(), e.w, e.h, e.frames, gop=e.gop,
                                     merange=e.merange, start_bit=_start(e), rle=e.rle, chunk_frames=2)
        done = 0
        try:
            while done < e.frames:
                try:
                    done += vd.next(out[done * fb:], e.frames)
                except IEError as x:
                    done += x.got
                    raise
        finally:
            vd.close()
            run.done, run.out = done, out
        return out

    with pytest.raises(IEError, match=msg) as err:
        run(e.data[: _cut(e, f, where)])
    assert err.value.code == IE_EFORMAT and run.done == f  # the whole frames before the cut came out
    assert np.array_equal(run.out[: f * fb].reshape(f, e.h, e.w), want[:f]) and (run.out[f * fb:] == FILL).all()
    _same_frames(e, run(e.data), want, "ie_vdec after a truncated stream")
