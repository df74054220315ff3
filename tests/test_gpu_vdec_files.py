"""The file and command-line layers over the streamed video decode: Codec.iter_video_file
(ieh_vdec_open / next / close) and the `decoder` command line, which writes its output as the chunks
arrive.  Expected bytes are the CPU oracle's: the files come from O.load().encode_video_gop, the
frames from O.load().decode_video_gop -- Y, then w*h/2 bytes of 0x80 per frame.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from imageencoder_amd import IE_EFORMAT, IEError, synth
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 29
BIN = os.path.join(O.ROOT, "imageencoder_amd", "lib")
W, H, F = 48, 32, 7
# (huffman, gop, merange)
FILES = [(False, 1, 0), (True, 1, 0), (False, 3, 8), (True, 3, 8)]
IDS = [f"{'huff' if hf else 'plain'}-gop{g}" for hf, g, _ in FILES]


@pytest.fixture(scope="module")
def codec():
    from imageencoder_amd import Codec
    c = Codec(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _file(huffman, gop, merange):
    y = synth.frames("P", W, H, F, SEED)
    q = O.read_matrix("matrix.txt", 4)
    return O.load().encode_video_gop(synth.yuv420(y), W, H, 4, q, huffman=huffman, gop=gop, merange=merange)


@functools.lru_cache(maxsize=None)
def _decoded(huffman, gop, merange, mc):
    return O.load().decode_video_gop(_file(huffman, gop, merange), 4, mc)


@pytest.mark.parametrize("chunk", [0, 1, 3, 100])
@pytest.mark.parametrize("mc", [True, False], ids=["motioncomp", "no-motioncomp"])
@pytest.mark.parametrize("huffman,gop,merange", FILES, ids=IDS)
def test_iter_video_file(codec, huffman, gop, merange, mc, chunk):
    want = _decoded(huffman, gop, merange, mc)
    pitch = W * H * 3 // 2
    parts, counts = [], []
    for nf, frames in codec.iter_video_file(_file(huffman, gop, merange), 4, motioncomp=mc, chunk_frames=chunk):
        assert frames.size == nf * pitch
        assert (frames.reshape(nf, pitch)[:, W * H:] == 0x80).all()
        counts.append(nf)
        parts.append(frames.tobytes())
    assert b"".join(parts) == want and sum(counts) == F
    if 0 < chunk < F:
        assert counts == [chunk] * (F // chunk) + ([F % chunk] if F % chunk else [])
    # the whole-file decoder gives the same bytes (second check)
    if mc and chunk == 3:
        assert codec.decode_video_file(_file(huffman, gop, merange), 4)[0].tobytes() == want


def test_iter_video_file_truncated(codec):
    """A file cut inside frame 4: the frames before it, then IE_EFORMAT."""
    enc = _file(False, 3, 8)
    y = synth.frames("P", W, H, F, SEED)
    q = O.read_matrix("matrix.txt", 4)
    _, hb = O.load().header(4, q, True, W, H, video=True, frames=F, gop=3, merange=8)
    _, _, fb = O.load().encode_gop(y, 4, q, 3, 8, start_bit=hb)
    cut = (hb + int(fb[:4].sum()) + int(fb[4]) // 2) // 8
    want = _decoded(False, 3, 8, True)
    pitch = W * H * 3 // 2
    got = []
    with pytest.raises(IEError, match="stream ends") as e:
        for nf, frames in codec.iter_video_file(enc[:cut], 4, chunk_frames=3):
            got.append(frames.tobytes())
    assert e.value.code == IE_EFORMAT
    assert b"".join(got) == want[: 3 * pitch]  # (whole chunks before the one the stream ends in)


# ------------------------------------------------------------------------------- the command line
def _decoder(work, enc, mc, env):
    exe = os.path.join(BIN, "decoder")
    assert os.path.exists(exe), "decoder not built"
    with open(os.path.join(work, "v.enc"), "wb") as f:
        f.write(enc)
    conf = os.path.join(work, "set.conf")
    with open(conf, "w") as f:
        f.write(f"encfile=v.enc\ndecfile=v.dec\nmotioncompensation={int(mc)}\n")
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([exe, conf], cwd=work, capture_output=True, text=True, timeout=120, env=e)


# IE_CHUNK_MB so small that a chunk is one frame (7 chunks), two frames, or the default (one chunk)
CHUNK_MB = {"1-frame": str(W * H / 1048576.0), "2-frames": str(2 * W * H / 1048576.0), "default": None}


@pytest.mark.parametrize("chunk", sorted(CHUNK_MB))
@pytest.mark.parametrize("mc", [1, 0])
@pytest.mark.parametrize("huffman,gop,merange", FILES, ids=IDS)
def test_decoder_cli_streams_the_same_bytes(tmp_path, huffman, gop, merange, mc, chunk):
    env = {"IE_CHUNK_MB": CHUNK_MB[chunk]} if CHUNK_MB[chunk] else {}
    r = _decoder(str(tmp_path), _file(huffman, gop, merange), mc, env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Saved file at: v.dec" in r.stdout
    assert (tmp_path / "v.dec").read_bytes() == _decoded(huffman, gop, merange, bool(mc))


@pytest.mark.parametrize("gop,merange", [(1, 0), (3, 8)])
def test_decoder_cli_truncated_file_leaves_no_output(tmp_path, gop, merange):
    """A truncated file: the same exit code (0, the reference's) and message as before, and no
    output file -- the chunks already written are removed."""
    enc = _file(False, gop, merange)
    r = _decoder(str(tmp_path), enc[: len(enc) * 2 // 3], 1, {"IE_CHUNK_MB": CHUNK_MB["1-frame"]})
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Error processing raw video for decoding! stream ends" in r.stdout
    assert not (tmp_path / "v.dec").exists()
