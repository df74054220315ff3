"""P-frame videos through the host library's two paths: the `encoder` command line, which streams
the .yuv file through a gop > 1 ie_vstream (IE_CHUNK_MB small enough for several chunks of one
group and one frame per read), and Codec.encode_video_file on an in-memory buffer, which encodes
the groups of pictures side by side (ie_encode_gop_groups).  Both write the reference's golden
file; with the Huffman pass on, the file is the oracle's, and Huffman-decoded it holds the golden's
bits behind the leading '0' bit that only a file without the pass carries (ImageEncoder.cpp:84-86).
"""
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

BIN = os.path.join(O.ROOT, "imageencoder_amd", "lib")
# groups of 2, 2, 1 and of 3, 2 frames, 3072 pixels a frame
CASES = ["gopM64x48x5_g2_m1", "gopP64x48x5_g3_m8"]


def _case(name):
    return next(c for c in O.manifest_gop() if c["name"] == name)


def _golden_bits_after_flag(c):
    return np.unpackbits(np.frombuffer(O.case_expected(c), dtype=np.uint8))[1:]


def _check_huffman_file(c, got):
    q = O.read_matrix(c["matrix"], c["n"])
    assert got == O.load().encode_video_gop(O.case_input(c), c["w"], c["h"], c["n"], q, rle=c["rle"], huffman=True,
                                            gop=c["gop"], merange=c["merange"])
    dec, passthrough = O.load().huffman_decode(got)
    assert not passthrough
    bits, want = np.unpackbits(np.frombuffer(dec, dtype=np.uint8)), _golden_bits_after_flag(c)
    # (the two streams end one bit apart, so their last bytes' padding differs: every bit before it)
    n = min(bits.size, want.size) - 8
    assert abs(bits.size - want.size) < 16 and (bits[:n] == want[:n]).all()


@pytest.mark.parametrize("huffman", [False, True], ids=["nohuff", "huff"])
@pytest.mark.parametrize("name", CASES)
def test_encoder_cli_streams_pframe_video(tmp_path, name, huffman):
    exe = os.path.join(BIN, "encoder" if huffman else "encoder_nohuff")
    assert os.path.exists(exe), "encoder not built"
    c = _case(name)
    for m in ("matrix.txt", "matrix4_2.txt"):
        (tmp_path / m).write_bytes(open(os.path.join(O.GOLDEN, m), "rb").read())
    (tmp_path / "in.yuv").write_bytes(O.case_input(c))
    conf = tmp_path / "set.conf"
    conf.write_text("".join(f"{k}={v}\n" for k, v in dict(
        rawfile="in.yuv", encfile="v.enc", decfile="v.dec", width=c["w"], height=c["h"], rle=c["rle"],
        quantfile=c["matrix"], logfile="", gop=c["gop"], merange=c["merange"]).items()))
    # 5 KiB: one frame per read and push, one group per chunk (the variable goes to the child only)
    env = dict(os.environ, IE_CHUNK_MB="0.005")
    r = subprocess.run([exe, str(conf)], cwd=str(tmp_path), capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = (tmp_path / "v.enc").read_bytes()
    if huffman:
        _check_huffman_file(c, got)
    else:
        assert got == O.case_expected(c)


@pytest.mark.parametrize("huffman", [False, True], ids=["nohuff", "huff"])
@pytest.mark.parametrize("name", CASES)
def test_encode_video_file_in_memory(name, huffman):
    from imageencoder_amd import Codec
    c = _case(name)
    q = O.read_matrix(c["matrix"], c["n"])
    codec = Codec(0, q, c["n"])
    try:
        yuv = np.frombuffer(O.case_input(c), dtype=np.uint8)
        got = codec.encode_video_file(yuv, c["w"], c["h"], q, c["n"], rle=bool(c["rle"]), huffman=huffman,
                                      merange=c["merange"], gop=c["gop"])
    finally:
        codec.close()
    if huffman:
        _check_huffman_file(c, got)
    else:
        assert got == O.case_expected(c)
