"""ieh_decode_image_scaled (Codec.decode_image_file_scaled): an image file at 1/scale of its size,
with or without the Huffman pass, on files the oracle wrote, against the box mean
(tests/scaled_common.py) of the existing file decode -- itself compared with the oracle's pixels."""
import ctypes as C

import numpy as np
import pytest

from imageencoder_amd import IE_ECAP, IE_EINVAL, load_host_library, synth
from tests import oracle_lib as O
from tests import scaled_common as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from imageencoder_amd import Codec
    return Codec(0)


def _file(n, w, h, huffman, kind="M"):
    q = O.read_matrix("matrix.txt" if n == 4 else "matrix8_1.txt", n)
    return O.load().encode_image(synth.frame(kind, w, h, seed=5 + n), n, q, rle=True, huffman=huffman)


@pytest.mark.parametrize("huffman", [True, False], ids=["huffman", "plain"])
@pytest.mark.parametrize("n", [4, 8])
def test_file_scaled_equals_the_box_mean_of_the_file_decode(codec, n, huffman):
    w, h = 200, 56
    enc = _file(n, w, h, huffman)
    full = codec.decode_image_file(enc, n)
    assert np.array_equal(full, O.load().decode_image(enc, n))
    for sc in SC.scales(n):
        got = codec.decode_image_file_scaled(enc, sc, n)
        assert got.shape == (h // sc, w // sc)
        assert np.array_equal(got, SC.box(full, sc)), sc


def test_bad_scale_and_short_cap(codec):
    n, w, h = 4, 64, 32
    enc = np.frombuffer(_file(n, w, h, True, "U"), np.uint8).copy()
    H = load_host_library()

    def raw(scale, cap):
        out = np.full(w * h, 0xA5, dtype=np.uint8)
        gw, gh = C.c_int(0), C.c_int(0)
        r = H.ieh_decode_image_scaled(codec.h, enc.ctypes.data, enc.size, n, scale, out.ctypes.data, cap, C.byref(gw),
                                      C.byref(gh))
        assert (gw.value, gh.value) == (w, h)  # the header's full size
        return r, out

    for scale in (0, -1, 3, 8, 16):
        r, out = raw(scale, w * h)
        assert r == IE_EINVAL and (out == 0xA5).all()
    r, out = raw(2, (w // 2) * (h // 2) - 1)
    assert r == IE_ECAP and (out == 0xA5).all()
    r, out = raw(2, (w // 2) * (h // 2))
    assert r == (w // 2) * (h // 2)
    full = codec.decode_image_file(enc.tobytes(), n)
    assert np.array_equal(out[:r].reshape(h // 2, w // 2), SC.box(full, 2))
    assert (out[r:] == 0xA5).all()
