"""ieh_decode_image_region (Codec.decode_image_file_region): the rectangle of an image file, with or
without the Huffman pass, against the crop of the existing file decode, and on one of the
reference-written golden files against the crop of the reference decoder's golden pixels."""
import ctypes as C
import os

import numpy as np
import pytest

from imageencoder_amd import IE_EINVAL, load_host_library, synth
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from imageencoder_amd import Codec
    return Codec(0)


def _rects(n, w, h):
    return [(0, 0, w, h), (3, 5, w // 2 + 1, h // 2 + 3), (w - 1, h - 1, 1, 1), (n + 1, n + 1, 2, 2),
            (w // 2 + 3, h // 2 + 1, w - (w // 2 + 3), h - (h // 2 + 1))]


@pytest.mark.parametrize("huffman", [True, False], ids=["huffman", "plain"])
@pytest.mark.parametrize("n", [4, 8])
def test_file_region_equals_the_crop_of_the_file_decode(codec, n, huffman):
    w, h = 200, 56
    q = O.read_matrix("matrix.txt" if n == 4 else "matrix8_1.txt", n)
    y = synth.frame("M", w, h, seed=5 + n)
    enc = codec.encode_image_file(y, w, h, q, n, rle=True, huffman=huffman)
    full = codec.decode_image_file(enc, n)
    assert np.array_equal(full, O.load().decode_image(enc, n))
    for x0, y0, rw, rh in _rects(n, w, h):
        got = codec.decode_image_file_region(enc, (x0, y0, rw, rh), n)
        assert got.shape == (rh, rw)
        assert np.array_equal(got, full[y0:y0 + rh, x0:x0 + rw]), (x0, y0, rw, rh)


def test_rectangle_outside_the_header_size(codec):
    n, w, h = 4, 64, 32
    q = O.read_matrix("matrix.txt", n)
    enc = np.frombuffer(codec.encode_image_file(synth.frame("U", w, h, seed=3), w, h, q, n), np.uint8).copy()
    H = load_host_library()
    for rect in ((60, 0, 8, 8), (0, 30, 4, 4), (-1, 0, 4, 4), (0, 0, 0, 1)):
        out = np.full(64, 0xA5, dtype=np.uint8)
        gw, gh = C.c_int(0), C.c_int(0)
        r = H.ieh_decode_image_region(codec.h, enc.ctypes.data, enc.size, n, *rect, out.ctypes.data, out.size, C.byref(gw),
                                      C.byref(gh))
        assert r == IE_EINVAL and (gw.value, gh.value) == (w, h)
        assert (out == 0xA5).all()


@pytest.mark.parametrize("name", ["synU256_4x4_huff", "synU200x56_8x8"])
def test_golden_file_region(codec, name):
    """A reference-written file (test_gpu_files.py decodes it whole) against the crop of the
    reference decoder's pixels."""
    c = next(c for c in O.manifest() if c["name"] == name)
    enc = O.case_expected(c)
    n, w, h = c["n"], c["w"], c["h"]
    ref = np.frombuffer(open(os.path.join(O.GOLDEN, c["dec_file"]), "rb").read(), np.uint8).reshape(h, w)
    for x0, y0, rw, rh in _rects(n, w, h):
        got = codec.decode_image_file_region(enc, (x0, y0, rw, rh), n)
        assert np.array_equal(got, ref[y0:y0 + rh, x0:x0 + rw]), (x0, y0, rw, rh)
