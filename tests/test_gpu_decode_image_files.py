"""ieh_decode_images (Codec.decode_image_files): a batch of image files decoded with the decoded
Huffman streams staying on the device -- one ie_huffman_decode_batch call into device slots, one
ie_decode_images call that reads them in place -- against the CPU oracle's decode of every file and
the single-file codec.decode_image_file.  Bit-exact is the bar for every pixel.

The files are the oracle encoder's (Huffman pass on); a file the pass gains nothing on carries no
dictionary and takes the passthrough route.
"""
import numpy as np
import pytest

from imageencoder_amd import IE_EFORMAT, IE_EINVAL, IEError, synth
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

W, H = 64, 48
_STATE = {}


def _codec():
    if "codec" not in _STATE:
        from imageencoder_amd import Codec
        _STATE["codec"] = Codec(0)
    return _STATE["codec"]


def _q(n):
    return O.read_matrix("matrix.txt" if n == 4 else "matrix8_1.txt", n)


def _images(w=W, h=H):
    """Five pictures of differing content, so that the dictionaries and the lengths differ: noise,
    a flat tile, 16 x 16 squares of differing grey, a constant and a ramp.  (At this size the
    Huffman pass gains nothing on the noise at 4 x 4, nor on the squares at 8 x 8: that file
    carries no dictionary and the batch is a mixed one.)"""
    yy, xx = np.mgrid[0:h, 0:w]
    squares = np.repeat(np.repeat(synth.uniform(w // 16, h // 16, seed=14), 16, axis=0), 16, axis=1)
    ramp = (((xx + 2 * yy) * 255) // (w + 2 * h)).astype(np.uint8)
    return [synth.frame("U", w, h, seed=11), synth.frame("M", w, h, seed=12), squares,
            np.full((h, w), 200, dtype=np.uint8), ramp]


def _files(n, rle=True, w=W, h=H):
    """(files, the oracle's pixels) of the five pictures: computed once per setting."""
    key = (n, rle, w, h)
    if key not in _STATE:
        o = O.load()
        files = [o.encode_image(y, n, _q(n), rle=rle, huffman=True) for y in _images(w, h)]
        ref = [np.asarray(o.decode_image(f, n)).reshape(h, w) for f in files]
        _STATE[key] = (files, ref)
    return _STATE[key]


def _passthrough_file(n, w=W, h=H):
    """A file of uniform noise under an all-ones matrix, on which the Huffman pass gains nothing."""
    key = ("pass", n, w, h)
    if key not in _STATE:
        o, c = O.load(), _codec()
        ones = np.ones(n * n, dtype=np.uint16)
        found = None
        for seed in range(40, 48):
            f = o.encode_image(synth.frame("U", w, h, seed=seed), n, ones, rle=True, huffman=True)
            if c.huffman_table(f) is None:
                found = f
                break
        _STATE[key] = found
    return _STATE[key]


def _check(files, ref, n):
    c = _codec()
    got = c.decode_image_files(files, n)
    assert got.shape == (len(files),) + ref[0].shape and got.dtype == np.uint8
    for k, f in enumerate(files):
        assert np.array_equal(got[k], ref[k]), k
        assert np.array_equal(got[k], c.decode_image_file(f, n)), k


@pytest.mark.parametrize("n", [4, 8])
def test_five_images(n):
    files, ref = _files(n)
    c = _codec()
    tabs = [c.huffman_table(f) for f in files]
    coded = [t for t in tabs if t is not None]
    assert len(coded) >= 4  # Huffman-coded files,
    assert len({t[1] for t in coded}) == len(coded) and len({len(f) for f in files}) > 1  # each with its own dictionary
    _check(files, ref, n)


def test_rle_off():
    files, ref = _files(4, rle=False)
    _check(files, ref, 4)


def test_mixed_batch_with_a_passthrough_file():
    n = 4
    o = O.load()
    p = _passthrough_file(n)
    assert p is not None, "no candidate file came out of the Huffman pass without a dictionary"
    assert _codec().huffman_table(p) is None
    ones = np.ones(n * n, dtype=np.uint16)
    # the coded files of the batch carry the same settings: the all-ones matrix
    coded = [o.encode_image(y, n, ones, rle=True, huffman=True) for y in _images()[1:4]]  # tile, squares, constant
    assert all(_codec().huffman_table(f) is not None for f in coded)
    files = [coded[0], p, coded[1], coded[2]]  # (neither group's files are adjacent)
    ref = [np.asarray(o.decode_image(f, n)).reshape(H, W) for f in files]
    _check(files, ref, n)
    _check([p, p], [ref[1], ref[1]], n)
    _check([p, coded[0]], [ref[1], ref[0]], n)


def test_a_differing_setting_names_the_file():
    n = 4
    files, _ = _files(n)
    other = O.load().encode_image(synth.frame("M", W + 16, H, seed=21), n, _q(n), rle=True, huffman=True)
    with pytest.raises(IEError) as e:
        _codec().decode_image_files([files[0], files[1], other, files[2]], n)
    assert e.value.code == IE_EINVAL and "file 2" in str(e.value), e.value


def test_a_truncated_file_names_the_file():
    n = 4
    files, _ = _files(n)
    assert _codec().huffman_table(files[4])[1] < 8 * (len(files[4]) * 2 // 3)  # (the cut leaves the dictionary whole)
    cut = files[4][: len(files[4]) * 2 // 3]
    with pytest.raises(IEError) as e:
        _codec().decode_image_files([files[1], cut, files[2]], n)
    assert e.value.code == IE_EFORMAT and "file 1" in str(e.value), e.value
