"""GPU: ie_probe_sizes (Codec.probe_sizes) against the CPU oracle.  The truth for candidate m and
frame f is the frame_bits[f] of oracle.encode_blocks under that matrix; for a few candidates the
library's own encode_frames after set_quant is compared too.

Shapes are the smallest that reach each way the kernel can go wrong (a tile is 256 4x4 or 64 8x8
blocks, a wave's step four 4x4 blocks or one 8x8 block): one block / one partly filled step (4x4 and
8x8 pixels), 200 x 56 (ragged: three tiles, the last partial, a partial last step), 64 x 48 x 3 with
padded rows and frames (per-frame sums and addressing, aligned and byte-wise loads), 520 x 264 (34
workgroups whose atomics meet in one sum).  Contents: splitmix noise, a flat frame (all-zero blocks:
5-bit records), a gradient, and the rounding-tie frames of tests/matrix_sweep.py, where a wrong
division or rounding shows.  Candidates: every matrix of the sweep in one call."""
import numpy as np
import pytest

from imageencoder_amd import IE_EINVAL, MODE_EXACT, MODE_FAST, IEError, stream_bound, synth
from tests import matrix_sweep as MS
from tests.probe_common import base as _base
from tests.probe_common import codec, device_table, fresh_context_refuses  # noqa: F401

pytestmark = pytest.mark.gpu


def _candidates(n):
    return np.stack([q for _, q in MS.sweep(n)])


def _expected(oracle, y, n, qs, rle):
    """(nq, frames) payload bits from the oracle, one encode per candidate."""
    return np.stack([oracle.encode_blocks(y, n, q, rle)[2] for q in qs]).astype(np.uint64)


def _gradient(f, h, w):
    i, j, k = np.mgrid[0:f, 0:h, 0:w]
    return ((3 * j + 2 * k + 17 * i) % 256).astype(np.uint8)


def _contents(n, f, h, w):
    ties = [("tie_" + name, MS.tie_frames(n, MS.by_name(n, name), w, h, f, seed=1))
            for name in (("jpeg_like", "primes") if n == 4 else ("annex_k", "primes"))]
    return [("noise", np.stack([synth.frame("U", w, h, seed=40 + k) for k in range(f)])),
            ("flat", np.full((f, h, w), 128, dtype=np.uint8)), ("gradient", _gradient(f, h, w))] + ties


@pytest.mark.parametrize("rle", [True, False], ids=["rle", "norle"])
@pytest.mark.parametrize("n", [4, 8])
def test_every_sweep_matrix_ragged(codec, oracle, n, rle):
    """200 x 56, every matrix of the sweep in ONE call, every content; then three candidates against
    the library's own encode in both modes."""
    w, h = 200, 56
    qs = _candidates(n)
    assert 1 < len(qs) <= 64
    codec.set_quant(_base(n), n)
    for kind, y in _contents(n, 1, h, w):
        exp = _expected(oracle, y, n, qs, rle)
        got = codec.probe_sizes(y, w, h, qs, rle=rle)
        assert got.dtype == np.uint64 and got.shape == (len(qs), 1)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (kind, "candidate, frame:", bad[:4].tolist(), got[bad[0][0]], exp[bad[0][0]])
        if kind == "flat":  # every block quantises to zeros under most matrices: 5 bits with RLE
            blocks = (w // n) * (h // n)
            assert (exp == (5 if rle else 4 + n * n) * blocks).any()
    y = _contents(n, 1, h, w)[-1][1]
    got = codec.probe_sizes(y, w, h, qs, rle=rle)
    for m in (0, 2, len(qs) - 1):
        codec.set_quant(qs[m], n)
        for mode in (MODE_FAST, MODE_EXACT):
            out = np.zeros(stream_bound(w, h, n), dtype=np.uint8)
            fb, _ = codec.encode_frames(y, w, h, out, rle=rle, mode=mode)
            assert fb[0] == got[m, 0], (m, mode)


@pytest.mark.parametrize("n,w,h", [(4, 4, 4), (4, 8, 8), (8, 8, 8)])
def test_one_block_and_one_partial_step(codec, oracle, n, w, h):
    qs = _candidates(n)
    codec.set_quant(_base(n), n)
    for kind, y in _contents(n, 1, h, w):
        for rle in (True, False):
            np.testing.assert_array_equal(codec.probe_sizes(y, w, h, qs, rle=rle), _expected(oracle, y, n, qs, rle),
                                          err_msg=f"{kind} rle={rle}")


@pytest.mark.parametrize("pad", [12, 13], ids=["stride+12", "stride+13"])
@pytest.mark.parametrize("n", [4, 8])
def test_frames_with_padded_rows_and_frames(codec, oracle, n, pad):
    """64 x 48 x 3, stride = w + pad (12: 4-byte row loads; 13: byte loads), padded frame_pitch;
    host and device y, host and device bits -- all four give the oracle's per-frame sums."""
    import torch
    w, h, f = 64, 48, 3
    stride, pitch = w + pad, (w + pad) * h + 4 * 37 + (pad - 12)
    qs = _candidates(n)
    codec.set_quant(_base(n), n)
    for kind, y in _contents(n, f, h, w)[:1] + _contents(n, f, h, w)[-1:]:
        buf = np.full(f * pitch, 0xA5, dtype=np.uint8)
        for k in range(f):
            rows = buf[k * pitch: k * pitch + h * stride].reshape(h, stride)
            rows[:, :w] = y[k]
        exp = _expected(oracle, y, n, qs, True)
        dbuf = torch.from_numpy(buf).cuda()
        for src in (buf, dbuf):
            got = codec.probe_sizes(src, w, h, qs, nframes=f, stride=stride, frame_pitch=pitch)
            np.testing.assert_array_equal(got, exp, err_msg=f"{kind} host bits")
            dev = torch.full((len(qs) * f,), -1, dtype=torch.int64, device="cuda")
            assert codec.probe_sizes(src, w, h, qs, nframes=f, stride=stride, frame_pitch=pitch, out=dev) is dev
            codec.sync()
            np.testing.assert_array_equal(device_table(dev, len(qs), f), exp, err_msg=f"{kind} device bits")


@pytest.mark.parametrize("n", [4, 8])
def test_many_workgroups_add_into_one_sum(codec, oracle, n):
    """520 x 264: 34 tiles; four candidates keep the oracle quick."""
    import torch
    w, h = 520, 264
    qs = _candidates(n)[[0, 1, 3, -1]]
    codec.set_quant(_base(n), n)
    for y in (synth.frame("U", w, h, seed=7)[None], MS.tie_frames(n, qs[0], w, h, 1, seed=3)):
        for rle in (True, False):
            exp = _expected(oracle, y, n, qs, rle)
            np.testing.assert_array_equal(codec.probe_sizes(torch.from_numpy(y).cuda(), w, h, qs, rle=rle), exp)


def test_candidate_count_boundaries(codec, oracle):
    n, w, h = 4, 64, 48
    y = synth.frame("U", w, h, seed=5)[None]
    codec.set_quant(_base(n), n)
    from imageencoder_amd import scale_matrix
    q64 = np.stack([scale_matrix(_base(n), 30 + 7 * k) for k in range(64)])
    exp = _expected(oracle, y, n, q64, True)
    np.testing.assert_array_equal(codec.probe_sizes(y, w, h, q64), exp)            # nq = 64
    np.testing.assert_array_equal(codec.probe_sizes(y, w, h, q64[5:6]), exp[5:6])  # nq = 1
    with pytest.raises(IEError) as e:
        codec.probe_sizes(y, w, h, np.concatenate([q64, q64[:1]]))                 # nq = 65
    assert e.value.code == IE_EINVAL
    bad = q64[:4].copy()
    bad[2, 9] = 0
    with pytest.raises(IEError) as e:
        codec.probe_sizes(y, w, h, bad)
    assert e.value.code == IE_EINVAL and "matrix 2" in str(e.value)
    with pytest.raises(IEError) as e:  # the checks of encode_frames, with their codes
        codec.probe_sizes(y, w + 2, h, q64[:1])
    assert e.value.code == IE_EINVAL


def test_fresh_context_has_no_block_size():
    fresh_context_refuses(lambda c: c.probe_sizes(np.zeros((8, 8), dtype=np.uint8), 8, 8, np.ones((1, 16), dtype=np.uint16)))


@pytest.mark.parametrize("n", [4, 8])
def test_probe_leaves_the_context_untouched(codec, n):
    """encode, probe, encode: the two streams, the two cos_table read-backs and the two fallback
    counts are identical."""
    w, h = 200, 56
    q = _base(n)
    y = MS.tie_frames(n, q, w, h, 1, seed=1)
    codec.set_quant(q, n)

    def encode():
        out = np.zeros(stream_bound(w, h, n), dtype=np.uint8)
        fb, end = codec.encode_frames(y, w, h, out)
        return out.tobytes(), int(fb[0]), end, codec.last_fallbacks(), codec.cos_table().tobytes()

    before = encode()
    got = codec.probe_sizes(y, w, h, _candidates(n))
    after = encode()
    assert before == after
    assert before[3] > 0  # the tie frame does ask for FP64 evaluations
    assert got[0, 0] == before[1]  # candidate 0 is the context's own matrix
