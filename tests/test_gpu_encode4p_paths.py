"""GPU parity of the wave-local 4x4 FAST encoder's less travelled paths: the multi-round FP64
fix-up (more than 64 requests in a wave), waves without requests beside dense ones, whole-block
requests, the slot-pair fallback with the two-coefficient record form, RLE off, the counting
instantiation and a partial last tile.  Every case compares the FAST stream and end bits with
EXACT mode and with the CPU oracle, bit for bit, and checks the request statistic where the
construction fixes it.  Shapes are the smallest that reach each path (a wave is 256 consecutive
blocks of a frame, a tile 1024).
"""
import numpy as np
import pytest

from imageencoder_amd import MODE_EXACT, MODE_FAST, stream_bound
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

N = 4
WAVE_BLOCKS = 256


@pytest.fixture(scope="module")
def codec():
    from imageencoder_amd import Codec
    return Codec(0)


def _tie_matrix():
    """q = 1 at the structural coefficients (0,2), (2,0), (2,2) -- natural indices 2, 8, 10: their
    quotient is J/4 for an integer pixel sum J, a rounding tie whenever J = 2 (mod 4), so about a
    quarter of them ask for the FP64 evaluation."""
    q = np.full(N * N, 16, dtype=np.uint16)
    q[[2, 8, 10]] = 1
    return q


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _encode(codec, oracle, y, q, rle=True, start_bit=5):
    """FAST and EXACT streams of the frames y ([f,] h, w) against the oracle's; returns the FAST
    run's (stream bytes, per-frame bits, end bit, FP64 requests)."""
    y = np.ascontiguousarray(y if y.ndim == 3 else y[None])
    f, h, w = y.shape
    codec.set_quant(q, N)
    exp, eend, efb = oracle.encode_blocks(y, N, q, rle, start_bit)
    nb = (eend + 7) // 8
    got = {}
    for mode in (MODE_FAST, MODE_EXACT):
        out = np.zeros(stream_bound(w, h, N, f, start_bit), dtype=np.uint8)
        fb, end = codec.encode_frames(y, w, h, out, start_bit=start_bit, nframes=f, rle=rle, mode=mode)
        if mode == MODE_FAST:
            got["req"] = codec.last_fallbacks()
        assert end == eend and np.array_equal(fb, efb), (mode, end, eend)
        assert out[:nb].tobytes() == exp[:nb].tobytes(), mode
    return exp[:nb].tobytes(), efb, eend, got["req"]


def _waves(y):
    """Non-empty waves of the launch: 256-block runs of every frame."""
    f, h, w = (1,) + y.shape if y.ndim == 2 else y.shape
    return f * -(-(w // N) * (h // N) // WAVE_BLOCKS)


@pytest.mark.parametrize("w,h,f", [(128, 32, 1), (256, 48, 3)], ids=["one_wave", "three_tile_chain"])
def test_dense_structural_ties_take_several_rounds(codec, oracle, w, h, f):
    """More than 64 requests in a wave: the fix-up runs its range-checked rounds.  128 x 32 is one
    wave of one tile; three frames of 256 x 48 are three tiles of three waves in one chain, whose
    records share words across waves and tiles."""
    y = _noise((f, h, w), 11)
    _, _, _, req = _encode(codec, oracle, y, _tie_matrix())
    # pigeonhole: more requests than 64 per wave puts more than 64 into at least one wave
    assert req > 64 * _waves(y), (req, _waves(y))


@pytest.mark.parametrize("split", ["left_right", "top_bottom"])
def test_wave_without_requests_beside_dense_waves(codec, oracle, split):
    """One half constant (no request in its blocks), the other noise, one tile.  left_right: every
    wave holds slots without a request beside dense ones; top_bottom: waves 0 and 1 have no request
    at all, waves 2 and 3 many.  The statistic is additive over blocks, so it equals the noise
    half's own."""
    h, w = 32, 512
    y = np.full((h, w), 128, dtype=np.uint8)
    half = (slice(None), slice(w // 2, None)) if split == "left_right" else (slice(h // 2, None), slice(None))
    y[half] = _noise(y[half].shape, 12)
    q = _tie_matrix()
    _, _, _, req = _encode(codec, oracle, y, q)
    _, _, _, req_flat = _encode(codec, oracle, np.full((h, w), 128, dtype=np.uint8), q)
    _, _, _, req_noise = _encode(codec, oracle, y[half], q)
    assert req_flat == 0
    assert req == req_noise and req > 0


def test_sparse_ties_take_one_round(codec, oracle):
    """The reference matrix on noise at one tile: few requests per wave (the single-round fix-up
    with its slot-by-slot read-back) and narrow records (the four-coefficient fields)."""
    y = _noise((64, 256), 13)
    _, _, _, req = _encode(codec, oracle, y, O.read_matrix("matrix.txt", N))
    assert 0 < req <= 64 * _waves(y)


@pytest.mark.parametrize("qfill", [1, 3, 255])
def test_whole_block_requests(codec, oracle, qfill):
    """Constant matrices on extreme 0/255 pixels and a checkerboard (the construction of
    test_extreme_matrices_fill_the_tile_image), one tile: non-structural coefficients near a tie
    ask for the whole block in FP64."""
    rng = np.random.default_rng(7 + qfill)
    q = np.full(N * N, qfill, dtype=np.uint16)
    h, w = 64, 256
    for y in ((rng.integers(0, 2, size=(h, w)) * 255).astype(np.uint8),
              (np.indices((h, w)).sum(axis=0) % 2 * 255).astype(np.uint8)):
        for rle in (True, False):
            _encode(codec, oracle, y, q, rle=rle)


def test_slot_pair_fallback_and_two_coefficient_records(codec, oracle):
    """All-ones matrix on noise: bl > 10, so records take the two-coefficient form, and a wave's
    256 records exceed its 32 768-bit region, so its slots are emitted and stored pair by pair."""
    y = _noise((64, 256), 14)
    _, fb, _, _ = _encode(codec, oracle, y, np.ones(N * N, dtype=np.uint16))
    blocks = (y.shape[0] // N) * (y.shape[1] // N)
    assert int(fb.sum()) > 128 * blocks, int(fb.sum()) / blocks


def test_rle_off(codec, oracle):
    y = _noise((64, 256), 15)
    _encode(codec, oracle, y, O.read_matrix("matrix.txt", N), rle=False)
    _encode(codec, oracle, y, _tie_matrix(), rle=False)


@pytest.mark.parametrize("w,h", [(384, 32), (416, 32)], ids=["empty_last_wave", "partial_last_wave"])
def test_partial_last_tile(codec, oracle, w, h):
    """groups_per_frame a multiple of 8 but not of 256: 384 x 32 leaves the tile's fourth wave
    empty, 416 x 32 fills a quarter of it."""
    assert (w // 16 * (h // N)) % 8 == 0 and (w // 16 * (h // N)) % 256 != 0
    for q in (O.read_matrix("matrix.txt", N), _tie_matrix()):
        _encode(codec, oracle, _noise((2, h, w), 16), q)


def test_counting_instantiation_on_dense_ties(codec, oracle):
    """The counted, segmented encode of the dense-tie frames: streams equal the oracle's and the
    fused byte histogram equals a histogram of the produced stream."""
    import torch
    w, h, f, start_bit = 256, 48, 3, 64
    y = _noise((f, h, w), 11)
    q = _tie_matrix()
    codec.set_quant(q, N)
    pitch = (stream_bound(w, h, N, 1, start_bit) + 255) // 256 * 256
    out = torch.zeros(pitch * f, dtype=torch.uint8, device="cuda")
    yd = torch.from_numpy(y).cuda()
    codec.encode_images(yd, w, h, out, out_pitch=pitch, nframes=f, start_bit=start_bit, count_bytes=True)
    hist, _ = codec.huffman_hist_after_encode(out, pitch, f)
    host = out.cpu().numpy()
    for k in range(f):
        exp, eend, _ = oracle.encode_blocks(y[k:k + 1], N, q, True, start_bit)
        nb = (eend + 7) // 8
        assert host[k * pitch: k * pitch + nb].tobytes() == exp[:nb].tobytes()
        np.testing.assert_array_equal(hist[k], np.bincount(host[k * pitch: k * pitch + nb], minlength=256))
