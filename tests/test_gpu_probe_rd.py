"""GPU: ie_probe_rd (Codec.probe_rd) against the library's own encode + decode.

Truth for the whole file: for every candidate, set_quant, encode_frames, decode_frames through the
existing ABI, then the integer squared error per frame in numpy (torch for the large frames);
`bits` is held against encode_frames' frame_bits.  At the small shapes the truth itself is pinned to
the reference: the oracle's encode_image -> decode_image on the CPU gives the same squared error.
Equality is exact everywhere.

Shapes are the smallest that reach each way the kernel can go wrong (a tile is 256 4x4 or 64 8x8
blocks, a wave's step four 4x4 blocks or one 8x8 block): one block and one partly filled step,
200 x 56 (ragged: tiles and a step that are partly filled), 64 x 48 x 3 with padded rows and frames
and a device input one byte off alignment, 64 x 48 under every sweep matrix, and two frames of more
tiles than the launch has workgroups (4x4: at most 1024 workgroups, 2048 x 2064 is 1032 tiles; 8x8:
at most 512, 2048 x 1032 is 516 tiles), so a workgroup flushes at a frame change and at its end."""
import numpy as np
import pytest

from imageencoder_amd import IE_EINVAL, IEError, scale_matrix, stream_bound
from tests import crafted_streams as CS
from tests import matrix_sweep as MS
from tests import oracle_lib as O
from tests.probe_common import codec, device_table, fresh_context_refuses  # noqa: F401

pytestmark = pytest.mark.gpu


def _base(n):
    return O.read_matrix("matrix.txt", 4) if n == 4 else np.array(MS.ANNEX_K, dtype=np.uint16)


def _candidates(n):
    """The shipped matrix at 25, 100, 400 and 5382 %, all ones, all 65535."""
    b = _base(n)
    return np.stack([scale_matrix(b, p) for p in (25, 100, 400, 5382)] +
                    [np.ones(n * n, dtype=np.uint16), np.full(n * n, 65535, dtype=np.uint16)])


def truth(codec, y, n, qs, rle, restore=None):
    """(bits, sse), each (nq, frames) uint64, by one encode + decode per candidate.  y: (frames, h, w)
    numpy.  The codec's matrix afterwards is `restore` (default: the block size's base)."""
    f, h, w = y.shape
    bits = np.zeros((len(qs), f), dtype=np.uint64)
    sse = np.zeros((len(qs), f), dtype=np.uint64)
    for m, q in enumerate(qs):
        codec.set_quant(q, n)
        out = np.zeros(stream_bound(w, h, n, f), dtype=np.uint8)
        fb, end = codec.encode_frames(y, w, h, out, nframes=f, rle=rle)
        dec = np.zeros((f, h, w), dtype=np.uint8)
        assert codec.decode_frames(out, w, h, dec, nframes=f, rle=rle) == end
        bits[m] = fb
        d = dec.astype(np.int64) - y.astype(np.int64)
        sse[m] = (d * d).reshape(f, -1).sum(axis=1)
    codec.set_quant(_base(n) if restore is None else restore, n)
    return bits, sse


def oracle_sse(oracle, y2d, n, q, rle):
    dec = oracle.decode_image(oracle.encode_image(y2d, n, q, rle=rle), n)
    d = dec.astype(np.int64) - y2d.astype(np.int64)
    return int((d * d).sum())


def check(codec, y, n, qs, rle, what=""):
    f, h, w = y.shape
    eb, es = truth(codec, y, n, qs, rle)
    bits, sse = codec.probe_rd(y, w, h, qs, nframes=f, rle=rle)
    assert bits.dtype == np.uint64 and sse.dtype == np.uint64 and bits.shape == sse.shape == (len(qs), f)
    np.testing.assert_array_equal(bits, eb, err_msg=f"bits {what}")
    np.testing.assert_array_equal(sse, es, err_msg=f"sse {what}")
    return bits, sse


@pytest.mark.parametrize("n", [4, 8])
def test_ragged_noise_frame(codec, oracle, n):
    """200 x 56 of 0 / 255 noise: under candidate 0 the frame holds blocks whose record loses its
    last value (zig-zag value N^2-1 non-zero, N^2-2 zero) and decoded pixels clamped at 0 and at
    255; RLE off changes a candidate's sse, so the drop rule is applied under RLE only."""
    w, h = 200, 56
    y = MS.noise_0_255((h, w), 7)
    qs = _candidates(n)
    z = oracle.quantize(y, n, qs[0])[:, oracle.zigzag(n)]
    assert int(((z[:, -1] != 0) & (z[:, -2] == 0)).sum()) >= 1
    dec = oracle.decode_image(oracle.encode_image(y, n, qs[0], rle=True), n)
    assert (dec == 0).any() and (dec == 255).any()
    res = {}
    for rle in (True, False):
        res[rle] = check(codec, y[None], n, qs, rle, f"rle={rle}")[1]
        for m in (0, 2, 5):  # the truth is the reference's
            assert int(res[rle][m, 0]) == oracle_sse(oracle, y, n, qs[m], rle), (m, rle)
    assert (res[True] != res[False]).any()
    assert (res[True] > 0).any()


@pytest.mark.parametrize("n,w,h", [(4, 4, 4), (8, 8, 8), (4, 8, 8)], ids=["one4", "one8", "partial_step4"])
def test_small_shapes(codec, oracle, n, w, h):
    qs = _candidates(n)
    for name, y in (("noise", MS.noise((h, w), 3)), ("noise_0_255", MS.noise_0_255((h, w), 5)),
                    ("flat", np.full((h, w), 77, dtype=np.uint8))):
        for rle in (True, False):
            _, sse = check(codec, y[None], n, qs, rle, f"{name} rle={rle}")
            for m in range(len(qs)):
                assert int(sse[m, 0]) == oracle_sse(oracle, y, n, qs[m], rle), (name, m, rle)


@pytest.mark.parametrize("n", [4, 8])
def test_padded_rows_frames_and_a_misaligned_device_input(codec, n):
    """64 x 48 x 3, stride = w + 13 and a padded frame_pitch: byte loads; then the same buffer on the
    device one byte past an aligned address.  The padding is 0xFF, so a read of it shows."""
    import torch
    w, h, f = 64, 48, 3
    stride = w + 13
    pitch = stride * h + 4 * 37 + 1
    y = np.stack([MS.noise((h, w), 11), MS.noise_0_255((h, w), 12), MS.low_noise((h, w), 13)])
    qs = _candidates(n)
    eb, es = truth(codec, y, n, qs, True)
    buf = np.full(f * pitch + 1, 0xFF, dtype=np.uint8)
    for k in range(f):
        buf[1 + k * pitch: 1 + k * pitch + h * stride].reshape(h, stride)[:, :w] = y[k]
    dbuf = torch.from_numpy(buf).cuda()
    assert dbuf.data_ptr() % 4 == 0
    for src in (buf[1:], dbuf[1:]):
        bits, sse = codec.probe_rd(src, w, h, qs, nframes=f, stride=stride, frame_pitch=pitch)
        np.testing.assert_array_equal(bits, eb)
        np.testing.assert_array_equal(sse, es)
    # aligned rows too (4-byte loads): stride = w + 12
    stride, pitch = w + 12, (w + 12) * h + 8
    buf = np.full(f * pitch, 0xFF, dtype=np.uint8)
    for k in range(f):
        buf[k * pitch: k * pitch + h * stride].reshape(h, stride)[:, :w] = y[k]
    bits, sse = codec.probe_rd(torch.from_numpy(buf).cuda(), w, h, qs, nframes=f, stride=stride, frame_pitch=pitch)
    np.testing.assert_array_equal(bits, eb)
    np.testing.assert_array_equal(sse, es)


@pytest.mark.parametrize("n", [4, 8])
def test_every_sweep_matrix(codec, n):
    """Every matrix of the sweep as one candidate list at 64 x 48, on noise and on the rounding-tie
    frame of the first matrix: quotients at .5 reach the dequantiser."""
    w, h = 64, 48
    qs = np.stack([q for _, q in MS.sweep(n)])
    assert 1 < len(qs) <= 64
    for name, y in (("noise", MS.noise((1, h, w), 21)), ("ties", MS.tie_frames(n, qs[0], w, h, 1, seed=1))):
        for rle in (True, False):
            check(codec, y, n, qs, rle, f"{name} rle={rle}")


@pytest.mark.parametrize("name", [e.name for e in CS.by_family("ties")])
def test_crafted_pixels_around_0_and_255(codec, oracle, name):
    """The crafted "ties" streams hold DC-only records whose pixel Y q / 4 + 128 lies around 0 and
    around 255, and records whose pixels are exact integers.  The records themselves cannot all be
    reached by an encoder: a flat block's unquantised DC lies in [-512, 508] (4x4; the same after
    scaling for 8x8), so a quantised value more than half a step outside that range is written by no
    encoder, and the decoder clamps what such a record yields.  What an encoder does reach is the
    frame those records decode to: flat blocks at and next to 0 and 255 and the integer-pixel
    blocks.  That frame (the oracle's CPU decode of the crafted file) is probed under the entry's
    own matrix, a finer and a coarser one, which puts decoded pixels on and across both clamps."""
    e = CS.by_name(name)
    y = oracle.decode_image(e.data, e.n)
    assert y.shape == (e.h, e.w) and (y == 0).any() and (y == 255).any()
    qs = np.stack([e.q, scale_matrix(e.q, 50), scale_matrix(e.q, 300)])
    _, sse = check(codec, y[None], e.n, qs, e.rle, name)
    for m in range(len(qs)):
        assert int(sse[m, 0]) == oracle_sse(oracle, y, e.n, qs[m], e.rle), m


def test_candidate_count_boundaries(codec):
    n, w, h = 4, 64, 48
    y = MS.noise((1, h, w), 5)
    q64 = np.stack([scale_matrix(_base(n), 30 + 7 * k) for k in range(64)])
    eb, es = truth(codec, y, n, q64, True)
    for sl in (slice(0, 64), slice(0, 63), slice(5, 6)):  # nq = 64, 63, 1
        bits, sse = codec.probe_rd(y, w, h, q64[sl])
        np.testing.assert_array_equal(bits, eb[sl])
        np.testing.assert_array_equal(sse, es[sl])
    with pytest.raises(IEError) as e:
        codec.probe_rd(y, w, h, np.concatenate([q64, q64[:1]]))  # nq = 65
    assert e.value.code == IE_EINVAL
    with pytest.raises(IEError) as e:
        codec.probe_rd(y, w, h, np.zeros((0, 16), dtype=np.uint16))  # nq = 0
    assert e.value.code == IE_EINVAL
    bad = q64[:4].copy()
    bad[2, 9] = 0
    with pytest.raises(IEError) as e:
        codec.probe_rd(y, w, h, bad)
    assert e.value.code == IE_EINVAL and "matrix 2" in str(e.value)
    with pytest.raises(IEError) as e:  # the checks of encode_frames, with their codes
        codec.probe_rd(y, w + 2, h, q64[:1])
    assert e.value.code == IE_EINVAL


def test_fresh_context_has_no_block_size():
    fresh_context_refuses(lambda c: c.probe_rd(np.zeros((8, 8), dtype=np.uint8), 8, 8, np.ones((1, 16), dtype=np.uint16)))


@pytest.mark.parametrize("n", [4, 8])
def test_null_bits_device_results_and_mixed_results(codec, n):
    import ctypes as C

    import torch
    w, h, f = 64, 48, 2
    y = MS.noise((f, h, w), 31)
    qs = _candidates(n)
    nq = len(qs)
    eb, es = truth(codec, y, n, qs, True)
    u64p = C.POINTER(C.c_uint64)
    qc = np.ascontiguousarray(qs)
    # bits = NULL, host sse
    sse = np.zeros((nq, f), dtype=np.uint64)
    r = codec.L.ie_probe_rd(codec.h, y.ctypes.data, w, h, w, w * h, f, 1, qc.ctypes.data, nq, None,
                            sse.ctypes.data_as(u64p))
    assert r == 0
    np.testing.assert_array_equal(sse, es)
    # sse = NULL
    bits = np.zeros((nq, f), dtype=np.uint64)
    assert codec.L.ie_probe_rd(codec.h, y.ctypes.data, w, h, w, w * h, f, 1, qc.ctypes.data, nq,
                               bits.ctypes.data_as(u64p), None) == IE_EINVAL
    # device results, with and without bits: asynchronous, equal to the host ones after a sync
    dy = torch.from_numpy(y).cuda()
    db = torch.full((nq * f,), -1, dtype=torch.int64, device="cuda")
    ds = torch.full((nq * f,), -1, dtype=torch.int64, device="cuda")
    out = codec.probe_rd(dy, w, h, qs, nframes=f, out=(db, ds))
    assert out[0] is db and out[1] is ds
    codec.sync()
    np.testing.assert_array_equal(device_table(db, nq, f), eb)
    np.testing.assert_array_equal(device_table(ds, nq, f), es)
    ds.fill_(-1)
    codec.probe_rd(dy, w, h, qs, nframes=f, out=(None, ds))
    codec.sync()
    np.testing.assert_array_equal(device_table(ds, nq, f), es)
    # host bits with device sse, and the reverse
    for b, s in ((bits.ctypes.data_as(u64p), C.cast(C.c_void_p(ds.data_ptr()), u64p)),
                 (C.cast(C.c_void_p(db.data_ptr()), u64p), sse.ctypes.data_as(u64p))):
        assert codec.L.ie_probe_rd(codec.h, y.ctypes.data, w, h, w, w * h, f, 1, qc.ctypes.data, nq, b, s) == IE_EINVAL
    with pytest.raises(IEError):
        codec.probe_rd(dy, w, h, qs, nframes=f, out=(db[:3], ds))


@pytest.mark.parametrize("n,w,h", [(4, 2048, 2064), (8, 2048, 1032)])
def test_many_workgroups_add_into_one_sum(codec, n, w, h):
    """Two frames of more tiles than the launch has workgroups: every workgroup walks several tiles,
    flushes its sums when the frame changes and again when its work ends."""
    import torch
    tiles = (w // n) * (h // n) // (256 if n == 4 else 64)
    assert tiles > (1024 if n == 4 else 512)
    f = 2
    g = torch.Generator().manual_seed(9)
    y = torch.randint(0, 256, (f, h, w), dtype=torch.uint8, generator=g)
    y[1] = (torch.randint(0, 2, (h, w), generator=g) * 255).to(torch.uint8)
    dy = y.cuda()
    qs = _candidates(n)[[0, 2, 3]]
    eb = np.zeros((len(qs), f), dtype=np.uint64)
    es = np.zeros((len(qs), f), dtype=np.uint64)
    out = torch.zeros(stream_bound(w, h, n, f), dtype=torch.uint8, device="cuda")
    dec = torch.zeros((f, h, w), dtype=torch.uint8, device="cuda")
    for m, q in enumerate(qs):
        codec.set_quant(q, n)
        out.zero_()
        fb, end = codec.encode_frames(dy, w, h, out, nframes=f)
        assert codec.decode_frames(out, w, h, dec, nframes=f) == end
        eb[m] = fb
        d = dec.long() - dy.long()
        es[m] = (d * d).sum(dim=(1, 2)).cpu().numpy().astype(np.uint64)
    codec.set_quant(_base(n), n)
    bits, sse = codec.probe_rd(dy, w, h, qs, nframes=f)
    np.testing.assert_array_equal(bits, eb)
    np.testing.assert_array_equal(sse, es)
    assert (es > 2 ** 32).any()  # a frame's sum does not fit 32 bits


@pytest.mark.parametrize("n", [4, 8])
def test_probe_leaves_the_context_untouched(codec, n):
    """encode, probe, encode: the two streams, the two cos_table read-backs, the fallback counts and
    the device end bits are identical; ie_probe_sizes on the same input gives the same bits."""
    import torch
    w, h = 200, 56
    q = _base(n)
    y = MS.tie_frames(n, q, w, h, 1, seed=1)
    codec.set_quant(q, n)

    def encode():
        out = np.zeros(stream_bound(w, h, n), dtype=np.uint8)
        fb, end = codec.encode_frames(y, w, h, out)
        return out.tobytes(), int(fb[0]), end, codec.last_fallbacks(), codec.cos_table().tobytes()

    def end_bits():
        t = torch.zeros(1, dtype=torch.int64, device="cuda")
        codec.end_bits_into(t)
        codec.sync()
        return int(t.item())

    before = encode()
    eb0 = end_bits()
    qs = _candidates(n)
    bits, sse = codec.probe_rd(y, w, h, qs)
    assert end_bits() == eb0 == before[2]
    assert codec.cos_table().tobytes() == before[4]
    after = encode()
    assert before == after
    np.testing.assert_array_equal(codec.probe_sizes(y, w, h, qs), bits)
    np.testing.assert_array_equal(codec.probe_sizes(y, w, h, qs, rle=False), codec.probe_rd(y, w, h, qs, rle=False)[0])
    assert bits[1, 0] == before[1]  # candidate 1 is the context's own matrix
