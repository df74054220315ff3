"""GPU: Codec.encode_image_quality (ieh_encode_image_quality) against its search rule recomputed in
Python from Codec.probe_rd: p0 = the largest percent of budget_ladder() whose sse meets the target,
then the largest of the integers p0 + ceil(i (p1 - p0) / 33) strictly below the next entry p1 that
meets it.  The returned sse equals the probe's value and the squared error of the oracle's CPU decode
of the returned file; the file equals encode_image under scale_matrix(q, percent) byte for byte."""
import math

import numpy as np
import pytest

from imageencoder_amd import (IE_ECAP, IEError, budget_ladder, psnr_of_sse, scale_matrix, sse_for_psnr,
                              stream_bound)
from tests import matrix_sweep as MS
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from imageencoder_amd import Codec
    return Codec(0)


def _frame(kind):
    if kind == "gradnoise":  # 64 x 48: a gradient with a little noise on it
        i, j = np.mgrid[0:48, 0:64]
        return np.clip(2 * i + 3 * j + np.random.default_rng(2).integers(-6, 7, size=(48, 64)), 0, 255).astype(np.uint8)
    return MS.noise((56, 200), 17)


def _base(n):
    return O.read_matrix("matrix.txt", 4) if n == 4 else np.array(MS.ANNEX_K, dtype=np.uint16)


class Sse:
    """sse by percent for one (frame, n), from Codec.probe_rd, one call per percent list."""

    def __init__(self, codec, y, n, base):
        self.c, self.y, self.n, self.base, self.memo = codec, y, n, base, {}

    def fill(self, percents):
        todo = [p for p in percents if p not in self.memo]
        if todo:
            h, w = self.y.shape
            self.c.set_quant(self.base, self.n)
            _, sse = self.c.probe_rd(self.y, w, h, np.stack([scale_matrix(self.base, p) for p in todo]))
            for p, s in zip(todo, sse[:, 0]):
                self.memo[p] = int(s)

    def __call__(self, p):
        self.fill([p])
        return self.memo[p]


def expected_percent(sse, max_sse):
    lad = budget_ladder()
    sse.fill(lad)
    meet = [p for p in lad if sse(p) <= max_sse]
    if not meet:
        return None
    p0 = meet[-1]
    if p0 == lad[-1]:
        return p0
    p1 = lad[lad.index(p0) + 1]
    fine = sorted({p0 + -(-i * (p1 - p0) // 33) for i in range(1, 33)})
    fine = [p for p in fine if p0 < p < p1]
    sse.fill(fine)
    return max([p for p in fine if sse(p) <= max_sse] + [p0])


CASES = [(kind, n, huffman) for kind in ("gradnoise", "noise200") for n in (4, 8) for huffman in (False, True)]


@pytest.mark.parametrize("kind,n,huffman", CASES, ids=[f"{k}-{n}x{n}-{'huff' if hf else 'plain'}" for k, n, hf in CASES])
def test_quality_encode(codec, oracle, kind, n, huffman):
    y = _frame(kind)
    h, w = y.shape
    base = _base(n)
    sse = Sse(codec, y, n, base)
    lad = budget_ladder()
    sse.fill(lad)
    assert sse(25) > 0  # the frame is not flat
    targets = {"mid_exact": sse(lad[12]), "mid_less": sse(lad[12]) - 1, "fine": sse(lad[3]) + 1,
               "coarse": sse(lad[28]), "everything": 2 ** 64 - 1, "psnr30": sse_for_psnr(30.0, w * h)}
    budget_before = codec.encode_image_budget(y, w, h, base, n, 1 << 20, huffman=huffman)
    for name, max_sse in targets.items():
        exp = expected_percent(sse, max_sse)
        if exp is None:
            with pytest.raises(IEError) as e:
                codec.encode_image_quality(y, w, h, base, n, max_sse=max_sse, huffman=huffman)
            assert e.value.code == IE_ECAP and e.value.percent == 25, name
            continue
        data, percent, got = codec.encode_image_quality(y, w, h, base, n, max_sse=max_sse, huffman=huffman)
        assert percent == exp, (name, max_sse, percent, exp)
        assert got == sse(percent) <= max_sse, name
        dec = oracle.decode_image(data, n)
        d = dec.astype(np.int64) - y.astype(np.int64)
        assert int((d * d).sum()) == got, name
        assert data == codec.encode_image_file(y, w, h, scale_matrix(base, percent), n, huffman=huffman), name
        assert data == oracle.encode_image(y, n, scale_matrix(base, percent), rle=True, huffman=huffman), name
    assert expected_percent(sse, 2 ** 64 - 1) == 5382
    # a budget encode before and after: the same bytes, the oracle's under the same scale
    budget_after = codec.encode_image_budget(y, w, h, base, n, 1 << 20, huffman=huffman)
    assert budget_before == budget_after and budget_after[1] == 25
    assert budget_after[0] == oracle.encode_image(y, n, scale_matrix(base, 25), rle=True, huffman=huffman)


@pytest.mark.parametrize("n", [4, 8])
def test_targets_at_both_ends_and_psnr(codec, oracle, n):
    import ctypes as C

    from imageencoder_amd import load_host_library
    y = _frame("noise200")
    h, w = y.shape
    base = _base(n)
    sse = Sse(codec, y, n, base)
    # nothing meets 0 on a frame that is not flat: IE_ECAP, 25 %, nothing written, the matrix is base
    assert sse(25) > 0
    with pytest.raises(IEError) as e:
        codec.encode_image_quality(y, w, h, base, n, max_sse=0)
    assert e.value.code == IE_ECAP and e.value.percent == 25
    assert "no scale down to 25 % meets the quality" in str(e.value)
    stream = np.zeros(stream_bound(w, h, n), dtype=np.uint8)
    assert codec.encode_frames(y, w, h, stream)[0][0] == codec.probe_rd(y, w, h, base[None])[0][0, 0]
    # everything meets 2^64 - 1: 5382 %, and the search ends after the ladder (the refinement above the last
    # entry does not exist); through the C entry point, rle off
    H = load_host_library()
    out = np.zeros(1 << 17, dtype=np.uint8)
    pc, se = C.c_int(0), C.c_uint64(0)
    r = H.ieh_encode_image_quality(codec.h, y.ctypes.data, w, h, base.ctypes.data, n, 0, 0, 0, 2 ** 64 - 1,
                                   out.ctypes.data, out.size, C.byref(pc), C.byref(se))
    assert r > 0 and pc.value == 5382
    q = scale_matrix(base, 5382)
    assert out[:r].tobytes() == oracle.encode_image(y, n, q, rle=False, huffman=False)
    codec.set_quant(base, n)
    assert se.value == int(codec.probe_rd(y, w, h, q[None], rle=False)[1][0, 0])
    # cap below the file: IE_ECAP with the other message
    r = H.ieh_encode_image_quality(codec.h, y.ctypes.data, w, h, base.ctypes.data, n, 1, 0, 0, 2 ** 64 - 1,
                                   out.ctypes.data, 8, C.byref(pc), C.byref(se))
    assert r == IE_ECAP and b"capacity" in codec.L.ie_last_error(codec.h)
    # the psnr form: the file's PSNR is at least the target
    ran = 0
    for target in (12.0, 20.0, 28.5):
        if sse(25) > sse_for_psnr(target, w * h):
            continue
        ran += 1
        data, percent, got = codec.encode_image_quality(y, w, h, base, n, psnr=target)
        assert psnr_of_sse(got, w * h) >= target
        assert percent == expected_percent(sse, sse_for_psnr(target, w * h))
        dec = oracle.decode_image(data, n)
        d = dec.astype(np.int64) - y.astype(np.int64)
        assert int((d * d).sum()) == got
    assert ran >= 1
    with pytest.raises(IEError):
        codec.encode_image_quality(y, w, h, base, n)
    with pytest.raises(IEError):
        codec.encode_image_quality(y, w, h, base, n, max_sse=5, psnr=30.0)
    assert math.isinf(psnr_of_sse(0, w * h))
