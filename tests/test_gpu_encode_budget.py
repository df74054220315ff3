"""GPU: Codec.encode_image_budget (ieh_encode_image_budget) against the search rule evaluated on
the CPU with oracle sizes: the file size of a percent is ceil((header bits + payload bits) / 8)
with the header of oracle.header (ieo_write_header) for the scaled matrix and the payload of
oracle.encode_blocks; the expected percent is the smallest fitting one of the ladder and of the
refinement between the first fitting ladder entry and the entry below it.  The file must equal
oracle.encode_image under the chosen matrix byte for byte, with and without the Huffman pass.

Budgets come from the oracle's own sizes, so every branch is reached by construction: at least the
25 % size (the search ends at once), below every ladder size (IE_ECAP), the exact size of a middle
ladder entry, and one byte less."""
import os

import numpy as np
import pytest

from imageencoder_amd import IE_ECAP, IEError, budget_ladder, scale_matrix, synth
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from imageencoder_amd import Codec
    return Codec(0)


def _image(kind):
    if kind == "synth64":
        return synth.frame("M", 64, 64, seed=3)
    raw = np.fromfile(os.path.join(O.GOLDEN, "ex3.raw"), dtype=np.uint8).reshape(400, 400)
    return np.ascontiguousarray(raw[136:264, 120:248])  # the reference's example image, 128 x 128 of it


def ladder_formula():
    """percent_j = round(100 * 2^(j/4)), j = -8 .. 23 (no value lies within 0.01 of a tie)."""
    return [int(np.floor(100.0 * 2.0 ** (j / 4.0) + 0.5)) for j in range(-8, 24)]


class Sizes:
    """File bytes by percent for one (image, n, rle, huffman flag), from the oracle, computed once."""

    def __init__(self, oracle, y, n, base, rle, huffman):
        self.o, self.y, self.n, self.base, self.rle, self.huffman = oracle, y, n, base, rle, huffman
        self.memo = {}

    def __call__(self, p):
        if p not in self.memo:
            q = scale_matrix(self.base, p)
            h, w = self.y.shape
            _, hb = self.o.header(self.n, q, self.rle, w, h, huffman=self.huffman)
            payload = int(self.o.encode_blocks(self.y, self.n, q, self.rle)[2][0])
            self.memo[p] = (hb + payload + 7) // 8
        return self.memo[p]


def expected_percent(size, budget):
    """The issue's search rule; None when no ladder entry fits."""
    lad = ladder_formula()
    fit = [p for p in lad if size(p) <= budget]
    if not fit:
        return None
    p1 = fit[0]
    if p1 == lad[0]:
        return p1
    p0 = lad[lad.index(p1) - 1]
    fine = sorted({p0 + -(-i * (p1 - p0) // 33) for i in range(1, 33)})
    fine = [p for p in fine if p0 < p < p1]
    return min([p for p in fine if size(p) <= budget] + [p1])


_SIZES = {}

CASES = [(kind, n, huffman) for kind in ("synth64", "ex3_128") for n in (4, 8) for huffman in (False, True)]


@pytest.mark.parametrize("kind,n,huffman", CASES, ids=[f"{k}-{n}x{n}-{'huff' if hf else 'plain'}" for k, n, hf in CASES])
def test_budget_encode(codec, oracle, kind, n, huffman):
    assert budget_ladder() == ladder_formula()
    y = _image(kind)
    h, w = y.shape
    base = O.read_matrix("matrix.txt" if n == 4 else "matrix8_annexk.txt", n)
    size = _SIZES.setdefault((kind, n, huffman), Sizes(oracle, y, n, base, True, huffman))
    lad = ladder_formula()
    mid = lad[12]
    budgets = {"roomy": size(25) + 3, "below_last": size(5382) - 1, "below_all": min(size(p) for p in lad) - 1,
               "mid_exact": size(mid), "mid_less": size(mid) - 1}
    assert expected_percent(size, budgets["roomy"]) == 25
    assert expected_percent(size, budgets["below_all"]) is None
    got_percent = {}
    for name, budget in budgets.items():
        exp = expected_percent(size, budget)
        if exp is None:
            with pytest.raises(IEError) as e:
                codec.encode_image_budget(y, w, h, base, n, budget, rle=True, huffman=huffman)
            assert e.value.code == IE_ECAP and e.value.percent == 5382, name
            assert "no scale up to 5382 % meets the budget" in str(e.value)
            continue
        data, percent = codec.encode_image_budget(y, w, h, base, n, budget, rle=True, huffman=huffman)
        assert percent == exp, (name, budget, percent, exp)
        got_percent[name] = percent
        assert data == oracle.encode_image(y, n, scale_matrix(base, percent), rle=True, huffman=huffman), name
        if not huffman:
            assert len(data) == size(percent) <= budget, name
        dec = codec.decode_image_file(data, n)
        assert dec.shape == (h, w), name
    # the exact size of a ladder entry: that entry or a finer refined one; a byte less: no finer
    assert got_percent["mid_exact"] <= mid
    assert got_percent["mid_less"] >= got_percent["mid_exact"]
    if size(got_percent["mid_exact"]) == budgets["mid_exact"]:
        assert got_percent["mid_less"] > got_percent["mid_exact"]


def test_budget_encode_device_frame_no_rle(codec, oracle):
    """A device-resident frame, RLE off, EXACT mode: the same choice and the same bytes."""
    import torch

    from imageencoder_amd import MODE_EXACT
    y = _image("synth64")
    base = O.read_matrix("matrix.txt", 4)
    size = Sizes(oracle, y, 4, base, False, False)
    budget = size(ladder_formula()[10]) + 1
    exp = expected_percent(size, budget)
    import ctypes as C

    from imageencoder_amd import load_host_library
    H = load_host_library()
    out = np.zeros(1 << 16, dtype=np.uint8)
    pc = C.c_int(0)
    dy = torch.from_numpy(y).cuda()
    r = H.ieh_encode_image_budget(codec.h, dy.data_ptr(), 64, 64, base.ctypes.data, 4, 0, 0, MODE_EXACT, budget,
                                  out.ctypes.data, out.size, C.byref(pc))
    assert r > 0 and pc.value == exp
    assert out[:r].tobytes() == oracle.encode_image(y, 4, scale_matrix(base, exp), rle=False, huffman=False)
    assert r <= budget
