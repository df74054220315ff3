"""What the GPU tests of the four probes (tests/test_gpu_probe_*.py) share: the context, the base
matrices, the candidates, contents and oracle tables of the two gop probes, the exact comparison of
two tables and the check that a context without a block size refuses a probe."""
import numpy as np
import pytest

from imageencoder_amd import IE_ENOQUANT, IEError, scale_matrix, synth
from tests import matrix_sweep as MS


@pytest.fixture(scope="module")
def codec():
    from imageencoder_amd import Codec
    return Codec(0)


def base(n):
    return MS.by_name(n, "jpeg_like" if n == 4 else "annex_k")


def gop_candidates(n):
    """The context's own matrix first, the sweep, the base scaled across the budget ladder's range."""
    qs = [base(n)] + [q for _, q in MS.sweep(n)] + [scale_matrix(base(n), p) for p in (25, 59, 336, 1345, 5382)]
    assert len(qs) <= 64
    return np.stack(qs)


def gop_few(n):
    return gop_candidates(n)[[0, 2, -5, -2, -1]]


def gop_contents(n, f, h, w):
    return [("noise", synth.frames("U", w, h, f, seed=31)), ("shift", synth.frames("shiftA", w, h, f, seed=5)),
            ("flat", synth.frames("flat128", w, h, f)), ("ties", MS.tie_frames(n, base(n), w, h, f, seed=2))]


def gop_bits(oracle, y, n, qs, gop, merange, rle=True, **layout):
    """(nq, frames) payload bits from the oracle, one encode_gop per candidate."""
    return np.stack([oracle.encode_gop(y, n, q, gop, merange, rle=rle, **layout)[2] for q in qs]).astype(np.uint64)


def check_table(got, exp, what):
    assert got.dtype == np.uint64 and got.shape == exp.shape
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (what, "candidate, frame:", bad[:4].tolist(), got[bad[0][0]], exp[bad[0][0]])


def device_table(t, nq, f):
    """A device result tensor of 64-bit entries as a (nq, f) uint64 numpy table."""
    return t.cpu().numpy().view(np.uint64).reshape(nq, f)


def fresh_context_refuses(call):
    """call(codec) probes with a context that has no block size yet: IE_ENOQUANT."""
    from imageencoder_amd import Codec
    c = Codec(0)
    try:
        with pytest.raises(IEError) as e:
            call(c)
        assert e.value.code == IE_ENOQUANT
    finally:
        c.close()
