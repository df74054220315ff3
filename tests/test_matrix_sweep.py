"""The sweep's own conditions, on the CPU: the matrix list is what it says, the integer tie rule
agrees with a float64 DCT, and every tie frame the GPU sweep encodes really holds ties."""
import numpy as np
import pytest

from tests import matrix_sweep as MS

# (n, w, h, frames) of the GPU sweep's encodes (tests/test_gpu_matrix_sweep.py)
SHAPES = [(4, 256, 48, 3), (4, 200, 56, 1), (8, 256, 128, 2)]
MIN_TIES = 32


def test_sweep_is_deterministic_and_in_range():
    for n, count in ((4, 29), (8, 11)):
        a, b = MS.sweep(n), MS.sweep(n)
        assert len(a) == count
        for (na, qa), (nb_, qb) in zip(a, b):
            assert na == nb_ and qa.dtype == np.uint16 and qa.shape == (n * n,) and qa.min() >= 1
            assert np.array_equal(qa, qb)
    q4, q8 = dict(MS.sweep(4)), dict(MS.sweep(8))
    assert q4["primes"][:5].tolist() == [3, 5, 7, 11, 13] and q4["ref_dc3"][0] == 3
    assert q4["primes_struct1"][[2, 8, 10]].tolist() == [1, 1, 1] and q8["primes_struct1"][[4, 32, 36]].tolist() == [1, 1, 1]
    assert q8["annex_k_div5"][0] == 3 and q8["annex_k"][63] == 99
    assert q4["rand16_0"].max() > 255


def test_golden_matrix_files_are_sweep_entries():
    """The matrix files of the reference-generated goldens are the sweep's own matrices."""
    from tests import oracle_lib as O
    for fn, n, name in (("matrix4_jpeg.txt", 4, "jpeg_like"), ("matrix4_primes.txt", 4, "primes"),
                        ("matrix4_dc3.txt", 4, "ref_dc3"), ("matrix8_annexk.txt", 8, "annex_k"),
                        ("matrix8_annexk5.txt", 8, "annex_k_div5")):
        assert np.array_equal(O.read_matrix(fn, n), MS.by_name(n, name)), fn


def _dct_f64(blocks, n):
    """D[u][v] = C(u) C(v) sum_ij c[u][i] c[v][j] (x - 128), C = (1/2, sqrt(1/2), ...) for every n."""
    i = np.arange(n)
    c = np.cos((2 * i[None, :] + 1) * i[:, None] * np.pi / (2 * n))
    C = np.where(i == 0, 0.5, np.sqrt(0.5))
    x = blocks.astype(np.float64) - 128.0
    return np.einsum("u,v,ui,vj,bij->buv", C, C, c, c, x)


@pytest.mark.parametrize("n", [4, 8])
def test_integer_tie_rule_matches_float64(n):
    """J = 2q (mod 4q) <=> D/q is within 1e-9 of a half-integer, on noise and on tie frames."""
    for name, q in MS.sweep(n):
        y = np.concatenate([MS.tie_frames(n, q, 32 * n, 8 * n, 1, seed=5), MS.noise((1, 8 * n, 32 * n), 6)])
        blocks = MS.to_blocks(y, n)
        D = _dct_f64(blocks, n).reshape(len(blocks), -1)
        for c in range(MS.TIE_COEFS):
            k = MS.tie_index(n, c)
            np.testing.assert_allclose(D[:, k], MS.tie_J(blocks, n, c) / 4.0, rtol=0, atol=1e-9)
            t = D[:, k] / float(q[k])
            near = np.abs(np.abs(t - np.floor(t)) - 0.5) < 1e-9
            assert np.array_equal(near, MS.on_tie(blocks, n, q, c)), (name, c)


@pytest.mark.parametrize("n,w,h,frames", SHAPES)
def test_tie_frames_hold_ties(n, w, h, frames):
    for name, q in MS.sweep(n):
        y = MS.tie_frames(n, q, w, h, frames, seed=1)
        assert y.shape == (frames, h, w) and y.dtype == np.uint8
        counts = MS.tie_counts(y, n, q)
        for c in range(MS.TIE_COEFS):
            if MS.tie_reachable(n, int(q[MS.tie_index(n, c)])):
                assert counts[c] >= MIN_TIES, (name, c, counts)
