"""The quantisation matrices every sweep test shares, and frames whose blocks sit on rounding ties.

sweep(n) returns named (name, q) pairs for n = 4 or 8: deterministic (fixed seeds), uint16, every
entry at least 1.  The five matrix files of tests/golden hold powers of two (and 255) only; these
do not: JPEG-like tables, primes, odd DC quantisers, 1 and 3 at the structural positions, the
extremes of the 16-bit range and seeded random matrices.

Ties.  The DC and the three structural coefficients (0,N/2), (N/2,0), (N/2,N/2) are D = J / 4 for
an integer J of the block's pixels x: J = sum_ij s_i s_j x_ij with s = (+,-,-,+) repeated along the
structural axis and all ones along the other; for the DC s is all ones and 128 N^2 is subtracted.
(cos((2i+1) pi/4) = +-sqrt(1/2) and C(0) = 1/2, C(u > 0) = sqrt(1/2) give the factor 1/4 in all four
cases; the reference keeps these N = 4 values of C for every N, algo.cpp:294-297, so the divisor
is 4 for 8 x 8 blocks too, not N.)
The quotient D / q_k is mathematically on a rounding tie iff J = 2 q_k (mod 4 q_k).
tests/test_matrix_sweep.py checks that rule against a float64 DCT before anything relies on it.
"""
from __future__ import annotations

import numpy as np

from tests import oracle_lib as O

JPEG_LIKE_4 = [16, 10, 24, 51, 14, 16, 40, 69, 18, 37, 68, 103, 49, 78, 103, 99]
# ITU-T T.81 Annex K, table K.1 (luminance)
ANNEX_K = [16, 11, 10, 16, 24, 40, 51, 61,
           12, 12, 14, 19, 26, 58, 60, 55,
           14, 13, 16, 24, 40, 57, 69, 56,
           14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77,
           24, 35, 55, 64, 81, 104, 113, 92,
           49, 64, 78, 87, 103, 121, 120, 101,
           72, 92, 95, 98, 112, 100, 103, 99]


def _primes(count: int) -> list[int]:
    """The first `count` odd primes: 3 5 7 11 ..."""
    out, v = [], 3
    while len(out) < count:
        if all(v % p for p in out if p * p <= v):
            out.append(v)
        v += 2
    return out


def structural(n: int) -> list[int]:
    """Natural indices of (0,N/2), (N/2,0), (N/2,N/2)."""
    h = n // 2
    return [h, h * n, h * n + h]


def _rand_u8(seed: int, nn: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(1, 256, size=nn).astype(np.uint16)


def _rand_log16(seed: int, nn: int) -> np.ndarray:
    v = np.exp(np.random.default_rng(seed).uniform(0.0, np.log(65536.0), size=nn))
    return np.clip(np.floor(v), 1, 65535).astype(np.uint16)


def sweep(n: int) -> list[tuple[str, np.ndarray]]:
    nn = n * n
    out: list[tuple[str, list | np.ndarray]] = []
    primes = _primes(nn)
    if n == 4:
        base = O.read_matrix("matrix.txt", 4)
        out.append(("jpeg_like", JPEG_LIKE_4))
        out.append(("primes", primes))
        for dc in (1, 3, 6, 100, 255, 32768, 65535):
            q = base.copy()
            q[0] = dc
            out.append((f"ref_dc{dc}", q))
        for v in (1, 3):
            q = np.array(primes)
            q[structural(4)] = v
            out.append((f"primes_struct{v}", q))
        q = np.ones(nn, dtype=np.int64)
        q[0] = 255
        out.append(("ones_dc255", q))
        q = np.full(nn, 65535)
        q[0] = 1
        out.append(("dc1_rest65535", q))
        out += [(f"rand8_{i}", _rand_u8(4100 + i, nn)) for i in range(8)]
        out += [(f"rand16_{i}", _rand_log16(4200 + i, nn)) for i in range(8)]
    else:
        base = O.read_matrix("matrix8_1.txt", 8)
        out.append(("annex_k", ANNEX_K))
        out.append(("annex_k_div5", [max(1, (v + 2) // 5) for v in ANNEX_K]))
        out.append(("primes", primes))
        for dc in (3, 100, 65535):
            q = base.copy()
            q[0] = dc
            out.append((f"ref_dc{dc}", q))
        q = np.array(primes)
        q[structural(8)] = 1
        out.append(("primes_struct1", q))
        out += [(f"rand8_{i}", _rand_u8(8100 + i, nn)) for i in range(2)]
        out += [(f"rand16_{i}", _rand_log16(8200 + i, nn)) for i in range(2)]
    res = []
    for name, q in out:
        q = np.asarray(q, dtype=np.int64)
        assert q.size == nn and q.min() >= 1 and q.max() <= 65535, name
        res.append((name, q.astype(np.uint16)))
    assert len({name for name, _ in res}) == len(res)
    return res


def by_name(n: int, name: str) -> np.ndarray:
    return dict(sweep(n))[name]


def ids(n: int) -> list[str]:
    return [name for name, _ in sweep(n)]


# ---------------------------------------------------------------------------------- ties
TIE_COEFS = 4  # the DC and the three structural coefficients


def tie_index(n: int, c: int) -> int:
    """Natural index of tie coefficient c: 0 the DC, 1..3 the structural ones."""
    return 0 if c == 0 else structural(n)[c - 1]


def tie_pattern(n: int, c: int) -> np.ndarray:
    """The n x n signs s_i s_j of tie coefficient c."""
    s = np.array([1, -1, -1, 1] * (n // 4), dtype=np.int64)
    one = np.ones(n, dtype=np.int64)
    rows, cols = [(one, one), (one, s), (s, one), (s, s)][c]  # (0,N/2) alternates along j
    return np.outer(rows, cols)


def to_blocks(y: np.ndarray, n: int) -> np.ndarray:
    """(..., h, w) frames -> (blocks, n, n) in the encoder's block order."""
    y = y.reshape((-1,) + y.shape[-2:])
    f, h, w = y.shape
    return y.reshape(f, h // n, n, w // n, n).transpose(0, 1, 3, 2, 4).reshape(-1, n, n)


def tie_J(blocks: np.ndarray, n: int, c: int) -> np.ndarray:
    J = (blocks.astype(np.int64) * tie_pattern(n, c)).sum(axis=(1, 2))
    return J - 128 * n * n if c == 0 else J


def tie_reachable(n: int, qk: int) -> bool:
    """Whether some block has J = 2 q (mod 4 q): |J| <= 255 N^2 / 2 for the structural sums."""
    return 2 * int(qk) <= 255 * n * n // 2


def on_tie(blocks: np.ndarray, n: int, q, c: int) -> np.ndarray:
    """The integer rule: which blocks have D / q exactly on a rounding tie for coefficient c."""
    qk = int(np.asarray(q).ravel()[tie_index(n, c)])
    return (tie_J(blocks, n, c) - 2 * qk) % (4 * qk) == 0


def tie_counts(y: np.ndarray, n: int, q) -> list[int]:
    b = to_blocks(y, n)
    return [int(on_tie(b, n, q, c).sum()) for c in range(TIE_COEFS)]


def _land_on_tie(blk: np.ndarray, n: int, qk: int, c: int, rng) -> None:
    """Move one block (int64, in place) to the nearest J = 2 q (mod 4 q) by unit steps on single
    pixels, as few as the distance needs."""
    pat = tie_pattern(n, c)
    J = int((blk * pat).sum()) - (128 * n * n if c == 0 else 0)
    lo = int((np.where(pat < 0, 255, 0) * pat).sum()) - (128 * n * n if c == 0 else 0)
    hi = int((np.where(pat > 0, 255, 0) * pat).sum()) - (128 * n * n if c == 0 else 0)
    m = round((J - 2 * qk) / (4 * qk))
    cands = [2 * qk + 4 * qk * (m + d) for d in (0, -1, 1, -2, 2)]
    cands = sorted((t for t in cands if lo <= t <= hi), key=lambda t: abs(t - J))
    if not cands:
        return
    d = cands[0] - J
    order = rng.permutation(n * n)
    step = max(1, -(-abs(d) // (n * n)))  # a few pixels by 1 when the distance is small
    while d != 0:
        moved = False
        for p in order:
            if d == 0:
                break
            i, j = divmod(int(p), n)
            want = (1 if d > 0 else -1) * int(pat[i, j])  # pixel direction that moves J towards the target
            room = 255 - blk[i, j] if want > 0 else blk[i, j]
            t = min(step, abs(d), int(room))
            if t > 0:
                blk[i, j] += want * t
                d -= (1 if d > 0 else -1) * t
                moved = True
        assert moved  # the target lies in [lo, hi], so some pixel always has room


def tie_frames(n: int, q, w: int, h: int, frames: int = 1, seed: int = 0) -> np.ndarray:
    """(frames, h, w) uint8: low-amplitude noise around a level per block; every fourth block is
    moved onto a rounding tie of the DC or a structural coefficient, the four in turn.
    Coefficients whose quantiser puts the tie out of reach are left as noise."""
    rng = np.random.default_rng(seed)
    q = np.asarray(q).ravel()
    nb = frames * (h // n) * (w // n)
    level = rng.integers(8, 248, size=(nb, 1, 1))
    blocks = np.clip(level + rng.integers(-6, 7, size=(nb, n, n)), 0, 255).astype(np.int64)
    for b in range(0, nb, 4):
        c = (b // 4) % TIE_COEFS
        qk = int(q[tie_index(n, c)])
        if tie_reachable(n, qk):
            _land_on_tie(blocks[b], n, qk, c, rng)
    y = blocks.reshape(frames, h // n, w // n, n, n).transpose(0, 1, 3, 2, 4).reshape(frames, h, w)
    return np.ascontiguousarray(y.astype(np.uint8))


# ---------------------------------------------------------------------------------- content
def noise(shape, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def noise_0_255(shape, seed: int) -> np.ndarray:
    return (np.random.default_rng(seed).integers(0, 2, size=shape) * 255).astype(np.uint8)


def low_noise(shape, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.clip(int(rng.integers(16, 240)) + rng.integers(-3, 4, size=shape), 0, 255).astype(np.uint8)
