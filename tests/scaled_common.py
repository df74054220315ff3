"""What the scaled decode's tests share: the frames the streams are encoded from (the seed rule
tests/test_capi_scaled.py checks on the CPU is the one the GPU tests decode) and the expected value,
the numpy box mean of a full decode."""
import numpy as np

from imageencoder_amd import synth


def frames(kind, w, h, count, seed):
    """(count, h, w) uint8: imageencoder_amd.synth content ("U" noise, "M" mixed) or a constant."""
    if isinstance(kind, int):
        return np.full((count, h, w), kind, dtype=np.uint8)
    return synth.frames(kind, w, h, count, seed)


def stream_seed(w, nframes):
    return 7 + w + nframes


def scales(n):
    return [s for s in (1, 2, 4, 8) if s <= n]


def box_sums(full, s):
    """Sums of the s x s cells of the last two axes of a uint8 array, as int64."""
    *lead, h, w = full.shape
    return full.astype(np.int64).reshape(*lead, h // s, s, w // s, s).sum(axis=(-3, -1))


def box(full, s):
    """out[..., Y, X] = (sum of full[..., Y*s+dy, X*s+dx] + s*s/2) >> (2 log2 s): the mean of the
    integer pixels, rounded half up."""
    return ((box_sums(full, s) + (s * s) // 2) // (s * s)).astype(np.uint8)
