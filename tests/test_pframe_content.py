"""The constructed P-frame contents of imageencoder_amd.synth reach the paths they were built for
(CPU only: the oracle's own output, before any kernel is compared with it): SAD ties, the
own-position skip, clamped candidates, five-bit records, wide records and saturation.
tests/test_gpu_pframe_paths.py runs the same contents through the HIP kernels.
"""
from __future__ import annotations

import numpy as np
import pytest

from imageencoder_amd import synth
from tests import oracle_lib as O

N, W, H, F, SEED = 4, 64, 48, 5, 7
NMB, NB = (W // 16) * (H // 16), (W // N) * (H // N)
ONES = np.ones(N * N, dtype=np.uint16)


def dc_matrix():
    """matrix.txt with a DC quantiser of 4096 (tests/golden/matrix4_dc4096.txt): the DC of any
    prediction error, at most 4 * (255 + 128) = 1532 in magnitude, rounds to 0."""
    q = O.read_matrix("matrix4_dc4096.txt", N)
    assert q[0] == 4096 and np.array_equal(q[1:], O.read_matrix("matrix.txt", N)[1:])
    return q


def _encode(kind, q, gop, merange, rle=True):
    y = synth.frames(kind, W, H, F, SEED)
    buf, end, fb = O.load().encode_gop(y, N, q, gop, merange, rle=rle)
    vec = {f: O.load().gop_vectors(buf, fb, 0, f, W, H, merange) for f in range(F) if f % gop}
    return y, fb, vec


def _mb_origin(mb):
    return (mb % (W // 16)) * 16, (mb // (W // 16)) * 16


def test_static_zero_vectors_and_five_bit_records():
    """Every P-frame follows an I-frame with the same pixels (gop 2): the centre candidate's SAD is
    0, every other one's is positive or skipped, so the vector is (0, 0); the error is 0 and, under
    a DC quantiser above 1024, every record is 4 + 1 + 0 bits (bl = ffs(0) = 1, no field)."""
    mv = O.load().bits_needed(8)
    _, fb, vec = _encode("static", dc_matrix(), 2, 8)
    assert sorted(vec) == [1, 3]
    for f, v in vec.items():
        assert v == [(0, 0)] * NMB
        assert int(fb[f]) == NMB * 2 * mv + 5 * NB
    # under the reference matrix (DC quantiser 2) the constant -128 the error carries is coded
    _, fb, vec = _encode("static", O.read_matrix("matrix.txt", N), 2, 8)
    assert all(v == [(0, 0)] * NMB for v in vec.values())
    assert all(int(fb[f]) > NMB * 2 * mv + 5 * NB for f in vec)


def test_flat_later_candidate_wins():
    """Constant frames: every candidate's SAD is 0, so each level takes its LAST candidate that is
    not skipped.  merange 8 searches radii 4, 2, 1 and the last pattern point is (+1, -1):
    a macroblock for which (mx + 4, my - 4) clamps to a position other than its own moves by
    (4, -4), (2, -2), (1, -1) = (7, -7).  The top right macroblock (mx = W - 16, my = 0) is the
    exception: (+1, -1), then (0, -1), clamp to its own position and are skipped, so (-1, -1)
    wins at radius 4 -- (-4, -4), clamped to (mx - 4, 0) -- and from there (+1, -1) wins twice:
    (-4 + 2 + 1, -4 - 2 - 1) = (-1, -7)."""
    for kind in ("flat128", "flat0255"):
        _, _, vec = _encode(kind, O.read_matrix("matrix.txt", N), F, 8)
        assert sorted(vec) == [1, 2, 3, 4]
        for v in vec.values():
            for mb, got in enumerate(v):
                assert got == ((-1, -7) if _mb_origin(mb) == (W - 16, 0) else (7, -7)), (kind, mb, got)
                assert got != (0, 0)


@pytest.mark.parametrize("kind", ["stripesV", "stripesH"])
def test_stripes_distinct_vectors(kind):
    _, _, vec = _encode(kind, O.read_matrix("matrix.txt", N), F, 8)
    for v in vec.values():
        assert len(set(v)) >= 2, v


@pytest.mark.parametrize("kind", ["checker", "flat0255"])
def test_wide_records_and_saturation(kind):
    """All-ones matrix, RLE off (with RLE on the search finds these contents' exact match and the
    error is one DC field): sixteen fields of 10 bits or more per record, above the 128 bits per
    block of test_slot_pair_fallback_and_two_coefficient_records, and P-frames that decode to both
    0 and 255."""
    o = O.load()
    mv = o.bits_needed(8)
    y, fb, vec = _encode(kind, ONES, F, 8, rle=False)
    rec_bits = sum(int(fb[f]) - NMB * 2 * mv for f in vec)
    assert rec_bits > 128 * NB * len(vec), rec_bits / (NB * len(vec))
    enc = o.encode_video_gop(synth.yuv420(y), W, H, N, ONES, rle=False, gop=F, merange=8)
    dec = np.frombuffer(o.decode_video_gop(enc, N), dtype=np.uint8).reshape(F, W * H * 3 // 2)[:, : W * H]
    pf = dec[sorted(vec)]
    assert pf.min() == 0 and pf.max() == 255, (pf.min(), pf.max())
    if kind == "checker":  # (a flat frame holds one of the two)
        assert all(dec[f].min() == 0 and dec[f].max() == 255 for f in vec)


def test_static_coarse_matrix_overshoots_255():
    """An all-65535 matrix codes no error at all: a P-frame is the reference block + 128, which the
    reconstruction has to clamp at 255 (sums up to 383), and every record is five bits whatever
    the content."""
    o = O.load()
    q = np.full(N * N, 65535, dtype=np.uint16)
    y = synth.frames("static", W, H, F, SEED)
    _, _, fb = o.encode_gop(y, N, q, F, 8)
    mv = o.bits_needed(8)
    assert all(int(fb[f]) == NMB * 2 * mv + 5 * NB for f in range(1, F))
    enc = o.encode_video_gop(synth.yuv420(y), W, H, N, q, gop=F, merange=8)
    dec = np.frombuffer(o.decode_video_gop(enc, N), dtype=np.uint8).reshape(F, W * H * 3 // 2)[:, : W * H]
    assert (y[0].astype(int) + 128).max() > 255 and dec[1].max() == 255


@pytest.mark.parametrize("kind,merange", [("shiftA", 8), ("shiftB", 40)])
def test_shift_true_motion_and_clamped_edge(kind, merange):
    """A translated picture: some macroblock's search descends to the true motion, and some
    macroblock on the frame's edge ends on a vector that points outside the frame (the copied
    block is the clamped one, Frame.cpp:221-224)."""
    _, _, vec = _encode(kind, O.read_matrix("matrix.txt", N), F, merange)
    for f, v in vec.items():
        assert synth.SHIFTS[kind] in v, (f, v)
    outside = 0
    for v in vec.values():
        for mb, (vx, vy) in enumerate(v):
            mx, my = _mb_origin(mb)
            edge = mx in (0, W - 16) or my in (0, H - 16)
            outside += edge and not (0 <= mx + vx <= W - 16 and 0 <= my + vy <= H - 16)
    assert outside >= 1


def test_coarse_matrix_on_noise_clamps_both_ways():
    """An all-255 matrix on noise (gop 2: every P-frame follows an I-frame) misses the error by up
    to +-63 per coefficient, so the reconstruction leaves [0, 255] on both sides: the decode holds
    more 0 and more 255 pixels than the source frame."""
    o = O.load()
    q = np.full(N * N, 255, dtype=np.uint16)
    y = synth.frames("U", W, H, F, SEED)
    enc = o.encode_video_gop(synth.yuv420(y), W, H, N, q, gop=2, merange=8)
    dec = np.frombuffer(o.decode_video_gop(enc, N), dtype=np.uint8).reshape(F, W * H * 3 // 2)[:, : W * H]
    assert (dec[1] == 0).sum() > (y[1] == 0).sum() and (dec[1] == 255).sum() > (y[1] == 255).sum()
