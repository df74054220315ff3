"""The device decoders on valid streams that no encoder here writes (tests/crafted_streams.py).

Every entry of the table goes through
  * Codec.decode_image_file on the default exact parse (composed transfer tables),
  * the same with the speculative parse first (ie_set_exact_parse(ctx, 0)), whichever way it went,
  * ie_decode_images, batched with the other entries of its settings (the boundary sweep and the
    fuzz images are a few launches in all): host streams to host pixels, and device streams read
    in place to device pixels with a stride larger than W,
and must equal the oracle's pixels (np.array_equal, the first differing block reported) and the
md5 of the REFERENCE's own decode (tests/golden/manifest_crafted.json).  The oracle's pixels are
computed once per entry and shared.  A P-frame video with bl = 0 and bl = 15 records in its I- and
P-frames (the entry gop_case of tests/crafted_videos.py, whose table tests/test_gpu_crafted_videos.py
runs in full) goes through ie_decode_gop against the oracle's decode_video_gop.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import crafted_streams as CS
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

MANIFEST = {m["name"]: m for m in json.load(open(os.path.join(O.GOLDEN, "manifest_crafted.json")))}
_CODECS = {}
_REF = {}


def _codec(n):
    """One context per block size for the whole module."""
    if n not in _CODECS:
        from imageencoder_amd import Codec
        _CODECS[n] = Codec(0, CS.matrix(n, "ref"), n)
    return _CODECS[n]


def _ref(e) -> np.ndarray:
    if e.name not in _REF:
        px = np.asarray(O.load().decode_image(e.data, e.n)).reshape(e.h, e.w)
        px.setflags(write=False)
        _REF[e.name] = px
    return _REF[e.name]


def _check(e, got, route):
    ref = _ref(e)
    got = np.asarray(got).reshape(e.h, e.w)
    if not np.array_equal(got, ref):
        n = e.n
        bad = (got != ref).reshape(e.h // n, n, e.w // n, n).any(axis=(1, 3)).ravel()
        b = int(np.argmax(bad))
        by, bx = divmod(b, e.w // n)
        rec = e.records()[b]
        raise AssertionError(f"{e.name} [{route}]: {int(bad.sum())} of {bad.size} blocks differ, first block {b} "
                             f"(bl {rec[0]}, lw {rec[1]}, bit {e.file()[1][b]}):\n got {got[by * n:(by + 1) * n, bx * n:(bx + 1) * n].tolist()}\n"
                             f" ref {ref[by * n:(by + 1) * n, bx * n:(bx + 1) * n].tolist()}")
    assert hashlib.md5(got.tobytes()).hexdigest() == MANIFEST[e.name]["dec_md5"], (e.name, route, "reference md5")


# ------------------------------------------------------------------ 1. files, exact and speculative
@pytest.mark.parametrize("name", [e.name for e in CS.entries()])
def test_file_exact_and_speculative_parse(name):
    e = CS.by_name(name)
    c = _codec(e.n)
    _check(e, c.decode_image_file(e.data, e.n), "file, exact parse")
    assert not c.last_decode_spec()
    if e.family == "big":  # the chunk plan restated on the CPU (test_crafted_streams) is the library's
        C, counts = e.chunk_record_counts()
        span = 8 * len(e.data) - e.file()[1][0]
        assert c.last_decode_info()[0] == (span + C - 1) // C and counts.max() > 256
    try:
        c.set_exact_parse(False)
        got = c.decode_image_file(e.data, e.n)
        went = c.last_decode_spec()
    finally:
        c.set_exact_parse(True)
    _check(e, got, f"file, speculative parse first ({'kept' if went else 'fell back to the exact parse'})")


# ------------------------------------------------------------------ 2. batches
def _groups():
    g = {}
    for e in CS.entries():
        g.setdefault((e.n, e.rle, e.w, e.h, e.mat), []).append(e)
    return list(g.items())


GROUPS = _groups()


@pytest.mark.parametrize("gi", range(len(GROUPS)), ids=["n{}_{}_{}x{}_{}".format(k[0], "rle" if k[1] else "norle", *k[2:])
                                                        for k, _ in GROUPS])
def test_decode_images_batch(gi):
    """The entries that share their settings as ONE ie_decode_images batch, one image each, behind
    0-3 bytes of padding (start_bit = the header's length + 0, 8, 16, 24: the chunk grid's phase
    against the 32-bit words moves with the group)."""
    import torch
    (n, rle, w, h, mat), es = GROUPS[gi]
    c = _codec(n)
    c.set_quant(CS.matrix(n, mat), n)
    pad = gi % 4
    hb = es[0].file()[1][0]
    assert all(e.file()[1][0] == hb for e in es)
    start = hb + 8 * pad
    pitch = (max(len(e.data) for e in es) + pad + 8 + 15) // 16 * 16
    slots = np.full(len(es) * pitch, 0xFF, dtype=np.uint8)  # (the bytes past every stream are ones)
    for k, e in enumerate(es):
        slots[k * pitch + pad: k * pitch + pad + len(e.data)] = np.frombuffer(e.data, np.uint8)
    nbits = np.array([8 * (pad + len(e.data)) for e in es], dtype=np.uint64)
    ends = np.array([e.file()[1][-1] + 8 * pad for e in es], dtype=np.uint64)
    try:
        out = np.zeros((len(es), h, w), dtype=np.uint8)
        got_ends = c.decode_images(slots, pitch, nbits, w, h, out, start_bit=start, rle=rle)
        for k, e in enumerate(es):
            _check(e, out[k], f"batch of {len(es)}, host")
        assert np.array_equal(got_ends, ends)
        # device streams read in place, device pixels with stride w + 24 and a gap between images
        stride, fp = w + 24, (w + 24) * h + 40
        dst = torch.full((len(es) * fp,), 0xA5, dtype=torch.uint8, device="cuda")
        dev = torch.from_numpy(slots).cuda()
        assert dev.data_ptr() % 16 == 0 and pitch % 16 == 0
        got_ends = c.decode_images(dev, pitch, nbits, w, h, dst, start_bit=start, rle=rle, stride=stride, frame_pitch=fp)
        got = dst.cpu().numpy()
        exp = np.full(len(es) * fp, 0xA5, dtype=np.uint8)
        for k, e in enumerate(es):
            rows = got[k * fp: k * fp + stride * h].reshape(h, stride)
            _check(e, np.ascontiguousarray(rows[:, :w]), f"batch of {len(es)}, device, stride {stride}")
            exp[k * fp: k * fp + stride * h].reshape(h, stride)[:, :w] = _ref(e)
        assert np.array_equal(got, exp)  # the bytes between rows and images are untouched
        assert np.array_equal(got_ends, ends)
    finally:
        c.set_quant(CS.matrix(n, "ref"), n)


def test_batches_cover_the_table():
    assert sorted(e.name for _, es in GROUPS for e in es) == sorted(MANIFEST)
    sizes = {k: len(es) for k, es in GROUPS}
    assert max(sizes.values()) >= 8  # the sweeps really are batches


# ------------------------------------------------------------------ 3. P-frames
@pytest.mark.parametrize("motioncomp", [True])
def test_gop_with_zero_and_full_width_records(motioncomp):
    """I P P, 64x48, records of bl = 0 and bl = 15 in every frame: ie_decode_gop (through the file
    decoder) == the oracle's decode_video_gop.  (The record reader is the one the image entries pin
    against the reference.)"""
    from tests import crafted_videos as CV
    e = CV.by_name("gop_case")
    data = e.data
    exp = O.load().decode_video_gop(data, e.n, motioncomp=motioncomp)
    c = _codec(e.n)
    got, (w, h, f) = c.decode_video_file(data, e.n)
    assert (w, h, f) == (e.w, e.h, e.frames)
    got = got.reshape(f, h * w * 3 // 2)
    ref = np.frombuffer(exp, dtype=np.uint8).reshape(f, h * w * 3 // 2)
    for k in range(f):
        assert np.array_equal(got[k], ref[k]), f"frame {k} ({'I' if k % e.gop == 0 else 'P'})"
