"""bench.py --dump-outputs: the sampling helper on host tensors (fixed offsets, bytes and bits past a
stream's end masked, float32 / float64 files within the size limit) and the option parsing."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _dump(tmp_path, name, buf, rows, pitch, ends):
    import torch
    d = str(tmp_path / name)
    bench.dump_outputs(torch, d, torch.from_numpy(buf), rows, pitch, ends)
    assert sorted(os.listdir(d)) == ["end_bits.npy", "streams.npy"]
    return np.load(os.path.join(d, "streams.npy")), np.load(os.path.join(d, "end_bits.npy"))


def test_small_rows_are_dumped_whole_and_masked(tmp_path):
    rows, pitch = 3, 5000  # rows x pitch below the sample size: every byte is an offset
    buf = np.random.default_rng(3).integers(1, 256, rows * pitch + 17, dtype=np.uint8)
    ends = [8 * 1234 + 3, 8 * 100, 0]  # inside a byte, byte-aligned, empty
    s, e = _dump(tmp_path, "a", buf, rows, pitch, ends)
    assert s.dtype == np.float32 and e.dtype == np.float64 and s.shape == (rows, pitch)
    assert e.tolist() == [float(x) for x in ends]
    b = buf[: rows * pitch].reshape(rows, pitch)
    assert np.array_equal(s[0, :1234], b[0, :1234])
    assert s[0, 1234] == (b[0, 1234] & 0xE0) and not s[0, 1235:].any()  # 3 bits of the last byte
    assert np.array_equal(s[1, :100], b[1, :100]) and not s[1, 100:].any()
    assert not s[2].any()


def test_large_rows_are_sampled_at_fixed_offsets(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_VALUES", 4096)
    monkeypatch.setattr(bench, "DUMP_HEAD", 64)
    rows, pitch = 4, 100003
    # every byte names its own offset (mod 251), so the sample tells which offsets were read
    row = (np.arange(pitch) % 251 + 1).astype(np.uint8)
    buf = np.tile(row, rows)
    ends = [8 * pitch] * rows
    s, _ = _dump(tmp_path, "a", buf, rows, pitch, ends)
    assert s.shape == (rows, 1024) and s.all()
    assert np.array_equal(s[0, :64], row[:64]) and all(np.array_equal(s[0], s[r]) for r in range(rows))
    # the offsets depend on rows and pitch alone: other contents and ends, same positions
    s2, _ = _dump(tmp_path, "b", np.tile(row[::-1].copy(), rows), rows, pitch, [8 * (pitch // 2)] * rows)
    off = _offsets(rows, pitch)
    assert np.array_equal(s[0], row[off])
    assert np.array_equal(s2[0], np.where(off < pitch // 2, row[::-1][off], 0))
    assert 0.4 < (off[64:] < pitch // 2).mean() < 0.6  # the strata cover the row evenly


def _offsets(rows, pitch):
    """The offsets dump_outputs samples, restated."""
    per_row = min(pitch, bench.DUMP_VALUES // rows)
    head = min(bench.DUMP_HEAD, per_row)
    k = per_row - head
    stride = (pitch - head) // k
    return np.concatenate([np.arange(head), head + np.arange(k) * stride
                           + np.random.default_rng(bench.DUMP_SEED).integers(0, stride, k)])


def test_dump_fits_the_size_limit():
    assert 4 * bench.DUMP_VALUES + 8 * 64 <= 64 * 10**6


def test_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"
