"""Batched against looped decode of Huffman-coded image FILES, alternating in ONE process: 16
3840x2160 4x4 synth "U" files (host memory) decoded into host pixels (a) by a loop of 16
ieh_decode_image calls and (b) by one ieh_decode_images call, both on the same context.

usage: python tools/decode_files_ab.py [--reps 11] [--images 16] [--w 3840 --h 2160] [--n 4] [--limit 120]

Every repetition times (a) then (b) with a host clock (both entry points return after their last
synchronisation); prints the medians in ms per batch, their ratio (b)/(a), (a)'s spread, how many
files carry a dictionary, IE_DEC_BATCH_MAX and the sub-batch size the 1 GiB scratch rule gives.  The
outputs of (a) and (b) are compared byte for byte before timing.  Every step (making the files, the
comparison, each repetition) runs under --limit seconds: a step that overruns ends the script.
"""
import argparse
import ctypes as C
import os
import signal
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from imageencoder_amd import Codec, load_host_library, read_matrix, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4)
ap.add_argument("--images", type=int, default=16)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--w", type=int, default=3840)
ap.add_argument("--h", type=int, default=2160)
ap.add_argument("--limit", type=int, default=120)
args = ap.parse_args()
assert args.reps >= 11, "at least 11 repetitions"


def overrun(signum, frame):
    print("step over its time limit: stopping", flush=True)
    os._exit(124)


signal.signal(signal.SIGALRM, overrun)


def step(fn, *a):
    signal.alarm(args.limit)
    try:
        return fn(*a)
    finally:
        signal.alarm(0)


n, w, h, cnt = args.n, args.w, args.h, args.images
golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
q = read_matrix(os.path.join(golden, "matrix.txt" if n == 4 else "matrix8_1.txt"), n)
codec = Codec(0, q, n)
H = load_host_library()
u64p = C.POINTER(C.c_uint64)

files = step(lambda: [codec.encode_image_file(synth.frame("U", w, h, seed=3 + k), w, h, q, n, huffman=True)
                      for k in range(cnt)])
coded = sum(codec.huffman_table(f) is not None for f in files)
lens = np.array([len(f) for f in files], dtype=np.uint64)
pitch = (int(lens.max()) + 15) // 16 * 16
src = np.zeros((cnt, pitch), dtype=np.uint8)
for k, f in enumerate(files):
    src[k, : len(f)] = np.frombuffer(f, dtype=np.uint8)
pix_a = np.zeros((cnt, h, w), dtype=np.uint8)
pix_b = np.zeros_like(pix_a)
wo, ho = C.c_int(0), C.c_int(0)


def loop():
    for k in range(cnt):
        r = H.ieh_decode_image(codec.h, src[k].ctypes.data, int(lens[k]), n, pix_a[k].ctypes.data, w * h, C.byref(wo),
                               C.byref(ho))
        assert r == w * h, (k, r, codec.L.ie_last_error(codec.h))


def batch():
    r = H.ieh_decode_images(codec.h, src.ctypes.data, pitch, lens.ctypes.data_as(u64p), cnt, n, pix_b.ctypes.data,
                            cnt * w * h, C.byref(wo), C.byref(ho))
    assert r == cnt * w * h, (r, codec.L.ie_last_error(codec.h))


step(loop)
step(batch)
assert np.array_equal(pix_a, pix_b), "pixels differ"
for _ in range(args.warmup):
    step(loop)
    step(batch)
ta, tb = [], []
for _ in range(args.reps):
    t0 = time.perf_counter()
    step(loop)
    t1 = time.perf_counter()
    step(batch)
    t2 = time.perf_counter()
    ta.append((t1 - t0) * 1e3)
    tb.append((t2 - t1) * 1e3)
med_a, med_b = statistics.median(ta), statistics.median(tb)
# the sub-batch size of ie_huffman_decode_batch: 1 GiB over the per-image scratch (1024-bit chunks;
# per chunk 15 x 2 bytes x (1 + 1/256 + 3) of tables, 16 of entries and bases, 4 of counts)
nch = (8 * int(lens.max()) + 1023) // 1024
sub = max(1, (1 << 30) // (nch * (30 * 4 + 20) + 2048))
env = os.environ.get("IE_DEC_BATCH_MAX")
if env and int(env) > 0:
    sub = min(sub, int(env))
print(f"{cnt} files of {w}x{h} {n}x{n}, {coded} with a dictionary, {int(lens.mean())} bytes on average, reps {args.reps}")
print(f"IE_DEC_BATCH_MAX={env!r}; Huffman sub-batch {min(sub, cnt)} images ({nch} chunks per image)")
print(f"(a) loop of ieh_decode_image : median {med_a:8.2f} ms/batch  min {min(ta):8.2f}  max {max(ta):8.2f}")
print(f"(b) one ieh_decode_images    : median {med_b:8.2f} ms/batch  min {min(tb):8.2f}  max {max(tb):8.2f}")
print(f"ratio (b)/(a) {med_b / med_a:.3f}")
print("raw (a) ms: " + " ".join(f"{t:.2f}" for t in ta))
print("raw (b) ms: " + " ".join(f"{t:.2f}" for t in tb))
codec.close()
