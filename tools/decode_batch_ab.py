"""Batched against looped record decode, alternating in ONE process: 16 device-resident 3840x2160
4x4 streams decoded (a) by a loop of 16 ie_decode_frames calls and (b) by one ie_decode_images
call, device input and output, both on the same context.

usage: python tools/decode_batch_ab.py [--reps 15] [--images 16] [--w 3840 --h 2160] [--n 4]

Two input sets, seeded: `noise` (16 U frames) and `mixed` (constant, M and U frames in one batch).
Every repetition times (a) then (b) with a host clock around calls that end in a stream
synchronisation (both entry points wait for their results); prints, per set, the median us per
image of both, the spread of (a) over the repetitions (min, max, quartiles), and whether the
difference of the medians exceeds (a)'s max - min.  The outputs of (a) and (b) are compared byte
for byte before timing.

The walk-again share (decode waves whose chunk holds more than kRecPosCap = 256 records and is
walked again instead of read from its position list) needs no profiling build for this workload: it
is estimated on the host from the end bits -- an image whose records average more than 256 per
chunk of the batch's chunk length takes it in (nearly) all its waves, the others in none (their
records average 24 per chunk) -- and printed as the share of the batch's non-empty decode waves.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from imageencoder_amd import Codec, read_matrix, stream_bound, synth, write_header  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4)
ap.add_argument("--images", type=int, default=16)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--w", type=int, default=3840)
ap.add_argument("--h", type=int, default=2160)
args = ap.parse_args()
assert args.reps >= 11, "at least 11 repetitions"

n, w, h, cnt = args.n, args.w, args.h, args.images
golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
q = read_matrix(os.path.join(golden, "matrix.txt" if n == 4 else "matrix8_1.txt"), n)
codec = Codec(0, q, n)
hb = write_header(n, q, True, w, h)[1]
nblocks = (w // n) * (h // n)


def make_set(name):
    if name == "noise":
        return synth.uniform_device(w, h, cnt, 3, "cuda", torch)
    y = torch.empty((cnt, h, w), dtype=torch.uint8, device="cuda")
    noise = synth.uniform_device(w, h, cnt, 5, "cuda", torch)
    for k in range(cnt):  # constant (128: 5-bit records; 77), M and U frames in turn
        kind = k % 4
        if kind == 0:
            y[k] = 128 if k % 8 == 0 else 77
        elif kind == 1 or kind == 3:
            y[k] = noise[k]
        else:
            y[k] = torch.from_numpy(synth.frame("M", w, h, seed=40 + k)).cuda()
    return y


def chunk_bits(span):
    recs = 24 if n == 4 else 28
    want = max((nblocks + recs - 1) // recs, 1)
    c = (span + want - 1) // want
    return min(max((c + 31) // 32 * 32, 256), 1 << 15)


def run_set(name):
    y = make_set(name)
    pitch = (stream_bound(w, h, n, 1, hb) + 15) // 16 * 16
    enc = torch.zeros(cnt * pitch, dtype=torch.uint8, device="cuda")
    ends = codec.encode_images(y, w, h, enc, pitch, cnt, start_bit=hb)
    del y
    lens = [(int(e) + 7) // 8 for e in ends]
    slots = [enc[k * pitch:] for k in range(cnt)]
    pix_a = torch.zeros((cnt, h, w), dtype=torch.uint8, device="cuda")
    pix_b = torch.zeros_like(pix_a)

    def loop():
        return [codec.decode_frames(slots[k], w, h, pix_a[k], start_bit=hb, length=lens[k]) for k in range(cnt)]

    def batch():
        return codec.decode_images(enc, pitch, ends, w, h, pix_b, start_bit=hb)

    ea, eb = loop(), batch()
    assert [int(e) for e in eb] == ea == [int(e) for e in ends], "end bits differ"
    assert torch.equal(pix_a, pix_b), "pixels differ"
    chunks, levels = codec.last_decode_info()
    for _ in range(args.warmup):
        loop()
        batch()
    ta, tb = [], []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop()
        t1 = time.perf_counter()
        batch()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e6 / cnt)
        tb.append((t2 - t1) * 1e6 / cnt)
    # walk-again estimate from the end bits (see the module text)
    spans = [int(e) - hb for e in ends]
    cb = chunk_bits(8 * max(lens) - hb)
    waves = [((s + cb - 1) // cb + 1) // 2 for s in spans]
    again = [wv for s, wv in zip(spans, waves) if nblocks / max((s + cb - 1) // cb, 1) > 256]
    qa = statistics.quantiles(ta, n=4)
    med_a, med_b = statistics.median(ta), statistics.median(tb)
    spread = max(ta) - min(ta)
    print(f"[{name}] {cnt} x {w}x{h} {n}x{n}, chunk bits {cb}, chunks/image {chunks}, levels {levels}, reps {args.reps}")
    print(f"[{name}] (a) loop of ie_decode_frames : median {med_a:8.1f} us/image  min {min(ta):8.1f}  max {max(ta):8.1f}"
          f"  q1 {qa[0]:8.1f}  q3 {qa[2]:8.1f}  spread(max-min) {spread:6.1f}")
    print(f"[{name}] (b) one ie_decode_images     : median {med_b:8.1f} us/image  min {min(tb):8.1f}  max {max(tb):8.1f}")
    print(f"[{name}] gain {med_a - med_b:8.1f} us/image ({med_a / med_b:.2f}x); exceeds (a)'s spread: {med_a - med_b > spread}")
    print(f"[{name}] walk-again (estimated from the end bits): {len(again)} of {cnt} images, "
          f"{sum(again)} of {sum(waves)} non-empty decode waves ({100.0 * sum(again) / max(sum(waves), 1):.1f} %)")
    print(f"[{name}] raw (a) us/image: " + " ".join(f"{t:.1f}" for t in ta))
    print(f"[{name}] raw (b) us/image: " + " ".join(f"{t:.1f}" for t in tb))


for s in ("noise", "mixed"):
    run_set(s)
codec.close()
