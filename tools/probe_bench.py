#!/usr/bin/env python3
"""ie_probe_sizes against the loop it replaces, on one 3840 x 2160 synthetic frame.

For 4x4 and 8x8 blocks and K = 1, 8, 32, 64 candidate matrices (scales of the block size's golden
matrix), two ways to the same K sizes, timed in the same process and alternating:

  probe  one Codec.probe_sizes call, device frame in, host sizes out (one synchronisation);
  loop   what the library offered before: for every candidate set_quant (host table build, a
         synchronisation) and encode_frames into a device scratch stream, reading frame_bits.

Both are host wall times around calls that end in a device synchronisation.  Every (n, K) pair is
warmed up, then timed `--reps` times alternately; the medians and the spread (min .. max) are
printed and, with --out, written as text.  The two answers are compared before anything is timed.

    python3 tools/probe_bench.py --reps 15 --out profiles/probe_sizes.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160
KS = (1, 8, 32, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from imageencoder_amd import Codec, read_matrix, scale_matrix, stream_bound, synth

    lines = [f"ie_probe_sizes vs set_quant + encode_frames per candidate; one {W} x {H} frame (synth U, seed 1), "
             f"device input, host sizes; host wall ms, median (min .. max) of {a.reps} alternating runs",
             f"{'n':>2} {'K':>3} {'probe ms':>26} {'loop ms':>28} {'loop/probe':>10}"]
    y = torch.from_numpy(synth.frame("U", W, H, seed=1)).cuda()
    for n, mfile in ((4, "matrix.txt"), (8, "matrix8_1.txt")):
        base = read_matrix(os.path.join(ROOT, "tests", "golden", mfile), n)
        codec = Codec(0, base, n)
        scratch = torch.zeros(stream_bound(W, H, n), dtype=torch.uint8, device="cuda")
        for K in KS:
            qs = np.stack([scale_matrix(base, 40 + 9 * k) for k in range(K)])

            def probe():
                return codec.probe_sizes(y, W, H, qs)[:, 0]

            def loop():
                out = np.zeros(K, dtype=np.uint64)
                for m in range(K):
                    codec.set_quant(qs[m], n)
                    fb, _ = codec.encode_frames(y, W, H, scratch)
                    out[m] = fb[0]
                return out

            assert np.array_equal(probe(), loop()), (n, K)
            for _ in range(a.warmup):
                probe()
                loop()
            tp, tl = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                probe()
                t1 = time.perf_counter()
                loop()
                t2 = time.perf_counter()
                tp.append((t1 - t0) * 1e3)
                tl.append((t2 - t1) * 1e3)
            mp, ml = statistics.median(tp), statistics.median(tl)
            lines.append(f"{n:>2} {K:>3} {mp:>9.3f} ({min(tp):.3f} .. {max(tp):.3f}) {ml:>10.3f} ({min(tl):.3f} .. {max(tl):.3f}) "
                         f"{ml / mp:>9.1f}x")
            print(lines[-1], flush=True)
        codec.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
