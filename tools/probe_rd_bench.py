#!/usr/bin/env python3
"""ie_probe_rd against the loop it replaces, on one 3840 x 2160 frame of uniform noise and one of
the smooth synthetic (the protocol of tools/probe_bench.py).

For 4x4 and 8x8 blocks and K = 1, 8, 32, 64 candidate matrices (scales of the block size's golden
matrix along the budget ladder), two ways to the same K sizes and K squared errors, timed in the
same process and alternating:

  probe  one Codec.probe_rd call, device frame in, host results out (one synchronisation);
  loop   what the library offered before: for every candidate set_quant (host table build, a
         synchronisation), encode_frames into a device scratch stream, decode_frames into a device
         frame and a torch squared-error sum on the device, read back.

Both are host wall times around calls that end in a device synchronisation.  Every (frame, n, K) is
warmed up, then timed `--reps` times alternately; the medians and the spread (min .. max) are
printed and, with --out, written as text.  The two answers are compared before anything is timed.

    python3 tools/probe_rd_bench.py --reps 15 --out profiles/probe_rd.txt

--sizes-only times Codec.probe_sizes alone (the same frames and candidates), for comparing two
builds of the library (IE_LIB) with each other.
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


def _fmt(t):
    return f"{statistics.median(t):>9.3f} ({min(t):.3f} .. {max(t):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes-only", action="store_true")
    a = ap.parse_args()

    import torch

    from imageencoder_amd import Codec, budget_ladder, read_matrix, scale_matrix, stream_bound, synth

    if a.sizes_only:
        lines = [f"ie_probe_sizes alone; one {W} x {H} frame, device input, host sizes; host wall ms, median (min .. max) "
                 f"of {a.reps} runs; library: {os.environ.get('IE_LIB', 'this build')}",
                 f"{'frame':>6} {'n':>2} {'K':>3} {'probe_sizes ms':>28}"]
    else:
        lines = [f"ie_probe_rd vs set_quant + encode_frames + decode_frames + torch SSE per candidate; one {W} x {H} frame, "
                 f"device input, host results; host wall ms, median (min .. max) of {a.reps} alternating runs",
                 f"{'frame':>6} {'n':>2} {'K':>3} {'probe_rd ms':>28} {'loop ms':>30} {'loop/probe':>10}"]
    ladder = budget_ladder()
    frames = (("noise", synth.frame("U", W, H, seed=1)), ("smooth", synth.smooth(W, H, seed=1)))
    for fname, yh in frames:
        y = torch.from_numpy(np.ascontiguousarray(yh)).cuda()
        yl = y.long()
        for n, mfile in ((4, "matrix.txt"), (8, "matrix8_1.txt")):
            base = read_matrix(os.path.join(ROOT, "tests", "golden", mfile), n)
            codec = Codec(0, base, n)
            scratch = torch.zeros(stream_bound(W, H, n), dtype=torch.uint8, device="cuda")
            dec = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
            for K in KS:
                # K scales along the ladder, around 100 %; distinct matrices
                pcs = [ladder[8]] if K == 1 else [ladder[(i * 32) // K] + (i % (K // 32) if K > 32 else 0) for i in range(K)]
                qs = np.stack([scale_matrix(base, p) for p in pcs])

                def sizes():
                    return codec.probe_sizes(y, W, H, qs)[:, 0]

                def probe():
                    b, s = codec.probe_rd(y, W, H, qs)
                    return b[:, 0], s[:, 0]

                def loop():
                    bits = np.zeros(K, dtype=np.uint64)
                    sse = torch.zeros(K, dtype=torch.int64, device="cuda")
                    for m in range(K):
                        codec.set_quant(qs[m], n)
                        fb, _ = codec.encode_frames(y, W, H, scratch)
                        codec.decode_frames(scratch, W, H, dec)
                        d = dec.long() - yl
                        sse[m] = (d * d).sum()
                        bits[m] = fb[0]
                    return bits, sse.cpu().numpy().astype(np.uint64)

                if a.sizes_only:
                    for _ in range(a.warmup):
                        sizes()
                    ts = []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        sizes()
                        ts.append((time.perf_counter() - t0) * 1e3)
                    lines.append(f"{fname:>6} {n:>2} {K:>3} {_fmt(ts)}")
                    print(lines[-1], flush=True)
                    continue
                pb, ps = probe()
                lb, ls = loop()
                codec.set_quant(base, n)
                assert np.array_equal(pb, lb) and np.array_equal(ps, ls), (fname, n, K)
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
                lines.append(f"{fname:>6} {n:>2} {K:>3} {_fmt(tp)} {_fmt(tl)} "
                             f"{statistics.median(tl) / statistics.median(tp):>9.1f}x")
                print(lines[-1], flush=True)
            codec.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
