"""Scaled decode against the full decode plus a box mean, for one 4K frame of the bench's noise
content (device-resident stream; 4x4 and 8x8; every scale >= 2).  Baseline, the way to the same bytes
without ie_decode_scaled: ie_decode_frames into a device frame, then a torch integer box mean on the
device -- or, with --host, ie_decode_frames into pinned host memory and the box mean there (numpy).
ie_decode_frames alone into the same destination is timed in the same alternation.  The paths
alternate run by run and the medians are compared (buffer placement moves single timings by several
per cent).
usage: python tools/prof_scaled.py [--host] [--runs K] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from imageencoder_amd import Codec, stream_bound, synth  # noqa: E402
from tests import oracle_lib as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--host", action="store_true")
ap.add_argument("--runs", type=int, default=41)
ap.add_argument("--json")
args = ap.parse_args()

w, h = 3840, 2160
rows = []
for n in (4, 8):
    c = Codec(0, O.read_matrix("matrix.txt" if n == 4 else "matrix8_1.txt", n), n)
    y = synth.frame("U", w, h, synth.DEFAULT_SEED)  # the bench's image 0
    out = torch.zeros(stream_bound(w, h, n, 1, 0), dtype=torch.uint8, device="cuda")
    _, end = c.encode_frames(torch.from_numpy(y).cuda(), w, h, out)
    stream = out[: (end + 7) // 8]
    pix = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    hpix = c.host_array(w * h).reshape(h, w) if args.host else None
    for s in (2, 4, 8):
        if s > n:
            continue
        ow, oh = w // s, h // s
        dsc = torch.empty((oh, ow), dtype=torch.uint8, device="cuda")
        dbox = torch.empty((oh, ow), dtype=torch.uint8, device="cuda")
        hsc = c.host_array(ow * oh).reshape(oh, ow) if args.host else None
        hbox = np.empty((oh, ow), dtype=np.uint8)

        def base():
            if args.host:  # the whole frame crosses, the mean is the host's
                c.decode_frames(stream, w, h, hpix)
                sums = hpix.reshape(oh, s, ow, s).sum(axis=(1, 3), dtype=np.uint32)
                np.copyto(hbox, (sums + (s * s) // 2) >> (2 * (s.bit_length() - 1)), casting="unsafe")
            else:
                c.decode_frames(stream, w, h, pix)
                sums = pix.view(oh, s, ow, s).sum(dim=(1, 3), dtype=torch.int32)
                dbox.copy_((sums + (s * s) // 2) >> (2 * (s.bit_length() - 1)))
                torch.cuda.synchronize()

        def scaled():
            c.decode_scaled(stream, w, h, s, out=hsc if args.host else dsc)

        def full_only():
            c.decode_frames(stream, w, h, hpix if args.host else pix)

        for f in (base, scaled, full_only):
            f()
        got = hsc if args.host else dsc.cpu().numpy()
        exp = hbox if args.host else dbox.cpu().numpy()
        assert np.array_equal(got, exp), (n, s)
        t = {"base": [], "scaled": [], "full": []}
        for _ in range(args.runs):  # alternating: every path sees the same drift
            for key, f in (("base", base), ("scaled", scaled), ("full", full_only)):
                t0 = time.perf_counter()
                f()
                t[key].append((time.perf_counter() - t0) * 1e6)
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = {k: (min(v), sorted(v)[len(v) * 9 // 10]) for k, v in t.items()}
        row = {"n": n, "scale": s, "dest": "host" if args.host else "device", "base_us": round(med["base"], 1),
               "scaled_us": round(med["scaled"], 1), "decode_frames_us": round(med["full"], 1),
               "base_over_scaled": round(med["base"] / med["scaled"], 2),
               "decode_frames_over_scaled": round(med["full"] / med["scaled"], 2),
               "scaled_min_p90_us": [round(x, 1) for x in spread["scaled"]],
               "base_min_p90_us": [round(x, 1) for x in spread["base"]],
               "decode_frames_min_p90_us": [round(x, 1) for x in spread["full"]]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    c.close()
if args.json:
    json.dump(rows, open(args.json, "w"), indent=1)
