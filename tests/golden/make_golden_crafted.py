#!/usr/bin/env python3
"""Pin the reference's decode of every constructed stream (tests/crafted_streams.py).

Like make_golden.py this runs on the CPU where oracle/_ref exists: every file of the table is
decoded by the REFERENCE ITSELF -- its `decoder` for 4x4 blocks, the Block<8> harness for 8x8 --
and manifest_crafted.json records name, n, rle, w, h, the file's md5 and the md5 of the reference's
pixels.  No stream and no pixels are stored: stream_craft.pack rebuilds the files from the table.

Usage:  python tests/golden/make_golden_crafted.py      (rewrites tests/golden/manifest_crafted.json)
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import REF, md5, ref_dec8, ref_decode  # noqa: E402
from tests import crafted_streams  # noqa: E402


def main():
    if not os.path.exists(os.path.join(REF, "decoder")):
        sys.exit("oracle/_ref not built: run `make -C oracle ref` where the reference sources exist")
    manifest = []
    for e in crafted_streams.entries():
        dec = ref_dec8(e.data) if e.n == 8 else ref_decode(e.data)
        assert len(dec) == e.w * e.h, (e.name, len(dec))
        manifest.append(dict(name=e.name, family=e.family, n=e.n, rle=int(e.rle), w=e.w, h=e.h, md5=md5(e.data),
                             dec_md5=md5(dec)))
        print(f"{e.name:28s} {len(e.data):8d} B  {manifest[-1]['dec_md5'][:12]}", flush=True)
    with open(os.path.join(HERE, "manifest_crafted.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
