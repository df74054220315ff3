#!/usr/bin/env python3
"""Pin the reference's decode of the image files wrapped in constructed Huffman dictionaries
(tests/crafted_huffman.py).

Like make_golden_crafted.py this runs on the CPU where oracle/_ref exists: every wrapped file -- one
per family, an image whose Huffman pass uses that family's dictionary -- is decoded by the REFERENCE
ITSELF (its `decoder`), and manifest_crafted_huffman.json records the entry's name, the image size,
the file's md5, the md5 of the reference's pixels and the md5 of the Huffman-decoded bytes (the
oracle's walk: the reference keeps that stream to itself).  No stream and no pixels are stored:
crafted_huffman.wrapped rebuilds the files from the table.

Usage:  python tests/golden/make_golden_crafted_huffman.py
        (rewrites tests/golden/manifest_crafted_huffman.json)
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import REF, md5, ref_decode  # noqa: E402
from tests import crafted_huffman, oracle_lib  # noqa: E402


def main():
    if not os.path.exists(os.path.join(REF, "decoder")):
        sys.exit("oracle/_ref not built: run `make -C oracle ref` where the reference sources exist")
    manifest = []
    for family in crafted_huffman.WRAPPED:
        name, data, plain = crafted_huffman.wrapped(family)
        w, h = crafted_huffman.wrap_dims(family)
        dec = ref_decode(data)
        assert len(dec) == w * h, (name, len(dec))
        huf = oracle_lib.load().huffman_decode(data)
        assert huf is not None and not huf[1] and huf[0].startswith(plain), name
        manifest.append(dict(name=name, family=family, n=4, w=w, h=h, md5=md5(data), dec_md5=md5(dec), huf_md5=md5(huf[0])))
        print(f"{name:24s} {len(data):8d} B  {manifest[-1]['dec_md5'][:12]}", flush=True)
    with open(os.path.join(HERE, "manifest_crafted_huffman.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
