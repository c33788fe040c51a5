#!/usr/bin/env python3
"""Writes tests/golden/rgb/pillow_cmyk_to_rgb.json: what Pillow's Image.convert("RGB") gives for the pixel formats the decoder writes
(DESIGN.md §4.12).  tests/test_rgb.py holds tests/rgb_ref.py — the numpy statement — to it, without Pillow.  Needs Pillow (the file
records the version used).

  table_sha256  sha256 of convert("RGB") of the CMYK image a[X, K] = (X, X, X, K) for all 65,536 (X, K) pairs, as 256 x 256 x 3 bytes
  pixels        explicit (C, M, Y, K) -> (R, G, B): K = 0, K = 255, X = 0, X = 255 and the half-way roundings of X * (255 - K) / 255
  gray          convert("RGB") of the L image arange(256), as 256 (R, G, B) triples
  cases         whole convert("RGB").resize((ow, oh), BILINEAR) runs of seeded random images of 1 and 4 channels, as sha256 hashes;
                the input of (seed, H, W, C) is np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "rgb", "pillow_cmyk_to_rgb.json")

# (H, W, C, ow, oh)
CASES = [(9, 17, 1, 224, 224), (9, 17, 4, 224, 224), (97, 161, 1, 37, 53), (97, 161, 4, 37, 53), (480, 640, 4, 224, 224), (34, 50, 1, 50, 34),
         (34, 50, 4, 50, 34), (1, 1, 4, 1, 1)]


def pixels():
    px = [(0, 0, 0, 0), (255, 255, 255, 0), (0, 0, 0, 255), (255, 255, 255, 255), (0, 128, 255, 0), (0, 128, 255, 255), (17, 99, 200, 0),
          (0, 255, 0, 77), (255, 0, 255, 200), (1, 2, 3, 254), (254, 253, 252, 1), (128, 128, 128, 128), (127, 128, 129, 127)]
    # half-way roundings: X * nk = 255 m + 127 / 128 for some m (t = X nk + 128 crosses a multiple of 255 there)
    seen = 0
    for k in range(1, 255):
        nk = 255 - k
        for x in range(1, 255):
            if (x * nk) % 255 in (127, 128) and seen < 24 and (x + k) % 7 == 0:
                px.append((x, 255 - x, (x * 3) & 255, k))
                seen += 1
    return px


def main():
    import PIL
    from PIL import Image
    X, K = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    table = np.asarray(Image.fromarray(np.ascontiguousarray(np.stack([X, X, X, K], axis=2)), "CMYK").convert("RGB"))
    px = pixels()
    a = np.array(px, np.uint8).reshape(1, -1, 4)
    rgb = np.asarray(Image.fromarray(a, "CMYK").convert("RGB")).reshape(-1, 3)
    gray = np.asarray(Image.fromarray(np.arange(256, dtype=np.uint8).reshape(1, 256), "L").convert("RGB")).reshape(256, 3)
    rows = []
    for k, (H, W, C, ow, oh) in enumerate(CASES):
        seed = 300 + k
        a = np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)
        im = Image.fromarray(a[:, :, 0] if C == 1 else a, {1: "L", 4: "CMYK"}[C])
        got = np.asarray(im.convert("RGB").resize((ow, oh), Image.BILINEAR)).reshape(oh, ow, 3)
        rows.append({"seed": seed, "H": H, "W": W, "C": C, "ow": ow, "oh": oh, "sha256": hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()})
    doc = {"pillow": PIL.__version__, "table_sha256": hashlib.sha256(np.ascontiguousarray(table).tobytes()).hexdigest(),
           "pixels": [{"cmyk": list(map(int, p)), "rgb": list(map(int, r))} for p, r in zip(px, rgb)],
           "gray": [list(map(int, r)) for r in gray], "filter": "BILINEAR", "cases": rows}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(json.dumps(doc, separators=(",", ":")).replace('},{', '},\n{').replace('"gray":', '\n"gray":').replace('"cases":', '\n"cases":'))
        f.write("\n")
    print(f"{len(px)} pixels, {len(rows)} cases -> {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
