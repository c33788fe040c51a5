#!/usr/bin/env python3
"""Writes tests/golden/resample/pillow_bilinear.json: what Pillow's Image.resize((ow, oh), BILINEAR) gives for seeded random images, as
sha256 hashes.  tests/test_resample.py holds tests/resample_ref.py — the numpy statement of DESIGN.md §4.10 — to every case, without
Pillow.  Needs Pillow (any version whose 8-bit resample has PRECISION_BITS = 22; the file records the one used).

A case is (seed, H, W, C, ow, oh); its input is np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8).  No case has
H > 100 W with oh < H: there Pillow's Python wrapper runs the vertical pass first (reducing_gap aside, Image.resize picks the order
that touches fewer pixels), which differs by +-1 from the horizontal-first order this project defines."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "resample", "pillow_bilinear.json")

FIXED = [(1080, 1920, 3, 224, 224), (540, 960, 3, 224, 224), (17, 23, 3, 224, 224), (224, 224, 3, 224, 224), (300, 224, 3, 224, 224),
         (224, 500, 3, 224, 224), (533, 801, 1, 224, 224), (97, 1301, 4, 256, 192), (1, 1, 3, 8, 8), (1, 1, 1, 1, 1), (640, 480, 3, 299, 299),
         (1200, 2000, 3, 37, 53), (3, 1079, 3, 300, 5), (64, 64, 4, 1, 1), (5, 5, 1, 2048, 3), (2160, 3840, 1, 224, 224), (480, 640, 4, 640, 480)]


def cases():
    out = [(100 + k, *c) for k, c in enumerate(FIXED)]
    rng = np.random.default_rng(2024)
    while len(out) < 40:
        H, W, C = int(rng.integers(1, 1200)), int(rng.integers(1, 2000)), int(rng.choice([1, 3, 4]))
        ow, oh = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        if H > 100 * W and oh < H:
            continue
        out.append((1000 + len(out), H, W, C, ow, oh))
    return out


def main():
    import PIL
    from PIL import Image
    rows = []
    for seed, H, W, C, ow, oh in cases():
        assert not (H > 100 * W and oh < H)
        a = np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)
        im = Image.fromarray(a[:, :, 0] if C == 1 else a, {1: "L", 3: "RGB", 4: "CMYK"}[C])
        got = np.asarray(im.resize((ow, oh), Image.BILINEAR)).reshape(oh, ow, C)
        rows.append({"seed": seed, "H": H, "W": W, "C": C, "ow": ow, "oh": oh, "sha256": hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()})
    with open(OUT, "w") as f:
        json.dump({"pillow": PIL.__version__, "filter": "BILINEAR", "cases": rows}, f, indent=1)
        f.write("\n")
    print(f"{len(rows)} cases -> {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
