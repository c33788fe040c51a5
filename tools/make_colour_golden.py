#!/usr/bin/env python3
"""Writes tests/golden/colour/pillow_colour.json: what Pillow gives for programs of colour operations — ImageEnhance.Brightness /
Contrast / Color, ImageOps.solarize / posterize / invert / autocontrast / equalize — on small RGB images, the expected bytes inline
(base64).  tests/test_workgroup_colour.py holds tests/colour_ref.py — the numpy statement of DESIGN.md §4.20 — to every case, without Pillow.
Needs Pillow (the file records the version used).

A case is its input (tests/colour_ref.py: make_input — a seed with an optional value range, a constant, runs of rows, or inline pixels;
at most 24 x 24, and the 30 x 30 two-level image) and its program, a list of [name, value]."""
import base64
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "colour", "pillow_colour.json")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import colour_ref as CR  # noqa: E402  (the inputs alone: make_input)

FACTORS = (0.0, 1.0, 0.37, 1.9)


def cases():
    out = []

    def add(inp, program):
        out.append(dict(inp, program=[[n, float(v)] for n, v in program]))

    rnd = lambda seed, H=12, W=20, **kw: dict({"seed": seed, "H": H, "W": W}, **kw)  # noqa: E731
    seed = 100
    # every operation alone; the factors reach both blend branches and the clamps at 0 and 255
    for name in ("brightness", "contrast", "saturation"):
        for f in FACTORS + (0.5, 3.0, 256.0):
            seed += 1
            add(rnd(seed), [(name, f)])
    for t in (0, 1, 128, 255, 256):
        seed += 1
        add(rnd(seed), [("solarize", t)])
    for b in (1, 2, 4, 7, 8):
        seed += 1
        add(rnd(seed), [("posterize", b)])
    add(rnd(seed + 1), [("invert", 0)])
    add(rnd(seed + 2), [("identity", 0)])
    add(rnd(seed + 3), [])
    seed += 3
    # AUTOCONTRAST: the whole range, narrow ranges, ranges of one and two values; EQUALIZE: sizes with step 0, 1, 2
    for lo, hi in ((0, 256), (50, 181), (3, 250), (100, 102), (77, 78), (0, 2), (254, 256), (10, 138)):
        seed += 1
        add(rnd(seed, 16, 16, range=[lo, hi]), [("autocontrast", 0)])
    for H, W, rng in ((24, 24, [0, 256]), (16, 16, [0, 256]), (20, 23, [40, 90]), (8, 8, [0, 256]), (24, 24, [0, 4]), (1, 2, [0, 256]), (17, 19, [200, 256])):
        seed += 1
        add(rnd(seed, H, W, range=rng), [("equalize", 0)])
    # the degenerate ones, each its own branch
    for program in ([("autocontrast", 0)], [("equalize", 0)], [("contrast", 0.37)], [("saturation", 1.9)]):
        add({"const": [9, 200, 77], "H": 7, "W": 5}, program)
    two_24 = {"rows": [[0, 20], [3, 2], [200, 2]], "H": 24, "W": 24}   # step 2, the clip at 255 behind value 3
    two_30 = {"rows": [[0, 26], [3, 2], [200, 2]], "H": 30, "W": 30}   # step 3
    for inp in (two_24, two_30):
        add(inp, [("equalize", 0)])
        add(inp, [("autocontrast", 0)])
    half = {"pixels": [10, 10, 10, 11, 11, 11], "H": 1, "W": 2}         # L = 10 and 11: the mean rounds at .5
    for f in FACTORS:
        add(half, [("contrast", f)])
    add({"pixels": [10, 10, 10, 11, 11, 11, 10, 10, 10], "H": 1, "W": 3}, [("contrast", 0.0)])  # (mean 10.33)
    # programs of 2..4 operations: statistics behind point operations and behind COLOR
    programs = [[("brightness", 1.9), ("autocontrast", 0)], [("saturation", 0.37), ("equalize", 0)], [("saturation", 0.0), ("contrast", 1.9)],
                [("solarize", 128), ("contrast", 1.9), ("saturation", 0.0), ("autocontrast", 0)], [("posterize", 3), ("saturation", 1.9), ("contrast", 0.37)],
                [("invert", 0), ("equalize", 0), ("brightness", 0.37)], [("contrast", 0.37), ("autocontrast", 0), ("equalize", 0), ("saturation", 1.9)],
                [("brightness", 0.37), ("saturation", 1.9), ("equalize", 0), ("autocontrast", 0)], [("equalize", 0), ("equalize", 0)],
                [("autocontrast", 0), ("posterize", 2), ("autocontrast", 0), ("invert", 0)]]
    for k, program in enumerate(programs):
        add(rnd(900 + k, 24, 24, range=[[0, 256], [30, 200]][k % 2]), program)
        add(rnd(950 + k, 13, 17), program)
    add(two_24, [("brightness", 1.9), ("equalize", 0), ("saturation", 0.37)])
    return out


def pillow(P, program):
    from PIL import Image, ImageEnhance, ImageOps
    im = Image.fromarray(P, "RGB")
    for name, v in program:
        if name == "brightness":
            im = ImageEnhance.Brightness(im).enhance(v)
        elif name == "contrast":
            im = ImageEnhance.Contrast(im).enhance(v)
        elif name == "saturation":
            im = ImageEnhance.Color(im).enhance(v)
        elif name == "solarize":
            im = ImageOps.solarize(im, int(v))
        elif name == "posterize":
            im = ImageOps.posterize(im, int(v))
        elif name == "invert":
            im = ImageOps.invert(im)
        elif name == "autocontrast":
            im = ImageOps.autocontrast(im)
        elif name == "equalize":
            im = ImageOps.equalize(im)
        elif name != "identity":
            raise ValueError(name)
    return np.asarray(im)


def main():
    import PIL
    rows = []
    for c in cases():
        P = CR.make_input(c)
        got = pillow(P, c["program"])
        assert got.shape == P.shape and got.dtype == np.uint8
        rows.append(dict(c, expect=base64.b64encode(np.ascontiguousarray(got).tobytes()).decode()))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write('{"pillow": "%s", "cases": [\n' % PIL.__version__)
        fh.write(",\n".join(json.dumps(r) for r in rows))
        fh.write("\n]}\n")
    print(f"{len(rows)} cases -> {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
