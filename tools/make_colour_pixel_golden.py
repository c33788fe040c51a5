#!/usr/bin/env python3
"""Writes tests/golden/colour_pixel/: what Pillow gives for the colour operations that are not tables.
    hue_sha256.json        the sha256 of Pillow's bytes over all 2^24 RGB colours (tests/colour_pixel_ref.py: all_colours) for
                           convert("HSV"), h + shift, convert("RGB") — torchvision's adjust_hue on a PIL image — per shift
    pillow_colour_pixel.json   small explicit cases, the expected bytes inline (base64): ImageEnhance.Sharpness at five factors on six
                           sizes (random, constant and checkerboard images), hue on small images, and programs that mix both with the
                           table operations (tools/make_colour_golden.py: pillow)
tests/test_workgroup_colour_pixel.py holds tests/colour_pixel_ref.py to every one of them, without Pillow.  Needs Pillow (the files
record the version used)."""
import base64
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "colour_pixel")
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import colour_pixel_ref as PR  # noqa: E402  (the inputs alone: make_input, all_colours)
import make_colour_golden as MG  # noqa: E402  (Pillow's table operations)

SHIFTS = (0, 1, 43, 128, 213, 255)
FACTORS = (0.0, 0.37, 1.0, 1.9, 256.0)
SIZES = ((1, 1), (2, 5), (5, 2), (3, 3), (7, 5), (33, 17))  # (W, H)
JITTER = [("brightness", 1.2), ("contrast", 0.8), ("saturation", 1.3), ("hue", 43)]


def cases():
    out = []

    def add(inp, program):
        out.append(dict(inp, program=[[n, float(v)] for n, v in program]))

    seed = 2100
    for f in FACTORS:
        for W, H in SIZES:
            seed += 1
            add({"seed": seed, "H": H, "W": W}, [("sharpen", f)])
        add({"const": [9, 200, 77], "H": 5, "W": 7}, [("sharpen", f)])
        add({"checker": 1, "H": 5, "W": 7}, [("sharpen", f)])
        add({"checker": 1, "H": 17, "W": 33}, [("sharpen", f)])
    for k, shift in enumerate(SHIFTS):
        add({"seed": 2200 + k, "H": 17, "W": 33}, [("hue", shift)])
        add({"seed": 2300 + k, "H": 5, "W": 7, "range": [100, 104]}, [("hue", shift)])  # (near-gray pixels: small chroma)
    add({"const": [9, 200, 77], "H": 5, "W": 7}, [("hue", 128)])
    add({"const": [77, 77, 77], "H": 2, "W": 5}, [("hue", 43)])
    # programs that mix the new operations with the table ones
    mixed = [[("sharpen", 1.9), ("contrast", 1.9)], [("sharpen", 0.37), ("contrast", 0.37)], [("hue", 43), ("equalize", 0)], [("hue", 213), ("equalize", 0)],
             JITTER, [JITTER[3], JITTER[1], JITTER[0], JITTER[2]], [("sharpen", 1.9), ("equalize", 0)], [("hue", 1), ("sharpen", 0.0), ("autocontrast", 0), ("sharpen", 256.0)]]
    for k, program in enumerate(mixed):
        add({"seed": 2400 + k, "H": 17, "W": 33}, program)
        add({"seed": 2450 + k, "H": 5, "W": 7, "range": [30, 200]}, program)
    return out


def pillow(P, program):
    from PIL import Image, ImageEnhance
    im = Image.fromarray(P, "RGB")
    for name, v in program:
        if name == "sharpen":
            im = ImageEnhance.Sharpness(im).enhance(v)
        elif name == "hue":
            hsv = np.array(im.convert("HSV"))
            hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(v)) & 255
            im = Image.fromarray(hsv, "HSV").convert("RGB")
        else:
            im = Image.fromarray(MG.pillow(np.asarray(im), [(name, v)]), "RGB")
    return np.asarray(im)


def main():
    import PIL
    os.makedirs(OUT, exist_ok=True)
    rows = []
    for c in cases():
        P = PR.make_input(c)
        got = pillow(P, c["program"])
        assert got.shape == P.shape and got.dtype == np.uint8
        rows.append(dict(c, expect=base64.b64encode(np.ascontiguousarray(got).tobytes()).decode()))
    with open(os.path.join(OUT, "pillow_colour_pixel.json"), "w") as fh:
        fh.write('{"pillow": "%s", "cases": [\n' % PIL.__version__)
        fh.write(",\n".join(json.dumps(r) for r in rows))
        fh.write("\n]}\n")
    colours = PR.all_colours()
    sums = {}
    for shift in SHIFTS:
        h = hashlib.sha256()
        for img in colours:  # (an image at a time: Pillow's own conversions, both ways)
            h.update(np.ascontiguousarray(pillow(img, [("hue", shift)])).tobytes())
        sums[str(shift)] = h.hexdigest()
    with open(os.path.join(OUT, "hue_sha256.json"), "w") as fh:
        json.dump({"pillow": PIL.__version__, "colours": "all 2^24, (r, g, b) at index r << 16 | g << 8 | b", "sha256": sums}, fh, indent=1)
        fh.write("\n")
    print(f"{len(rows)} cases, {len(sums)} shifts -> {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
