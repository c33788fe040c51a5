"""The seeded plan of the output-stage fuzzer (tools/fuzz_gpu_output.py, tests/test_gpu_output_fuzz.py, tests/test_output_fuzz_plan.py):
rounds of 2-6 images through everything behind "a fixed output size" — windows, the five filters, RGB output, tensor formats with flips,
placements, warps and the JPGPU_RS_ROLL knob — crossed.  No GPU and no library in here: numpy and the
tests/*_ref.py statements only.  A round is a plain dict of ints, floats, strings, lists, tuples and None, so `repr` of it is the
fuzzer's `--replay` argument.

    round = {"kind": the template's name (information only),
             "images": [{"layout": "420" | "444" | "gray" | "cmyk444", "w", "h": the frame's size, "coef": "sparse" | "hostile" (the
                         sources of test_gpu_resize._case) | "block" (test_gpu_filters.block_case: 0 / 255 blocks of 8 by x 8 bx pixels),
                         "by", "bx", "seed", "scale": 8 | 4 | 2 | 1 (reduced IDCT; block sources: 8), "window": (x, y, w, h) | None}, ...],
             "size": (ow, oh), "filter": name, "rgb": bool, "tensor": dtype name | None,
             "flips": [first decode's, second decode's] | None (None without a tensor),
             "placements": [(rw, rh, x, y) | None per image] | None, "fill": four bytes,
             "warp": None | {"filter": "nearest" | "bilinear", "fill": four bytes, "warps": [first decode's, second decode's] (six floats or
                             None per image), "pins": [{"set", "image", "px", "py", "axis", "target", "value"}, ...]},
             "roll": None | 1 | 2 | 4 | 8 (JPGPU_RS_ROLL: unset, or that value),
             "pipeline": None | {"files": [(layout, encoder, (w, h), pic), ...], "windows": [...], "fit": (mode, size) | None}}

The templates take turns (SCHEDULE); inside one everything else is drawn from the seed.  Shapes are the smallest that reach a branch:
sources of 9..100 x 7..64, outputs of 1..64 on a side (224 now and then), and for the chunked, rb == 1 and run plans the shapes of
tests/test_gpu_filters.py."""
import numpy as np

import filter_ref as F
import tensor_ref as T
import warp_ref as WR

FILTERS = ["bilinear", "box", "hamming", "bicubic", "lanczos"]
WIDE = ("bicubic", "lanczos")
NC = {"420": 3, "444": 3, "gray": 1, "cmyk444": 4}
LAYOUTS = list(NC)
DTYPES = ["float32", "float16", "bfloat16"]
FORMATS = {"float32": T.IMAGENET, "float16": T.CLIP, "bfloat16": T.HALF}  # dtype -> (mean, std): the formats of tests/test_gpu_tensor.py
ROLLS = (None, 1, 2, 4, 8)
PFILL, WFILL = (114, 7, 200, 33), (9, 250, 77, 140)
MAX_SIDE = 2048
# the turn of the templates; its length is odd, so that the pipeline leg (every fourth round) meets every template
SCHEDULE = ["plain", "tensor", "placed", "warp", "run", "forced", "chunked", "placed-warp", "rb1", "tensor", "forced-warp", "chunked-placed", "run"]
# files of the pipeline leg: (layout, encoder, size argument of test_gpu_pipeline_windows._file, picture) and the size the file decodes to
# (the four-component ones are fixtures of tests/golden/reftest: their sizes are what they are)
FILES = [(("420", "base", (161, 97)), (161, 97, 3)), (("444", "base", (97, 61)), (97, 61, 3)), (("gray", "base", (97, 61)), (97, 61, 1)),
         (("420", "base", (50, 34)), (50, 34, 3)), (("cmyk", "base", (32, 32)), (32, 32, 4)), (("cmyk", "base", (256, 256)), (256, 256, 4)),
         (("ycck", "base", (161, 97)), (500, 333, 4)), (("gray", "base", (50, 34)), (50, 34, 1))]


class _State:
    """Counters that make the turns even: window residues per channel count, tensor formats, placement kinds, matrix kinds."""

    def __init__(self, seed):
        self.seed = seed
        self.res = {1: seed, 3: seed + 1, 4: seed + 2}
        self.dtype = seed
        self.place = seed
        self.matrix = seed
        self.roll = seed
        self.window = seed
        self.file = seed
        self.turns = {}

    def turn(self, kind):
        """How often the template has had its turn."""
        self.turns[kind] = self.turns.get(kind, 0) + 1
        return self.turns[kind] - 1


def source_size(img):
    """(W, H) of the image's whole output: the frame at its reduced scale."""
    s = img["scale"]
    return -(-img["w"] * s // 8), -(-img["h"] * s // 8)


def effective_size(img):
    """(w, h) of what the image gives without an output size: its window, or its whole output."""
    win = img["window"]
    return (win[2], win[3]) if win is not None else source_size(img)


def _image(rng, layout, w, h, coef, scale=8, by=1, bx=1):
    return {"layout": layout, "w": int(w), "h": int(h), "coef": coef, "by": int(by), "bx": int(bx), "seed": int(rng.integers(0, 1 << 30)), "scale": int(scale),
            "window": None}


def _small_image(rng, layout, name):
    """9..100 x 7..64: a block source under the wide filters (both clamps), else one of test_gpu_resize._case, now and then reduced."""
    w, h = int(rng.integers(9, 101)), int(rng.integers(7, 65))
    if name in WIDE:
        return _image(rng, layout, w, h, "block")
    scale = int(rng.choice([4, 2, 1])) if int(rng.integers(0, 5)) == 0 else 8
    return _image(rng, layout, w, h, "hostile" if int(rng.integers(0, 6)) == 0 else "sparse", scale)


def _x_with_residue(rng, st, nc, lo, hi):
    """x in [lo, hi] whose byte offset x * nc takes the next residue modulo 4 (what the horizontal pass's aligned dwords see)."""
    want = st.res[nc] % 4
    st.res[nc] += 1
    cand = [x for x in range(lo, hi + 1) if (x * nc) % 4 == want]
    return int(cand[int(rng.integers(0, len(cand)))]) if cand else int(rng.integers(lo, hi + 1))


def _window(rng, st, img, size, mode=None):
    """A window of the image: "one" (1 x 1), "equal" (the output's size where it fits), "odd" (anything, x by residue)."""
    W, H = source_size(img)
    nc = NC[img["layout"]]
    if mode is None:
        mode = ["odd", "odd", "one", "equal", "odd", "none", "odd", "equal"][st.window % 8]
        st.window += 1
    if mode == "none" or W < 5 or H < 2:
        return None
    if mode == "one":
        return (_x_with_residue(rng, st, nc, 0, W - 1), int(rng.integers(0, H)), 1, 1)
    if mode == "equal" and size[0] <= W - 3 and size[1] <= H:
        ww, hh = size
    elif mode == "equal-w" and size[0] <= W - 3:
        ww, hh = size[0], int(rng.integers(1, H + 1))
    else:
        ww, hh = int(rng.integers(max(1, W // 3), W - 2)), int(rng.integers(max(1, H // 3), H + 1))
    return (_x_with_residue(rng, st, nc, 0, W - ww), int(rng.integers(0, H - hh + 1)), int(ww), int(hh))


def _out_size(rng, four=None):
    """1..64 on a side; 1 x 1 and 224 x 224 now and then.  four: True a width that is a multiple of four, False one that is not."""
    pick = int(rng.integers(0, 10))
    if pick == 0 and not four:
        return (1, 1)
    if pick == 1 and four is not False:
        return (224, 224)
    ow, oh = int(rng.integers(1, 65)), int(rng.integers(1, 65))
    if four is True:
        ow = max(4, ow & ~3)
    elif four is False and ow % 4 == 0:
        ow += 1 + int(rng.integers(0, 3))
    return (ow, oh)


def _flips(rng, n):
    """Two lists with both values in each (one image: one of each over the two decodes)."""
    a = [bool(v) for v in rng.integers(0, 2, n)]
    a[0], a[-1] = True, (False if n > 1 else True)
    b = [not v for v in a] if n > 1 else [False]
    return [a, b]


def _dtype(st):
    st.dtype += 1
    return DTYPES[st.dtype % 3]


# ---- placements ---------------------------------------------------------------------------------------------------------------------------
def _placement(rng, st, size):
    """(rw, rh, x, y) by turns: padded on every side, cropped at negative x and y, one visible column, one visible row, a letterbox, a
    pillar box, none.  The first visible column takes the values 0..15 in turn, so that `shift` = (vx * nc) & 15 takes many."""
    ow, oh = size
    kind = st.place % 8
    st.place += 1
    vx = st.place * 5 % 16  # (5 is coprime with 16: every value in sixteen turns)
    if kind == 7 or ow < 4 or oh < 4:
        if kind % 2 or ow < 2 or oh < 2:
            return None
        return (int(rng.integers(1, 2 * ow + 1)), int(rng.integers(1, 2 * oh + 1)), -int(rng.integers(0, 2)), int(rng.integers(0, 2)))  # (tiny canvases)
    if kind == 0:  # fill on all four sides, rows above the image that are no multiple of its bands
        x, y = min(vx, ow - 2), int(rng.integers(1, max(2, oh // 2)))
        return (int(rng.integers(1, ow - x)), int(rng.integers(1, oh - y)), x, y)
    if kind == 1:  # cropped left and top: range tables with first > 0
        rw, rh = int(rng.integers(ow // 2 + 2, 2 * ow + 2)), int(rng.integers(oh // 2 + 2, 2 * oh + 2))
        return (rw, rh, -int(rng.integers(1, rw - ow // 2)), -int(rng.integers(1, rh - oh // 2)))
    if kind == 2:  # one visible column: at the right edge, or a resample one pixel wide
        if int(rng.integers(0, 2)):
            return (int(rng.integers(2, ow + 2)), int(rng.integers(1, oh + 1)), ow - 1, int(rng.integers(0, 3)))
        return (1, int(rng.integers(1, oh + 1)), min(vx, ow - 1), 0)
    if kind == 3:  # one visible row: the resample's last row at the canvas's first, or a resample one pixel high
        if int(rng.integers(0, 2)):
            rh = int(rng.integers(2, oh + 2))
            return (int(rng.integers(1, ow + 1)), rh, min(vx, ow - 1) if ow > 1 else 0, 1 - rh)
        rw = int(rng.integers(1, ow + 1))
        return (rw, 1, int(rng.integers(0, ow - rw + 1)), int(rng.integers(0, oh)))
    if kind == 4:  # letterbox: fill above and below
        rh = int(rng.integers(1, oh - 1))
        return (ow, rh, 0, (oh - rh) // 2)
    if kind == 5:  # pillar box at a column of its own: fill left and right
        x = min(vx, ow - 2)
        return (int(rng.integers(1, ow - x)), oh, x, 0)
    x = min(vx, ow - 1)  # cropped right and bottom, padded left and top
    y = int(rng.integers(1, oh))
    return (int(rng.integers(ow - x, 2 * ow)), int(rng.integers(oh - y, 2 * oh)), x, y)


def visible(pl, size):
    """(vx, vy, vw, vh) of a placement in the canvas, or None when it shows no pixel."""
    rw, rh, x, y = pl
    x0, x1, y0, y1 = max(x, 0), min(x + rw, size[0]), max(y, 0), min(y + rh, size[1])
    return (x0, y0, x1 - x0, y1 - y0) if (rw > 0 and rh > 0 and x0 < x1 and y0 < y1) else None


# ---- warps --------------------------------------------------------------------------------------------------------------------------------
SEP_KINDS = ["identity", "itrans", "ftrans", "scale", "mirror", "outside", "pin-sep"]
MIX_KINDS = ["rot", "quarter", "shear", "pin-mix", "rot"]


def _pinned(rng, size, mix, target):
    """A matrix built backwards from an output pixel (px, py): on `axis` its source position is exactly 0.0 ("zero"), exactly the
    source's size ("size") or exactly an interior pixel edge ("edge").  Every coefficient is a dyadic rational of a few bits and every
    position a small multiple of 1 / 16, so the doubles of rule B, the 16.16 integers of rule N and the running sums of rule N-sep all
    hold the value exactly (tests/test_output_fuzz_plan.py asserts it on the reference's own arithmetic).  -> (m, pin)."""
    w, h = size
    px, py = int(rng.integers(0, w)), int(rng.integers(0, h))
    axis = int(rng.integers(0, 2))
    n = (w, h)[axis]
    value = 0.0 if target == "zero" else float(n) if target == "size" else float(int(rng.integers(1, n)) if n > 1 else 0)
    a = float(rng.choice([1.0, 0.75, 1.25, 0.5]))
    b = float(rng.choice([0.25, -0.25, 0.5])) if mix else 0.0
    cx, cy = px + 0.5, py + 0.5
    # the pinned axis lands on `value`; the other axis lands on the pixel's own centre (inside the source)
    if axis == 0:
        m = [a, b, value - (a * cx + b * cy), b, 1.0, cy - (b * cx + 1.0 * cy)]
    else:
        m = [1.0, b, cx - (1.0 * cx + b * cy), b, a, value - (b * cx + a * cy)]
    return tuple(float(v) for v in m), {"px": px, "py": py, "axis": axis, "target": target, "value": value}


def _matrix(rng, st, size):
    """-> (six floats or None, pin or None): the separable and the mixing kinds in turn."""
    w, h = size
    k = st.matrix
    st.matrix += 1
    kind = (SEP_KINDS[(k // 2) % len(SEP_KINDS)] if k % 2 == 0 else MIX_KINDS[(k // 2) % len(MIX_KINDS)])
    u = lambda lo, hi: float(rng.uniform(lo, hi))  # noqa: E731
    if kind == "identity":
        return None, None
    if kind == "itrans":
        return (1.0, 0.0, float(int(rng.integers(-3, 4))), 0.0, 1.0, float(int(rng.integers(-3, 4)))), None
    if kind == "ftrans":
        return (1.0, 0.0, u(-4, 4), 0.0, 1.0, u(-4, 4)), None
    if kind == "scale":
        return (u(0.5, 1.6), 0.0, u(-5, 5), 0.0, u(0.5, 1.6), u(-5, 5)), None
    if kind == "mirror":
        return (-1.0, 0.0, float(w), 0.0, 1.0, 0.0), None
    if kind == "outside":
        return (1.0, 0.0, 5000.0, 0.0, 1.0, 5000.0), None
    if kind == "rot":
        return tuple(float(v) for v in WR.rotate_matrix(u(-60, 60), size)), None
    if kind == "quarter":
        return tuple(float(v) for v in WR.rotate_matrix(90, size)), None
    if kind == "shear":
        return (1.0, u(-0.4, 0.4), u(-3, 3), u(-0.4, 0.4), 1.0, u(-3, 3)), None
    return _pinned(rng, size, kind == "pin-mix", ["zero", "size", "edge"][(k // 4) % 3])


def _warp(rng, st, n, size):
    filt = ("nearest", "bilinear")[(st.seed + st.turn("warp filter")) % 2]
    sets, pins = [], []
    for k in range(2):
        ms = []
        for i in range(n):
            m, pin = _matrix(rng, st, size)
            ms.append(m)
            if pin is not None:
                pins.append(dict(pin, set=k, image=i))
        sets.append(ms)
    st.matrix += 1  # (the parity of the next round's kinds moves on)
    return {"filter": filt, "fill": WFILL, "warps": sets, "pins": pins}


# ---- the templates ------------------------------------------------------------------------------------------------------------------------
def _round(kind, images, size, name, rgb=False, tensor=None, flips=None, placements=None, warp=None, roll=None):
    return {"kind": kind, "images": images, "size": tuple(int(v) for v in size), "filter": name, "rgb": bool(rgb), "tensor": tensor, "flips": flips,
            "placements": placements, "fill": PFILL, "warp": warp, "roll": roll, "pipeline": None}


def _mixed_layouts(rng, n):
    """n layouts, mixed inside the batch: the four in a random order, repeated."""
    order = [LAYOUTS[i] for i in rng.permutation(4)]
    return [order[i % 4] for i in range(n)]


def _plain(rng, st, v, tensor=False, placed=False, warp=False):
    n = int(rng.integers(2, 7))
    name = FILTERS[int(rng.integers(0, 5))]
    four = (v % 2 == 0) if tensor else None
    size = _out_size(rng, four)
    if placed and min(size) < 4:
        size = (size[0] + 7, size[1] + 5)
    images = [_small_image(rng, lay, name) for lay in _mixed_layouts(rng, n)]
    for img in images:
        img["window"] = _window(rng, st, img, size)
    fmt = _dtype(st) if (tensor or ((placed or warp) and v % 2)) else None
    if placed and fmt and not warp and size[0] % 4 == 0:
        size = (size[0] + 1, size[1])  # (a placed tensor whose canvas rows are no multiple of four elements)
    pls = None
    if placed:
        pls = [_placement(rng, st, size) for _ in images]
        if all(p is None for p in pls):
            pls[0] = (size[0], max(1, size[1] - 2), 1, 1)
    return _round("plain", images, size, name, rgb=bool(rng.integers(0, 2)), tensor=fmt, flips=_flips(rng, n) if fmt else None, placements=pls,
                  warp=_warp(rng, st, n, size) if warp else None)


def _tall_blocks(rng, layout):
    """64 x ~1080 in 0 / 255 blocks of 16 rows: what the run route's plans are made of."""
    return _image(rng, layout, int(rng.integers(56, 73)), int(rng.integers(1040, 1121)), "block", by=2, bx=1)


def _run(rng, st, v, turn):
    """About 224 x 225 from 64 x ~1080 under a wide filter: bands whose source rows overlap 1.4 / 2.2 times — the rule takes the run
    route — for one-, three- and four-channel sources (two each of gray and CMYK), beside an up-scaled image that keeps its bands.
    By turns: RGB output into tensors, RGB output as bytes with a warp behind it, the sources' own channels into tensors, RGB output
    as bytes — the last one with the knob at `1` (never) every other time."""
    name = WIDE[(v // 4 + turn) % 2]
    size = (int(rng.integers(221, 228)), int(rng.integers(222, 229)))
    images = [_tall_blocks(rng, lay) for lay in ["444", "gray", "cmyk444", "gray", "cmyk444"]]
    images.append(_image(rng, LAYOUTS[int(rng.integers(0, 4))], 97, 61, "block"))
    rgb, tensor, warp = [(True, True, False), (True, False, True), (False, True, False), (True, False, False)][v % 4]
    if warp:
        images[0]["window"] = _window(rng, st, images[0], size, "odd")
    fmt = _dtype(st) if tensor else None
    return _round("run", images, size, name, rgb=rgb, tensor=fmt, flips=_flips(rng, len(images)) if fmt else None,
                  warp=_warp(rng, st, len(images), size) if warp else None, roll=1 if (v % 4 == 3 and turn % 2) else None)


def _forced(rng, st, v, warp=False):
    """JPGPU_RS_ROLL = 2 / 4 / 8 on plans the rule leaves alone: two to four bands of up to 64 rows from small sources (up-scaled: a
    band's first source row can be its neighbour's, shift == 0), and wide outputs whose rows fill LDS after a few.  Every candidate —
    BICUBIC or LANCZOS, at least two one-chunk bands — then takes the route with that many bands per run."""
    st.roll += 1
    roll = (2, 4, 8)[st.roll % 3]
    name = WIDE[(v // 2) % 2]
    n = int(rng.integers(4, 7))
    if v % 2 == 0:  # tall outputs: bands of 64 rows, the last one shorter
        size = (int(rng.integers(5, 41)), int(rng.integers(129, 226)))
        images = [_image(rng, lay, int(rng.integers(9, 101)), int(rng.integers(7, 65)), "block") for lay in _mixed_layouts(rng, n)]
    else:  # wide outputs: LDS holds a dozen rows, bands of a few output rows
        size = (int(rng.integers(400, 601)), int(rng.integers(24, 49)))
        images = [_image(rng, lay, int(rng.integers(9, 101)), int(rng.integers(20, 65)), "block") for lay in _mixed_layouts(rng, n)]
    images[0] = _image(rng, images[0]["layout"], 97, 61, "block")  # (the image of test_runs_of_bands that keeps its bands by the rule)
    for img in images[1:]:
        img["window"] = _window(rng, st, img, size, ["odd", "none", "equal-w"][int(rng.integers(0, 3))])
    fmt = _dtype(st) if v % 4 in (1, 2) else None
    return _round("forced", images, size, name, rgb=bool(v % 3), tensor=fmt, flips=_flips(rng, n) if fmt else None,
                  warp=_warp(rng, st, n, size) if warp else None, roll=roll)


def _chunked(rng, st, v, turn, placed=False):
    """16 x ~1200 to a height of 1 or 3: one output row's source rows take several chunks of LDS.  Two images each of one, three and
    four channels; RGB output, so that every row in LDS has three channels (1200 gray rows of 40 bytes would fit)."""
    name = FILTERS[int(rng.integers(0, 5))]
    ow = int(rng.integers(40, 49))
    images = [_image(rng, lay, int(rng.integers(16, 33)), int(rng.integers(1180, 1241)), "block", by=19, bx=1) for lay in ["444", "gray", "cmyk444", "420", "gray", "cmyk444"]]
    n = len(images)
    if not placed:
        tensor, vh = [(True, 1), (True, 3), (False, (1, 3)[turn % 2])][v % 3]
        fmt = _dtype(st) if tensor else None
        return _round("chunked", images, (ow, vh), name, rgb=True, tensor=fmt, flips=_flips(rng, n) if fmt else None)
    # placed: the visible rows are 1 or 3 of a canvas a little larger; every image's inner job is the chunked one
    tensor, rgb, vh = [(False, True, 3), (True, False, 1), (False, False, 1)][v % 3]
    fmt = _dtype(st) if tensor else None
    size = (ow + int(rng.integers(0, 8)), vh + 2 + int(rng.integers(0, 3)))
    pls = []
    for i, img in enumerate(images):
        x = (st.place * 5 + i) % 16
        rw = int(rng.integers(28, 41))  # (gray without RGB output: 28 visible columns or more, so that 1200 rows do not fit)
        y = int(rng.integers(-1, 3))
        pls.append((rw, vh if y >= 0 else vh + 1, x, y))
    st.place += 1
    return _round("chunked", images, size, name, rgb=rgb, tensor=fmt, flips=_flips(rng, n) if fmt else None, placements=pls)


def _rb1(rng, st, v):
    """Rows so wide that LDS holds four (2048 CMYK pixels) or six (1707 three-channel pixels) of them at an output height equal to the
    source's: one output row's support fits, two neighbours' do not — rb == 1 in ONE chunk.  Such bands overlap four- or sixfold and
    the rule sends them down the run route; every other time the knob is `1` and they stay on the band kernels."""
    name = WIDE[v % 2]
    h = int(rng.integers(8, 17))
    if name == "bicubic":
        size, lays = (2048, h), ["cmyk444", "cmyk444"]
    else:
        size, lays = (1707, h), ["444", "420"]
    images = [_image(rng, lay, int(rng.integers(16, 33)), h, "block") for lay in lays]
    fmt = _dtype(st) if v % 2 else None
    return _round("rb1", images, size, name, tensor=fmt, flips=_flips(rng, len(images)) if fmt else None, roll=1 if (v // 2) % 2 else None)


def _pipeline(rng, st, rd):
    """The pipeline leg of a round: as many files as the round has images, with windows of their own (the files have their own sizes)
    and a fit rule where the round has placements."""
    n = len(rd["images"])
    files, wins = [], []
    for i in range(n):
        (layout, enc, sz), (W, H, nc) = FILES[(st.file + i) % len(FILES)]
        files.append((layout, enc, sz, int(rng.integers(0, 3))))
        if int(rng.integers(0, 3)) == 0:
            wins.append(None)
            continue
        ww, hh = int(rng.integers(max(1, W // 4), W - 2)), int(rng.integers(max(1, H // 4), H + 1))
        wins.append((_x_with_residue(rng, st, nc, 0, W - ww), int(rng.integers(0, H - hh + 1)), ww, hh))
    st.file += n
    fit = None
    if rd["placements"] is not None:
        fit = ("letterbox", 0) if st.file % 2 else ("shorter_side_crop", max(1, min(rd["size"])))
    return {"files": files, "windows": wins, "fit": fit}


def check_round(rd):
    """The documented rules, checked here so that the library never refuses a round: raises AssertionError."""
    n = len(rd["images"])
    ow, oh = rd["size"]
    assert 2 <= n <= 6 and 1 <= ow <= MAX_SIDE and 1 <= oh <= MAX_SIDE, (n, rd["size"])
    assert rd["filter"] in FILTERS and rd["roll"] in ROLLS and rd["tensor"] in (None, *DTYPES)
    assert (rd["flips"] is None) == (rd["tensor"] is None), "flips only with a tensor"
    if rd["flips"] is not None:
        assert len(rd["flips"]) == 2 and all(len(f) == n for f in rd["flips"])
    for img in rd["images"]:
        assert img["layout"] in NC and img["coef"] in ("sparse", "hostile", "block") and img["scale"] in (8, 4, 2, 1)  # (no planar layout at all)
        assert img["coef"] != "block" or img["scale"] == 8
        assert rd["filter"] not in WIDE or img["coef"] == "block", "block sources under the wide filters"
        W, H = source_size(img)
        assert 1 <= W <= 65535 and 1 <= H <= 65535
        win = img["window"]
        if win is not None:
            x, y, w, h = win
            assert x >= 0 and y >= 0 and w >= 1 and h >= 1 and x + w <= W and y + h <= H and (w, h) != (W, H), (win, W, H)
    if rd["placements"] is not None:
        assert len(rd["placements"]) == n
        for pl in rd["placements"]:
            assert pl is None or (0 < pl[0] <= 65535 and 0 < pl[1] <= 65535 and visible(pl, rd["size"]) is not None), ("the placement shows no pixel", pl)
    if rd["warp"] is not None:
        wp = rd["warp"]
        assert wp["filter"] in ("nearest", "bilinear") and len(wp["warps"]) == 2
        for ms in wp["warps"]:
            assert len(ms) == n
            for m in ms:
                assert m is None or WR.check(m, ow, oh), m
    if rd["pipeline"] is not None:
        pp = rd["pipeline"]
        sizes = dict(FILES)
        assert len(pp["files"]) == len(pp["windows"]) == n
        for f, win in zip(pp["files"], pp["windows"]):
            W, H, _nc = sizes[tuple(f[:3])]
            assert win is None or (win[0] >= 0 and win[1] >= 0 and win[2] >= 1 and win[3] >= 1 and win[0] + win[2] <= W and win[1] + win[3] <= H)
    return rd


def plan(seed, rounds):
    """-> the list of `rounds` rounds of `seed`."""
    rng = np.random.default_rng(seed)
    st = _State(int(seed))
    out = []
    for r in range(rounds):
        kind = SCHEDULE[r % len(SCHEDULE)]
        turn = st.turn({"forced-warp": "forced"}.get(kind, kind))
        v = int(seed) + turn  # (the variant: another one at the template's next turn, and for the other seed)
        if kind == "plain":
            rd = _plain(rng, st, v)
        elif kind == "tensor":
            rd = _plain(rng, st, v, tensor=True)
        elif kind == "placed":
            rd = _plain(rng, st, v, placed=True)
        elif kind == "warp":
            rd = _plain(rng, st, v, warp=True)
        elif kind == "placed-warp":
            rd = _plain(rng, st, v, placed=True, warp=True)
        elif kind == "run":
            rd = _run(rng, st, v, turn)
        elif kind == "forced":
            rd = _forced(rng, st, v)
        elif kind == "forced-warp":
            rd = _forced(rng, st, v, warp=True)
        elif kind == "chunked":
            rd = _chunked(rng, st, v, turn)
        elif kind == "chunked-placed":
            rd = _chunked(rng, st, v, turn, placed=True)
        else:
            rd = _rb1(rng, st, v)
        rd["kind"] = kind
        if r % 4 == 3:
            rd["pipeline"] = _pipeline(rng, st, rd)
        out.append(check_round(rd))
    return out


def image_count(rounds):
    """The comparisons the GPU fuzzer owes: every image of both decodes, once more under knob `1` where the round forces a run route,
    and every file of a pipeline leg."""
    total = 0
    for rd in rounds:
        n = len(rd["images"])
        total += 2 * n + (n if rd["roll"] in (2, 4, 8) else 0) + (len(rd["pipeline"]["files"]) if rd["pipeline"] else 0)
    return total


def stand_in(img):
    """A numpy stand-in for the image's effective source, (h, w, nc) u8, for the CPU checks (the GPU leg decodes the real coefficients):
    0 / 255 blocks of 8 by x 8 bx pixels for a block source, noise else — the whole output first, then the window."""
    W, H = source_size(img)
    nc = NC[img["layout"]]
    rng = np.random.default_rng(img["seed"])
    if img["coef"] == "block":
        sy, sx = 8 * img["by"], 8 * img["bx"]
        a = rng.integers(0, 2, (-(-H // sy), -(-W // sx), nc), dtype=np.uint8) * np.uint8(255)
        full = a.repeat(sy, axis=0).repeat(sx, axis=1)[:H, :W]
    else:
        full = rng.integers(0, 256, (H, W, nc), dtype=np.uint8)
    win = img["window"]
    if win is not None:
        x, y, w, h = win
        full = full[y:y + h, x:x + w]
    return np.ascontiguousarray(full)


def filter_id(name):
    return F.NAMES[name]
