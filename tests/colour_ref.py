"""The numpy statement of the colour operations (include/jpgpu.h): a program of Pillow operations on a u8 image of
H x W x 3, each operation on the current image.  tests/test_workgroup_colour.py pins it to Pillow's bytes (tests/golden/colour/), the library's
host functions and the emulated kernel bodies to it; the GPU tests apply it to the existing references.

`rounded` (blend rounds instead of truncating) and `clip` = False (EQUALIZE's table wraps instead of clipping at 255) are the two wrong
statements the golden set must tell from the right one."""
import base64

import numpy as np

IDENTITY, BRIGHTNESS, CONTRAST, COLOR, SOLARIZE, POSTERIZE, INVERT, AUTOCONTRAST, EQUALIZE = range(9)
NAMES = {"identity": 0, "brightness": 1, "contrast": 2, "saturation": 3, "color": 3, "solarize": 4, "posterize": 5, "invert": 6, "autocontrast": 7, "equalize": 8}
MAX_OPS, MAX_FACTOR = 4, 256.0


def op_id(name):
    return NAMES[name.lower()] if isinstance(name, str) else int(name)


def check_op(op, value):
    """The refusal rule of one operation."""
    v = np.float32(value)
    if not 0 <= op <= 8:
        return False
    if op in (BRIGHTNESS, CONTRAST, COLOR):
        return bool(np.isfinite(v) and 0 <= v <= MAX_FACTOR)
    if op == SOLARIZE:
        return bool(np.isfinite(v) and 0 <= v <= 256 and v == np.floor(v))
    if op == POSTERIZE:
        return bool(np.isfinite(v) and 1 <= v <= 8 and v == np.floor(v))
    return True


def check(program):
    program = list(program)
    return len(program) <= MAX_OPS and all(check_op(op_id(n), v) for n, v in program)


def blend(a, b, f, rounded=False):
    """blend(a, b, f) of integer arrays in 0..255: float32, the product and the sum rounded once each, truncated."""
    f = np.float32(f)
    a = np.asarray(a, np.int32)
    b = np.asarray(b, np.int32)
    d = (b - a).astype(np.float32)
    prod = (f * d).astype(np.float32)
    t = (a.astype(np.float32) + prod).astype(np.float32)
    if rounded:
        t = np.floor(t + np.float32(0.5))
    if 0 <= f <= 1:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def luma(P):
    P = P.astype(np.uint32)
    return (P[..., 0] * 19595 + P[..., 1] * 38470 + P[..., 2] * 7471 + 0x8000) >> 16


def mean(P):
    s, n = int(luma(P).sum()), P.shape[0] * P.shape[1]
    m = int(s / n + 0.5)
    assert m == (2 * s + n) // (2 * n)
    return m


def point_lut(op, value, m=0, rounded=False):
    i = np.arange(256, dtype=np.int32)
    if op == BRIGHTNESS:
        return blend(np.zeros(256, np.int32), i, value, rounded)
    if op == CONTRAST:
        return blend(np.full(256, m, np.int32), i, value, rounded)
    if op == SOLARIZE:
        return np.where(i < int(value), i, 255 - i).astype(np.uint8)
    if op == POSTERIZE:
        return (i & ~((1 << (8 - int(value))) - 1) & 255).astype(np.uint8)
    if op == INVERT:
        return (255 - i).astype(np.uint8)
    return i.astype(np.uint8)


def autocontrast_lut(h):
    present = np.nonzero(np.asarray(h))[0]
    if len(present) == 0 or present[-1] <= present[0]:
        return np.arange(256, dtype=np.uint8)
    lo, hi = int(present[0]), int(present[-1])
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(max(int(i * scale + offset), 0), 255) for i in range(256)], np.uint8)


def equalize_lut(h, clip=True):
    h = [int(v) for v in h]
    nz = [v for v in h if v]
    if len(nz) <= 1:
        return np.arange(256, dtype=np.uint8)
    step = (sum(nz) - nz[-1]) // 255
    if not step:
        return np.arange(256, dtype=np.uint8)
    acc, lut = step // 2, []
    for i in range(256):
        lut.append(min(acc // step, 255) if clip else (acc // step) & 255)
        acc += h[i]
    return np.array(lut, np.uint8)


def histograms(P):
    return [np.bincount(P[..., c].reshape(-1), minlength=256) for c in range(3)]


def apply_op(P, op, value, rounded=False, clip=True):
    op = op_id(op)
    if op == IDENTITY:
        return P.copy()
    if op == COLOR:
        y = luma(P).astype(np.int32)[..., None]
        return blend(np.broadcast_to(y, P.shape), P, value, rounded)
    if op == AUTOCONTRAST:
        luts = [autocontrast_lut(h) for h in histograms(P)]
    elif op == EQUALIZE:
        luts = [equalize_lut(h, clip) for h in histograms(P)]
    else:
        luts = [point_lut(op, value, mean(P) if op == CONTRAST else 0, rounded)] * 3
    return np.stack([luts[c][P[..., c]] for c in range(3)], axis=-1)


def apply(P, program, rounded=False, clip=True):
    """The program (a list of (name or id, value) pairs; None: empty) on P (H x W x 3, uint8)."""
    P = np.ascontiguousarray(P, np.uint8)
    assert P.ndim == 3 and P.shape[2] == 3
    for name, value in (program or []):
        P = apply_op(P, name, value, rounded, clip)
    return P.copy() if not program else P


# ---- the golden file's inputs ----

def make_input(c):
    """A case's input image (H x W x 3): 'seed' with an optional value range, 'const', 'rows' ([value, count] runs of whole rows),
    or 'pixels' (inline)."""
    H, W = c["H"], c["W"]
    if "pixels" in c:
        return np.array(c["pixels"], np.uint8).reshape(H, W, 3)
    if "const" in c:
        return np.broadcast_to(np.array(c["const"], np.uint8), (H, W, 3)).copy()
    if "rows" in c:
        vals = np.concatenate([np.full(n, v, np.uint8) for v, n in c["rows"]])
        assert len(vals) == H
        return np.broadcast_to(vals[:, None, None], (H, W, 3)).copy()
    lo, hi = c.get("range", [0, 256])
    return np.random.default_rng(c["seed"]).integers(lo, hi, (H, W, 3), dtype=np.uint8)


def expected(c):
    return np.frombuffer(base64.b64decode(c["expect"]), np.uint8).reshape(c["H"], c["W"], 3)
