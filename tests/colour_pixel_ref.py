"""The numpy statement of the colour operations that are not tables (include/jpgpu.h): HUE — Pillow's rgb2hsv, a shift
of h, hsv2rgb — and SHARPNESS — blend(SMOOTH(P), P, f).  `apply` runs a program that mixes them with the table operations, which it
hands to tests/colour_ref.py.  tests/test_workgroup_colour_pixel.py pins the statement to Pillow's bytes (tests/golden/colour_pixel/), the
emulated kernel bodies to the statement; the GPU tests apply it to the references the other colour tests use.

"f32": rounded to float32 once per written operation; "f64": double."""
import base64

import numpy as np

import colour_ref as CR

HUE, SHARPNESS = 16, 17
NAMES = dict(CR.NAMES, hue=HUE, sharpen=SHARPNESS)
f32, f64 = np.float32, np.float64


def op_id(name):
    return NAMES[name.lower()] if isinstance(name, str) else int(name)


def check_op(op, value):
    """The refusal rule of one operation: ids 9..15 and from 18 on are unknown."""
    v = np.float32(value)
    if op == HUE:
        return bool(np.isfinite(v) and 0 <= v <= 255 and v == np.floor(v))
    if op == SHARPNESS:
        return bool(np.isfinite(v) and 0 <= v <= CR.MAX_FACTOR)
    return CR.check_op(op, value)


def check(program):
    program = list(program)
    return len(program) <= CR.MAX_OPS and all(check_op(op_id(n), v) for n, v in program)


def hue_value(factor):
    """The shift of torchvision's adjust_hue(factor): truncated toward zero, modulo 256."""
    return int(factor * 255) & 255


def rgb2hsv(a):
    """(..., 3) uint8 RGB -> (..., 3) uint8 HSV, Pillow's convert("HSV")."""
    r, g, b = (a[..., c].astype(np.int32) for c in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    gray = mx == mn
    cr = np.where(gray, 1, mx - mn).astype(f32)  # (a gray pixel divides by 1: its h and s are set to 0 below)
    s = ((mx - mn).astype(f32) / np.where(mx == 0, 1, mx).astype(f32)).astype(f32)
    rc, gc, bc = (((mx - c).astype(f32) / cr).astype(f32) for c in (r, g, b))
    h_r = (bc - gc).astype(f32)
    h_g = ((f64(2.0) + rc.astype(f64)) - bc.astype(f64)).astype(f32)
    h_b = ((f64(4.0) + gc.astype(f64)) - rc.astype(f64)).astype(f32)
    hh = np.where(r == mx, h_r, np.where(g == mx, h_g, h_b))
    hh = np.fmod(hh.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((hh.astype(f64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(f64) * 255.0).astype(np.int32), 0, 255)
    return np.stack([np.where(gray, 0, uh), np.where(gray, 0, us), mx], -1).astype(np.uint8)


def _round(x):
    """C's round for x >= 0: halves away from zero (x - floor(x) is exact)."""
    fl = np.floor(x)
    return (fl + ((x - fl) >= 0.5)).astype(np.int32)


def hsv2rgb(a):
    """(..., 3) uint8 HSV -> (..., 3) uint8 RGB, Pillow's convert("RGB") of an HSV image."""
    h, s = a[..., 0].astype(f32), a[..., 1].astype(f32)
    vi = a[..., 2].astype(np.int32)
    x = h.astype(f64) * 6.0 / 255.0
    i = np.floor(x)
    f = (x - i.astype(f32).astype(f64)).astype(f32)
    fs = (s.astype(f64) / 255.0).astype(f32)
    vd = vi.astype(f64)
    p = _round(vd * (1.0 - fs.astype(f64)))
    q = _round(vd * (1.0 - (fs * f).astype(f32).astype(f64)))
    t = _round(vd * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64))))
    p, q, t = (np.clip(v, 0, 255) for v in (p, q, t))
    k = i.astype(np.int32) % 6
    R = np.choose(k, [vi, q, p, p, t, vi])
    G = np.choose(k, [t, vi, vi, q, p, p])
    B = np.choose(k, [p, p, t, vi, vi, q])
    gray = (a[..., 1] == 0)[..., None]
    return np.where(gray, vi[..., None], np.stack([R, G, B], -1)).astype(np.uint8)


def hue(P, shift):
    hsv = rgb2hsv(P)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) & 255
    return hsv2rgb(hsv)


def smooth(P):
    """ImageFilter.SMOOTH: (1 1 1, 1 5 1, 1 1 1) / 13 in f32 — 0.5, then rows y + 1, y, y - 1, each (left + middle) + right —
    truncated; the outermost rows and columns copied."""
    H, W = P.shape[:2]
    out = P.copy()
    if H < 3 or W < 3:
        return out
    k1, k5 = f32(1.0 / 13), f32(5.0 / 13)
    x = P.astype(f32)

    def row(dy, km):
        r = x[1 + dy:H - 1 + dy]
        return ((r[:, 0:W - 2] * k1).astype(f32) + (r[:, 1:W - 1] * km).astype(f32)).astype(f32) + (r[:, 2:W] * k1).astype(f32)

    ss = np.full((H - 2, W - 2, P.shape[2]), f32(0.5), f32)
    for dy, km in ((1, k1), (0, k5), (-1, k1)):
        ss = (ss + row(dy, km).astype(f32)).astype(f32)
    out[1:-1, 1:-1] = np.clip(ss.astype(np.int32), 0, 255)
    return out


def sharpness(P, f):
    return CR.blend(smooth(P), P, f)


def apply_op(P, op, value):
    op = op_id(op)
    if op == HUE:
        return hue(P, int(value))
    if op == SHARPNESS:
        return sharpness(P, value)
    return CR.apply_op(P, op, value)


def apply(P, program):
    """The program (a list of (name or id, value) pairs; None: empty) on P (H x W x 3, uint8)."""
    P = np.ascontiguousarray(P, np.uint8)
    assert P.ndim == 3 and P.shape[2] == 3
    for name, value in (program or []):
        P = apply_op(P, name, value)
    return P.copy() if not program else np.ascontiguousarray(P)


# ---- all 2^24 colours ----

def all_colours():
    """Every RGB colour once, as four images of 2048 x 2048: colour (r, g, b) at flat index r << 16 | g << 8 | b."""
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], -1).astype(np.uint8).reshape(4, 2048, 2048, 3)


def hsv2rgb_table():
    """hsv2rgb of every (h, s, v) -> uint32 r | g << 8 | b << 16 at index h << 16 | s << 8 | v: the factors of p, q and t once per
    (h, s), their products with v and the roundings per entry — the same operations as hsv2rgb, in the same formats."""
    h, s = np.meshgrid(np.arange(256, dtype=f32), np.arange(256, dtype=f32), indexing="ij")
    x = h.astype(f64) * 6.0 / 255.0
    i = np.floor(x)
    f = (x - i.astype(f32).astype(f64)).astype(f32)
    fs = (s.astype(f64) / 255.0).astype(f32)
    vd = np.arange(256, dtype=f64)
    v = np.broadcast_to(np.arange(256, dtype=np.uint32), (256, 256, 256))
    p, q, t = (np.clip(_round(a[..., None] * vd), 0, 255).astype(np.uint32) for a in
               (1.0 - fs.astype(f64), 1.0 - (fs * f).astype(f32).astype(f64), 1.0 - fs.astype(f64) * (1.0 - f.astype(f64))))
    out = np.empty((256, 256, 256), np.uint32)
    k = i.astype(np.int32) % 6
    for n, (R, G, B) in enumerate(((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))):
        m = k == n
        out[m] = R[m] | (G[m] << 8) | (B[m] << 16)
    out[:, 0, :] = np.arange(256, dtype=np.uint32) * 0x010101  # (s == 0)
    return out.reshape(-1)


class RoundTrip:
    """HUE over all colours for any shift: rgb2hsv of every colour once, hsv2rgb of every (h, s, v) once as a table."""

    def __init__(self):
        hsv = rgb2hsv(all_colours().reshape(-1, 3)).astype(np.uint32)
        self.h, self.sv = hsv[:, 0], (hsv[:, 1] << 8) | hsv[:, 2]
        self.table = hsv2rgb_table()

    def hue(self, shift):
        packed = self.table[(((self.h + np.uint32(shift)) & 255) << 16) | self.sv]
        return np.ascontiguousarray(packed.view(np.uint8).reshape(-1, 4)[:, :3]).reshape(4, 2048, 2048, 3)


# ---- the golden file's inputs ----

def make_input(c):
    """colour_ref's inputs, and 'checker': a checkerboard of 0 and 255."""
    if "checker" in c:
        yy, xx = np.mgrid[0:c["H"], 0:c["W"]]
        return np.broadcast_to((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], (c["H"], c["W"], 3)).copy()
    return CR.make_input(c)


def expected(c):
    return np.frombuffer(base64.b64decode(c["expect"]), np.uint8).reshape(c["H"], c["W"], 3)
