"""The numpy statement of DESIGN.md §4.16: Pillow's Image.transform(size, Image.AFFINE, m, resample, fillcolor=) for 8-bit images of
1, 3 or 4 channels — rule N (NEAREST, 16.16 fixed point), rule N-sep (NEAREST with m[1] == m[3] == 0: an index table per axis) and rule
B (BILINEAR in IEEE double, truncated) — and the refusal rule.  Python floats are IEEE doubles and numpy's float64 arithmetic rounds
once per operation, so every statement below is one rounding, as in the C they restate."""
import math

import numpy as np

NEAREST, BILINEAR = 0, 1
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
MAX_COEF, MAX_POS = 16000.0, 32000.0


def check(m, ow, oh):
    """True when the matrix is accepted for an output of ow x oh."""
    m = [float(v) for v in m]
    if len(m) != 6 or not all(math.isfinite(v) for v in m):
        return False
    if max(abs(m[0]), abs(m[1]), abs(m[3]), abs(m[4])) > MAX_COEF:
        return False
    for Y in (0.0, float(oh)):
        for X in (0.0, float(ow)):
            px = (X * m[0] + Y * m[1]) + m[2]
            py = (X * m[3] + Y * m[4]) + m[5]
            if not abs(px) <= MAX_POS or not abs(py) <= MAX_POS:
                return False
    return True


def fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def nearest_axis(a, b, out_size):
    """The N-sep index table of one axis (jpgpu_warp_nearest_axis): int32, -1 left of the source."""
    a, b = float(a), float(b)
    idx = np.empty(out_size, np.int32)
    xo = b + a * 0.5
    for x in range(out_size):
        idx[x] = -1 if not xo >= 0.0 else (2147483647 if xo >= 2147483647.0 else int(xo))
        xo = xo + a
    return idx


def _fill_image(src, fill):
    H, W, C = src.shape
    out = np.empty((H, W, C), np.uint8)
    out[:] = np.asarray(list(fill)[:C] + [0] * max(0, C - len(fill)), np.uint8)[:C]
    return out


def nearest_fixed(src, m, fill=(0, 0, 0, 0)):
    """Rule N whatever m[1] and m[3] are (the test of the N-sep cases asks what it WOULD give)."""
    H, W, _ = src.shape
    m = [float(v) for v in m]
    a0, a1, a3, a4 = fix(m[0]), fix(m[1]), fix(m[3]), fix(m[4])
    a2 = fix(m[2] + m[0] * 0.5 + m[1] * 0.5)
    a5 = fix(m[5] + m[3] * 0.5 + m[4] * 0.5)
    X = np.arange(W, dtype=np.int64)[None, :]
    Y = np.arange(H, dtype=np.int64)[:, None]
    xi = (a2 + X * a0 + Y * a1) >> 16
    yi = (a5 + X * a3 + Y * a4) >> 16
    ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
    out = _fill_image(src, fill)
    out[ok] = src[yi[ok], xi[ok]]
    return out


def nearest_separable(src, m, fill=(0, 0, 0, 0)):
    H, W, _ = src.shape
    xs, ys = nearest_axis(m[0], m[2], W).astype(np.int64), nearest_axis(m[4], m[5], H).astype(np.int64)
    okx, oky = (xs >= 0) & (xs < W), (ys >= 0) & (ys < H)
    ok = oky[:, None] & okx[None, :]
    out = _fill_image(src, fill)
    yi, xi = np.broadcast_to(ys[:, None], (H, W)), np.broadcast_to(xs[None, :], (H, W))
    out[ok] = src[yi[ok], xi[ok]]
    return out


def bilinear(src, m, fill=(0, 0, 0, 0), rounded=False):
    """Rule B.  rounded=True: the last step rounded to nearest instead of truncated — what Pillow does NOT do (the golden test's control)."""
    H, W, C = src.shape
    m = [np.float64(v) for v in m]
    xin = np.arange(W, dtype=np.float64)[None, :] + 0.5
    yin = np.arange(H, dtype=np.float64)[:, None] + 0.5
    xo = (m[0] * xin + m[1] * yin) + m[2]
    yo = (m[3] * xin + m[4] * yin) + m[5]
    ok = ~((xo < 0) | (xo >= W) | (yo < 0) | (yo >= H))
    xo, yo = np.where(ok, xo, 0.5) - 0.5, np.where(ok, yo, 0.5) - 0.5
    x, y = np.floor(xo), np.floor(yo)
    dx, dy = (xo - x)[..., None], (yo - y)[..., None]
    x, y = x.astype(np.int64), y.astype(np.int64)
    x0, x1, r0 = np.clip(x, 0, W - 1), np.clip(x + 1, 0, W - 1), np.clip(y, 0, H - 1)
    p = src.astype(np.float64)
    v1 = p[r0, x0] + (p[r0, x1] - p[r0, x0]) * dx
    two = (y + 1 >= 0) & (y + 1 < H)
    r1 = np.where(two, y + 1, r0)
    v2 = np.where(two[..., None], p[r1, x0] + (p[r1, x1] - p[r1, x0]) * dx, v1)
    v = v1 + (v2 - v1) * dy
    px = (np.floor(v + 0.5) if rounded else np.trunc(v)).astype(np.int64).clip(0, 255).astype(np.uint8)
    out = _fill_image(src, fill)
    out[ok] = px[ok]
    return out


def warp(src, m, filter=NEAREST, fill=(0, 0, 0, 0)):
    """`src`: (H, W, C) uint8 -> the warped image of the same size."""
    src = np.ascontiguousarray(src, np.uint8)
    if src.ndim == 2:
        src = src[:, :, None]
    if filter == BILINEAR:
        return bilinear(src, m, fill)
    if float(m[1]) == 0.0 and float(m[3]) == 0.0:
        return nearest_separable(src, m, fill)
    return nearest_fixed(src, m, fill)


def rotate_matrix(angle, size, center=None, translate=None):
    """The six coefficients Image.rotate builds without `expand` (the package's rotate_matrix restated)."""
    w, h = size
    angle = angle % 360.0
    cx, cy = (w / 2.0, h / 2.0) if center is None else center
    tx, ty = (0, 0) if translate is None else translate
    r = -math.radians(angle)
    mt = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]

    def T(x, y):
        a, b, c, d, e, f = mt
        return a * x + b * y + c, d * x + e * y + f

    mt[2], mt[5] = T(-cx - tx, -cy - ty)
    mt[2] += cx
    mt[5] += cy
    return tuple(mt)
