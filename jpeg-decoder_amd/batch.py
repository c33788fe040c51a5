"""Batch driver mirror (include/jpgpu.h jpgpu_batch_*): N independent images per launch."""
import ctypes as C
import math

import numpy as np

from . import _native as N
from .colour import program_structs
from .error import check
from .worker import color_transform_id


def image_desc(components, quantization_tables, out_w, out_h, color_transform):
    d = N.ImageDesc()
    d.ncomp = len(components)
    for i, c in enumerate(components):
        d.components[i] = c
        q = np.ascontiguousarray(quantization_tables[i], dtype=np.uint16).reshape(64)
        for k in range(64):
            d.quantization_tables[i][k] = int(q[k])
    d.out_w, d.out_h = out_w, out_h
    d.color_transform = color_transform_id(color_transform)
    return d


def window_structs(windows, n):
    """`windows`: None, one (x, y, w, h) for every image, or a list with a tuple or None per image -> jpgpu_window[n] (or None)."""
    if windows is None:
        return None
    if len(windows) == 4 and all(isinstance(v, (int, np.integer)) for v in windows):
        windows = [tuple(windows)] * n
    if len(windows) != n:
        raise ValueError(f"{len(windows)} windows for {n} images")
    arr = (N.Window * n)()
    for i, w in enumerate(windows):
        if w is not None:
            x, y, ww, hh = (int(v) for v in w)
            if min(x, y, ww, hh) < 0 or max(x, y, ww, hh) > 65535:
                raise ValueError(f"window {w!r} of image {i}")
            arr[i].x, arr[i].y, arr[i].w, arr[i].h = x, y, ww, hh
    return arr


def output_size_pair(output_size):
    """(w, h) of an output size as two ints that fit the C ABI's uint16 (the library checks the range 1..2048 itself)."""
    w, h = (int(v) for v in output_size)
    if min(w, h) < 0 or max(w, h) > 65535:
        raise ValueError(f"output size {output_size!r}")
    return w, h


class TensorFormat:
    """The tensor a decode writes instead of resized bytes (jpgpu_tensor_format): ``dtype`` "float32", "float16" or "bfloat16",
    ``mean`` and ``std`` per channel (up to four; missing channels: mean 0, std 1).  Element (c, r, x) of an image is
    ``T[c][u8[r, x, c]]`` with ``T[c][v] = (v / 255 - mean[c]) / std[c]`` computed in float32, one operation after the other, then rounded
    once to the dtype: what ``torch.from_numpy(u8).permute(2, 0, 1).to(float32).div(255).sub(mean).div(std).to(dtype)``
    gives, bit for bit."""
    DTYPES = {"float32": (N.TENSOR_F32, np.float32), "float16": (N.TENSOR_F16, np.float16), "bfloat16": (N.TENSOR_BF16, np.uint16)}

    def __init__(self, dtype="float32", mean=(0.0, 0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0, 1.0)):
        dtype = str(dtype).replace("torch.", "")
        if dtype not in self.DTYPES:
            raise ValueError(f"tensor dtype {dtype!r}: one of {sorted(self.DTYPES)}")
        mean, std = [float(v) for v in mean], [float(v) for v in std]
        if len(mean) > 4 or len(std) > 4:
            raise ValueError("at most four means / stds")
        self.dtype = dtype
        self.mean = tuple(mean + [0.0] * (4 - len(mean)))
        self.std = tuple(std + [1.0] * (4 - len(std)))

    @property
    def numpy_dtype(self):
        """The dtype of the arrays returned: np.float32, np.float16, and np.uint16 bit patterns for bfloat16 (numpy has no such type)."""
        return self.DTYPES[self.dtype][1]

    @property
    def itemsize(self):
        return np.dtype(self.numpy_dtype).itemsize

    def struct(self):
        s = N.TensorFormatStruct()
        s.dtype, s.reserved = self.DTYPES[self.dtype][0], 0
        for c in range(4):
            s.mean[c], s.std[c] = self.mean[c], self.std[c]
        return s

    def table(self, nc):
        """jpgpu_tensor_table: the (nc, 256) lookup table as the library computes it."""
        out = np.zeros((nc, 256), self.numpy_dtype)
        s = self.struct()
        check(N.lib().jpgpu_tensor_table(C.byref(s), nc, out.ctypes.data), b"jpgpu_tensor_table: refused format")
        return out

    def __repr__(self):
        return f"TensorFormat({self.dtype!r}, mean={self.mean}, std={self.std})"


class Fit:
    """A placement rule (jpgpu_fit): how a source of its own size is laid into the fixed output size.  ``mode`` "stretch" (the whole
    output, today's behaviour), "shorter_side_crop" (torchvision's ``Resize(size)`` then ``CenterCrop``: the evaluation transform) or
    "letterbox" (the aspect-preserving fit with constant padding).  ``fill``: up to four bytes in the output's channel order."""
    MODES = {"stretch": N.FIT_STRETCH, "shorter_side_crop": N.FIT_SHORTER_SIDE_CROP, "letterbox": N.FIT_LETTERBOX}

    def __init__(self, mode="stretch", size=0, fill=(0, 0, 0, 0)):
        if mode not in self.MODES:
            raise ValueError(f"fit mode {mode!r}: one of {sorted(self.MODES)}")
        self.mode, self.size, self.fill = mode, int(size), fill_tuple(fill)

    def struct(self):
        s = N.FitStruct()
        s.mode, s.size, s.reserved = self.MODES[self.mode], self.size, 0
        for c in range(4):
            s.fill[c] = self.fill[c]
        return s

    def __repr__(self):
        return f"Fit({self.mode!r}, size={self.size}, fill={self.fill})"


def fill_tuple(fill):
    """Up to four fill bytes -> a tuple of four (missing channels: 0)."""
    fill = [int(v) for v in (fill if fill is not None else ())]
    if len(fill) > 4 or any(v < 0 or v > 255 for v in fill):
        raise ValueError(f"fill {fill!r}: at most four bytes")
    return tuple(fill + [0] * (4 - len(fill)))


def filter_id(filter):
    """`filter`: None (bilinear), one of "bilinear", "box", "hamming", "bicubic", "lanczos" (any case), or a JPGPU_FILTER_* id (an id
    the library does not know is refused there: FormatError) -> the id."""
    if filter is None:
        return N.FILTER_BILINEAR
    if isinstance(filter, str):
        name = filter.lower()
        if name not in N.FILTER_NAMES:
            raise ValueError(f"filter {filter!r}: one of {', '.join(N.FILTER_NAMES)}")
        return N.FILTER_NAMES.index(name)
    f = int(filter)
    if not 0 <= f <= 15:
        raise ValueError(f"filter id {f}: 0..15")
    return f


def resample_coefficients(in_size, out_size, filter=None):
    """jpgpu_resample_coefficients_filtered: the tables of one axis as the batch computes them (pure host function) -> (bounds int32
    (out_size, 2) of (xmin, n), coefs int32 (out_size, ksize), zero beyond n)."""
    f = filter_id(filter)
    ks = C.c_uint32(0)
    check(N.lib().jpgpu_resample_coefficients_filtered(f, int(in_size), int(out_size), None, None, C.byref(ks)), b"jpgpu_resample_coefficients_filtered: refused")
    bounds = np.zeros((int(out_size), 2), np.int32)
    coefs = np.zeros((int(out_size), ks.value), np.int32)
    check(N.lib().jpgpu_resample_coefficients_filtered(f, int(in_size), int(out_size), bounds.ctypes.data, coefs.ctypes.data, C.byref(ks)),
          b"jpgpu_resample_coefficients_filtered: refused")
    return bounds, coefs


def fit_placement(fit, src_size, output_size):
    """jpgpu_fit_placement: the placement (rw, rh, x, y) of a source of ``src_size`` = (w, h) in ``output_size`` = (w, h) under ``fit``
    (a Fit, or a raw N.FitStruct).  A refused rule (a side above 65535, an unknown mode) raises FormatError."""
    s = fit.struct() if isinstance(fit, Fit) else fit
    pl = N.Placement()
    check(N.lib().jpgpu_fit_placement(C.byref(s), int(src_size[0]), int(src_size[1]), int(output_size[0]), int(output_size[1]), C.byref(pl)),
          b"jpgpu_fit_placement: refused")
    return (pl.rw, pl.rh, pl.x, pl.y)


def placement_structs(placements, n):
    """`placements`: None or a list with (rw, rh, x, y) or None per image -> (ctypes array or None)."""
    if placements is None:
        return None
    placements = list(placements)
    if len(placements) != n:
        raise ValueError(f"{len(placements)} placements for {n} images")
    arr = (N.Placement * max(n, 1))()
    for i, pl in enumerate(placements):
        if pl is None:
            continue
        rw, rh, x, y = (int(v) for v in pl)
        if not (0 <= rw <= 65535 and 0 <= rh <= 65535 and -2 ** 31 <= x < 2 ** 31 and -2 ** 31 <= y < 2 ** 31):
            raise ValueError(f"placement {pl!r}")
        arr[i].rw, arr[i].rh, arr[i].x, arr[i].y = rw, rh, x, y
    return arr


class WarpOptions:
    """The warp stage of a batch or a pipeline (jpgpu_warp_options): ``filter`` "nearest" or "bilinear" — Pillow's
    ``Image.transform(size, Image.AFFINE, m, Image.NEAREST / Image.BILINEAR, fillcolor=fill)`` — and ``fill``, up to four bytes in the
    output's channel order: the warp's own fill, separate from a placement's."""
    FILTERS = {"nearest": N.WARP_NEAREST, "bilinear": N.WARP_BILINEAR}

    def __init__(self, filter="nearest", fill=(0, 0, 0, 0)):
        name = str(filter).lower()
        if name not in self.FILTERS:
            raise ValueError(f"warp filter {filter!r}: one of {sorted(self.FILTERS)}")
        self.filter, self.fill = name, fill_tuple(fill)

    def struct(self):
        s = N.WarpOptionsStruct()
        s.filter, s.reserved = self.FILTERS[self.filter], 0
        for c in range(4):
            s.fill[c] = self.fill[c]
        return s

    def __eq__(self, other):
        return isinstance(other, WarpOptions) and (self.filter, self.fill) == (other.filter, other.fill)

    def __repr__(self):
        return f"WarpOptions({self.filter!r}, fill={self.fill})"


def warp_structs(warps, n):
    """`warps`: None or a list with six coefficients or None (the identity) per image -> (ctypes array of jpgpu_warp or None)."""
    if warps is None:
        return None
    warps = list(warps)
    if len(warps) != n:
        raise ValueError(f"{len(warps)} warps for {n} images")
    arr = (N.Warp * max(n, 1))()
    for i, m in enumerate(warps):
        m = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0) if m is None else tuple(float(v) for v in m)
        if len(m) != 6:
            raise ValueError(f"warp {m!r} of image {i}: six coefficients")
        arr[i].m[:] = m
    return arr


def warp_check(m, output_size):
    """jpgpu_warp_check: True when the six coefficients are accepted for ``output_size`` = (w, h) (finite, |m0|, |m1|, |m3|,
    |m4| <= 16000, every corner of the output within +-32000 of the source's origin)."""
    arr = warp_structs([m], 1)
    return N.lib().jpgpu_warp_check(arr, int(output_size[0]), int(output_size[1])) == N.OK


def warp_nearest_axis(a, b, out_size):
    """jpgpu_warp_nearest_axis: the index table of one axis of a NEAREST warp without rotation or shear (scale a, offset b) as the batch
    computes it (pure host function) -> int32 (out_size,)."""
    idx = np.zeros(max(int(out_size), 1), np.int32)
    check(N.lib().jpgpu_warp_nearest_axis(float(a), float(b), int(out_size), idx.ctypes.data), b"jpgpu_warp_nearest_axis: refused")
    return idx[: int(out_size)]


def rotate_matrix(angle, size, center=None, translate=None):
    """The six coefficients ``Image.rotate(angle, center=, translate=)`` builds without ``expand`` for an image of ``size`` = (w, h):
    counter-clockwise by ``angle`` degrees about ``center`` (default (w / 2, h / 2)), then moved by ``translate``."""
    w, h = size
    angle = angle % 360.0
    cx, cy = (w / 2.0, h / 2.0) if center is None else (center[0], center[1])
    tx, ty = (0, 0) if translate is None else (translate[0], translate[1])
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    x, y = -cx - tx, -cy - ty
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def flip_bytes(flips, n):
    """`flips`: None or one truth value per image -> (ctypes array of n bytes or None)."""
    if flips is None:
        return None
    flips = [1 if f else 0 for f in flips]
    if len(flips) != n:
        raise ValueError(f"{len(flips)} flips for {n} images")
    return (C.c_uint8 * max(n, 1))(*flips)


def orientation_bytes(orientations, n):
    """`orientations`: None or one EXIF orientation (1..8; None: 1) per image -> (ctypes array of n bytes or None).  A value outside
    0..255 is a ValueError; one outside 1..8 is for the library to refuse (FormatError)."""
    if orientations is None:
        return None
    vals = [1 if o is None else int(o) for o in orientations]
    if len(vals) != n:
        raise ValueError(f"{len(vals)} orientations for {n} images")
    if any(v < 0 or v > 255 for v in vals):
        raise ValueError(f"orientations {vals!r}")
    return (C.c_uint8 * max(n, 1))(*vals)


def exif_orientation(exif):
    """jpgpu_exif_orientation: the orientation (1..8) an EXIF blob states — the payload behind ``Exif\\0\\0``, as ``Decoder.exif_data()``
    returns it — and 1 for None, no tag, or anything damaged (pure host function; XMP is not read)."""
    b = bytes(exif) if exif is not None else b""
    return int(N.lib().jpgpu_exif_orientation(b, len(b)))


def oriented_window(orientation, size, window=None):
    """jpgpu_oriented_window: for a source of ``size`` = (w, h) under an EXIF orientation -> ((ow, oh), source_window): the oriented
    image's size, and the window (x, y, w, h) of the oriented image (None: all of it) as the window of the source whose orientation it
    is (None for all of it).  An orientation outside 1..8 or a window outside the oriented image raises FormatError."""
    wn = N.Window()
    if window is not None:
        wn.x, wn.y, wn.w, wn.h = (int(v) for v in window)
    ow, oh, src = C.c_uint32(0), C.c_uint32(0), N.Window()
    check(N.lib().jpgpu_oriented_window(int(orientation), int(size[0]), int(size[1]), C.byref(wn), C.byref(ow), C.byref(oh), C.byref(src)),
          b"jpgpu_oriented_window: refused")
    return (ow.value, oh.value), (None if (src.w == 0 or src.h == 0) else (src.x, src.y, src.w, src.h))


def oriented_size(orientation, size):
    """The size (w, h) of the oriented image for a source of ``size`` = (w, h): swapped for the orientations 5..8."""
    return oriented_window(orientation, size)[0]


class Batch:
    """N independent images decoded per launch (jpgpu_batch_*).

    windows: None, one (x, y, w, h) for every image, or a list with a tuple or None per image.  A window lies in the pixel grid
    of the image's output (out_w x out_h after a scale; for one component the component's size); the image's pixels are then
    the window's rows and columns of the whole decode, packed (row pitch w * ncomp bytes):
    ``full.reshape(H, W, nc)[y:y+h, x:x+w]`` for interleaving colour functions, ``full.reshape(H, nc, W)[y:y+h, :, x:x+w]`` for
    ColorTransform None with more than one component.  out_bytes / download / the output arena hold the window's bytes.  A
    window that covers the whole image (or None, or w == 0 or h == 0) is no window; one outside its image fails creation
    (FormatError).

    output_size: None or (w, h), each 1..2048 (jpgpu_batch_create_resized).  Every image's pixels are then the 8-bit bilinear resample
    with antialiasing (Pillow's ``Image.resize((w, h), BILINEAR)`` arithmetic, crop first, horizontal pass first)
    of what it gives without: its window, or its whole output.  out_bytes / out_offset / download / the output arena hold h * w * nc
    bytes per image, interleaved; `path` ends in "+resize".  Planar output (ColorTransform None, more than one component) is refused
    (UnsupportedError), a size of 0 or above 2048 is a FormatError.

    tensor: None or a TensorFormat (jpgpu_batch_create_tensor; needs an output_size, else FormatError).  Every image's output is then
    its resized pixels normalised and channel-first: nc x h x w elements of the format's dtype, written by the resample itself;
    out_bytes / out_offset / the output arena hold them, ``download(i)`` returns an array of shape (nc, h, w) (np.uint16 bit patterns
    for bfloat16), `path` ends in "+resize+tensor".  ``set_flips([...])`` mirrors images' columns from the next decode on.  Images of
    3 x 224 x 224 follow each other without a gap: a ``torch.empty(N, 3, 224, 224)`` bound with BATCH_EXTERNAL_BUFFERS is the result.

    rgb: True adds BATCH_RGB_OUTPUT (needs an output_size, else UnsupportedError): every image gives three channels — gray replicated,
    CMYK / YCCK through Pillow's integer cmyk2rgb, before the resample (``Image.convert("RGB")`` then crop and resize)
    — so arrays are (h * w * 3,) uint8 or (3, h, w) whatever the files hold; `path` gains "+rgb" before "+resize".

    placements: None, or a list with (rw, rh, x, y) or None per image (jpgpu_batch_create_placed; needs an output_size).  The image's
    source is resampled to rw x rh — a size of its own — and laid with its top-left pixel at (x, y) in the output: what falls outside
    is cropped, what it does not cover is ``fill`` (up to four bytes, the output's channel order).  Pillow's
    ``canvas = Image.new(mode, (w, h), fill); canvas.paste(src.resize((rw, rh), BILINEAR), (x, y))``; with a tensor a filled element is
    ``T[c][fill[c]]`` and a flip mirrors the finished canvas.  `path` gains "+place" before "+resize" when some image
    has a placement other than (w, h, 0, 0); one that shows no pixel is a FormatError, a list of another length a ValueError.

    filter: None or "bilinear" (the default: nothing changes), "box", "hamming", "bicubic", "lanczos", or a JPGPU_FILTER_* id
    (JPGPU_BATCH_FILTER in the flags; needs an output_size, else UnsupportedError): every resample of the batch is Pillow's
    ``Image.resize(size, F)`` with that filter; `path` names it behind "+resize", as in "+resize:bicubic".

    warp: None or a WarpOptions (jpgpu_batch_create_warped; needs an output_size, else FormatError).  Every image's result of the above —
    its u8 pixels of the output size, placement fill included, mirrored first when the image is flipped — is then read through six
    coefficients per image, ``Image.transform((w, h), Image.AFFINE, m, NEAREST or BILINEAR, fillcolor=warp.fill)``, and written as bytes
    or, with `tensor`, through the table.  Every image starts with the identity; ``set_warps([...])`` sets the
    matrices from the next decode on.  `path` gains "+warp" or "+warp:bilinear" before "+tensor".

    orientations: None, or one EXIF orientation (1..8) per image (jpgpu_batch_create_oriented; needs an output_size, else
    UnsupportedError).  Every image is oriented first — ``ImageOps.exif_transpose`` — and everything above is meant on the oriented image:
    the window lies in it and is checked against its size (``oriented_size``), placements are those of the oriented window, and the
    resample's horizontal pass runs on its rows.  `path` gains "+orient" in front; all ones is the batch without the
    argument.  A value outside 1..8 is a FormatError.

    colour: None / False, or True (jpgpu_batch_create_coloured; needs an output_size, else UnsupportedError).  Every image's u8 result of
    the above — RGB conversion, orientation, resample and placement fill included — then goes through a program of at most four Pillow
    colour operations, before the warp and the tensor table (the helpers of ``colour.py``: brightness, contrast,
    saturation, solarize, posterize, invert, autocontrast, equalize, hue, sharpness).  Every image starts with the empty program;
    ``set_colour([...])`` sets the programs from the next decode on.  Only images with three output channels take a non-empty
    program.  `path` gains "+colour" before "+warp" / "+tensor"."""

    def __init__(self, descs, device=0, flags=N.BATCH_DEFAULT, windows=None, output_size=None, tensor=None, rgb=False, placements=None, fill=None,
                 filter=None, warp=None, orientations=None, colour=None):
        self._h = C.c_void_p()
        arr = (N.ImageDesc * len(descs))(*descs)
        wins = window_structs(windows, len(descs))
        self.output_size = None if output_size is None else output_size_pair(output_size)
        self.tensor = tensor
        self.rgb = bool(rgb) or bool(flags & N.BATCH_RGB_OUTPUT)
        if rgb:
            flags |= N.BATCH_RGB_OUTPUT
        if filter is not None:
            flags = (flags & ~N.BATCH_FILTER(15)) | N.BATCH_FILTER(filter_id(filter))
        self.filter = N.FILTER_NAMES[(flags >> 8) & 15] if (flags >> 8) & 15 < len(N.FILTER_NAMES) else (flags >> 8) & 15
        pls = placement_structs(placements, len(descs))
        self.fill = fill_tuple(fill)
        self.warp = warp
        ors = orientation_bytes(orientations, len(descs))
        self.orientations = None if ors is None else list(ors)[: len(descs)]
        self.colour = bool(colour)
        if self.colour:
            w, h = self.output_size if self.output_size is not None else (0, 0)
            fmt = tensor.struct() if tensor is not None else None
            wo = warp.struct() if warp is not None else None
            co = N.ColourOptionsStruct(0)
            st = N.lib().jpgpu_batch_create_coloured(device, arr, wins, pls, (C.c_uint8 * 4)(*self.fill), w, h, C.byref(fmt) if fmt is not None else None,
                                                     C.byref(wo) if wo is not None else None, ors, C.byref(co), len(descs), flags, C.byref(self._h))
        elif ors is not None and (self.output_size is not None or any(v != 1 for v in self.orientations)):  # (all ones without a size: no argument)
            w, h = self.output_size if self.output_size is not None else (0, 0)
            fmt = tensor.struct() if tensor is not None else None
            wo = warp.struct() if warp is not None else None
            st = N.lib().jpgpu_batch_create_oriented(device, arr, wins, pls, (C.c_uint8 * 4)(*self.fill), w, h, C.byref(fmt) if fmt is not None else None,
                                                     C.byref(wo) if wo is not None else None, ors, len(descs), flags, C.byref(self._h))
        elif warp is not None:
            w, h = self.output_size if self.output_size is not None else (0, 0)
            fmt = tensor.struct() if tensor is not None else None
            wo = warp.struct()
            st = N.lib().jpgpu_batch_create_warped(device, arr, wins, pls, (C.c_uint8 * 4)(*self.fill), w, h, C.byref(fmt) if fmt is not None else None,
                                                   C.byref(wo), len(descs), flags, C.byref(self._h))
        elif pls is not None:
            w, h = self.output_size if self.output_size is not None else (0, 0)
            fmt = tensor.struct() if tensor is not None else None
            st = N.lib().jpgpu_batch_create_placed(device, arr, wins, pls, (C.c_uint8 * 4)(*self.fill), w, h, C.byref(fmt) if fmt is not None else None,
                                                   len(descs), flags, C.byref(self._h))
        elif tensor is not None:
            w, h = self.output_size if self.output_size is not None else (0, 0)
            fmt = tensor.struct()
            st = N.lib().jpgpu_batch_create_tensor(device, arr, wins, w, h, C.byref(fmt), len(descs), flags, C.byref(self._h))
        elif self.output_size is not None:
            st = N.lib().jpgpu_batch_create_resized(device, arr, wins, self.output_size[0], self.output_size[1], len(descs), flags, C.byref(self._h))
        elif wins is None:
            st = N.lib().jpgpu_batch_create(device, arr, len(descs), flags, C.byref(self._h))
        else:
            st = N.lib().jpgpu_batch_create_windowed(device, arr, wins, len(descs), flags, C.byref(self._h))
        if st:
            msg = N.lib().jpgpu_batch_last_error(self._h) if self._h else b"jpgpu_batch_create"
            msg = bytes(msg)
            self.close()
            check(st, msg)
        self.n_images = len(descs)
        self.descs = descs
        self.windows = None if wins is None else [None if (w.w == 0 or w.h == 0) else (w.x, w.y, w.w, w.h) for w in wins]

    def close(self):
        if getattr(self, "_h", None):
            lib = N.lib() if N is not None and getattr(N, "lib", None) else None  # (interpreter shutdown: module globals may be gone)
            if lib is not None:
                lib.jpgpu_batch_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _check(self, st):
        check(st, N.lib().jpgpu_batch_last_error(self._h) if st else b"")

    @property
    def path(self):
        return N.lib().jpgpu_batch_path(self._h).decode()

    def coef_arena_bytes(self):
        return N.lib().jpgpu_batch_coef_arena_bytes(self._h)

    def out_arena_bytes(self):
        return N.lib().jpgpu_batch_out_arena_bytes(self._h)

    def coef_offset(self, image, comp):
        return N.lib().jpgpu_batch_coef_offset(self._h, image, comp)

    def coef_bytes(self, image, comp):
        return N.lib().jpgpu_batch_coef_bytes(self._h, image, comp)

    def out_offset(self, image):
        return N.lib().jpgpu_batch_out_offset(self._h, image)

    def out_bytes(self, image):
        return N.lib().jpgpu_batch_out_bytes(self._h, image)

    def bind(self, coef_ptr, out_ptr):
        self._check(N.lib().jpgpu_batch_bind(self._h, coef_ptr, out_ptr))

    def coef_arena(self):
        return N.lib().jpgpu_batch_coef_arena(self._h)

    def out_arena(self):
        return N.lib().jpgpu_batch_out_arena(self._h)

    def set_quantization_table(self, image, comp, table):
        """jpgpu_batch_set_quantization_table: replace the descriptor's table (the component's range class becomes 0 if it changes)."""
        q = np.ascontiguousarray(table, dtype=np.uint16).reshape(64)
        self._check(N.lib().jpgpu_batch_set_quantization_table(self._h, image, comp, q.ctypes.data))
        for k in range(64):
            self.descs[image].quantization_tables[comp][k] = int(q[k])

    def upload(self, image, comp, coefficients):
        a = np.ascontiguousarray(coefficients, dtype=np.int16).reshape(-1)
        self._check(N.lib().jpgpu_batch_upload(self._h, image, comp, a.ctypes.data, a.size))

    def upload_compact(self, image, comp, coefficients, stream=None, classify=True):
        """Same result as upload(), but PCIe carries only the non-zero coefficients (bitmap + index + values per block,
        include/jpgpu.h); a kernel expands them into the arena at the start of the next decode().  classify=False sends
        range_class = -1: the expansion kernel ranges the values on the device instead of the host encoder."""
        a = np.ascontiguousarray(coefficients, dtype=np.int16).reshape(-1)
        q = np.ascontiguousarray(np.ctypeslib.as_array(self.descs[image].quantization_tables[comp]), dtype=np.uint16)
        buf = np.empty(N.lib().jpgpu_compact_max_bytes(a.size // 64), np.uint8)
        rc = C.c_int(0)
        n = N.lib().jpgpu_compact_encode(a.ctypes.data, a.size // 64, q.ctypes.data, buf.ctypes.data, C.byref(rc))
        self._check(N.lib().jpgpu_batch_upload_compact(self._h, image, comp, buf.ctypes.data, n, rc.value if classify else -1, stream))
        self.synchronize(stream)  # the host buffer is pageable and about to go away
        return n

    def set_range_hint(self, image, range_class):
        """0 unknown/hostile, 1 every |c*q| < 2^15, 3 additionally every block-column sum of |c*q| <= 5900."""
        self._check(N.lib().jpgpu_batch_set_range_hint(self._h, image, int(range_class)))

    def scan_ranges(self, stream=None):
        """Range classes from the coefficients as they stand in the device arena (one pass at HBM speed): [image][comp]."""
        out = np.zeros((self.n_images, 4), np.uint8)
        self._check(N.lib().jpgpu_batch_scan_ranges(self._h, stream, out.ctypes.data))
        return out

    def classify_on_device(self, stream=None):
        """jpgpu_batch_classify_on_device: range statistics of the arena's coefficients gathered and kept ON THE DEVICE
        (asynchronous, no read-back); decode() then takes the classes from them there.  The device entropy decoder and
        upload_compact(..., classify=False) leave the same statistics as a by-product."""
        self._check(N.lib().jpgpu_batch_classify_on_device(self._h, stream))

    def class_counts(self):
        """Images of the fused launch groups per arithmetic variant: (wrap-exact, range class 1, range class 3)."""
        c = (C.c_uint32 * 3)()
        self._check(N.lib().jpgpu_batch_class_counts(self._h, c))
        return tuple(int(x) for x in c)

    def decode(self, stream=None):
        self._check(N.lib().jpgpu_batch_decode(self._h, stream))

    def synchronize(self, stream=None):
        self._check(N.lib().jpgpu_batch_synchronize(self._h, stream))

    def set_flips(self, flips):
        """jpgpu_batch_set_flips: one truth value per image (None: no image flipped), in force from the next decode on.  A batch
        without `tensor` raises UnsupportedError."""
        arr = flip_bytes(flips, self.n_images)
        self._check(N.lib().jpgpu_batch_set_flips(self._h, arr))

    def set_warps(self, warps):
        """jpgpu_batch_set_warps: six coefficients (or None: the identity) per image, None for identities throughout; in force from the
        next decode on.  One refused matrix raises FormatError and changes nothing; a batch without `warp` raises UnsupportedError."""
        arr = warp_structs(warps, self.n_images)
        self._check(N.lib().jpgpu_batch_set_warps(self._h, arr))

    def set_colour(self, programs):
        """jpgpu_batch_set_colour_programs: a program (a list of at most four ``(name, value)`` pairs, or None: the empty one) per image,
        None for empty programs throughout; in force from the next decode on.  One refused program raises FormatError — a non-empty one
        for an image without three output channels UnsupportedError — and changes nothing; a batch without `colour` raises
        UnsupportedError."""
        arr = program_structs(programs, self.n_images)
        self._check(N.lib().jpgpu_batch_set_colour_programs(self._h, arr))

    def download(self, image):
        n = self.out_bytes(image)
        out = np.empty(max(n, 1), dtype=np.uint8)
        got = C.c_size_t(0)
        self._check(N.lib().jpgpu_batch_download(self._h, image, out.ctypes.data, out.size, C.byref(got)))
        if self.tensor is not None:
            w, h = self.output_size
            return out[: got.value].view(self.tensor.numpy_dtype).reshape(-1, h, w)
        return out[: got.value]

    def time(self, iters, stream=None):
        ms = C.c_float(0)
        self._check(N.lib().jpgpu_batch_time(self._h, stream, iters, C.byref(ms)))
        return ms.value
