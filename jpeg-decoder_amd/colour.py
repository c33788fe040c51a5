"""Colour programs of the fixed-output stage (jpgpu_batch_create_coloured): a program is a list of at most four
operations, each a ``(name, value)`` pair or what one of the helpers below returns — ``[brightness(1.2), contrast(0.8), equalize()]``;
``[brightness(b), contrast(c), saturation(s), hue(h)]`` in any order is torchvision's ``ColorJitter`` on a PIL image."""
import ctypes as C

import numpy as np

from . import _native as N
from .error import check

OPS = {"identity": 0, "brightness": 1, "contrast": 2, "saturation": 3, "color": 3, "solarize": 4, "posterize": 5, "invert": 6, "autocontrast": 7,
       "equalize": 8, "hue": 16, "sharpen": 17}


def identity():
    return ("identity", 0.0)


def brightness(f):
    """``ImageEnhance.Brightness(im).enhance(f)``"""
    return ("brightness", float(f))


def contrast(f):
    """``ImageEnhance.Contrast(im).enhance(f)``"""
    return ("contrast", float(f))


def saturation(f):
    """``ImageEnhance.Color(im).enhance(f)``; 0 is ``RandomGrayscale``'s three equal channels"""
    return ("saturation", float(f))


def solarize(t):
    """``ImageOps.solarize(im, t)``, t an integer 0..256"""
    return ("solarize", float(t))


def posterize(b):
    """``ImageOps.posterize(im, b)``, b an integer 1..8"""
    return ("posterize", float(b))


def invert():
    return ("invert", 0.0)


def autocontrast():
    return ("autocontrast", 0.0)


def equalize():
    return ("equalize", 0.0)


def hue(factor):
    """torchvision's ``adjust_hue(im, factor)`` on a PIL image, -0.5 <= factor <= 0.5: the hue channel of ``im.convert("HSV")`` moved by
    ``int(factor * 255) & 255`` (truncated toward zero, as ``np.int32(factor * 255).astype(np.uint8)``) and converted back.  Factor 0 is
    the lossy round trip through HSV, not the identity — as in torchvision."""
    if not -0.5 <= factor <= 0.5:
        raise ValueError(f"hue factor {factor!r}: -0.5..0.5")
    return ("hue", float(int(factor * 255) & 255))


def sharpness(f):
    """``ImageEnhance.Sharpness(im).enhance(f)``: 0 is Pillow's SMOOTH filter, 1 the image itself, 2 RandAugment's strongest.  The
    operation's name is ``"sharpen"``: programs have always refused the name ``"sharpness"`` as unknown, and callers who probe for an
    operation by its name keep getting that answer."""
    return ("sharpen", float(f))


def op_id(name):
    if isinstance(name, str):
        if name.lower() not in OPS:
            raise ValueError(f"colour operation {name!r}: one of {sorted(OPS)}")
        return OPS[name.lower()]
    return int(name)


def program_struct(program):
    """A program (None: the empty one) -> N.ColourProgram.  More than four operations keep their count, for the library to refuse."""
    s = N.ColourProgram()
    ops = [] if program is None else list(program)
    s.n = len(ops)
    for k, (name, value) in enumerate(ops[:4]):
        s.ops[k].op = op_id(name)
        s.ops[k].value = float(value)
    return s


def program_structs(programs, n):
    """`programs`: None or a list with a program or None per image -> (ctypes array of n programs or None)."""
    if programs is None:
        return None
    programs = list(programs)
    if len(programs) != n:
        raise ValueError(f"{len(programs)} colour programs for {n} images")
    return (N.ColourProgram * max(n, 1))(*[program_struct(p) for p in programs])


def colour_check(program):
    """jpgpu_colour_check: True when the library accepts the program."""
    s = program_struct(program)
    return N.lib().jpgpu_colour_check(C.byref(s)) == N.OK


def colour_point_lut(op, value=0.0, mean=0):
    """jpgpu_colour_point_lut: the 256-entry table of a point operation (CONTRAST: for the image mean `mean`) -> uint8 (256,)."""
    lut = np.zeros(256, np.uint8)
    check(N.lib().jpgpu_colour_point_lut(op_id(op), float(value), int(mean), lut.ctypes.data), b"jpgpu_colour_point_lut: refused")
    return lut


def colour_autocontrast_lut(hist):
    """jpgpu_colour_autocontrast_lut: one channel's table from its histogram (256 counts) -> uint8 (256,)."""
    h = np.ascontiguousarray(hist, dtype=np.uint32).reshape(256)
    lut = np.zeros(256, np.uint8)
    check(N.lib().jpgpu_colour_autocontrast_lut(h.ctypes.data, lut.ctypes.data), b"jpgpu_colour_autocontrast_lut: refused")
    return lut


def colour_equalize_lut(hist):
    """jpgpu_colour_equalize_lut: one channel's table from its histogram (256 counts) -> uint8 (256,)."""
    h = np.ascontiguousarray(hist, dtype=np.uint32).reshape(256)
    lut = np.zeros(256, np.uint8)
    check(N.lib().jpgpu_colour_equalize_lut(h.ctypes.data, lut.ctypes.data), b"jpgpu_colour_equalize_lut: refused")
    return lut


def colour_apply(tensor, programs):
    """jpgpu_colour_apply: the programs (one per image, or None for the empty one) on a contiguous uint8 torch tensor of N x H x W x 3 on
    the device, in place, on the tensor's device and torch's current stream; returns the tensor when the work is complete.  Its first
    byte must be 256-byte aligned and 3 W H a multiple of 4 (UnsupportedError); one refused program refuses the call (FormatError) and
    nothing is written."""
    import torch

    if not (isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.dtype == torch.uint8 and tensor.dim() == 4 and tensor.shape[3] == 3
            and tensor.is_contiguous()):
        raise ValueError("colour_apply: a contiguous uint8 N x H x W x 3 tensor on the device")
    n, h, w, _ = tensor.shape
    arr = program_structs(programs if programs is not None else [None] * n, n)
    with torch.cuda.device(tensor.device):
        stream = torch.cuda.current_stream().cuda_stream
        check(N.lib().jpgpu_colour_apply(tensor.data_ptr(), n, w, h, arr, stream), b"jpgpu_colour_apply: refused (a program, or the base / size rule)")
    return tensor
