"""jpeg-decoder_amd — MI355X (gfx950) pixel-pipeline backend for image-rs/jpeg-decoder.

Python face of the C ABI in include/jpgpu.h: the Worker boundary (HipWorker,
compute_image_parallel), the batch driver and the Decoder front-end.  The product path is
HIP-only: nothing here falls back to a CPU implementation."""
from . import _native
from ._native import Component, ImageDesc, build, device_count, lib, process_init
from .batch import (Batch, Fit, TensorFormat, WarpOptions, exif_orientation, fit_placement, image_desc, oriented_size, oriented_window,
                    resample_coefficients, rotate_matrix, warp_check, warp_nearest_axis)
from .colour import (autocontrast, brightness, colour_apply, colour_autocontrast_lut, colour_check, colour_equalize_lut, colour_point_lut, contrast,
                     equalize, hue, invert, posterize, saturation, sharpness, solarize)
from .decoder import CODING_PROCESSES, PIXEL_FORMATS, Decoder, ImageInfo, decode_batch
from .error import Error, FormatError, InternalError, IoError, NoDeviceError, UnsupportedError
from .pipeline import PinnedFiles, Pipeline
from .parser import Dimensions, choose_idct_size, make_components, scaled_output_size, update_component_sizes
from .worker import COLOR_TRANSFORMS, HipWorker, RowData, color_transform_id, compute_image_parallel

__all__ = [
    "Batch", "Fit", "WarpOptions", "autocontrast", "brightness", "colour_apply", "colour_autocontrast_lut", "colour_check", "colour_equalize_lut", "colour_point_lut", "contrast",
    "equalize", "hue", "invert", "posterize", "saturation", "sharpness", "solarize", "exif_orientation", "oriented_size", "oriented_window", "rotate_matrix", "warp_check", "warp_nearest_axis", "fit_placement", "resample_coefficients", "CODING_PROCESSES", "COLOR_TRANSFORMS", "Component", "Decoder", "Dimensions", "ImageInfo", "PIXEL_FORMATS", "PinnedFiles", "Pipeline", "TensorFormat", "decode_batch", "Error", "FormatError", "HipWorker", "ImageDesc",
    "InternalError", "IoError", "NoDeviceError", "RowData", "UnsupportedError", "build", "choose_idct_size",
    "color_transform_id", "compute_image_parallel", "device_count", "image_desc", "lib", "make_components",
    "scaled_output_size", "update_component_sizes",
]
