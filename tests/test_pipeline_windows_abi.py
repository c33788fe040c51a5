"""The ABI of windows on Pipeline and Decoder (include/jpgpu_decoder.h), without a GPU: the new symbols are declared and exported,
jpgpu_pipeline_timings grew at its end only, and the Python layer carries the new arguments and checks them before any native call."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import jpeg_decoder_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jpgpu_pipeline_decode_windowed", "jpgpu_pipeline_image_window", "jpgpu_decoder_set_window")


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "jpgpu_decoder.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(jpgpu_[a-z0-9_]+)\s*\(", text))
    J.build()
    lib = C.CDLL(J._native.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in J._native.exported_symbols(), name
    proto = J._native._PROTOS["jpgpu_pipeline_decode_windowed"][1]
    assert proto[3] == C.POINTER(J._native.Window) and len(proto) == 6


def test_timings_struct_matches_the_header(tmp_path):
    """sizeof and the offsets of the fields around the new one, as the host compiler lays the C struct out."""
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "jpgpu_decoder.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu %zu %zu %zu %zu\\n", sizeof(jpgpu_pipeline_timings), offsetof(jpgpu_pipeline_timings, images_windowed),\n'
                   "           offsetof(jpgpu_pipeline_timings, images_entry_pixels), offsetof(jpgpu_pipeline_timings, cpu_ms), sizeof(jpgpu_window));\n"
                   "    return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    size, off_win, off_entry, off_cpu, win_size = (int(v) for v in subprocess.check_output([exe]).split())
    T = J._native.PipelineTimings
    assert C.sizeof(T) == size
    assert T.images_windowed.offset == off_win and T.images_entry_pixels.offset == off_entry and T.cpu_ms.offset == off_cpu
    assert T._fields_[-1][0] == "images_windowed"
    assert off_win == max(getattr(T, n).offset for n, _ in T._fields_)  # nothing lies behind it, nothing before it moved
    assert T._fields_[-2][0] == "images_entry_pixels" and off_win == off_entry + 4
    assert C.sizeof(J._native.Window) == win_size == 8


def test_python_layer_carries_the_new_arguments():
    assert "windows" in inspect.signature(J.Pipeline.decode).parameters
    assert inspect.signature(J.Pipeline.decode).parameters["windows"].default is None
    assert callable(J.Pipeline.window) and callable(J.Decoder.set_window)
    assert list(inspect.signature(J.Decoder.set_window).parameters) == ["self", "x", "y", "w", "h"]


def test_a_windows_list_of_the_wrong_length_is_refused_before_any_native_call(monkeypatch):
    def no_native():
        raise AssertionError("the native library was reached")

    monkeypatch.setattr(J._native, "lib", no_native)
    p = J.Pipeline.__new__(J.Pipeline)  # (no device needed: decode() must raise before it touches the handle)
    p._h = None
    files = [b"\xff\xd8", b"\xff\xd8", b"\xff\xd8"]
    with pytest.raises(ValueError, match="2 windows for 3"):
        p.decode(files, windows=[(0, 0, 8, 8), None])
    with pytest.raises(ValueError):
        p.decode(files, windows=[(0, 0, 8, 8), None, None, None])
    with pytest.raises(ValueError):
        p.decode(files, windows=[(0, 0, 70000, 8), None, None])
    with pytest.raises(ValueError):
        p.decode(files, windows=[(-1, 0, 8, 8), None, None])


def test_decoder_window_is_stored_and_sizes_the_output_without_a_device():
    data = open(os.path.join(ROOT, "tests", "golden", "benches", "tower.jpg"), "rb").read()
    d = J.Decoder(data, device=-1)  # host-only object
    try:
        d.set_window(13, 5, 101, 77)
        lib = J._native.lib()
        assert lib.jpgpu_decoder_output_bytes(d._h) == 0  # no info yet
        d.read_info()
        assert (d.info().width, d.info().height) == (512, 512)  # info() keeps the image's size
        assert lib.jpgpu_decoder_output_bytes(d._h) == 101 * 77 * 3
        d.set_window(0, 0, 0, 9)  # w or h 0: the whole image again
        assert lib.jpgpu_decoder_output_bytes(d._h) == 512 * 512 * 3
        with pytest.raises(ValueError):
            d.set_window(0, 0, 65536, 1)
        d.set_window(500, 500, 20, 20)  # outside: decode() refuses it before anything else (a host-only object would say "no device")
        with pytest.raises(J.FormatError, match="window"):
            d.decode()
    finally:
        d.close()


# ---- the rows the device entropy route keeps for a windowed image (HIP-free planner) ---------------------------------------------------
def test_kept_rows_hold_every_block_the_window_kernel_enumerates(tmp_path):
    """window_kept_rows / window_kept_mcu_rows (csrc/window_band.hpp) over the layouts, scales and window shapes of
    tests/test_window_emulation.py: no block window_tile_blocks enumerates lies outside the rows kept, the rows kept are exactly the
    union of the tiles' rows, and they lie inside the MCU rows the expansion stores."""
    import numpy as np

    import oracle as O
    import test_window_emulation as E

    so = str(tmp_path / "libemurows.so")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call([os.environ.get("CXX", "g++"), *E._FLAGS, "-shared", "-I", emu, "-include", os.path.join(emu, "hip_shim.hpp"), "-o", so,
                           os.path.join(emu, "emu_window_rows.cpp"), os.path.join(ROOT, "jpeg-decoder_amd", "csrc", "image_job.cpp")])
    L = C.CDLL(so)
    L.emu_window_rows.argtypes = [C.c_void_p] * 5
    L.emu_window_rows.restype = C.c_int
    checked = 0
    for samp, ct in E.LAYOUTS:
        for scale in (8, 4, 2, 1):
            for (w_, h_) in E.SIZES + [(1921, 1083)]:
                try:
                    ocomps, _ = O.make_components(w_, h_, samp, dct_scale=scale)
                except O.OracleError:
                    continue
                ow, oh = J.scaled_output_size(w_, h_, scale)
                desc = J.image_desc(list(E._to_j(ocomps)), [np.ones(64, np.uint16)] * len(samp), ow, oh, ct)
                W, H = E.grid_of(ocomps, ow, oh)
                for win in E.windows_for(W, H, seed=W * 31 + H + scale):
                    rows, mcu, counts = np.zeros(8, np.uint32), np.zeros(2, np.uint32), np.zeros(4, np.uint32)
                    rc = L.emu_window_rows(C.byref(desc), np.array(win, np.uint32).ctypes.data, rows.ctypes.data, mcu.ctypes.data, counts.ctypes.data)
                    if rc > 0:
                        continue  # (build_image_job refuses the frame, as the reference does)
                    assert rc == 0, (samp, ct, scale, (w_, h_), win)
                    assert counts[0] > 0 and counts[1] == 0 and counts[2] == 0 and counts[3] == 0, (samp, ct, scale, (w_, h_), win, rows, mcu, counts)
                    vmax = max(v for _, v in samp)
                    mcu_h = ocomps[0].block_h // samp[0][1]
                    assert 0 <= mcu[0] < mcu[1] <= mcu_h
                    # whole-row granularity, but no more than the window's MCU rows and one ring row on either side
                    assert mcu[0] >= max(0, win[1] // (vmax * scale) - 1) and mcu[1] <= min(mcu_h, -(-(win[1] + win[3]) // (vmax * scale)) + 1)
                    checked += 1
    assert checked > 2000
