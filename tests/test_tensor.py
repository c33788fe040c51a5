"""The tensor output without a GPU: the numpy statement of the lookup table equals torch's CPU arithmetic bit for
bit, jpgpu_tensor_table equals the numpy statement and refuses what it must, the new symbols are declared, exported and bound, the
C struct has the documented size and the Python layer carries the new arguments."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import jpeg_decoder_amd as J
import tensor_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jpgpu_batch_create_tensor", "jpgpu_batch_set_flips", "jpgpu_tensor_table", "jpgpu_pipeline_set_tensor_output", "jpgpu_pipeline_decode_augmented")
NEGATIVE = ((-0.75, -1e-3, -123.5, -0.0), (0.25, 3.0, 1e-3, 7.0))
TINY = ((0.485, 0.0, 0.25, 0.5), (1e-30, 1e-30, 1e-30, 1e-30))  # (overflows to inf in f16: fine)
FORMATS = {"imagenet": T.IMAGENET, "clip": T.CLIP, "half": T.HALF, "identity": T.IDENTITY, "negative": NEGATIVE, "tiny": TINY}


@pytest.mark.parametrize("name", sorted(FORMATS))
def test_numpy_table_is_torch_cpu_bit_for_bit(name):
    torch = pytest.importorskip("torch")
    mean, std = FORMATS[name]
    for c in range(4):
        m, s = float(np.float32(mean[c])), float(np.float32(std[c]))
        t32 = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).sub_(m).div_(s)
        f32 = T.table(("float32", mean, std), 4)[c]
        f16 = T.table(("float16", mean, std), 4)[c]
        b16 = T.table(("bfloat16", mean, std), 4)[c]
        assert np.array_equal(T.bits(f32), T.bits(t32.numpy())), (name, c)
        assert np.array_equal(T.bits(f16), T.bits(t32.to(torch.float16).numpy())), (name, c)
        assert np.array_equal(b16.view(np.int16), t32.to(torch.bfloat16).view(torch.int16).numpy()), (name, c)
    if name == "tiny":
        assert np.isinf(T.table(("float16", mean, std), 1)).any()


def _fmt(dtype, mean, std, reserved=0):
    s = J._native.TensorFormatStruct()
    s.dtype, s.reserved = dtype, reserved
    for c in range(4):
        s.mean[c], s.std[c] = mean[c], std[c]
    return s


@pytest.mark.parametrize("nc", [1, 3, 4])
def test_library_table_is_the_numpy_table(nc):
    lib = J.lib()
    for name, (mean, std) in sorted(FORMATS.items()):
        for dtype in T.DTYPES:
            want = T.table((dtype, mean, std), nc)
            got = np.full((nc + 1, 256), 0x5A5A, want.dtype) if dtype != "float32" else np.full((nc + 1, 256), 7.0, np.float32)
            guard = got[nc].copy()
            f = _fmt(J.TensorFormat.DTYPES[dtype][0], mean, std)
            assert lib.jpgpu_tensor_table(C.byref(f), nc, got.ctypes.data) == 0
            assert np.array_equal(T.bits(got[:nc]), T.bits(want)), (name, dtype, nc)
            assert np.array_equal(T.bits(got[nc]), T.bits(guard)), "wrote past nc x 256 elements"
            assert np.array_equal(T.bits(J.TensorFormat(dtype, mean, std).table(nc)), T.bits(want))


def test_library_table_refusals():
    lib = J.lib()
    out = np.zeros((4, 256), np.float32)
    ok_m, ok_s = (0.5,) * 4, (0.5,) * 4

    def rc(dtype=1, mean=ok_m, std=ok_s, reserved=0, nc=3):
        f = _fmt(dtype, mean, std, reserved)
        return lib.jpgpu_tensor_table(C.byref(f), nc, out.ctypes.data)

    assert rc() == 0
    for bad in (0.0, -0.0, float("nan"), float("inf"), float("-inf")):
        assert rc(std=(0.5, bad, 0.5, 0.5)) == J._native.ERR_FORMAT, bad
        assert rc(std=(0.5, 0.5, 0.5, bad)) == 0  # (channel 3 of a three-channel image: not looked at)
        assert rc(std=(0.5, 0.5, 0.5, bad), nc=4) == J._native.ERR_FORMAT
    for bad in (float("nan"), float("inf")):
        assert rc(mean=(bad, 0.5, 0.5, 0.5)) == J._native.ERR_FORMAT
    for dtype in (0, 4, 255):
        assert rc(dtype=dtype) == J._native.ERR_FORMAT
    assert rc(reserved=1) == J._native.ERR_FORMAT
    assert rc(nc=0) == J._native.ERR_FORMAT and rc(nc=5) == J._native.ERR_FORMAT
    assert lib.jpgpu_tensor_table(None, 3, out.ctypes.data) == J._native.ERR_FORMAT


def test_new_symbols_are_declared_exported_and_bound():
    text = ""
    for h in ("jpgpu.h", "jpgpu_decoder.h"):
        text += re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
    declared = set(re.findall(r"\b(jpgpu_[a-z0-9_]+)\s*\(", text))
    J.build()
    lib = C.CDLL(J._native.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in J._native.exported_symbols(), name
    for k, v in (("JPGPU_TENSOR_F32", 1), ("JPGPU_TENSOR_F16", 2), ("JPGPU_TENSOR_BF16", 3)):
        assert re.search(rf"\b{k}\s*=\s*{v}\b", text), k
    assert (J._native.TENSOR_F32, J._native.TENSOR_F16, J._native.TENSOR_BF16) == (1, 2, 3)


def test_tensor_format_struct_is_40_bytes(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "jpgpu_decoder.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu %zu %zu %zu %zu\\n", sizeof(jpgpu_tensor_format), offsetof(jpgpu_tensor_format, dtype), offsetof(jpgpu_tensor_format, reserved),\n'
                   "           offsetof(jpgpu_tensor_format, mean), offsetof(jpgpu_tensor_format, std));\n"
                   "    return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    size, o_dtype, o_res, o_mean, o_std = (int(v) for v in subprocess.check_output([exe]).split())
    S = J._native.TensorFormatStruct
    assert size == 40 == C.sizeof(S)
    assert (o_dtype, o_res, o_mean, o_std) == (0, 4, 8, 24) == (S.dtype.offset, S.reserved.offset, S.mean.offset, S.std.offset)


def test_timings_struct_did_not_grow():
    assert J._native.PipelineTimings._fields_[-1][0] == "images_windowed"


def test_python_layer_carries_the_new_arguments():
    for fn, names in ((J.Batch.__init__, ("output_size", "tensor")), (J.Pipeline.decode, ("output_size", "tensor", "flips"))):
        params = inspect.signature(fn).parameters
        for name in names:
            assert name in params and params[name].default is None, (fn, name)
    assert callable(J.Batch.set_flips)
    f = J.TensorFormat()
    assert f.dtype == "float32" and f.mean == (0.0,) * 4 and f.std == (1.0,) * 4 and f.numpy_dtype is np.float32
    f = J.TensorFormat("bfloat16", mean=(0.5, 0.25, 0.125), std=(2, 4, 8))
    assert f.numpy_dtype is np.uint16 and f.itemsize == 2 and f.mean == (0.5, 0.25, 0.125, 0.0) and f.std == (2.0, 4.0, 8.0, 1.0)
    s = f.struct()
    assert s.dtype == 3 and s.reserved == 0 and list(s.mean) == [0.5, 0.25, 0.125, 0.0] and list(s.std) == [2.0, 4.0, 8.0, 1.0]
    with pytest.raises(ValueError):
        J.TensorFormat("float64")
    with pytest.raises(ValueError):
        J.TensorFormat("float32", mean=(0,) * 5)


def test_a_flips_list_of_the_wrong_length_is_refused_before_any_native_call(monkeypatch):
    def no_native():
        raise AssertionError("the native library was reached")

    monkeypatch.setattr(J._native, "lib", no_native)
    p = J.Pipeline.__new__(J.Pipeline)
    p._h = None
    with pytest.raises(ValueError, match="2 flips for 3"):
        p.decode([b"\xff\xd8"] * 3, output_size=(8, 8), tensor=J.TensorFormat(), flips=[True, False])
