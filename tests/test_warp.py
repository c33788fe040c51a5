"""Affine warps on the CPU (no GPU): the numpy statement of DESIGN.md §4.16 (tests/warp_ref.py) against Pillow's golden hashes, the
library's pure host functions — jpgpu_warp_check, jpgpu_warp_nearest_axis, rotate_matrix — against the statement, every warp kernel
body emulated lane by lane (tests/emu/emu_warp.cpp, -ffp-contract=off) against it, and the bodies plus the job builder as a stand-alone
program under AddressSanitizer + UBSan."""
import ctypes as C
import hashlib
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_decoder_amd as J
import warp_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "warp", "pillow_warp.json")
_EMU = os.path.join(ROOT, "tests", "emu")
# the flags of tests/emu/Makefile, and no contraction of a * b + c (rule B rounds every operation)
_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DJPGPU_HOST_EMULATION", "-ffp-contract=off"]
N = J._native


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _source(c):
    return np.random.default_rng(c["seed"]).integers(0, 256, (c["H"], c["W"], c["C"]), dtype=np.uint8)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_the_numpy_statement_is_what_pillow_computes(golden):
    cases = golden["cases"]
    assert len(cases) >= 60
    seen, nsep_differs, rounding_differs = set(), 0, 0
    for c in cases:
        a, m = _source(c), c["m"]
        assert WR.check(m, c["W"], c["H"]), c
        assert _sha(WR.warp(a, m, c["filter"], c["fill"])) == c["sha256"], c
        seen.add((c["C"], c["filter"]))
        if c["filter"] == WR.NEAREST and m[1] == 0 and m[3] == 0 and c["W"] >= 1000:
            nsep_differs += _sha(WR.nearest_fixed(a, m, c["fill"])) != c["sha256"]
        if c["filter"] == WR.BILINEAR:
            rounding_differs += _sha(WR.bilinear(a, m, c["fill"], rounded=True)) != c["sha256"]
    assert seen == {(C_, f) for C_ in (1, 3, 4) for f in (0, 1)}
    # the set discriminates: rule N on an N-sep case and a rounded rule B give other pixels
    assert nsep_differs >= 1 and rounding_differs >= 1


def test_golden_cases_cover_the_matrix_kinds(golden):
    kinds = set()
    for c in golden["cases"]:
        m, W, H = c["m"], c["W"], c["H"]
        if tuple(m) == WR.IDENTITY:
            kinds.add("identity")
        elif m[1] == 0 and m[3] == 0:
            kinds.add("negative m0" if m[0] < 0 else "scale" if (m[0], m[4]) != (1.0, 1.0) else "translation")
            kinds.add("zoom" if 0 < m[0] < 0.01 else "sep")
        else:
            kinds.add("quarter turn" if (abs(m[1]) == 1.0 and m[0] == 0.0 and W != H) else "shear" if (m[0] == 1.0 and m[4] == 1.0) else "rotation")
        if max(abs(m[0]), abs(m[1]), abs(m[3]), abs(m[4])) == 16000.0 or max(abs(m[2]), abs(m[5])) == 32000.0:
            kinds.add("bounds")
        if not np.any(WR.warp(np.full((H, W, 1), 255, np.uint8), m, c["filter"], (0,)) != 0):
            kinds.add("outside")
    assert {"identity", "translation", "scale", "negative m0", "quarter turn", "rotation", "shear", "outside", "zoom", "bounds"} <= kinds, kinds


# ---- host functions ----

def _random_matrix(rng, k):
    """Matrices around and beyond the refusal bounds."""
    mag = [1.0, 100.0, 16000.0, 40000.0][k % 4]
    m = [float(v) for v in rng.uniform(-mag, mag, 6)]
    m[2], m[5] = (float(v) for v in rng.uniform(-34000, 34000, 2))
    if k % 7 == 0:
        m[int(rng.integers(0, 6))] = [math.nan, math.inf, -math.inf][k % 3]
    if k % 5 == 0:
        m[1] = m[3] = 0.0
    return m


def test_warp_check_is_the_reference_rule():
    rng = np.random.default_rng(416)
    accepted = refused = 0
    for k in range(3000):
        m = _random_matrix(rng, k)
        ow, oh = (int(v) for v in rng.integers(1, 2049, 2))
        want = WR.check(m, ow, oh)
        assert J.warp_check(m, (ow, oh)) == want, (m, ow, oh)
        accepted, refused = accepted + want, refused + (not want)
    assert accepted > 100 and refused > 100
    edge = [((16000.0, 0, -32000.0, 0, 16000.0, -16000.0), (4, 3), True), ((16000.000001, 0, -32000.0, 0, 1, 0), (1, 1), False),
            ((1, 0, 32000.0, 0, 1, 0), (224, 224), False), ((1, 0, 32000.0 - 224, 0, 1, -32000.0), (224, 224), True),
            ((1, 0, 0, 0, 1, -32000.0000001), (224, 224), False), ((0, -16000.0, 32000.0, 16000.0, 0, -32000.0), (4, 4), True),
            (WR.IDENTITY, (2048, 2048), True), ((1, 0, 0, 0, 1, math.nan), (8, 8), False), ((1, math.inf, 0, 0, 1, 0), (8, 8), False)]
    for m, size, want in edge:
        assert WR.check(m, *size) == want and J.warp_check(m, size) == want, (m, size)
    assert N.lib().jpgpu_warp_check(None, 8, 8) != 0


def test_warp_nearest_axis_is_the_reference_table():
    rng = np.random.default_rng(417)
    for k in range(300):
        a = float(rng.uniform(-3, 3)) if k % 3 else float(rng.uniform(-16000, 16000))
        b = float(rng.uniform(-32000, 32000)) if k % 2 else float(rng.uniform(-50, 50))
        n = int(rng.integers(1, 2049))
        assert np.array_equal(J.warp_nearest_axis(a, b, n), WR.nearest_axis(a, b, n)), (a, b, n)
    for a, b in [(1.0, 0.0), (0.0, 5.0), (1e300, 0.0), (-1e300, 5.0), (math.nan, 1.0), (1.0, math.inf), (1.0, -0.5), (0.1, 0.05)]:
        assert np.array_equal(J.warp_nearest_axis(a, b, 40), WR.nearest_axis(a, b, 40)), (a, b)
    assert np.array_equal(J.warp_nearest_axis(1.0, 0.0, 5), [0, 1, 2, 3, 4]) and np.array_equal(J.warp_nearest_axis(1.0, -0.5, 3), [0, 1, 2])
    assert np.array_equal(J.warp_nearest_axis(1.0, -0.6, 3), [-1, 0, 1]) and len(J.warp_nearest_axis(1.0, 0.0, 0)) == 0


ANCHORS = [((0, (224, 224), None, None), (1.0, -0.0, 0.0, 0.0, 1.0, 0.0)),
           ((90, (48, 40), None, None), (0.0, -1.0, 44.0, 1.0, 0.0, -4.0)),
           ((15, (224, 224), None, None), (0.965925826289068, -0.258819045102521, 32.804040507106734, 0.258819045102521, 0.965925826289068, -25.171425595857983)),
           ((-30.5, (33, 21), (3.5, 4.25), (2, -1)), (0.861629160441526, 0.507538362960704, -2.8884600620506813, -0.507538362960704, 0.861629160441526, 4.241166224848913))]


def test_rotate_matrix_anchors():
    for (angle, size, center, translate), want in ANCHORS:
        got = J.rotate_matrix(angle, size, center, translate)
        assert got == WR.rotate_matrix(angle, size, center, translate)
        assert got == want, (angle, got)
    rng = np.random.default_rng(5)
    for _ in range(200):
        args = (float(rng.uniform(-720, 720)), (int(rng.integers(1, 500)), int(rng.integers(1, 500))), tuple(rng.uniform(-9, 300, 2)), tuple(rng.uniform(-20, 20, 2)))
        assert J.rotate_matrix(*args) == WR.rotate_matrix(*args)


def test_rotate_matrix_is_image_rotate():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)
    sq = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    for arr in (a, sq):
        img = Image.fromarray(arr, "RGB")
        for angle in (0, 90, 180, 270, 15, -33.3, 123.4, 360, 450):
            for center, translate in ((None, None), ((10.5, 7), None), (None, (3, -2)), ((5, 30.25), (-4, 6))):
                for resample in (Image.NEAREST, Image.BILINEAR):
                    want = img.rotate(angle, resample, center=center, translate=translate, fillcolor=(9, 8, 7))
                    got = img.transform(img.size, Image.AFFINE, J.rotate_matrix(angle, img.size, center, translate), resample, fillcolor=(9, 8, 7))
                    assert np.array_equal(np.asarray(want), np.asarray(got)), (angle, center, translate, resample)


# ---- the kernel bodies, lane by lane ----

@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    so = str(tmp_path_factory.mktemp("emu_warp") / "libemuwarp.so")
    subprocess.check_call([cxx, *_FLAGS, "-shared", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"), "-o", so, os.path.join(_EMU, "emu_warp.cpp")])
    L = C.CDLL(so)
    u, p = C.c_uint32, C.c_void_p
    L.emu_warp.argtypes = [p, u, u, u, u, u, p, p, p, u, p, p]
    L.emu_warp.restype = C.c_int
    return L


def _emu_warp(L, src, m, filter, fill, flip=0, table=None):
    H, W, nc = src.shape
    src = np.ascontiguousarray(src)
    mm = (C.c_double * 6)(*[float(v) for v in m])
    ff = (C.c_uint8 * 4)(*(list(fill) + [0] * 4)[:4])
    kind = C.c_uint32(9)
    guard = 64
    if table is None:
        out = np.full(H * W * nc + guard, 0x5A, np.uint8)
        rc = L.emu_warp(src.ctypes.data, W, H, nc, flip, filter, mm, ff, out.ctypes.data, 0, None, C.byref(kind))
        assert rc == 0 and np.all(out[H * W * nc:] == 0x5A)
        return out[: H * W * nc].reshape(H, W, nc), kind.value
    table = np.ascontiguousarray(table)
    out = np.full(H * W * nc + guard, 0x5A5A, table.dtype)
    rc = L.emu_warp(src.ctypes.data, W, H, nc, flip, filter, mm, ff, out.ctypes.data, table.dtype.itemsize, table.ctypes.data, C.byref(kind))
    assert rc == 0 and np.all(out[H * W * nc:] == 0x5A5A)
    return out[: H * W * nc].reshape(nc, H, W), kind.value


def test_every_kernel_body_gives_the_reference_on_the_golden_cases(golden, emu):
    kinds = set()
    for c in golden["cases"]:
        a = _source(c)
        got, kind = _emu_warp(emu, a, c["m"], c["filter"], c["fill"])
        assert _sha(got) == c["sha256"], c
        kinds.add(kind)
    assert kinds == {0, 1, 2}


def test_kernel_bodies_flips_and_tensor_stores(golden, emu):
    rng = np.random.default_rng(3)
    for k, c in enumerate(golden["cases"][::3]):
        a, nc = _source(c), c["C"]
        flip = k & 1
        want = WR.warp(a[:, ::-1] if flip else a, c["m"], c["filter"], c["fill"])
        got, _ = _emu_warp(emu, a, c["m"], c["filter"], c["fill"], flip)
        assert np.array_equal(got, want), c
        table = rng.integers(0, 1 << 16, (nc, 256)).astype([np.uint32, np.uint16][k % 2])
        got, _ = _emu_warp(emu, a, c["m"], c["filter"], c["fill"], flip, table)
        for ch in range(nc):
            assert np.array_equal(got[ch], table[ch][want[:, :, ch]]), (c, ch)


def test_bodies_and_job_builder_under_the_sanitizers(tmp_path):
    """A stand-alone program (its own main): nothing is loaded into Python."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "warp_asan")
    cmd = [cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17", "-Wall",
           "-Wno-unknown-pragmas", "-Wno-unused-function", "-ffp-contract=off", "-DJPGPU_HOST_EMULATION", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"),
           "-o", exe, os.path.join(_EMU, "warp_asan.cpp")]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "warp_asan: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
