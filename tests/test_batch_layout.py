"""The window rule, the output layout and the headroom rule of a batch (csrc/batch_layout.hpp), without a GPU: the functions batch_create,
batch_check_window, batch_rewindow and the pipeline share, compiled with g++ (tests/emu/emu_batch_layout.cpp) and checked against the
rule as it is stated — empty: no window; outside the grid: a format error; the whole grid: no window — and against each other:
planning a window group with one list of windows and rewindowing it to another gives what planning with the other gives."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpeg_decoder_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EMU = os.path.join(ROOT, "tests", "emu")
# the flags of tests/emu/Makefile
_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DJPGPU_HOST_EMULATION"]
OK, ERR_FORMAT, ERR_UNSUPPORTED = 0, 1, 2

# struct WindowGeom (csrc/window_band.hpp), word by word
GEOM_FIELDS = ["scale", "ncomp", "hmax", "vmax", "mcu_w", "mcu_h", "align", "tx", "ry", "ox", "oy", "ex", "ey", "tiles_x", "bands"] + \
              [f"{n}[{c}]" for n in ("h", "v", "halo", "block_w", "block_h", "lds_off", "pitch") for c in range(4)] + \
              ["lds_bytes", "margin", "out_w", "out_h", "wx", "wy", "ww", "wh", "first_plane_job"]

LAYOUTS = {"420": ([(2, 2), (1, 1), (1, 1)], "YCbCr"), "444": ([(1, 1)] * 3, "YCbCr"), "422": ([(2, 1), (1, 1), (1, 1)], "YCbCr"),
           "gray": ([(1, 1)], "Grayscale"), "cmyk": ([(2, 2), (1, 1), (1, 1), (1, 1)], "CMYK")}
SCALES = (8, 4, 2, 1)
SIZES = ((8, 8), (17, 9), (333, 200))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_batch_layout") / "libemulayout.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), *_FLAGS, "-shared", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"), "-o", so,
                           os.path.join(_EMU, "emu_batch_layout.cpp"), os.path.join(ROOT, "jpeg-decoder_amd", "csrc", "image_job.cpp")])
    L = C.CDLL(so)
    L.emu_window_rule.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32]
    L.emu_arena_layout.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.emu_arena_layout.restype = C.c_size_t
    L.emu_arena_headroom.argtypes = [C.c_size_t, C.c_size_t]
    L.emu_arena_headroom.restype = C.c_size_t
    L.emu_plan_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.emu_plan_create.restype = C.c_void_p
    L.emu_plan_rewindow.argtypes = [C.c_void_p, C.c_void_p]
    L.emu_plan_members.argtypes = [C.c_void_p]
    L.emu_plan_members.restype = C.c_uint32
    L.emu_plan_read.argtypes = [C.c_void_p] * 6
    L.emu_plan_read.restype = C.c_size_t
    L.emu_plan_destroy.argtypes = [C.c_void_p]
    L.emu_plan_destroy.restype = None
    assert L.emu_window_geom_words() == len(GEOM_FIELDS)
    return L


def _desc(w_, h_, layout, scale, out=None):
    samp, ct = LAYOUTS[layout]
    comps, _ = J.make_components(w_, h_, samp, dct_scale=scale)
    ow, oh = out or J.scaled_output_size(w_, h_, scale)
    return J.image_desc(list(comps), [np.ones(64, np.uint16)] * len(samp), ow, oh, ct)


def _grid(desc):
    """The output grid: out_w x out_h, or the component's size for one component."""
    c = desc.components[0]
    return (c.size_width, c.size_height) if desc.ncomp == 1 else (desc.out_w, desc.out_h)


def _expected(desc, win):
    """(status, windowed, reason) from the rule as stated, for descriptors the window planner takes."""
    gw, gh = _grid(desc)
    x, y, w, h = win
    if w == 0 or h == 0:
        return OK, False, ""
    if x + w > gw or y + h > gh:
        return ERR_FORMAT, False, f"window ({x}, {y}) {w}x{h} outside the {gw}x{gh} image"
    return OK, (x, y, w, h) != (0, 0, gw, gh), ""


def _rule(lib, desc, win):
    out = np.zeros(3, np.uint32)
    why = C.create_string_buffer(256)
    rc = lib.emu_window_rule(C.byref(desc), C.byref(J._native.Window(*win)), out.ctypes.data, why, 256)
    return rc, bool(out[0]), (int(out[1]), int(out[2])), why.value.decode()


def _windows_of(gw, gh):
    return [(3, 2, 0, 5), (3, 2, 5, 0), (0, 0, gw, gh), (0, 0, gw - 1, gh), (gw - 1, gh - 1, 1, 1), (gw - 1, 0, 2, gh), (1, 0, gw, 1),
            (0, gh - 1, 1, 2), (65535, 0, 1, 1), (0, 65535, 1, 1)]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_window_rule_verdicts(lib, layout):
    checked = 0
    for scale in SCALES:
        for (w_, h_) in SIZES:
            desc = _desc(w_, h_, layout, scale)
            gw, gh = _grid(desc)
            for win in _windows_of(gw, gh):
                rc, windowed, grid, why = _rule(lib, desc, win)
                assert (rc, windowed, why) == _expected(desc, win), (layout, scale, (w_, h_), win, why)
                assert grid == (gw, gh)
                checked += 1
    assert checked == len(SCALES) * len(SIZES) * 10


@pytest.mark.parametrize("scale", (4, 2, 1))
def test_window_rule_judges_a_gray_image_by_its_component_not_by_out_size(lib, scale):
    """One component: the grid is the component's size whatever out_w x out_h say (here: the unscaled size)."""
    for (w_, h_) in SIZES:
        desc = _desc(w_, h_, "gray", scale, out=(w_, h_))
        gw, gh = desc.components[0].size_width, desc.components[0].size_height
        assert (gw, gh) != (w_, h_) and _grid(desc) == (gw, gh)
        assert _rule(lib, desc, (0, 0, gw, gh)) == (OK, False, (gw, gh), "")
        assert _rule(lib, desc, (0, 0, w_, h_)) == (ERR_FORMAT, False, (gw, gh), f"window (0, 0) {w_}x{h_} outside the {gw}x{gh} image")
        if gw > 1:
            assert _rule(lib, desc, (1, 0, gw - 1, gh)) == (OK, True, (gw, gh), "")


def test_output_layout(lib):
    rng = np.random.default_rng(7)
    cases = [[0], [1], [256], [257], [0, 0, 0], [255, 0, 1, 513], [83 * 59 * 3, 1, 40 * 30, 65535 * 3]]
    cases += [list(rng.integers(0, 5000, size=int(n))) for n in rng.integers(1, 40, size=20)]
    for lens in cases:
        n = len(lens)
        src, off, ln = np.array(lens, np.uintp), np.zeros(n, np.uintp), np.zeros(n, np.uintp)
        total = lib.emu_arena_layout(src.ctypes.data, n, off.ctypes.data, ln.ctypes.data)
        assert list(ln) == lens
        assert all(int(o) % 256 == 0 for o in off) and off[0] == 0
        for i in range(n - 1):  # image order, no overlap, no gap beyond the alignment
            assert off[i] + ln[i] <= off[i + 1] < off[i] + ln[i] + 256 and off[i + 1] >= off[i]
        padded = sum((v + 255) // 256 * 256 for v in lens)
        assert total == max(padded, 256) and off[-1] + ln[-1] <= total


def test_headroom(lib):
    def rule(need, full):
        return max(need, min(max(full, 256), need + need // 4))

    for need, full, want in ((1000, 10000, 1250),   # need < full: a quarter more
                             (4096, 4096, 4096),    # need = full: no more than the whole images take
                             (1000, 1100, 1100),    # need + need / 4 > full: capped at full
                             (256, 0, 256),         # full = 0: counts as the smallest arena
                             (1024, 0, 1024),       # ... and never below need
                             (3, 7, 3 + 0)):        # (3 + 3 // 4 = 3)
        assert rule(need, full) == want
        assert lib.emu_arena_headroom(need, full) == want, (need, full)


# ---- create / rewindow ------------------------------------------------------------------------------------------------------------------
def _mixed_descs():
    kinds = list(LAYOUTS)
    return [_desc(83 + 7 * (i % 5), 59 + 5 * (i % 3), kinds[i % len(kinds)], SCALES[(i // 2) % 4]) for i in range(16)]


def _structs(descs, wins):
    d = (J._native.ImageDesc * len(descs))(*descs)
    w = (J._native.Window * len(wins))(*[J._native.Window(*v) for v in wins])
    return d, w


def _read(lib, plan, n):
    m = lib.emu_plan_members(plan)
    ids, geoms = np.zeros(m, np.uint32), np.zeros((m, len(GEOM_FIELDS)), np.uint32)
    off, ln, full = np.zeros(n, np.uintp), np.zeros(n, np.uintp), np.zeros(n, np.uintp)
    total = lib.emu_plan_read(plan, ids.ctypes.data, geoms.ctypes.data, off.ctypes.data, ln.ctypes.data, full.ctypes.data)
    return {"ids": list(ids), "geoms": geoms, "off": list(off), "len": list(ln), "full": list(full), "bytes": total}


def _plan(lib, descs, wins):
    d, w = _structs(descs, wins)
    status = C.c_int(-1)
    plan = lib.emu_plan_create(d, w, len(descs), C.byref(status))
    return plan, status.value


def _sub_window(rng, gw, gh):
    """A window inside the gw x gh grid that is not the whole grid (gw * gh > 1)."""
    while True:
        w, h = int(rng.integers(1, gw + 1)), int(rng.integers(1, gh + 1))
        x, y = int(rng.integers(0, gw - w + 1)), int(rng.integers(0, gh - h + 1))
        if (w, h) != (gw, gh):
            return x, y, w, h


def _window_lists(rng, descs):
    """W1, W2 with the same windowed set; some members of W2 get their whole grid (or an empty window) instead."""
    members = sorted(rng.choice(len(descs), size=10, replace=False).tolist())
    w1, w2, whole = [], [], []
    for i, d in enumerate(descs):
        gw, gh = _grid(d)
        if i in members:
            w1.append(_sub_window(rng, gw, gh))
            r = rng.random()
            w2.append((0, 0, gw, gh) if r < 0.15 else (0, 0, 0, 0) if r < 0.25 else _sub_window(rng, gw, gh))
            if r < 0.25:
                whole.append(i)
        else:
            w1.append((0, 0, gw, gh) if rng.random() < 0.5 else (0, 0, 0, 0))
            w2.append((0, 0, 0, 7) if rng.random() < 0.5 else (0, 0, gw, gh))
    return members, w1, w2, whole


@pytest.mark.parametrize("seed", range(12))
def test_rewindow_equals_planning_anew(lib, seed):
    rng = np.random.default_rng(1000 + seed)
    descs = _mixed_descs()
    n = len(descs)
    members, w1, w2, whole = _window_lists(rng, descs)
    plan, status = _plan(lib, descs, w1)
    anew, status2 = _plan(lib, [d for i, d in enumerate(descs) if i not in whole], [w for i, w in enumerate(w2) if i not in whole])
    try:
        assert status == OK and status2 == OK
        before = _read(lib, plan, n)
        assert before["ids"] == members
        assert lib.emu_plan_rewindow(plan, _structs(descs, w2)[1]) == OK
        got, ref = _read(lib, plan, n), _read(lib, anew, n - len(whole))
        assert got["ids"] == members and got["full"] == before["full"]
        kept = [i for i in range(n) if i not in whole]                       # images of `anew`, in order
        assert [kept[j] for j in ref["ids"]] == [i for i in members if i not in whole]
        assert [got["len"][i] for i in kept] == ref["len"]
        # the layout is that of planning W2 with the whole-grid members as whole images of full length
        lens = [before["full"][i] if i in whole else ref["len"][kept.index(i)] for i in range(n)]
        assert got["len"] == lens
        off = np.concatenate(([0], np.cumsum([(v + 255) // 256 * 256 for v in lens])))
        assert got["off"] == list(off[:-1]) and got["bytes"] == max(int(off[-1]), 256)
        rk = 0
        first = 0
        for k, i in enumerate(members):
            g = dict(zip(GEOM_FIELDS, got["geoms"][k]))
            assert g["first_plane_job"] == first
            first += descs[i].ncomp
            gw, gh = _grid(descs[i])
            if i in whole:  # stays in the group with a whole-grid geometry
                assert (g["wx"], g["wy"], g["ww"], g["wh"]) == (0, 0, gw, gh) and got["len"][i] == before["full"][i]
                continue
            r = dict(zip(GEOM_FIELDS, ref["geoms"][rk]))
            rk += 1
            for name in GEOM_FIELDS:
                if name != "first_plane_job":  # (numbered within each group: `anew` has fewer members in front)
                    assert g[name] == r[name], (seed, i, name)
            assert (g["wx"], g["wy"], g["ww"], g["wh"]) == w2[i] and got["len"][i] == w2[i][2] * w2[i][3] * descs[i].ncomp
    finally:
        lib.emu_plan_destroy(plan)
        lib.emu_plan_destroy(anew)


@pytest.mark.parametrize("seed", range(6))
def test_rewindow_refuses_and_changes_nothing(lib, seed):
    rng = np.random.default_rng(2000 + seed)
    descs = _mixed_descs()
    n = len(descs)
    members, w1, w2, _ = _window_lists(rng, descs)
    plan, status = _plan(lib, descs, w1)
    try:
        assert status == OK
        before = _read(lib, plan, n)
        outsider = next(i for i in range(n) if i not in members)
        member = members[seed % len(members)]
        gw, gh = _grid(descs[member])
        for bad in ({outsider: _sub_window(rng, *_grid(descs[outsider]))},   # another windowed set
                    {member: (gw - 1, 0, 2, 1)},                             # a window outside its image
                    {outsider: (0, 65535, 1, 1)}):                           # ... on an image outside the set
            wins = [bad.get(i, w) for i, w in enumerate(w2)]
            assert lib.emu_plan_rewindow(plan, _structs(descs, wins)[1]) == ERR_UNSUPPORTED
            after = _read(lib, plan, n)
            assert all(np.array_equal(after[k], before[k]) for k in before)
    finally:
        lib.emu_plan_destroy(plan)


def test_creation_reports_the_rule_per_image(lib):
    descs = _mixed_descs()
    wins = [(0, 0, 0, 0)] * len(descs)
    gw, gh = _grid(descs[5])
    wins[5] = (1, 1, gw, gh)
    plan, status = _plan(lib, descs, wins)
    lib.emu_plan_destroy(plan)
    assert status == ERR_FORMAT
