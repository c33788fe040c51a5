"""The plan of the output-stage fuzzer (tests/output_fuzz_plan.py) examined on the CPU, for the seeds and round counts
tests/test_gpu_output_fuzz.py runs on the MI355X: every round is legal and replayable; every branch the stage chooses by geometry is
reached by at least three images (classified by the product's own planners through tests/emu/emu_filters.cpp, else from
filter_ref.coefficients); the references discriminate where the plan claims they do; the references equal Pillow itself on every
configuration of the plan; and the emulated kernel bodies — band, tensor, placed, run and warp — give the references' bytes with
their guard bytes untouched.  The sources here are numpy stand-ins of the planned shapes (output_fuzz_plan.stand_in): the decode in
front of the stage is the GPU leg's.  No GPU needed."""
import collections

import numpy as np
import pytest

import filter_ref as F
import output_fuzz_plan as OP
import rgb_ref as G
import tensor_ref as T
import test_filters_emulation as FE
import warp_ref as WR
from test_filters_emulation import lib  # noqa: F401  (the fixture that compiles tests/emu/emu_filters.cpp)
from test_warp import _emu_warp, emu  # noqa: F401  (and tests/emu/emu_warp.cpp)

# the seeds and rounds of tests/test_gpu_output_fuzz.py
SEEDS = (2026, 2027)
ROUNDS = 26
NEED = 3
LDS = 32 * 1024
MODES = {1: "L", 3: "RGB", 4: "CMYK"}


def fmt_of(dtype):
    return (dtype,) + OP.FORMATS[dtype]


def _pil():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def _image_of(Image, a):
    return Image.frombytes(MODES[a.shape[2]], (a.shape[1], a.shape[0]), np.ascontiguousarray(a).tobytes())


def _array_of(im, nc):
    return np.asarray(im).reshape(im.size[1], im.size[0], nc)


def _pil_filter(Image, name):
    return {"bilinear": Image.BILINEAR, "box": Image.BOX, "hamming": Image.HAMMING, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]


def spans_of(name, in_h, rh, first, count, rb):
    """The source rows [s0, s1) of every band of `rb` rows over entries [first, first + count) of the vertical axis (plan_of of
    tests/test_gpu_filters.py on the reference's tables)."""
    vb, _ = F.coefficients_range(in_h, rh, first, count, F.NAMES[name])
    return [(int(vb[r0, 0]), int(vb[min(r0 + rb, count) - 1].sum())) for r0 in range(0, count, rb)]


def positions(m, kind, px, py, w, h):
    """The source position of output pixel (px, py) as the reference's rules compute it: rule B's doubles, rule N's 16.16 integers
    (as a fraction of 65536), rule N-sep's running sums -> (x, y) as floats that hold the rule's value exactly."""
    m = [float(v) for v in m]
    if kind == "B":
        xin, yin = np.float64(px) + 0.5, np.float64(py) + 0.5
        return float((m[0] * xin + m[1] * yin) + m[2]), float((m[3] * xin + m[4] * yin) + m[5])
    if kind == "N":
        a2, a5 = WR.fix(m[2] + m[0] * 0.5 + m[1] * 0.5), WR.fix(m[5] + m[3] * 0.5 + m[4] * 0.5)
        return (a2 + px * WR.fix(m[0]) + py * WR.fix(m[1])) / 65536.0, (a5 + px * WR.fix(m[3]) + py * WR.fix(m[4])) / 65536.0
    xo = m[2] + m[0] * 0.5
    for _ in range(px):
        xo = xo + m[0]
    yo = m[5] + m[4] * 0.5
    for _ in range(py):
        yo = yo + m[4]
    return xo, yo


class Study:
    def __init__(self):
        self.classes = collections.Counter()
        self.shifts = set()
        self.bad_emulation, self.bad_pillow, self.bad_pins = [], [], []
        self.no_entry_point = 0
        self.emulated = self.pillow_checked = self.images = 0
        self.discriminates = collections.Counter()
        self.keeps = []

    def hit(self, *names):
        for n in names:
            self.classes[n] += 1


def examine(st, L, W, Image, seed, r, rd):
    """One round: every image's reference chain, its classes, the Pillow comparisons and the emulations."""
    ow, oh = rd["size"]
    name, f = rd["filter"], F.NAMES[rd["filter"]]
    rgb, dtype, wp = rd["rgb"], rd["tensor"], rd["warp"]
    pls = rd["placements"]
    placed = pls is not None and any(p is not None and tuple(p) != (ow, oh, 0, 0) for p in pls)
    knob = rd["roll"]
    for i, img in enumerate(rd["images"]):
        where = (seed, r, i)
        st.images += 1
        src = OP.stand_in(img)
        sh, sw, nc = src.shape
        kind = nc if (rgb and nc != 3) else 0
        onc = 3 if rgb else nc
        conv = G.to_rgb(src) if rgb else src
        pl = (tuple(pls[i]) if pls[i] is not None else (ow, oh, 0, 0)) if placed else None
        win = img["window"]
        src_off = 0 if (nc == 4 or win is None) else (win[0] * nc) & 3
        sums = []
        want = F.resize(conv, ow, oh, f, sums=sums) if pl is None else F.placed(conv, *pl, ow, oh, rd["fill"], f)
        rw, rh = (ow, oh) if pl is None else pl[:2]
        # ---- Pillow: convert, resize / paste ----
        if Image is not None:
            st.pillow_checked += 1
            im = _image_of(Image, src)
            if rgb:
                im = im.convert("RGB")
                if not np.array_equal(_array_of(im, 3), conv):
                    st.bad_pillow.append((where, "convert"))
            if pl is None:
                got = _array_of(im.resize((ow, oh), _pil_filter(Image, name)), onc)
            else:
                canvas = Image.new(MODES[onc], (ow, oh), tuple(rd["fill"][:onc]) if onc > 1 else rd["fill"][0])
                canvas.paste(im.resize((rw, rh), _pil_filter(Image, name)), (pl[2], pl[3]))
                got = _array_of(canvas, onc)
            if not np.array_equal(got, want):
                st.bad_pillow.append((where, "resize" if pl is None else "paste", name, (sw, sh), rd["size"], pl))
        # ---- the resample stage's kernel: u8 (also in front of a warp), or the tensor kernel ----
        tensor_kernel = dtype is not None and wp is None
        got, info = FE.run(L, f, src, ow, oh, kind, pl, rd["fill"], src_off=src_off)
        st.emulated += 1
        if not np.array_equal(got, want):
            st.bad_emulation.append((where, "u8", info, np.argwhere(got != want)[:4].tolist()))
        flips = [bool(rd["flips"][k][i]) for k in range(2)] if dtype is not None else [False, False]
        if tensor_kernel:
            for flip in sorted(set(flips)):
                gt, _info = FE.run_tensor(L, f, src, ow, oh, fmt_of(dtype), flip, kind, pl, rd["fill"], src_off=src_off)
                st.emulated += 1
                if not np.array_equal(T.bits(gt), T.bits(T.to_tensor(want, T.table(fmt_of(dtype), onc), flip))):
                    st.bad_emulation.append((where, "tensor", dtype, flip, info))
        # ---- the run route: what the rule or the knob gives for this job ----
        route, rinfo = "chunked" if info["chunks"] > 1 else "band", None
        if pl is None and name in OP.WIDE and knob != 1:
            for flip in (sorted(set(flips)) if tensor_kernel else [False]):
                rc, gr, rinfo_ = FE.run_runs(L, f, src, ow, oh, knob or 0, kind, src_off=src_off, fmt=fmt_of(dtype) if tensor_kernel else None, flip=flip)
                assert rc in (0, -4), (where, rc)
                if rc == 0:
                    st.emulated += 1
                    route, rinfo = "run", rinfo_
                    w_ = T.bits(T.to_tensor(want, T.table(fmt_of(dtype), onc), flip)) if tensor_kernel else want
                    if not np.array_equal(T.bits(gr) if tensor_kernel else gr, w_):
                        st.bad_emulation.append((where, "run", knob, rinfo_, flip))
        elif placed and name in OP.WIDE and knob in (2, 4, 8):
            st.no_entry_point += 1  # (a placed batch never takes the run route: nothing to emulate, nothing to count as reached)
        # ---- classes of the resample stage ----
        out = "tensor" if tensor_kernel else "u8"
        vis = OP.visible(pl, rd["size"]) if pl is not None else (0, 0, ow, oh)
        vw, vh = vis[2], vis[3]
        st.hit(f"src_nc {kind} {route} {out}", f"row bytes % 4 == {(ow * onc) % 4}")
        if route == "band" and info["rb"] > 1:
            st.hit("bands of rb > 1")
        if route == "band" and info["rb"] == 1 and vh > 1:
            st.hit("rb == 1 in one chunk")
        if route == "chunked" and pl is None and oh in (1, 3):
            st.hit(f"chunked to a height of {oh}")
        if route == "run":
            st.hit("run route by the rule" if knob is None else f"run route forced by {knob}")
            if 0 < rinfo["last_run"] < rinfo["bpr"]:
                st.hit("run route: a shorter last run")
            sp = spans_of(name, sh, oh, 0, oh, rinfo["rb"])
            for b in range(1, len(sp)):
                if b % rinfo["bpr"]:  # (neighbours inside a run)
                    st.keeps.append(sp[b - 1][1] - sp[b][0])
                    if sp[b][0] == sp[b - 1][0]:
                        st.hit("run route: shift == 0 between neighbouring bands")
                        break
        if win is not None and nc in (1, 3):
            st.hit(f"window x * nc % 4 == {(win[0] * nc) % 4} of a {nc}-channel source")
        if win is not None and win[2:] == (1, 1):
            st.hit("a 1 x 1 window")
        if (ow, oh) == (1, 1):
            st.hit("a 1 x 1 output")
        st.hit("x " + ("up" if rw > sw else "down" if rw < sw else "equal"), "y " + ("up" if rh > sh else "down" if rh < sh else "equal"))
        if tensor_kernel:
            st.hit("tensor " + dtype, "tensor: four-pixel items" if ((ow | (ow * oh)) & 3) == 0 else "tensor: flat items")
            for flip in flips:
                st.hit("tensor flipped" if flip else "tensor not flipped")
                if flip and route == "chunked":
                    st.hit("tensor flipped on the chunked path")
                if flip and not np.array_equal(want[:, ::-1], want):
                    st.discriminates["a flipped expectation differs"] += 1
        if placed:
            vx, vy = vis[0], vis[1]
            shift = (vx * onc) & 15
            st.shifts.add(shift)
            pre = -(-vy // info["rb"])
            row0 = vy - pre * info["rb"]
            st.hit("placed")
            if shift % 4:
                st.hit("placed: shift % 4 != 0")
            if pre > 0 and row0 < 0:
                st.hit("placed: pre > 0 with row0 < 0")
            if route == "chunked":
                st.hit("placed: a chunked inner job")
                assert info["rb"] == 1 and row0 == 0  # (chunked means rb == 1: row0 < 0 cannot meet a chunked inner job)
            st.hit(*[n for n, c in (("placed: negative x", pl[2] < 0), ("placed: negative y", pl[3] < 0), ("placed: fill left", vx > 0), ("placed: fill above", vy > 0),
                                    ("placed: fill right", vx + vw < ow), ("placed: fill below", vy + vh < oh), ("placed: one visible column", vw == 1),
                                    ("placed: one visible row", vh == 1)) if c])
            if tensor_kernel and any(flips) and ow % 4:
                st.hit("placed: tensor, flipped, ow % 4 != 0")
        # ---- discrimination of the resample stage ----
        if kind == 4 and pl is None and not np.array_equal(want, G.to_rgb(F.resize(src, ow, oh, f))):
            st.discriminates["CMYK: convert-then-resample differs from resample-then-convert"] += 1
        if name in OP.WIDE and pl is None and FE.clamps_at_both_ends(sums):
            st.discriminates["wide filters clamp at both ends in both passes"] += 1
        if name != "bilinear":
            other = F.resize(conv, ow, oh) if pl is None else F.placed(conv, *pl, ow, oh, rd["fill"])
            st.discriminates["the filter's result differs from bilinear's"] += not np.array_equal(other, want)
        # ---- the warp behind it ----
        if wp is None:
            continue
        wfilt = WR.BILINEAR if wp["filter"] == "bilinear" else WR.NEAREST
        both_fills = False
        for k in range(2):
            m = wp["warps"][k][i]
            mm = WR.IDENTITY if m is None else tuple(m)
            flip = flips[k]
            wkind = "B" if wfilt == WR.BILINEAR else ("N-sep" if (mm[1] == 0.0 and mm[3] == 0.0) else "N")
            r_ = want[:, ::-1] if flip else want
            ww = WR.warp(r_, mm, wfilt, wp["fill"])
            if Image is not None:
                fillc = tuple(wp["fill"][:onc]) if onc > 1 else wp["fill"][0]
                pw = _image_of(Image, np.ascontiguousarray(r_)).transform((ow, oh), Image.AFFINE, mm, Image.BILINEAR if wfilt else Image.NEAREST, fillcolor=fillc)
                if not np.array_equal(_array_of(pw, onc), ww):
                    st.bad_pillow.append((where, "transform", k, mm, wp["filter"]))
            table = None if dtype is None else T.bits(T.table(fmt_of(dtype), onc))
            gw, ekind = _emu_warp(W, want, mm, wfilt, wp["fill"], 1 if flip else 0, table)
            st.emulated += 1
            assert ekind == {"N": 0, "N-sep": 1, "B": 2}[wkind], (where, ekind, wkind)
            ok = np.array_equal(gw, ww) if table is None else all(np.array_equal(gw[c], table[c][ww[:, :, c]]) for c in range(onc))
            if not ok:
                st.bad_emulation.append((where, "warp", k, mm, wp["filter"], flip))
            st.hit(f"warp {wkind} " + ("flipped" if flip else "not flipped"), f"warp of {onc} channels", "warp " + ("tensor" if dtype else "u8"))
            if not (ww != np.asarray(wp["fill"][:onc], np.uint8)).any() and (want != np.asarray(wp["fill"][:onc], np.uint8)).any():
                st.hit("warp: everything outside")
            if mm == WR.IDENTITY:
                st.hit("warp: the identity")
                assert np.array_equal(ww, r_)
            elif mm[:2] == (1.0, 0.0) and mm[3:5] == (0.0, 1.0) and mm[2] == int(mm[2]) and mm[5] == int(mm[5]) and abs(mm[2]) < 100:
                st.hit("warp: an integer translation")
            st.hit(*[n for n, c in (("warp behind a run-route plan", route == "run"), ("warp behind a placement", placed), ("warp behind a window", win is not None)) if c])
            if flip and not np.array_equal(ww, WR.warp(want, mm, wfilt, wp["fill"])[:, ::-1]):
                st.discriminates["warp-then-mirror differs from mirror-then-warp"] += 1
            if placed and not both_fills and tuple(rd["fill"][:onc]) != tuple(wp["fill"][:onc]):
                px = ww.reshape(-1, onc)
                if (px == np.asarray(rd["fill"][:onc], np.uint8)).all(axis=1).any() and (px == np.asarray(wp["fill"][:onc], np.uint8)).all(axis=1).any():
                    both_fills = True
                    st.discriminates["placement fill and warp fill both show, and differ"] += 1
        for pin in wp["pins"]:
            if pin["image"] != i:
                continue
            m = wp["warps"][pin["set"]][i]
            wkind = "B" if wfilt == WR.BILINEAR else ("N-sep" if (m[1] == 0.0 and m[3] == 0.0) else "N")
            pos = positions(m, wkind, pin["px"], pin["py"], ow, oh)
            n = (ow, oh)[pin["axis"]]
            value = {"zero": 0.0, "size": float(n)}.get(pin["target"], pin["value"])
            if pos[pin["axis"]] != value or value != pin["value"] or (pin["target"] == "edge" and not (value == int(value) and 0 <= value <= n)):
                st.bad_pins.append((where, pin, m, pos))
            st.hit({"zero": "warp: a source position exactly 0.0", "size": "warp: a source position exactly w or h", "edge": "warp: a source position exactly on a pixel edge"}[pin["target"]])


@pytest.fixture(scope="module")
def study(lib, emu):  # noqa: F811
    st = Study()
    Image = _pil()
    for seed in SEEDS:
        for r, rd in enumerate(OP.plan(seed, ROUNDS)):
            examine(st, lib, emu, Image, seed, r, rd)
    return st


def test_plans_are_seeded_legal_and_literal():
    total = 0
    for seed in SEEDS:
        a, b = OP.plan(seed, ROUNDS), OP.plan(seed, ROUNDS)
        assert a == b and len(a) == ROUNDS
        assert OP.plan(seed, 5) == a[:5]  # (a round depends on the rounds before it only)
        for rd in a:
            assert eval(repr(rd), {"__builtins__": {}}) == rd  # (what --replay prints is what it accepts)
            OP.check_round(rd)
            assert 2 <= len(rd["images"]) <= 6
            for img in rd["images"]:
                sw, sh = OP.effective_size(img)
                assert OP.stand_in(img).shape == (sh, sw, OP.NC[img["layout"]])
        assert sum(rd["pipeline"] is not None for rd in a) == ROUNDS // 4
        total += OP.image_count(a)
    assert OP.plan(SEEDS[0], ROUNDS) != OP.plan(SEEDS[1], ROUNDS)
    assert {rd["roll"] for s in SEEDS for rd in OP.plan(s, ROUNDS)} == set(OP.ROLLS)
    assert total > 400


def test_the_plan_speaks_the_library_s_sizes():
    """What the plan assumes about the decode in front of the stage: reduced sizes, and the fixture files' sizes."""
    import jpeg_decoder_amd as J
    import oracle as O
    import test_gpu_pipeline_windows as PW
    for w in (1, 9, 50, 97, 100):
        for s in (8, 4, 2, 1):
            img = {"w": w, "h": w + 3, "scale": s}
            assert OP.source_size(img) == tuple(J.scaled_output_size(w, w + 3, s))
    for (layout, enc, sz), (W, H, nc) in OP.FILES:
        if layout in ("cmyk", "ycck"):
            d = O.decode(PW._file(layout, enc, sz))
            assert (d.width, d.height, d.ncomp) == (W, H, nc), (layout, sz)
        else:
            assert (W, H) == sz and nc == (1 if layout == "gray" else 3)


CLASSES = (
    ["bands of rb > 1", "rb == 1 in one chunk", "chunked to a height of 1", "chunked to a height of 3", "run route by the rule", "run route forced by 2",
     "run route forced by 4", "run route forced by 8", "run route: a shorter last run", "run route: shift == 0 between neighbouring bands"]
    + [f"src_nc {k} {route} {out}" for k in (0, 1, 4) for route in ("band", "chunked", "run") for out in ("u8", "tensor")]
    + [f"row bytes % 4 == {k}" for k in range(4)]
    + [f"window x * nc % 4 == {k} of a {nc}-channel source" for k in range(4) for nc in (1, 3)]
    + [f"{a} {d}" for a in "xy" for d in ("up", "down", "equal")] + ["a 1 x 1 window", "a 1 x 1 output"]
    + ["tensor: four-pixel items", "tensor: flat items", "tensor float32", "tensor float16", "tensor bfloat16", "tensor flipped", "tensor not flipped",
       "tensor flipped on the chunked path"]
    + ["placed: shift % 4 != 0", "placed: pre > 0 with row0 < 0", "placed: negative x", "placed: negative y", "placed: fill left", "placed: fill above",
       "placed: fill right", "placed: fill below", "placed: one visible column", "placed: one visible row", "placed: a chunked inner job",
       "placed: tensor, flipped, ow % 4 != 0"]
    + [f"warp {k} {fl}" for k in ("N", "N-sep", "B") for fl in ("flipped", "not flipped")] + [f"warp of {c} channels" for c in (1, 3, 4)]
    + ["warp u8", "warp tensor", "warp: everything outside", "warp: the identity", "warp: an integer translation", "warp: a source position exactly 0.0",
       "warp: a source position exactly w or h", "warp: a source position exactly on a pixel edge", "warp behind a run-route plan", "warp behind a placement",
       "warp behind a window"])
# Dropped as unreachable: "keep == 0 between neighbouring bands of a run".  Only BICUBIC and LANCZOS jobs are candidates; their support is
# at least two source pixels times max(scale, 1) on each side while neighbouring output rows' centres lie `scale` apart, so the last row
# of a band and the first row of the next share at least one source row whatever the sizes (clipping at the image's edges keeps the
# shared row).  test_every_class_is_reached asserts it on every pair of neighbouring bands the plan's runs have.  shift == 0 is reached
# (up-scaled bands begin at the same source row).  And `row0 < 0` cannot meet a chunked inner job: chunked means rb == 1, and with one
# row per band row0 is 0 (asserted in examine()); the two are classes of their own above.
DISCRIMINATES = ["a flipped expectation differs", "warp-then-mirror differs from mirror-then-warp", "placement fill and warp fill both show, and differ",
                 "CMYK: convert-then-resample differs from resample-then-convert", "wide filters clamp at both ends in both passes",
                 "the filter's result differs from bilinear's"]


def test_every_class_is_reached(study):
    counts = {c: study.classes[c] for c in CLASSES}
    report = "\n".join(f"{n:6d}  {c}" for c, n in counts.items()) + f"\n{len(study.shifts):6d}  distinct values of shift: {sorted(study.shifts)}"
    print(report)
    short = [c for c, n in counts.items() if n < NEED]
    assert not short and len(study.shifts) >= 8, f"classes short of {NEED} images: {short}\n{report}"
    assert study.keeps and min(study.keeps) > 0, "keep == 0 IS reachable: make it a class"
    assert study.images == sum(len(rd["images"]) for s in SEEDS for rd in OP.plan(s, ROUNDS))


def test_the_references_discriminate(study):
    print({d: study.discriminates[d] for d in DISCRIMINATES})
    short = [d for d in DISCRIMINATES if study.discriminates[d] < NEED]
    assert not short, (short, dict(study.discriminates))


def test_pinned_positions_hold_on_the_reference_s_own_arithmetic(study):
    assert not study.bad_pins, study.bad_pins[:5]


def test_the_references_are_pillow_on_every_configuration(study):
    pytest.importorskip("PIL")
    assert study.pillow_checked == study.images and not study.bad_pillow, (len(study.bad_pillow), study.bad_pillow[:8])


def test_the_emulated_kernels_give_the_references_bytes(study):
    print("emulations", study.emulated, "placed jobs under a forced knob (no run route, no entry point)", study.no_entry_point)
    assert study.emulated >= study.images and not study.bad_emulation, (len(study.bad_emulation), study.bad_emulation[:8])
