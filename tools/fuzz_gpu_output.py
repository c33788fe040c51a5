#!/usr/bin/env python3
"""Differential fuzzing of the fixed-output stage: the rounds of tests/output_fuzz_plan.py — windows x filters x
RGB output x tensor formats with flips x placements x warps x JPGPU_RS_ROLL, crossed — through Batch and (every fourth round) through
one Pipeline kept for the whole run.  Every image of every decode must equal, bit for bit, the reference chain the feature tests use:
the oracle's decode sliced (test_gpu_resize.source_of), rgb_ref.to_rgb, filter_ref.resize / placed, warp_ref.warp, tensor_ref.to_tensor.
A round with the knob at 2 / 4 / 8 must also give the bytes of the same round under knob 1, the path string names `+roll` exactly where
the planner's rule (or the knob) sends an image down the run route, and a caller-owned output arena keeps its guard byte everywhere
outside the images.
    python tools/fuzz_gpu_output.py <seed> <rounds>            (on the GPU box; prints "bad 0")
    python tools/fuzz_gpu_output.py --replay '<round dict>'    (one round alone: the dict a mismatch prints)"""
import ast
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("oracle", "", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import numpy as np
import jpeg_decoder_amd as J
J.process_init()  # GPU_MAX_HW_QUEUES before the HIP runtime starts
import filter_ref as F
import output_fuzz_plan as OP
import rgb_ref as G
import tensor_ref as T
import test_gpu_filters as FT
import test_gpu_pipeline_windows as PW
import test_gpu_resize as RZ
import warp_ref as WR

KNOB = "JPGPU_RS_ROLL"
GUARD_TAIL = 4096
ROLL_MIN_PERCENT = 130  # RS_ROLL_MIN_PERCENT of csrc/resample_band.hpp
_SOURCES = {}


def _source(img):
    """(case, whole decode of the oracle) of a planned image, made once."""
    key = tuple(sorted((k, v) for k, v in img.items() if k != "window"))
    if key not in _SOURCES:
        if img["coef"] == "block":
            for bump in range(64):  # (block_case asserts that enough bytes are 0 / 255; a YCbCr pattern of a few blocks can miss that: the next one)
                try:
                    _SOURCES[key] = FT.block_case(img["layout"], img["w"], img["h"], img["by"], img["bx"], img["seed"] + bump)
                    break
                except AssertionError:
                    if bump == 63:
                        raise
        else:
            samp, ct = FT.LAYOUTS[img["layout"]]
            case = RZ._case(np.random.default_rng(img["seed"]), img["w"], img["h"], samp, ct, img["scale"], img["coef"])
            _SOURCES[key] = (case, RZ._full(case))
    return _SOURCES[key]


def ref_fmt(dtype):
    return (dtype,) + OP.FORMATS[dtype]


def resized_u8(rd, src, pl):
    """The image's u8 result without a warp and before the table: convert, then resize or place."""
    src = G.to_rgb(src) if rd["rgb"] else src
    f = F.NAMES[rd["filter"]]
    ow, oh = rd["size"]
    return F.resize(src, ow, oh, f) if pl is None else F.placed(src, *pl, ow, oh, rd["fill"], f)


def finished(rd, u8, flip, m):
    """A decode's expected bits from the image's u8 result: the warp (behind the flip), the table."""
    if rd["warp"] is not None:
        u8 = WR.warp(u8[:, ::-1] if flip else u8, WR.IDENTITY if m is None else m, WR.BILINEAR if rd["warp"]["filter"] == "bilinear" else WR.NEAREST, rd["warp"]["fill"])
        flip = False
    if rd["tensor"] is None:
        return u8.reshape(-1)
    return T.bits(T.to_tensor(u8, T.table(ref_fmt(rd["tensor"]), u8.shape[2]), flip)).reshape(-1)


def takes_run_route(rd, img, knob):
    """resample_roll_bpr restated on the library's own tables: does this image's job take the run route under `knob`?"""
    if knob == 1 or rd["filter"] not in OP.WIDE or placed_batch(rd):
        return False
    ow, oh = rd["size"]
    nc = 3 if rd["rgb"] else OP.NC[img["layout"]]
    _rb, bands, cap, spans = FT.plan_of(rd["filter"], OP.effective_size(img)[1], ow, oh, nc)
    if bands < 2 or any(s1 - s0 > cap for s0, s1 in spans):
        return False
    if knob in (2, 4, 8):
        return True
    return sum(s1 - s0 for s0, s1 in spans) * 100 > (spans[-1][1] - spans[0][0]) * ROLL_MIN_PERCENT


def placed_batch(rd):
    ow, oh = rd["size"]
    return rd["placements"] is not None and any(p is not None and tuple(p) != (ow, oh, 0, 0) for p in rd["placements"])


class _Knob:
    """JPGPU_RS_ROLL set or cleared for the creation of a batch (the tables are made there), and restored."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get(KNOB)
        if self.value is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = str(self.value)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = self.old


def _hip():
    hip = RZ._hip()
    hip.hipMalloc.restype = hip.hipFree.restype = hip.hipMemset.restype = hip.hipMemcpy.restype = C.c_int
    return hip


def _batch(rd, cases, knob, flags=0):
    wins = [img["window"] for img in rd["images"]]
    fmt = J.TensorFormat(rd["tensor"], *OP.FORMATS[rd["tensor"]]) if rd["tensor"] else None
    warp = J.WarpOptions(rd["warp"]["filter"], rd["warp"]["fill"]) if rd["warp"] else None
    with _Knob(knob):
        return J.Batch([RZ._desc(c) for c in cases], flags=flags, windows=wins if any(w is not None for w in wins) else None, output_size=rd["size"], tensor=fmt,
                       rgb=rd["rgb"], placements=rd["placements"], fill=rd["fill"], filter=rd["filter"], warp=warp)


def _set(b, rd, k):
    if rd["flips"] is not None:
        b.set_flips(rd["flips"][k])
    if rd["warp"] is not None:
        b.set_warps(rd["warp"]["warps"][k])


def batch_leg(rd, report):
    """Both decodes of the round on one batch whose output arena is the caller's, poisoned; then the knob-1 twin of a forced round.
    -> (comparisons made, path)."""
    hip = _hip()
    n = len(rd["images"])
    sources = [_source(img) for img in rd["images"]]
    cases = [c for c, _f in sources]
    pls = rd["placements"] if placed_batch(rd) else None
    u8s = [resized_u8(rd, RZ.source_of(case, full, img["window"]), None if pls is None else (pls[i] if pls[i] is not None else rd["size"] + (0, 0)))
           for i, ((case, full), img) in enumerate(zip(sources, rd["images"]))]
    made = 0
    b = _batch(rd, cases, rd["roll"], J._native.BATCH_EXTERNAL_BUFFERS)
    coef, out = C.c_void_p(), C.c_void_p()
    nco, nout = b.coef_arena_bytes(), b.out_arena_bytes()
    first = []
    try:
        assert hip.hipMalloc(C.byref(coef), max(nco, 1)) == 0 and hip.hipMalloc(C.byref(out), nout + GUARD_TAIL) == 0
        b.bind(coef.value, out.value)
        RZ._upload(b, cases)
        path = b.path
        want_roll = any(takes_run_route(rd, img, rd["roll"]) for img in rd["images"])
        if ("+roll" in path) != want_roll:
            report("path", -1, f"`+roll` in {path!r} is {'+roll' in path}, the planner's rule says {want_roll}")
        if "+roll" in path and "+warp" in path and path.index("+roll") > path.index("+warp"):
            report("path", -1, f"`+roll` behind `+warp` in {path!r}")
        if (rd["warp"] is not None) != ("+warp" in path) or (rd["tensor"] is not None) != ("+tensor" in path) or (pls is not None) != ("+place" in path):
            report("path", -1, f"{path!r} does not name the round's options")
        host = np.empty(nout + GUARD_TAIL, np.uint8)
        for k, guard in enumerate((0xA5, 0x3C)):
            _set(b, rd, k)
            assert hip.hipMemset(out, guard, nout + GUARD_TAIL) == 0
            b.decode()
            b.synchronize()
            assert hip.hipMemcpy(host.ctypes.data, out, nout + GUARD_TAIL, 2) == 0
            covered = np.zeros(nout + GUARD_TAIL, bool)
            for i in range(n):
                flip = bool(rd["flips"][k][i]) if rd["flips"] else False
                want = finished(rd, u8s[i], flip, rd["warp"]["warps"][k][i] if rd["warp"] else None)
                off, nb = b.out_offset(i), b.out_bytes(i)
                got = host[off: off + nb].view(want.dtype)
                covered[off: off + nb] = True
                made += 1
                if k == 0:
                    first.append(got.copy())
                if got.size != want.size or not np.array_equal(got, want):
                    report(f"decode {k}", i, f"{got.size} / {want.size} elements, first differing {np.nonzero(got != want)[0][:10].tolist() if got.size == want.size else '-'}")
            if not (host[~covered] == guard).all():
                report(f"decode {k}", -1, f"guard byte {guard:#x} overwritten outside the images at {np.nonzero(~covered & (host != guard))[0][:10].tolist()}")
    finally:
        b.close()
        hip.hipFree(coef)
        hip.hipFree(out)
    if rd["roll"] in (2, 4, 8):  # the same round under knob 1: the band route's bytes
        twin = _batch(rd, cases, 1)
        try:
            RZ._upload(twin, cases)
            _set(twin, rd, 0)
            twin.decode()
            twin.synchronize()
            if "+roll" in twin.path:
                report("knob 1", -1, f"`+roll` in {twin.path!r}")
            for i in range(n):
                made += 1
                got = T.bits(twin.download(i)).reshape(-1) if rd["tensor"] else twin.download(i)
                if not np.array_equal(got, first[i]):
                    report("knob 1", i, f"differs from knob {rd['roll']} at {np.nonzero(got != first[i])[0][:10].tolist() if got.size == first[i].size else 'another size'}")
        finally:
            twin.close()
    return made, path


def pipeline_leg(p, rd, report):
    """The round's options on JPEG bytes through the kept pipeline, compared as test_gpu_filters._p_check does.  -> (comparisons, path)."""
    pp = rd["pipeline"]
    files = [PW._file(layout, enc, tuple(sz), pic=pic) for layout, enc, sz, pic in pp["files"]]
    fit = J.Fit(pp["fit"][0], size=pp["fit"][1], fill=rd["fill"]) if pp["fit"] else None
    fmt = J.TensorFormat(rd["tensor"], *OP.FORMATS[rd["tensor"]]) if rd["tensor"] else None
    warp = J.WarpOptions(rd["warp"]["filter"], rd["warp"]["fill"]) if rd["warp"] else None
    flips = rd["flips"][0] if rd["flips"] else None
    warps = rd["warp"]["warps"][0] if rd["warp"] else None
    out = p.decode(files, windows=pp["windows"], output_size=rd["size"], fit=fit, filter=rd["filter"], tensor=fmt, flips=flips, rgb=rd["rgb"], warp=warp, warps=warps)
    for i, data in enumerate(files):
        if isinstance(out[i], Exception):
            report("pipeline", i, repr(out[i]))
            continue
        src, eff, _g = RZ._p_source(data, None, None, pp["windows"][i])
        pl = None
        if fit is not None:
            pl = J.fit_placement(fit, (eff[2], eff[3]), rd["size"])
            if p.placement(i) != pl:
                report("pipeline", i, f"placement {p.placement(i)} for {pl}")
        want = finished(rd, resized_u8(rd, src, pl), bool(flips[i]) if flips else False, warps[i] if warps else None)
        got = T.bits(out[i]).reshape(-1) if rd["tensor"] else out[i]
        if got.size != want.size or not np.array_equal(got, want):
            report("pipeline", i, f"{got.size} / {want.size} elements, first differing {np.nonzero(got != want)[0][:10].tolist() if got.size == want.size else '-'}")
    return len(files), p.kernel_path


def run(seed, rounds, verbose=True, replay=None):
    """-> (bad, total, paths): mismatching comparisons, comparisons made (output_fuzz_plan.image_count of the plan), path strings seen."""
    FT.J = RZ.J = PW.J = J
    plan = [OP.check_round(replay)] if replay is not None else OP.plan(seed, rounds)
    bad = total = 0
    paths = {}
    p = None
    last_files = None
    try:
        for r, rd in enumerate(plan):
            found = []

            def report(leg, image, what):
                found.append((leg, image))
                if verbose:
                    print("MISMATCH seed", seed, "round", r, leg, "image", image, what, flush=True)

            made, path = batch_leg(rd, report)
            total += made
            paths[path] = paths.get(path, 0) + 1
            if rd["pipeline"] is not None:
                if p is None:
                    p = J.Pipeline(threads=4)
                made, path = pipeline_leg(p, rd, report)
                total += made
                paths["pipeline " + path] = paths.get("pipeline " + path, 0) + 1
                last_files = [PW._file(layout, enc, tuple(sz), pic=pic) for layout, enc, sz, pic in rd["pipeline"]["files"]]
            bad += len(found)
            if found and verbose:
                print("replay with: python tools/fuzz_gpu_output.py --replay", repr(repr(rd)), flush=True)
        if p is not None:  # every option switched off again: what the pipeline always gave
            out = p.decode(last_files)
            for i, data in enumerate(last_files):
                full = PW._want(data, None, None)[0]
                if isinstance(out[i], Exception) or not np.array_equal(out[i], full):
                    bad += 1
                    if verbose:
                        print("MISMATCH seed", seed, "after the last round: the pipeline without options, image", i, flush=True)
    finally:
        if p is not None:
            p.close()
    if verbose:
        print("seed", seed, "rounds", len(plan), "comparisons", total, "paths", paths, "bad", bad, flush=True)
    return bad, total, paths


if __name__ == "__main__":
    if sys.argv[1] == "--replay":
        sys.exit(1 if run(0, 1, replay=ast.literal_eval(sys.argv[2]))[0] else 0)
    sys.exit(1 if run(int(sys.argv[1]), int(sys.argv[2]))[0] else 0)
