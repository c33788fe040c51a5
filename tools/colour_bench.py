"""The colour stage on the BASELINE workload (1920x1080 4:2:0 q85): what it adds to a loader's call.

Pixel stage (coefficients resident in HBM -> tensors in HBM, 256 resident images, a quarter window of each to 224 x 224 f32), all in one
run, interleaved call by call, each figure the median over --reps calls of jpgpu_batch_time (--iters decodes between two events):
    off          — the tensor batch without colour
    empty        — a coloured batch with empty programs: the u8 resample, the colour launch that leaves at once, the finishing launch
    bcs          — brightness + contrast + saturation on every image
    equalize     — equalize alone
    solarize     — solarize alone
    hue          — hue alone (the HSV round trip per pixel, §4.21)
    sharpen      — sharpen alone (strips through LDS, §4.21)
    jitter       — ColorJitter's four: brightness + contrast + saturation + hue
beside the window kernel alone (the same windows without an output size: the resample launch's own time is `off` minus it).

    python tools/colour_bench.py --out profiles/colour/colour_bench.json --commit <sha>

--e2e: from JPEG bytes to HBM through Pipeline.decode(windows=, output_size=, tensor=[, colour=, colours=]), 256 files, off and the program
--program names (bcs), one pipeline per configuration, interleaved call by call, median of --reps warm calls.  --first off|on: which pipeline the process creates
first (the pipeline a process creates first runs its calls faster than a later one whatever it decodes, DESIGN.md §4.11: run both orders,
a process each, and take the mean).

    python tools/colour_bench.py --e2e --first off --out profiles/colour/colour_e2e_off_first.json --commit <sha>
    python tools/colour_bench.py --e2e --first on --out profiles/colour/colour_e2e_on_first.json --commit <sha>"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import colour_pixel_ref as CR  # noqa: E402  (apply: the table operations and the pixel ones)
import jpeg_decoder_amd as J  # noqa: E402
import resize_bench as RB  # noqa: E402
import synth  # noqa: E402
import tensor_ref as T  # noqa: E402
import window_bench as WB  # noqa: E402

W, H, N = WB.W, WB.H, WB.N
SIZE = (224, 224)
RB.SOURCES = RB.SOURCES + ("warp_band.hpp", "warp.hip", "colour_band.hpp", "colour_pixel_band.hpp", "colour.hip")
FMT = J.TensorFormat("float32", T.IMAGENET[0], T.IMAGENET[1])
PROGRAMS = {"empty": None, "bcs": [("brightness", 1.2), ("contrast", 0.8), ("saturation", 1.3)], "equalize": [("equalize", 0)], "solarize": [("solarize", 128)],
            "hue": [("hue", 43)], "sharpen": [("sharpen", 1.9)], "jitter": [("brightness", 1.2), ("contrast", 0.8), ("saturation", 1.3), ("hue", 43)]}


def quarter(k):
    """A quarter of the image (half of each side) at a position of its own."""
    return ((k * 37) % (W // 2 + 1), (k * 23) % (H // 2 + 1), W // 2, H // 2)


def pixel_stage(args):
    assert J.device_count() >= 1, "needs an MI355X"
    comps, _ = J.make_components(W, H, [(2, 2), (1, 1), (1, 1)])
    lum, chroma = synth.quality_tables(85)
    qts = [lum, chroma, chroma]
    coefs = synth.coefficients_from_rgb(synth.synthetic_rgb(W, H), comps, "ycbcr", qts)
    desc = J.image_desc(list(comps), qts, W, H, "YCbCr")
    wins = [quarter(k) for k in range(N)]
    full = J.Batch([desc] * N, windows=wins)  # (the window kernel alone; its coefficient arena serves every batch below)
    for i in range(N):
        for c in range(3):
            full.upload(i, c, coefs[c])
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    configs, arenas = {}, []
    for name in ["off"] + list(PROGRAMS):
        b = J.Batch([desc] * N, flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wins, output_size=SIZE, tensor=FMT, colour=name != "off")
        ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(ptr), b.out_arena_bytes()) == 0
        arenas.append(ptr)
        b.bind(full.coef_arena(), ptr.value)
        if name != "off":
            b.set_colour([PROGRAMS[name]] * N)
        configs[name] = b
    full.decode()
    full.synchronize()
    for b in configs.values():
        b.decode()
        b.synchronize()
    off = configs["off"]
    table = T.table(("float32", FMT.mean, FMT.std), 3)
    inv = [{float(v): k for k, v in enumerate(table[c])} for c in range(3)]
    for name, program in PROGRAMS.items():  # correctness spot check: the programs on the uncoloured batch's own pixels (through the table)
        for i in (0, N - 1):
            t = off.download(i)
            u8 = np.stack([np.vectorize(inv[c].get)(t[c]).astype(np.uint8) for c in range(3)], axis=-1)
            want = CR.apply(u8, program)
            got = configs[name].download(i)
            for c in range(3):
                assert np.array_equal(got[c], table[c][want[:, :, c]]), (name, i, c)
    times = {n: [] for n in configs}
    win_times = []
    for _ in range(args.reps):
        win_times.append(full.time(args.iters))
        for name, b in configs.items():
            times[name].append(b.time(args.iters))
    med = {n: float(np.median(t)) for n, t in times.items()}
    window_ms = float(np.median(win_times))
    rows = [{"config": name, "path": b.path, "ms_median": round(med[name], 4), "ms_all": [round(t, 4) for t in times[name]],
             "added_ms": round(med[name] - med["off"], 4)} for name, b in configs.items()]
    doc = RB.header("tools/colour_bench.py", args)
    doc.update({"workload": f"{W}x{H} 4:2:0 q85 x {N} resident images, a quarter window of each to 224x224 f32 (coefficients in HBM -> tensors in HBM)",
                "iters_per_rep": args.iters, "window_kernel_alone_ms": round(window_ms, 4), "resample_launch_ms": round(med["off"] - window_ms, 4),
                "programs": {k: v for k, v in PROGRAMS.items()}, "pixel_stage": rows})
    RB.emit(doc, args)
    for b in configs.values():
        b.close()
    full.close()
    for ptr in arenas:
        hip.hipFree(ptr)


def e2e_order(args, files, wins, order):
    n = len(files)
    pipes = {name: J.Pipeline() for name in order}
    rows = []
    try:
        ts = {name: [] for name in order}
        for call in range(args.cold + args.reps):
            for name in order:
                p = pipes[name]
                kw = {} if name == "off" else {"colour": True, "colours": [PROGRAMS[name]] * n}
                p.decode(files, download=False, windows=wins, output_size=SIZE, tensor=FMT, flips=[k % 2 == 0 for k in range(n)], **kw)
                t = p.timings()
                assert t["images_ok"] == n and t["images_resized"] == n, (name, t)
                if call >= args.cold:
                    ts[name].append(t)
        for name in order:
            o = sorted(ts[name], key=lambda t: t["total_ms"])
            m = o[(len(o) - 1) // 2]
            rows.append({"images": n, "config": name, "path": pipes[name].kernel_path, "total_ms": round(m["total_ms"], 3),
                         "all_ms": [round(t["total_ms"], 3) for t in ts[name]], "images_per_s": round(n / m["total_ms"] * 1e3, 1)})
    finally:
        for p in pipes.values():
            p.close()
    return rows


def e2e(args):
    J.process_init()
    assert J.device_count() >= 1, "needs an MI355X"
    distinct, who = WB.e2e_files()
    n = 256
    files = [distinct[k % len(distinct)] for k in range(n)]
    wins = [quarter(k) for k in range(n)]
    doc = RB.header("tools/colour_bench.py --e2e", args)
    doc.update({"files": who, "workload": f"{W}x{H} 4:2:0 q85 files ({len(distinct)} distinct), a quarter window of each to 224x224 f32, through Pipeline.decode to HBM",
                "program": PROGRAMS[args.program]})
    doc["created_first"] = args.first
    doc["e2e"] = e2e_order(args, files, wins, ["off", args.program] if args.first == "off" else [args.program, "off"])
    RB.emit(doc, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default=os.environ.get("COLOUR_BENCH_COMMIT", "unknown"))
    ap.add_argument("--e2e", action="store_true", help="the whole call from JPEG bytes through Pipeline.decode(..., colour=, colours=)")
    ap.add_argument("--first", choices=["off", "on"], default="off", help="--e2e: the pipeline created first")
    ap.add_argument("--program", choices=[k for k in PROGRAMS if k != "empty"], default="bcs", help="--e2e: the program on every file")
    ap.add_argument("--cold", type=int, default=2, help="--e2e: uncounted calls per configuration")
    args = ap.parse_args()
    return e2e(args) if args.e2e else pixel_stage(args)


if __name__ == "__main__":
    main()
