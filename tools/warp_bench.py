"""The warp stage on the BASELINE workload (1920x1080 4:2:0 q85): what it adds to a loader's call.

Pixel stage (coefficients resident in HBM -> tensors in HBM, 256 resident images, a quarter window of each to 224 x 224 f32), all in one
run, interleaved call by call, each figure the median over --reps calls of jpgpu_batch_time (--iters decodes between two events):
    off          — the tensor batch without a warp
    nearest15    — rule N, every image rotated by 15 degrees
    bilinear15   — rule B, the same matrices
    translate    — rule N-sep, a fractional translation
beside the window kernel alone (the same windows without an output size: the resample launch's own time is `off` minus it) and a plain
device-to-device copy of the warp's source bytes (256 x 224 x 224 x 3: the floor of a stage that reads and writes them once).

    python tools/warp_bench.py --out profiles/warp/warp_bench.json --commit <sha>

--e2e: from JPEG bytes to HBM through Pipeline.decode(windows=, output_size=, tensor=[, warp=, warps=]), 256 files, off and on, one
pipeline per configuration, interleaved call by call, median of --reps warm calls.

    python tools/warp_bench.py --e2e --out profiles/warp/warp_e2e.json --commit <sha>"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import jpeg_decoder_amd as J  # noqa: E402
import resize_bench as RB  # noqa: E402
import synth  # noqa: E402
import tensor_ref as T  # noqa: E402
import warp_ref as WR  # noqa: E402
import window_bench as WB  # noqa: E402

W, H, N = WB.W, WB.H, WB.N
SIZE = (224, 224)
RB.SOURCES = RB.SOURCES + ("warp_band.hpp", "warp.hip")
FMT = J.TensorFormat("float32", T.IMAGENET[0], T.IMAGENET[1])
WARPS = {"nearest15": ("nearest", WR.rotate_matrix(15, SIZE)), "bilinear15": ("bilinear", WR.rotate_matrix(15, SIZE)),
         "translate": ("nearest", (1.0, 0.0, 3.3, 0.0, 1.0, -2.7))}


def quarter(k):
    """A quarter of the image (half of each side) at a position of its own."""
    return ((k * 37) % (W // 2 + 1), (k * 23) % (H // 2 + 1), W // 2, H // 2)


def copy_ms(hip, nbytes, iters):
    """A device-to-device copy of nbytes between two events, per copy."""
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    a, b, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(a), nbytes) == 0 and hip.hipMalloc(C.byref(b), nbytes) == 0
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    assert hip.hipMemcpyAsync(b, a, nbytes, 3, None) == 0
    assert hip.hipEventRecord(e0, None) == 0
    for _ in range(iters):
        assert hip.hipMemcpyAsync(b, a, nbytes, 3, None) == 0
    assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
    ms = C.c_float(0)
    assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    for ptr in (a, b):
        hip.hipFree(ptr)
    return ms.value / iters


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
    for name in ["off"] + list(WARPS):
        filt, m = WARPS.get(name, (None, None))
        b = J.Batch([desc] * N, flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wins, output_size=SIZE, tensor=FMT,
                    warp=None if filt is None else J.WarpOptions(filt, (124, 116, 104)))
        ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(ptr), b.out_arena_bytes()) == 0
        arenas.append(ptr)
        b.bind(full.coef_arena(), ptr.value)
        if filt is not None:
            b.set_warps([m] * N)
        configs[name] = b
    full.decode()
    full.synchronize()
    for b in configs.values():
        b.decode()
        b.synchronize()
    off = configs["off"]
    table = T.table(("float32", FMT.mean, FMT.std), 3)
    inv = {float(v): k for k, v in enumerate(table[0])}
    for name, (filt, m) in WARPS.items():  # correctness spot check: the warp of the unwarped batch's own pixels (channel 0, through the table)
        for i in (0, N - 1):
            u8 = np.vectorize(inv.get)(off.download(i)[0]).astype(np.uint8)[:, :, None]
            want = WR.warp(u8, m, WR.BILINEAR if filt == "bilinear" else WR.NEAREST, (124,))
            assert np.array_equal(configs[name].download(i)[0], table[0][want[:, :, 0]]), (name, i)
    times = {n: [] for n in configs}
    win_times = []
    for _ in range(args.reps):
        win_times.append(full.time(args.iters))
        for name, b in configs.items():
            times[name].append(b.time(args.iters))
    med = {n: float(np.median(t)) for n, t in times.items()}
    window_ms = float(np.median(win_times))
    src_bytes = N * SIZE[0] * SIZE[1] * 3
    copies = [copy_ms(hip, src_bytes, 50) for _ in range(args.reps)]
    rows = [{"config": name, "path": b.path, "ms_median": round(med[name], 4), "ms_all": [round(t, 4) for t in times[name]],
             "added_ms": round(med[name] - med["off"], 4)} for name, b in configs.items()]
    doc = RB.header("tools/warp_bench.py", args)
    doc.update({"workload": f"{W}x{H} 4:2:0 q85 x {N} resident images, a quarter window of each to 224x224 f32 (coefficients in HBM -> tensors in HBM)",
                "iters_per_rep": args.iters, "window_kernel_alone_ms": round(window_ms, 4), "resample_launch_ms": round(med["off"] - window_ms, 4),
                "device_copy_of_the_source_bytes_ms": round(float(np.median(copies)), 4), "source_bytes": src_bytes, "pixel_stage": rows})
    RB.emit(doc, args)
    for b in configs.values():
        b.close()
    full.close()
    for ptr in arenas:
        hip.hipFree(ptr)


def e2e(args):
    J.process_init()
    assert J.device_count() >= 1, "needs an MI355X"
    distinct, who = WB.e2e_files()
    n = 256
    files = [distinct[k % len(distinct)] for k in range(n)]
    wins = [quarter(k) for k in range(n)]
    doc = RB.header("tools/warp_bench.py --e2e", args)
    doc.update({"files": who, "workload": f"{W}x{H} 4:2:0 q85 files ({len(distinct)} distinct), a quarter window of each to 224x224 f32, through Pipeline.decode to HBM",
                "e2e": []})
    configs = {"off": (None, None), **WARPS}
    pipes = {name: J.Pipeline() for name in configs}
    try:
        ts = {name: [] for name in configs}
        for call in range(args.cold + args.reps):
            for name, (filt, m) in configs.items():
                p = pipes[name]
                kw = {} if filt is None else {"warp": J.WarpOptions(filt, (124, 116, 104)), "warps": [m] * n}
                p.decode(files, download=False, windows=wins, output_size=SIZE, tensor=FMT, flips=[k % 2 == 0 for k in range(n)], **kw)
                t = p.timings()
                assert t["images_ok"] == n and t["images_resized"] == n, (name, t)
                if call >= args.cold:
                    ts[name].append(t)
        base = sorted(ts["off"], key=lambda t: t["total_ms"])
        for name in configs:
            order = sorted(ts[name], key=lambda t: t["total_ms"])
            m = order[(len(order) - 1) // 2]
            doc["e2e"].append({"images": n, "config": name, "path": pipes[name].kernel_path, "total_ms": round(m["total_ms"], 3),
                               "all_ms": [round(t["total_ms"], 3) for t in ts[name]], "images_per_s": round(n / m["total_ms"] * 1e3, 1),
                               "vs_off": round(m["total_ms"] / base[(len(base) - 1) // 2]["total_ms"], 4)})
    finally:
        for p in pipes.values():
            p.close()
    RB.emit(doc, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default=os.environ.get("WARP_BENCH_COMMIT", "unknown"))
    ap.add_argument("--e2e", action="store_true", help="the whole call from JPEG bytes through Pipeline.decode(..., warp=, warps=)")
    ap.add_argument("--cold", type=int, default=2, help="--e2e: uncounted calls per configuration")
    args = ap.parse_args()
    return e2e(args) if args.e2e else pixel_stage(args)


if __name__ == "__main__":
    main()
