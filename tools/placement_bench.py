"""Placements against the stretch a caller does today, on the BASELINE workload (1920x1080 4:2:0 q85).

Pixel stage (coefficients resident in HBM -> pixels in HBM, 256 resident images), all in one run, interleaved call by call, each figure
the median over --reps calls of jpgpu_batch_time (--iters decodes between two events):
    (a) the whole image stretched to 224 x 224                   — today's call, resample_band_kernel
    (b) shorter side 256 + centre crop 224 (455 x 256 at (-116, -16)) — the evaluation transform, resample_placed_kernel
    (c) letterbox to 640 x 640 (640 x 360 at (0, 140), fill 114)      — resample_placed_kernel
    (c0) the whole image stretched to 640 x 640                   — the unplaced call of (c)'s output size

    python tools/placement_bench.py --out profiles/placement/placement_bench.json --commit <sha>

--e2e: (a) and (b) from JPEG bytes to HBM through Pipeline.decode(output_size=, fit=), 256 files, with and without scale=(256, 256), one
pipeline per configuration, interleaved call by call, median of --reps warm calls.

    python tools/placement_bench.py --e2e --out profiles/placement/placement_e2e.json --commit <sha>

Both documents carry the hashes of the sources they ran and the box's GPU_MAX_HW_QUEUES."""
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
import placement_ref as P  # noqa: E402
import resize_bench as RB  # noqa: E402
import synth  # noqa: E402
import window_bench as WB  # noqa: E402

W, H, N = WB.W, WB.H, WB.N
RB.SOURCES = RB.SOURCES + ("placed_band.hpp", "placed.hip")
EVAL = J.Fit("shorter_side_crop", size=256)
BOX = J.Fit("letterbox", fill=(114, 114, 114))


def pixel_stage(args):
    assert J.device_count() >= 1, "needs an MI355X"
    comps, _ = J.make_components(W, H, [(2, 2), (1, 1), (1, 1)])
    lum, chroma = synth.quality_tables(85)
    qts = [lum, chroma, chroma]
    coefs = synth.coefficients_from_rgb(synth.synthetic_rgb(W, H), comps, "ycbcr", qts)
    desc = J.image_desc(list(comps), qts, W, H, "YCbCr")
    full = J.Batch([desc] * N)
    for i in range(N):
        for c in range(3):
            full.upload(i, c, coefs[c])
    # name -> (output size, placement, fill)
    specs = {"a_stretch_224": ((224, 224), None, None), "b_shorter256_crop224": ((224, 224), J.fit_placement(EVAL, (W, H), (224, 224)), EVAL.fill),
             "c0_stretch_640": ((640, 640), None, None), "c_letterbox_640": ((640, 640), J.fit_placement(BOX, (W, H), (640, 640)), BOX.fill)}
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    configs, arenas = {}, []
    for name, (size, pl, fill) in specs.items():  # (every batch reads the full batch's coefficient arena: same layout)
        b = J.Batch([desc] * N, flags=J._native.BATCH_EXTERNAL_BUFFERS, output_size=size, placements=None if pl is None else [pl] * N, fill=fill)
        ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(ptr), b.out_arena_bytes()) == 0
        arenas.append(ptr)
        b.bind(full.coef_arena(), ptr.value)
        configs[name] = b
    full.decode()
    full.synchronize()
    ref = full.download(0).reshape(H, W, 3)
    for name, b in configs.items():  # correctness spot check against the numpy statement
        size, pl, fill = specs[name]
        b.decode()
        b.synchronize()
        want = P.place(ref, size[0], size[1], pl, fill or (0, 0, 0, 0)).reshape(-1)
        for i in (0, N - 1):
            assert np.array_equal(b.download(i), want), (name, i)
    times = {n: [] for n in configs}
    for _ in range(args.reps):
        for name, b in configs.items():
            times[name].append(b.time(args.iters))
    med = {n: float(np.median(t)) for n, t in times.items()}
    whole = float(np.median([full.time(args.iters) for _ in range(3)]))
    rows = []
    for name, b in configs.items():
        size, pl, _f = specs[name]
        rows.append({"config": name, "path": b.path, "output_size": list(size), "placement": None if pl is None else list(pl), "ms_median": round(med[name], 4),
                     "ms_all": [round(t, 4) for t in times[name]], "resample_ms": round(med[name] - whole, 4), "vs_a": round(med[name] / med["a_stretch_224"], 4),
                     "out_arena_bytes": b.out_arena_bytes()})
    doc = RB.header("tools/placement_bench.py", args)
    doc.update({"workload": f"{W}x{H} 4:2:0 q85 x {N} resident images (pixel stage: coefficients in HBM -> pixels in HBM)", "iters_per_rep": args.iters,
                "whole_image_without_resample_ms": round(whole, 4), "pixel_stage": rows})
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
    doc = RB.header("tools/placement_bench.py --e2e", args)
    doc.update({"files": who, "workload": f"{W}x{H} 4:2:0 q85 files ({len(distinct)} distinct) through Pipeline.decode to HBM, device entropy decoding", "e2e": []})
    configs = {"a_stretch_224": (None, None), "b_shorter256_crop224": (EVAL, None), "a_stretch_224+scale256": (None, (256, 256)),
               "b_shorter256_crop224+scale256": (EVAL, (256, 256))}
    pipes = {name: J.Pipeline() for name in configs}
    try:
        ts = {name: [] for name in configs}
        for call in range(args.cold + args.reps):
            for name, (fit, scale) in configs.items():
                p = pipes[name]
                p.decode(files, download=False, output_size=(224, 224), fit=fit, scale=scale)
                t = p.timings()
                assert t["images_ok"] == n and t["images_resized"] == n, (name, t)
                if call >= args.cold:
                    ts[name].append(t)
        for name in configs:
            order = sorted(ts[name], key=lambda t: t["total_ms"])
            m = order[(len(order) - 1) // 2]
            base = sorted(ts[name.replace("b_shorter256_crop224", "a_stretch_224")], key=lambda t: t["total_ms"])
            row = {"images": n, "config": name, "path": pipes[name].kernel_path, "total_ms": round(m["total_ms"], 3),
                   "all_ms": [round(t["total_ms"], 3) for t in ts[name]], "images_per_s": round(n / m["total_ms"] * 1e3, 1),
                   "vs_stretch": round(m["total_ms"] / base[(len(base) - 1) // 2]["total_ms"], 4)}
            if m["dev_times_valid"]:
                row["device_ms"] = {k: round(m[f"dev_{k}_ms"], 3) for k in ("fill", "sync", "write", "pixel")}
            doc["e2e"].append(row)
    finally:
        for p in pipes.values():
            p.close()
    RB.emit(doc, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default=os.environ.get("PLACEMENT_BENCH_COMMIT", "unknown"))
    ap.add_argument("--e2e", action="store_true", help="the whole call from JPEG bytes through Pipeline.decode(output_size=, fit=)")
    ap.add_argument("--cold", type=int, default=2, help="--e2e: uncounted calls per configuration")
    args = ap.parse_args()
    return e2e(args) if args.e2e else pixel_stage(args)


if __name__ == "__main__":
    main()
