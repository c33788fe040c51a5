"""A fixed output size against the windowed decode a caller does today, on the BASELINE workload (1920x1080 4:2:0 q85).

Pixel stage (coefficients resident in HBM -> pixels in HBM, 256 resident images): the window kernel alone against window + resample
(csrc/resample_band.hpp) on the same coefficient arena, for the centred quarter window and for RandomResizedCrop windows (8-100 % of
the area, aspect 3/4 .. 4/3), each to 224 x 224; and the whole image against whole image + resample.  The configurations are
interleaved call by call, each figure is the median over --reps calls of jpgpu_batch_time (--iters decodes between two events).

    python tools/resize_bench.py --out profiles/resize/resize_bench.json --commit <sha>

--e2e: the whole call from JPEG bytes (Pipeline.decode(windows=..., output_size=...)), 256 and 4,096 files, pixels left in HBM and
copied to pinned host memory: the windowed call without an output size (what a caller does today: the crops come back at their own
sizes) against the same windows with output_size=(224, 224), IN THE SAME RUN, one pipeline per configuration, interleaved call by
call, median of --reps warm calls.  The to-host ratio is the headline: only 150 kB per image cross the link.

    python tools/resize_bench.py --e2e --out profiles/resize/resize_e2e.json --commit <sha>

Both documents carry the hashes of the sources they ran and the box's GPU_MAX_HW_QUEUES."""
import argparse
import ctypes as C
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import jpeg_decoder_amd as J  # noqa: E402
import resample_ref as R  # noqa: E402
import synth  # noqa: E402
import window_bench as WB  # noqa: E402

W, H, N = WB.W, WB.H, WB.N
SIZE = (224, 224)
SOURCES = ("resample_band.hpp", "resample.hip", "window_band.hpp", "window.hip", "batch.cpp", "batch_internal.hpp", "batch_layout.hpp", "batch_entropy.cpp", "pipeline.cpp")


def header(tool, args):
    return {"tool": tool, "commit": args.commit, "sources_sha256": WB.sources_sha256(SOURCES), "library": os.path.basename(J._native.LIB_PATH),
            "host": socket.gethostname(), "device": WB.device_identity(), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
            "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "output_size": list(SIZE), "reps": args.reps,
            "env": {k: os.environ[k] for k in sorted(os.environ) if k.startswith("JPGPU_")}}


def emit(doc, args):
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


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
    rng = np.random.default_rng(2024)
    wins = {"whole_image": None, "w25": [WB.centred(0.25)] * N, "random_crop": WB.random_crops(rng, N)}
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    configs, arenas = {}, []
    for name, wl in wins.items():  # (every batch reads the full batch's coefficient arena: same layout)
        for size in (None, SIZE):
            if name == "whole_image" and size is None:
                configs[name] = (full, wl, size)
                continue
            b = J.Batch([desc] * N, flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wl, output_size=size)
            ptr = C.c_void_p()
            assert hip.hipMalloc(C.byref(ptr), b.out_arena_bytes()) == 0
            arenas.append(ptr)
            b.bind(full.coef_arena(), ptr.value)
            configs[name + ("+resize" if size else "")] = (b, wl, size)
    # correctness spot check: three images of every configuration against the full decode sliced (and resampled by the numpy statement)
    full.decode()
    full.synchronize()
    ref = full.download(0).reshape(H, W, 3)
    for name, (b, wl, size) in configs.items():
        b.decode()
        b.synchronize()
        for i in (0, N // 2, N - 1):
            x, y, w, h = wl[i] if wl else (0, 0, W, H)
            want = ref[y:y + h, x:x + w]
            want = R.resize(want, *size) if size else want
            assert np.array_equal(b.download(i), want.reshape(-1)), (name, i)
    times = {n: [] for n in configs}
    for _ in range(args.reps):
        for name, (b, _w, _s) in configs.items():
            times[name].append(b.time(args.iters))
    med = {n: float(np.median(t)) for n, t in times.items()}
    rows = []
    for name, (b, wl, size) in configs.items():
        area = 1.0 if wl is None else sum(w * h for (_x, _y, w, h) in wl) / (N * W * H)
        base = med[name.replace("+resize", "")]
        rows.append({"config": name, "path": b.path, "area_fraction": round(area, 4), "ms_median": round(med[name], 4),
                     "ms_all": [round(t, 4) for t in times[name]], "vs_without_resize": round(med[name] / base, 4),
                     "resample_ms": round(med[name] - base, 4) if size else 0.0, "out_arena_bytes": b.out_arena_bytes()})
    doc = header("tools/resize_bench.py", args)
    doc.update({"workload": f"{W}x{H} 4:2:0 q85 x {N} resident images (pixel stage: coefficients in HBM -> pixels in HBM)", "iters_per_rep": args.iters,
                "pixel_stage": rows})
    emit(doc, args)
    for name, (b, _w, _s) in configs.items():
        b.close()
    for ptr in arenas:
        hip.hipFree(ptr)


def e2e(args):
    J.process_init()
    assert J.device_count() >= 1, "needs an MI355X"
    distinct, who = WB.e2e_files()
    cu = WB.centred(0.25)
    doc = header("tools/resize_bench.py --e2e", args)
    doc.update({"files": who, "workload": f"{W}x{H} 4:2:0 q85 files ({len(distinct)} distinct) through Pipeline.decode, device entropy decoding", "e2e": []})
    rate = WB.d2h_rate_gbps()
    doc["d2h_gbps"] = None if rate is None else round(rate, 2)
    ref = None
    for n in [int(v) for v in args.e2e_images.split(",")]:
        files = [distinct[k % len(distinct)] for k in range(n)]
        # name -> (windows of call c, output size, the configuration it is compared with)
        configs = {
            "w25": (lambda call: [cu] * n, None, None),
            "w25+resize": (lambda call: [cu] * n, SIZE, "w25"),
            "random_crop_fresh": (lambda call: WB.random_crops(np.random.default_rng(1000 + call), n), None, None),
            "random_crop_fresh+resize": (lambda call: WB.random_crops(np.random.default_rng(1000 + call), n), SIZE, "random_crop_fresh"),
        }
        if args.only:
            keep = args.only.split(",")
            configs = {k: v for k, v in configs.items() if k.replace("+resize", "") in keep}
        pipes = {name: J.Pipeline() for name in configs}
        try:
            for dest, download in (("hbm", False), ("host", "pinned")):
                ts = {name: [] for name in configs}
                for call in range(args.cold + args.reps):
                    for name, (make, size, _vs) in configs.items():
                        wins = make(call)
                        p = pipes[name]
                        p.decode(files, windows=wins, download=download, output_size=size)
                        t = p.timings()
                        assert t["images_ok"] == n and t["images_device_rejected"] == 0 and t["images_resized"] == (n if size else 0), (name, t)
                        if call == 0 and dest == "host":  # spot check: the resized bytes against the windowed bytes of the same run, resampled
                            for i in (0, n - 1):
                                x, y, w, h = wins[i]
                                if size is None:
                                    if ref is None and i == 0:
                                        ref = {}
                                    ref[(name, i)] = p.pixels_host(i).reshape(h, w, 3).copy()
                                elif (name.replace("+resize", ""), i) in (ref or {}):
                                    assert np.array_equal(p.pixels_host(i), R.resize(ref[(name.replace("+resize", ""), i)], *size).reshape(-1)), (name, i)
                        if call >= args.cold:
                            ts[name].append(t)
                med = {}
                for name in configs:
                    order = sorted(ts[name], key=lambda t: t["total_ms"])
                    med[name] = order[(len(order) - 1) // 2]  # (lower median: a call that happened, whose other fields go with it)
                for name, (_make, size, vs) in configs.items():
                    m = med[name]
                    row = {"images": n, "pixels_to": dest, "config": name, "total_ms": round(m["total_ms"], 3),
                           "min_ms": round(min(t["total_ms"] for t in ts[name]), 3), "max_ms": round(max(t["total_ms"] for t in ts[name]), 3),
                           "all_ms": [round(t["total_ms"], 3) for t in ts[name]], "images_per_s": round(n / m["total_ms"] * 1e3, 1),
                           "pixel_bytes": int(m["pixel_bytes"]), "entropy_and_upload_ms": round(m["entropy_and_upload_ms"], 3),
                           "drain_ms": round(m["download_ms"], 3), "images_windowed": m["images_windowed"], "images_resized": m["images_resized"]}
                    if vs:
                        row["vs_windowed_call"] = round(m["total_ms"] / med[vs]["total_ms"], 4)
                    if m["dev_times_valid"]:
                        row["device_ms"] = {k: round(m[f"dev_{k}_ms"], 3) for k in ("fill", "sync", "write", "pixel")}
                    if dest == "host" and rate:
                        row["link_floor_ms"] = round(m["pixel_bytes"] / (rate * 1e9) * 1e3, 3)
                    doc["e2e"].append(row)
        finally:
            for p in pipes.values():
                p.close()
    for row in doc["e2e"]:  # the headline: a to-host call against its own to-HBM call
        if row["pixels_to"] == "host":
            hbm = [r for r in doc["e2e"] if r["pixels_to"] == "hbm" and r["images"] == row["images"] and r["config"] == row["config"]]
            if hbm:
                row["vs_own_hbm_call"] = round(row["total_ms"] / hbm[0]["total_ms"], 4)
    emit(doc, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default=os.environ.get("RESIZE_BENCH_COMMIT", "unknown"))
    ap.add_argument("--only", default="", help="--e2e: comma-separated window configurations (w25, random_crop_fresh)")
    ap.add_argument("--e2e", action="store_true", help="the whole call from JPEG bytes through Pipeline.decode(windows=..., output_size=...)")
    ap.add_argument("--e2e-images", default="256,4096")
    ap.add_argument("--cold", type=int, default=2, help="--e2e: uncounted calls per configuration (the first allocates arenas and staging)")
    args = ap.parse_args()
    return e2e(args) if args.e2e else pixel_stage(args)


if __name__ == "__main__":
    main()
