"""Windowed decodes against whole-image decodes on the BASELINE workload (1920x1080 4:2:0 q85, 256 resident images).

The pixel stage (coefficients resident in HBM -> pixels in HBM) of the window kernel (csrc/window_band.hpp) next to the
full-image fused kernel on the same coefficients (the batch the bench's K measures, classes handed over by the host):
  - centred windows of about 99 / 50 / 25 / 8 % of the area, x, y, w, h multiples of 16 (every window row 4-byte aligned); the 99 %
    window is one MCU column short of the image (a whole-image window takes the full-image route);
  - w25_unaligned: the centred quarter with odd x, y, w, h (window rows at every alignment, partial units at both edges);
  - w25_varied / w25_varied_aligned: a window of a quarter of the area per image, position and aspect (3/4 .. 4/3) drawn per
    image, with odd / multiple-of-16 coordinates (images of one launch with different tile grids);
  - random_crop: RandomResizedCrop-style windows (8-100 % of the area, aspect 3/4 .. 4/3) per image.  Every configuration
shares one coefficient arena; the configurations are interleaved call by call, each figure is the median over --reps calls of
jpgpu_batch_time (--iters decodes between two events).  One JSON document on stdout (and in --out).

    python tools/window_bench.py --out profiles/window/window_bench.json --commit <sha>

--e2e: the whole call from JPEG bytes (Pipeline.decode(windows=...)), 256 and 4,096 files of the same workload, pixels left in HBM
and copied to pinned host memory, for: no windows (what a caller does today: the whole decode, then a slice on the host; once more
with JPGPU_PIPE_ENTRY_PIXELS=0, the expansion route that windowed 4:2:0 images take); the centred
quarter on a 16-pixel grid; the same at odd coordinates; RandomResizedCrop windows (8-100 % of the area, aspect 3/4 .. 4/3) drawn
anew for every call, and one such draw repeated.  One pipeline per configuration (a pipeline keeps its sub-batches from call to
call), the configurations interleaved call by call, median of --reps warm calls, the device work by phase from
JPGPU_BATCH_KERNEL_TIMES.  Every windowed figure is compared with the whole decode of the same files in the same run.

    JPGPU_BATCH_KERNEL_TIMES=1 python tools/window_bench.py --e2e --out profiles/window/window_e2e.json --commit <sha>
"""
import argparse
import ctypes as C
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import jpeg_decoder_amd as J  # noqa: E402
import synth  # noqa: E402

W, H, N = 1920, 1080, 256


def centred(frac):
    s = frac ** 0.5
    w, h = max(16, int(round(W * s)) & ~15), max(16, int(round(H * s)) & ~15)
    return ((W - w) // 2 & ~15, (H - h) // 2 & ~15, w, h)


def random_crops(rng, n):
    out = []
    for _ in range(n):
        for _try in range(10):
            area = W * H * rng.uniform(0.08, 1.0)
            ar = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
            w, h = int(round((area * ar) ** 0.5)), int(round((area / ar) ** 0.5))
            if 0 < w <= W and 0 < h <= H:
                break
        else:
            w, h = W, H
        out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return out


def varied(rng, n, frac, aligned):
    out = []
    for _ in range(n):
        ar = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
        w, h = int(round((W * H * frac * ar) ** 0.5)), int(round((W * H * frac / ar) ** 0.5))
        w, h = (w & ~15, h & ~15) if aligned else (w | 1, h | 1)
        x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        if aligned:
            x, y = x & ~15, y & ~15
        else:
            x, y = min(x | 1, W - w), min(y | 1, H - h)
        out.append((x, y, w, h))
    return out


def sources_sha256(files=("window_band.hpp", "window.hip", "batch.cpp", "batch_internal.hpp", "batch_layout.hpp")):
    """sha256 over the window kernel's sources as they were built (ties the figures to a tree)."""
    import hashlib
    hsh = hashlib.sha256()
    for f in files:
        with open(os.path.join(ROOT, "jpeg-decoder_amd", "csrc", f), "rb") as fh:
            hsh.update(fh.read())
    return hsh.hexdigest()[:16]


def device_identity():
    hip = C.CDLL("libamdhip64.so")
    bus = C.create_string_buffer(64)
    uuid = C.create_string_buffer(16)
    out = {}
    if hip.hipDeviceGetPCIBusId(bus, 64, 0) == 0:
        out["pci_bus_id"] = bus.value.decode()
    if hip.hipDeviceGetUuid(uuid, 0) == 0:
        out["uuid"] = uuid.raw.hex()
    return out


def e2e_files(distinct=4):
    """The bench's E workload: `distinct` baseline 4:2:0 q85 files of the synthetic image (seeds 0x5EED + k), written by Pillow where
    it is installed (as tools/bench_e2e.py does), else by tools/baseline_encoder.py."""
    rgbs = [synth.synthetic_rgb(W, H, seed=0x5EED + k) for k in range(distinct)]
    try:
        import io
        import PIL
        from PIL import Image
        out = []
        for rgb in rgbs:
            buf = io.BytesIO()
            Image.fromarray(rgb).save(buf, format="JPEG", quality=85, subsampling="4:2:0")
            out.append(buf.getvalue())
        return out, f"Pillow {PIL.__version__}, quality 85, 4:2:0"
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import baseline_encoder as E
        return [E.encode_rgb(rgb, 85, "420") for rgb in rgbs], "tools/baseline_encoder.py, quality 85, 4:2:0"


def d2h_rate_gbps(nbytes=1 << 30):
    """One pinned 1-GB device-to-host copy, best of 3, in this run: the link floor of a call that hands its pixels to the host."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipHostFree.argtypes = [C.c_void_p]
    d, h = C.c_void_p(), C.c_void_p()
    if hip.hipMalloc(C.byref(d), nbytes) != 0 or hip.hipHostMalloc(C.byref(h), nbytes, 0) != 0:
        return None
    best = None
    for _ in range(4):
        t0 = time.perf_counter()
        assert hip.hipMemcpy(h, d, nbytes, 2) == 0
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    hip.hipFree(d)
    hip.hipHostFree(h)
    return nbytes / best / 1e9


def knob_ab(args, files, n, cu):
    """Two knobs the library reads per call, each A/B in one process, interleaved call by call, pixels left in HBM:
    JPGPU_PIPE_WINDOW_ROWS (the expansion limited to the MCU rows a window reads) on the centred quarter, by dev_fill_ms + dev_write_ms;
    JPGPU_PIPE_REWINDOW (fresh windows set in place in the kept sub-batches, against new sub-batches) on fresh random crops, by total_ms."""
    out = []
    for knob, key, make in (("JPGPU_PIPE_WINDOW_ROWS", "fill+write", lambda call: [cu] * n),
                            ("JPGPU_PIPE_WINDOW_ROWS", "fill+write", lambda call: random_crops(np.random.default_rng(77), n)),
                            ("JPGPU_PIPE_REWINDOW", "total", lambda call: random_crops(np.random.default_rng(5000 + call), n))):
        p = J.Pipeline()
        got = {"1": [], "0": []}
        try:
            for call in range(args.cold + args.reps):
                for v in ("1", "0"):
                    os.environ[knob] = v
                    p.decode(files, windows=make(2 * call + (v == "0")), download=False)
                    t = p.timings()
                    assert t["images_ok"] == n and t["images_windowed"] > 0
                    if call >= args.cold:
                        got[v].append((t["dev_fill_ms"] + t["dev_write_ms"]) if key == "fill+write" else t["total_ms"])
        finally:
            os.environ.pop(knob, None)
            p.close()
        row = {"knob": knob, "images": n, "figure": "dev_fill_ms + dev_write_ms" if key == "fill+write" else "total_ms",
               "windows": "centred quarter" if make(0)[0] == cu else "random crops", "on_ms": round(float(np.median(got["1"])), 4),
               "off_ms": round(float(np.median(got["0"])), 4), "on_all": [round(v, 4) for v in got["1"]], "off_all": [round(v, 4) for v in got["0"]]}
        row["on_vs_off"] = round(row["on_ms"] / row["off_ms"], 4) if row["off_ms"] else None
        out.append(row)
    return out


def e2e(args):
    J.process_init()
    assert J.device_count() >= 1, "needs an MI355X"
    distinct, who = e2e_files()
    ref = None
    cu = centred(0.25)
    doc = {"tool": "tools/window_bench.py --e2e", "commit": args.commit,
           "sources_sha256": sources_sha256(("window_band.hpp", "window.hip", "batch.cpp", "batch_internal.hpp", "batch_layout.hpp", "batch_entropy.cpp", "pipeline.cpp", "huff.hip", "huff_job.hpp")),
           "library": os.path.basename(J._native.LIB_PATH), "host": socket.gethostname(), "device": device_identity(),
           "date": time.strftime("%Y-%m-%d %H:%M:%S"), "files": who,
           "workload": f"{W}x{H} 4:2:0 q85 files ({len(distinct)} distinct) through Pipeline.decode, device entropy decoding",
           "reps": args.reps, "env": {k: os.environ[k] for k in sorted(os.environ) if k.startswith("JPGPU_")},
           "d2h_gbps": None, "e2e": []}
    rate = d2h_rate_gbps()
    doc["d2h_gbps"] = None if rate is None else round(rate, 2)
    for n in [int(v) for v in args.e2e_images.split(",")]:
        files = [distinct[k % len(distinct)] for k in range(n)]
        fixed = random_crops(np.random.default_rng(77), n)
        configs = {
            "whole_image": lambda call: None,
            "whole_image_expanded": lambda call: None,  # JPGPU_PIPE_ENTRY_PIXELS=0: the route windowed 4:2:0 images take in front of their pixel kernel
            "w25": lambda call: [cu] * n,
            "w25_unaligned": lambda call: [(cu[0] + 1, cu[1] + 1, cu[2] - 1, cu[3] - 1)] * n,
            "random_crop_fresh": lambda call: random_crops(np.random.default_rng(1000 + call), n),
            "random_crop_repeated": lambda call: fixed,
        }
        if n > 1024:  # (six pipelines of 4,096 1080p images do not fit the device's memory side by side)
            configs.pop("whole_image_expanded")
        if args.only:
            configs = {k: v for k, v in configs.items() if k == "whole_image" or k in args.only.split(",")}
        pipes = {name: J.Pipeline() for name in configs}
        try:
            for dest, download in (("hbm", False), ("host", "pinned")):
                ts = {name: [] for name in configs}
                for call in range(args.cold + args.reps):
                    for name, make in configs.items():
                        wins = make(call)
                        p = pipes[name]
                        if name == "whole_image_expanded":
                            os.environ["JPGPU_PIPE_ENTRY_PIXELS"] = "0"
                        t0 = time.perf_counter()
                        p.decode(files, windows=wins, download=download)
                        wall = (time.perf_counter() - t0) * 1e3
                        os.environ.pop("JPGPU_PIPE_ENTRY_PIXELS", None)
                        t = p.timings()
                        assert t["images_ok"] == n and t["images_device_rejected"] == 0, (name, t)
                        if call == 0 and dest == "host":  # spot check against the whole decode of the same run, sliced
                            if ref is None:
                                ref = pipes["whole_image"].pixels_host(0).reshape(H, W, 3).copy() if name == "whole_image" else None
                            if ref is not None and wins is not None:
                                for i in (0, len(distinct), n - len(distinct)):
                                    x, y, w, h = wins[i]
                                    assert np.array_equal(p.pixels_host(i), ref[y:y + h, x:x + w].reshape(-1)), (name, i)
                        if call >= args.cold:
                            t["python_wall_ms"] = wall
                            ts[name].append(t)
                base = None
                for name in configs:
                    order = sorted(ts[name], key=lambda t: t["total_ms"])
                    med = order[(len(order) - 1) // 2]  # (lower median: a call that happened, whose other fields go with it)
                    if name == "whole_image":
                        base = med["total_ms"]
                    row = {"images": n, "pixels_to": dest, "config": name, "total_ms": round(med["total_ms"], 3), "min_ms": round(order[0]["total_ms"], 3),
                           "max_ms": round(order[-1]["total_ms"], 3), "all_ms": [round(t["total_ms"], 3) for t in ts[name]],
                           "python_wall_ms": round(float(np.median([t["python_wall_ms"] for t in ts[name]])), 3),
                           "vs_whole_image": round(med["total_ms"] / base, 4), "images_per_s": round(n / med["total_ms"] * 1e3, 1),
                           "pixel_bytes": int(med["pixel_bytes"]), "area_fraction": round(med["pixel_bytes"] / (n * W * H * 3), 4),
                           "headers_ms": round(med["headers_ms"], 3), "setup_ms": round(med["setup_ms"], 3),
                           "entropy_and_upload_ms": round(med["entropy_and_upload_ms"], 3), "drain_ms": round(med["download_ms"], 3), "images_windowed": med["images_windowed"], "images_entry_pixels": med["images_entry_pixels"]}
                    if med["dev_times_valid"]:
                        row["device_ms"] = {k: round(med[f"dev_{k}_ms"], 3) for k in ("fill", "sync", "write", "pixel")}
                    if dest == "host" and rate:
                        row["link_floor_ms"] = round(med["pixel_bytes"] / (rate * 1e9) * 1e3, 3)
                        row["frac_of_link_floor"] = round(row["link_floor_ms"] / med["total_ms"], 4)
                    doc["e2e"].append(row)
        finally:
            for p in pipes.values():
                p.close()
        if n == 256 and not args.no_ab:
            doc.setdefault("ab", []).extend(knob_ab(args, files, n, cu))
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default=os.environ.get("WINDOW_BENCH_COMMIT", "unknown"))
    ap.add_argument("--variant", default="", help="label of the build measured (e.g. the JPGPU_LIBRARY it runs)")
    ap.add_argument("--only", default="", help="comma-separated windowed configurations (the full-image batch always runs)")
    ap.add_argument("--e2e", action="store_true", help="the whole call from JPEG bytes through Pipeline.decode(windows=...)")
    ap.add_argument("--e2e-images", default="256,4096")
    ap.add_argument("--no-ab", action="store_true", help="--e2e: leave out the A/B of JPGPU_PIPE_WINDOW_ROWS and JPGPU_PIPE_REWINDOW")
    ap.add_argument("--cold", type=int, default=2, help="--e2e: uncounted calls per configuration (the first allocates arenas and staging)")
    args = ap.parse_args()
    if args.e2e:
        return e2e(args)
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
    configs = {"full_image_fused": (full, None)}
    mcu_short = (0, 0, W - 16, H)  # one MCU column short of the whole image
    rng = np.random.default_rng(2024)
    wins = {"w99": [mcu_short] * N, "w50": [centred(0.50)] * N, "w25": [centred(0.25)] * N, "w08": [centred(0.08)] * N,
            "random_crop": random_crops(rng, N)}
    cu = centred(0.25)
    wins["w25_unaligned"] = [(cu[0] + 1, cu[1] + 1, cu[2] - 1, cu[3] - 1)] * N
    wins["w25_varied"] = varied(rng, N, 0.25, aligned=False)
    wins["w25_varied_aligned"] = varied(rng, N, 0.25, aligned=True)
    if args.only:
        keep = args.only.split(",")
        wins = {k: v for k, v in wins.items() if k in keep}
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    out_arenas = []
    for name, wl in wins.items():  # (the windowed batches read the full batch's coefficient arena: same layout)
        b = J.Batch([desc] * N, flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wl)
        ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(ptr), b.out_arena_bytes()) == 0
        out_arenas.append(ptr)
        b.bind(full.coef_arena(), ptr.value)
        configs[name] = (b, sum(w * h for (_x, _y, w, h) in wl) / (N * W * H))
    assert all(b.path == "window" for n, (b, _a) in configs.items() if n != "full_image_fused")
    # correctness spot check: four images of every windowed configuration against the full decode sliced
    full.decode()
    full.synchronize()
    ref = full.download(0).reshape(H, W, 3)
    for name, (b, _a) in configs.items():
        if name == "full_image_fused":
            continue
        b.decode()
        b.synchronize()
        for i in (0, 1, N // 2, N - 1):
            x, y, w, h = wins[name][i]
            assert np.array_equal(b.download(i), ref[y:y + h, x:x + w].reshape(-1)), (name, i)
    times = {n: [] for n in configs}
    for _ in range(args.reps):
        for name, (b, _a) in configs.items():
            times[name].append(b.time(args.iters))
    med = {n: float(np.median(t)) for n, t in times.items()}
    base = med["full_image_fused"]
    rows = []
    for name, (b, area) in configs.items():
        rows.append({"config": name, "path": b.path, "area_fraction": 1.0 if area is None else round(area, 4), "ms_median": round(med[name], 4),
                     "ms_all": [round(t, 4) for t in times[name]], "vs_full_image": round(med[name] / base, 4)})
    doc = {"tool": "tools/window_bench.py", "commit": args.commit, "sources_sha256": sources_sha256(), "variant": args.variant,
           "library": os.path.basename(J._native.LIB_PATH), "host": socket.gethostname(), "device": device_identity(),
           "date": time.strftime("%Y-%m-%d %H:%M:%S"),
           "workload": f"{W}x{H} 4:2:0 q85 x {N} resident images (pixel stage: coefficients in HBM -> pixels in HBM)",
           "reps": args.reps, "iters_per_rep": args.iters, "pixel_stage": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for name, (b, _a) in configs.items():
        b.close()
    for ptr in out_arenas:
        hip.hipFree(ptr)


if __name__ == "__main__":
    main()
