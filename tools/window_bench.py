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


def sources_sha256():
    """sha256 over the window kernel's sources as they were built (ties the figures to a tree)."""
    import hashlib
    hsh = hashlib.sha256()
    for f in ("window_band.hpp", "window.hip", "batch.cpp"):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default=os.environ.get("WINDOW_BENCH_COMMIT", "unknown"))
    ap.add_argument("--variant", default="", help="label of the build measured (e.g. the JPGPU_LIBRARY it runs)")
    ap.add_argument("--only", default="", help="comma-separated windowed configurations (the full-image batch always runs)")
    args = ap.parse_args()
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
