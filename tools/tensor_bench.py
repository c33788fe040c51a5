"""The tensor output against what a caller does today with the resized bytes, on the BASELINE workload (1920x1080 4:2:0 q85 -> 224 x 224).

Pixel stage (coefficients resident in HBM, 256 resident images, centred-quarter and RandomResizedCrop windows, float32 and float16),
two routes IN THE SAME RUN, interleaved call by call, each figure the median over --reps calls of --iters decodes between two events:

  (a) today:  Batch(output_size=) bound to a torch uint8 tensor, then
              x.view(N, 224, 224, 3).permute(0, 3, 1, 2).to(dtype).div(255).sub(mean).div(std), then torch.where(flip, y.flip(-1), y)
  (b) tensor: Batch(output_size=, tensor=) bound to a torch.empty(N, 3, 224, 224, dtype), half of the images flipped

    python tools/tensor_bench.py --out profiles/tensor/tensor_bench.json --commit <sha>

--e2e: the same two routes from JPEG bytes through Pipeline.decode for 256 files, the result left in HBM and brought to pinned host
memory (route (a) copies its float tensor down; route (b) is download="pinned"), wall-clock per call, median of --reps warm calls.

    python tools/tensor_bench.py --e2e --first today  --out profiles/tensor/tensor_e2e_today_first.json --commit <sha>
    python tools/tensor_bench.py --e2e --first tensor --out profiles/tensor/tensor_e2e_tensor_first.json --commit <sha>

(one pipeline per route; the pipeline a process creates first is one to three ms per call faster whatever it decodes, hence both orders)

Both documents carry the hashes of the sources they ran and the box's GPU_MAX_HW_QUEUES."""
import argparse
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
import synth  # noqa: E402
import tensor_ref as T  # noqa: E402
import window_bench as WB  # noqa: E402

W, H, N = WB.W, WB.H, WB.N
SIZE = (224, 224)
MEAN, STD = T.IMAGENET
SOURCES = ("tensor_band.hpp", "resample_band.hpp", "resample.hip", "window_band.hpp", "window.hip", "batch.cpp", "batch_internal.hpp", "batch_layout.hpp",
           "batch_entropy.cpp", "pipeline.cpp")


def header(tool, args):
    import torch
    return {"tool": tool, "commit": args.commit, "sources_sha256": WB.sources_sha256(SOURCES), "library": os.path.basename(J._native.LIB_PATH),
            "host": socket.gethostname(), "device": WB.device_identity(), "date": time.strftime("%Y-%m-%d %H:%M:%S"), "torch": torch.__version__,
            "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "output_size": list(SIZE), "reps": args.reps,
            "mean": list(MEAN[:3]), "std": list(STD[:3]), "env": {k: os.environ[k] for k in sorted(os.environ) if k.startswith("JPGPU_")}}


def emit(doc, args):
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def follow_up(torch, u8, dtype, mean, std, flip):
    """What every loader runs on the resized bytes today."""
    y = u8.view(-1, SIZE[1], SIZE[0], 3).permute(0, 3, 1, 2).to(dtype).div(255).sub(mean).div(std)
    return torch.where(flip, y.flip(-1), y)


def check_against_reference(torch, x, u8, dtype_name, flips, images):
    """Route (b)'s tensor against the numpy statement applied to route (a)'s bytes."""
    tab = T.table((dtype_name, MEAN, STD), 3)
    it = torch.int16 if dtype_name != "float32" else torch.int32
    for i in images:
        want = T.bits(T.to_tensor(u8[i].cpu().numpy().reshape(SIZE[1], SIZE[0], 3), tab, flips[i]))
        got = x[i].cpu().view(it).numpy().view(want.dtype)
        assert np.array_equal(got, want), (dtype_name, i)


def pixel_stage(args):
    import torch
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
    wins = {"w25": [WB.centred(0.25)] * N, "random_crop": WB.random_crops(rng, N)}
    flips = [i % 2 == 1 for i in range(N)]
    flip_t = torch.tensor(flips, device="cuda").view(N, 1, 1, 1)
    configs = {}
    for wname, wl in wins.items():  # (every batch reads the full batch's coefficient arena: same layout)
        a = J.Batch([desc] * N, flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wl, output_size=SIZE)
        u8 = torch.empty(a.out_arena_bytes(), dtype=torch.uint8, device="cuda")
        assert u8.numel() == N * SIZE[0] * SIZE[1] * 3
        a.bind(full.coef_arena(), u8.data_ptr())
        for dname in ("float32", "float16"):
            dtype = getattr(torch, dname)
            mean = torch.tensor(MEAN[:3], dtype=dtype, device="cuda").view(1, 3, 1, 1)
            std = torch.tensor(STD[:3], dtype=dtype, device="cuda").view(1, 3, 1, 1)
            b = J.Batch([desc] * N, flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wl, output_size=SIZE, tensor=J.TensorFormat(dname, MEAN, STD))
            x = torch.empty(N, 3, SIZE[1], SIZE[0], dtype=dtype, device="cuda")
            assert b.out_arena_bytes() == x.numel() * x.element_size()
            b.bind(full.coef_arena(), x.data_ptr())
            b.set_flips(flips)
            configs[f"{wname}/{dname}"] = (a, u8, b, x, dtype, mean, std, dname)

    def run(name, route, iters):
        a, u8, b, x, dtype, mean, std, _d = configs[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            if route == "today":
                a.decode()
                y = follow_up(torch, u8, dtype, mean, std, flip_t)
            else:
                b.decode()
                y = x
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters, y

    for name, (a, u8, b, x, _dt, _m, _s, dname) in configs.items():  # warm-up and a spot check
        run(name, "today", 2)
        run(name, "tensor", 2)
        check_against_reference(torch, x, u8.view(N, -1), dname, flips, (0, 1, N // 2, N - 1))
    times = {(n, r): [] for n in configs for r in ("today", "tensor")}
    for _ in range(args.reps):
        for name in configs:
            for route in ("today", "tensor"):
                times[(name, route)].append(run(name, route, args.iters)[0])
    rows = []
    for name, (a, _u8, b, x, *_r) in configs.items():
        ta, tb = float(np.median(times[(name, "today")])), float(np.median(times[(name, "tensor")]))
        rows.append({"config": name, "today_ms": round(ta, 4), "tensor_ms": round(tb, 4), "tensor_vs_today": round(tb / ta, 4),
                     "today_ms_all": [round(t, 4) for t in times[(name, "today")]], "tensor_ms_all": [round(t, 4) for t in times[(name, "tensor")]],
                     "today_path": a.path, "tensor_path": b.path, "tensor_bytes": x.numel() * x.element_size()})
    doc = header("tools/tensor_bench.py", args)
    doc.update({"workload": f"{W}x{H} 4:2:0 q85 x {N} resident images (pixel stage: coefficients in HBM -> the model's input tensor in HBM)",
                "iters_per_rep": args.iters, "flipped_images": sum(flips), "pixel_stage": rows})
    emit(doc, args)
    for a, _u8, b, *_r in configs.values():
        b.close()
    for a in {id(c[0]): c[0] for c in configs.values()}.values():
        a.close()
    full.close()


class _DevicePtr:
    """n bytes of device memory at `ptr` for torch.as_tensor (the pipeline's arenas stay the pipeline's)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def e2e(args):
    import torch
    J.process_init()
    assert J.device_count() >= 1, "needs an MI355X"
    distinct, who = WB.e2e_files()
    n = args.e2e_images
    files = [distinct[k % len(distinct)] for k in range(n)]
    doc = header("tools/tensor_bench.py --e2e", args)
    doc.update({"files": who, "workload": f"{W}x{H} 4:2:0 q85 files ({len(distinct)} distinct) x {n} through Pipeline.decode, device entropy decoding", "e2e": []})
    rate = WB.d2h_rate_gbps()
    doc["d2h_gbps"] = None if rate is None else round(rate, 2)
    one = SIZE[0] * SIZE[1] * 3
    # (the pipeline a process creates first runs its calls one to three ms faster than a later one, whatever it decodes; so the
    # comparison is run in both creation orders: --first)
    order = ("today", "tensor") if args.first == "today" else ("tensor", "today")
    pipes = {name: J.Pipeline() for name in order}
    pipes = {name: pipes[name] for name in ("today", "tensor")}
    doc["pipeline_created_first"] = args.first
    try:
        for dname in ("float32", "float16"):
            dtype = getattr(torch, dname)
            mean = torch.tensor(MEAN[:3], dtype=dtype, device="cuda").view(1, 3, 1, 1)
            std = torch.tensor(STD[:3], dtype=dtype, device="cuda").view(1, 3, 1, 1)
            fmt = J.TensorFormat(dname, MEAN, STD)
            host = torch.empty(n, 3, SIZE[1], SIZE[0], dtype=dtype).pin_memory()
            for wname in ("w25", "random_crop_fresh"):
                for dest in ("hbm", "host"):
                    ts = {"today": [], "tensor": []}
                    for call in range(args.cold + args.reps):
                        rng = np.random.default_rng(1000 + call)
                        wins = [WB.centred(0.25)] * n if wname == "w25" else WB.random_crops(rng, n)
                        flips = [bool(v) for v in rng.integers(0, 2, n)]
                        flip_t = torch.tensor(flips).view(n, 1, 1, 1)
                        for route, p in pipes.items():
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            if route == "today":
                                p.decode(files, windows=wins, download=False, output_size=SIZE)
                                ptrs = [p.device_pointer(i) for i in range(n)]
                                parts, i = [], 0
                                while i < n:  # (consecutive images of a sub-batch are one tensor)
                                    k = i + 1
                                    while k < n and ptrs[k] == ptrs[k - 1] + one:
                                        k += 1
                                    u8 = torch.as_tensor(_DevicePtr(ptrs[i], (k - i) * one), device="cuda")
                                    parts.append(follow_up(torch, u8, dtype, mean, std, flip_t[i:k].cuda(non_blocking=True)))
                                    i = k
                                y = torch.cat(parts)
                                if dest == "host":
                                    host.copy_(y, non_blocking=True)
                                torch.cuda.synchronize()
                            else:
                                p.decode(files, windows=wins, flips=flips, download="pinned" if dest == "host" else False, output_size=SIZE, tensor=fmt)
                            dt = (time.perf_counter() - t0) * 1e3
                            t = p.timings()
                            assert t["images_ok"] == t["images_resized"] == n and t["images_device_rejected"] == 0, (route, t)
                            if call >= args.cold:
                                ts[route].append(dt)
                            if call == 0 and dest == "host" and route == "today":  # (the resized bytes of this call, for the spot check below)
                                seen = {i: torch.as_tensor(_DevicePtr(ptrs[i], one), device="cuda").cpu().numpy().reshape(SIZE[1], SIZE[0], 3).copy() for i in (0, n - 1)}
                            if call == 0 and dest == "host" and route == "tensor":  # spot check: the numpy statement applied to the other route's bytes
                                for i in (0, n - 1):
                                    want = T.bits(T.to_tensor(seen[i], T.table((dname, MEAN, STD), 3), flips[i]))
                                    assert np.array_equal(T.bits(p.pixels_host(i)), want), (dname, wname, i)
                    ma, mb = float(np.median(ts["today"])), float(np.median(ts["tensor"]))
                    row = {"images": n, "dtype": dname, "windows": wname, "result_in": dest, "today_ms": round(ma, 3), "tensor_ms": round(mb, 3),
                           "tensor_vs_today": round(mb / ma, 4), "today_ms_all": [round(v, 3) for v in ts["today"]], "tensor_ms_all": [round(v, 3) for v in ts["tensor"]],
                           "tensor_bytes": n * one * fmt.itemsize}
                    if dest == "host" and rate:
                        row["link_floor_ms"] = round(n * one * fmt.itemsize / (rate * 1e9) * 1e3, 3)
                    doc["e2e"].append(row)
    finally:
        for p in pipes.values():
            p.close()
    emit(doc, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default=os.environ.get("TENSOR_BENCH_COMMIT", "unknown"))
    ap.add_argument("--e2e", action="store_true", help="the whole call from JPEG bytes through Pipeline.decode")
    ap.add_argument("--e2e-images", type=int, default=256)
    ap.add_argument("--first", default="today", choices=["today", "tensor"], help="--e2e: the route whose pipeline is created first")
    ap.add_argument("--cold", type=int, default=2, help="--e2e: uncounted calls per configuration (the first allocates arenas and staging)")
    args = ap.parse_args()
    return e2e(args) if args.e2e else pixel_stage(args)


if __name__ == "__main__":
    main()
