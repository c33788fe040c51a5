"""Where the fixed part of bench.py's timed window comes from (profiles/warp/README.md): bench.py run in this process, from the directory
it lies in, with Python's cyclic collector switched off or watched.

    python tools/bench_collector_probe.py off 0 --gpus 1 --steps 200 --warmup 20 --no-e2e ...
    python tools/bench_collector_probe.py log <pad> --gpus 1 ...

`log` prints, at exit, on stderr: the perf_counter times of every torch event record (the first and the last bracket the timed window),
of every torch.cuda.synchronize, gc.get_count() behind each, and every collection from 5 ms before the window on (generation, start,
duration, collected).  pad > 0: that many container objects kept alive before bench.py starts; pad < 0: -pad of them allocated at the
first synchronize of the timed region, i.e. behind the last collection before the window — this moves the collector's counter at the
window by exactly -pad."""
import atexit
import gc
import runpy
import sys
import time

mode = sys.argv[1]
pad_n = int(sys.argv[2])
sys.argv = ["bench.py"] + sys.argv[3:]
log = []
if mode == "off":
    gc.disable()
else:
    state = {}

    def cb(phase, info):
        if phase == "start":
            state["t"] = time.perf_counter()
        else:
            log.append(("gc", info["generation"], state["t"], time.perf_counter() - state["t"], info["collected"]))
    gc.callbacks.append(cb)
    import torch
    orig = torch.cuda.Event.record

    def record(self, *a, **k):
        t = time.perf_counter()
        r = orig(self, *a, **k)
        log.append(("record", t, time.perf_counter() - t, gc.get_count()))
        return r
    torch.cuda.Event.record = record
    osync = torch.cuda.synchronize

    kept = []

    def sync(*a, **k):
        if not kept and pad_n < 0:  # (the first synchronise of the timed region: -pad_n allocations kept alive, behind the last collection before the window)
            kept.append([[] for _ in range(-pad_n)])
        t = time.perf_counter()
        r = osync(*a, **k)
        log.append(("sync", t, time.perf_counter() - t, gc.get_count()))
        return r
    torch.cuda.synchronize = sync

    def dump():
        recs = [e for e in log if e[0] == "record"]
        if len(recs) >= 2:
            t0, t1 = recs[0][1], recs[-1][1]
            print("GCLOG window %.3f ms; records:" % ((t1 - t0) * 1e3), [(round((e[1] - t0) * 1e3, 3), round(e[2] * 1e3, 3), e[3]) for e in recs], file=sys.stderr)
            print("GCLOG syncs:", [(round((e[1] - t0) * 1e3, 3), round(e[2] * 1e3, 3), e[3]) for e in log if e[0] == "sync"], file=sys.stderr)
            print("GCLOG collections from 5 ms before the window on:", [(e[1], round((e[2] - t0) * 1e3, 3), round(e[3] * 1e3, 3), e[4]) for e in log if e[0] == "gc" and e[2] > t0 - 5e-3],
                  file=sys.stderr)
    atexit.register(dump)
pad = [[] for _ in range(pad_n)]  # (kept alive: shifts the collector's phase by pad_n allocations)
runpy.run_path("bench.py", run_name="__main__")
