"""Calls of one Batch on a caller's stream with the host running ahead (tests/test_gpu_batch_streams.py, the deferred mode of
tests/test_gpu_call_sequences.py::_run_ops).  Three things make the race between a decode still queued and the next host-side call
deterministic:

* ballast: in front of each decode the stream gets a chain of ordinary torch kernels, its length chosen from one unit timed at set-up
  so that the chain runs for BALLAST_MS — far longer than the host needs for the calls that follow;
* precondition: an event recorded directly behind each decode is queried immediately before a mutating call and must be unready (the
  decode really was pending): `expect_pending` fails the test otherwise, it never lets it pass on a race that did not happen;
* snapshot: behind each decode the output arena is copied, device to device on the same stream, into a buffer of its own; the host
  waits once, at the very end, and every snapshot is compared with what the model held at that decode.

The streams are the null stream (the control), a blocking stream and a hipStreamNonBlocking one — what torch's side streams and the
pipeline's compute streams are, and the only kind a blocking copy on the null stream does not order against."""
import ctypes as C
import math

# torch brings its own copy of the HIP runtime, and a process can drive the GPU through one copy only (the second one to initialise finds
# no device).  libjpgpu.so takes the copy that is loaded when it is loaded itself, so torch comes first — as in bench.py — and this
# module is imported at collection time by the test modules that use it, before any test loads the library.
import torch

KINDS = ("null", "blocking", "nonblocking")
BALLAST_MS = 20.0       # per chain; the host-side calls between two decodes of these tests take well under a millisecond
UNIT_ELEMS = 32 << 20   # one unit: x.add_(1.0) over 128 MiB of float32
HIP_STREAM_NON_BLOCKING = 1
HIP_MEMCPY_DEVICE_TO_DEVICE = 3

_HIP = None
_UNIT = {}


def hip():
    """The HIP runtime of this process (the one copy torch and libjpgpu.so share)."""
    global _HIP
    if _HIP is None:
        with open("/proc/self/maps") as f:
            loaded = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
        assert len(loaded) == 1, f"the process holds {len(loaded)} copies of the HIP runtime ({loaded}): libjpgpu.so was loaded before torch"
        h = C.CDLL(loaded[0])
        h.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        h.hipStreamDestroy.argtypes = [C.c_void_p]
        h.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
        h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        _HIP = h
    return _HIP


class StreamHarness:
    def __init__(self, kind):
        assert kind in KINDS, kind
        assert torch.cuda.is_available(), "torch sees no GPU (was libjpgpu.so loaded before torch? see the top of this module)"
        hip()
        self.torch, self.kind, self._own = torch, kind, None
        if kind == "null":
            self.handle, self.ts = None, torch.cuda.default_stream()
            assert self.ts.cuda_stream == 0, "torch's default stream is not the null stream"
        else:
            flags = HIP_STREAM_NON_BLOCKING if kind == "nonblocking" else 0
            s = C.c_void_p()
            assert hip().hipStreamCreateWithFlags(C.byref(s), flags) == 0
            got = C.c_uint(99)
            assert hip().hipStreamGetFlags(s, C.byref(got)) == 0 and got.value == flags, (kind, got.value)
            self._own = s
            self.handle, self.ts = s.value, torch.cuda.ExternalStream(s.value)
        if "x" not in _UNIT:
            _UNIT["x"] = torch.zeros(UNIT_ELEMS, dtype=torch.float32, device="cuda")
        self.x = _UNIT["x"]
        # one unit, timed with events on this very stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self._units(3)
        e0.record(self.ts)
        self._units(10)
        e1.record(self.ts)
        e1.synchronize()
        self.unit_ms = e0.elapsed_time(e1) / 10.0
        assert self.unit_ms > 0.01, f"a ballast unit took {self.unit_ms} ms: too short to build a chain from"
        self.n_units = max(1, math.ceil(BALLAST_MS / self.unit_ms))
        self.checked = 0  # preconditions that held

    def _units(self, n):
        with self.torch.cuda.stream(self.ts):
            for _ in range(n):
                self.x.add_(1.0)

    def ballast(self):
        self._units(self.n_units)

    def buffers(self, n, nbytes):
        """n snapshot buffers of nbytes, allocated (and zeroed) before anything is pending."""
        t = self.torch.zeros((n, max(nbytes, 1)), dtype=self.torch.uint8, device="cuda")
        self.torch.cuda.synchronize()
        return t

    def mark(self):
        ev = self.torch.cuda.Event()
        ev.record(self.ts)
        return ev

    def snapshot(self, dst, src_ptr, nbytes):
        """dst (a row of `buffers`) <- nbytes at device address src_ptr, behind everything enqueued on the stream so far."""
        assert dst.numel() >= nbytes
        assert hip().hipMemcpyAsync(dst.data_ptr(), src_ptr, nbytes, HIP_MEMCPY_DEVICE_TO_DEVICE, self.handle) == 0

    def expect_pending(self, ev, what):
        """The precondition of a mutating call: the decode in front of it has not run yet."""
        assert not ev.query(), (f"ballast too short: the decode had completed before {what} ({self.kind} stream, {self.n_units} units of "
                                f"{self.unit_ms:.3f} ms) — the call raced with nothing")
        self.checked += 1

    def finish(self):
        """The one host synchronisation, at the very end."""
        self.torch.cuda.synchronize()

    def close(self):
        self.torch.cuda.synchronize()
        if self._own is not None:
            hip().hipStreamDestroy(self._own)
            self._own = None
