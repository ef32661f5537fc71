"""How Python calls libd3hip.so: the pointer / stream conversions, the device guard, the cached workspace and the checked call.
Every module of the package takes them from here; `pointgroup_ops` re-exports the underscore names for tests and tools."""
import ctypes as C
import threading

import torch

from . import _lib

_ws_cache = {}


# the calling thread's current stream / device straight from the runtime bindings: `torch.cuda.current_stream()` builds a
# Stream object (~5 us) and `torch.cuda.current_device()` walks the lazy-init checks; at ~45 library calls per step inside
# the host-bound stretches of the step (after a count phase the host has no lead over the GPU) that is time the GPU waits for
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_RAW_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    if _RAW_STREAM is not None and _RAW_DEVICE is not None:
        return C.c_void_p(_RAW_STREAM(_RAW_DEVICE()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def workspace(nbytes, device, tag):
    """A cached, growing device scratch buffer per (device, tag, host thread, current stream)."""
    # per host thread AND per stream: the two clustering branches of PointGroup.forward run concurrently on their own streams, from
    # two threads (the helper-thread fallback beyond the padded lists' budget) or from one -- and a call may return with kernels that read its workspace still in flight
    # (d3_bfs_cluster_run's speculative fill), so one thread driving two streams must never hand both the same buffer (r05_f: the
    # 16-scene batch, whose lists go the compact way, faulted exactly so)
    key = (device.index if device.index is not None else torch.cuda.current_device(), tag, threading.get_ident(),
           (stream().value or 0) if device.type == "cuda" else 0)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


class _NoGuard:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NOGUARD = _NoGuard()


def on(device):
    """device guard for the raw library calls: a no-op (sub-microsecond) when `device` is already current --
    `torch.cuda.device(...)` costs ~10 us per use, which at ~600 operator calls per step is host time the GPU waits for"""
    if device.index is None:
        return _NOGUARD
    cur = _RAW_DEVICE() if _RAW_DEVICE is not None else torch.cuda.current_device()
    return _NOGUARD if device.index == cur else torch.cuda.device(device)


def call(name, *args):
    """d3_<name>(*args), its status checked.  The library is looked up through `_lib` at call time.  Use inside `on(device)`
    with `stream()` as the call's stream argument, so the stream is read under the guard."""
    return _lib.check(getattr(_lib.lib(), "d3_" + name)(*args), name)


_stream, _ptr, _on, _workspace = stream, ptr, on, workspace
