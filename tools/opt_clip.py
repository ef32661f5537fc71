"""Cost of gradient clipping on the detector's real parameter set: (a) FusedAdamW.step() with clipping off,
(b) with max_grad_norm set, (c) torch.nn.utils.clip_grad_norm_ followed by (a).  One process, the routes alternating, every step
between two HIP events behind a synchronise; medians after warm-up, the host's enqueue time beside them, and the library calls
of one step of (a) and (b).  Prints one JSON object.
    python tools/opt_clip.py"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from d3net_amd import _lib  # noqa: E402
from d3net_amd.config import default_conf  # noqa: E402
from d3net_amd.optim import FusedAdamW  # noqa: E402
from d3net_amd.pointgroup import PointGroup  # noqa: E402

dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = PointGroup(default_conf()).to(dev)
base = [p for p in model.parameters() if p.requires_grad]
V = 1.0


def clone_set():
    ps = [torch.nn.Parameter(p.detach().clone()) for p in base]
    for p in ps:
        p.grad = torch.randn_like(p) * 0.01
    return ps


pa, pb, pc = clone_set(), clone_set(), clone_set()
kw = dict(lr=1e-5, weight_decay=1e-4)
oa, ob, oc = FusedAdamW(pa, **kw), FusedAdamW(pb, max_grad_norm=V, **kw), FusedAdamW(pc, **kw)


def route_a():
    oa.step()


def route_b():
    ob.step()


def route_c():
    torch.nn.utils.clip_grad_norm_(pc, V)
    oc.step()


routes = {"a_off": route_a, "b_native_clip": route_b, "c_torch_clip_then_a": route_c}
for _ in range(30):
    for f in routes.values():
        f()
torch.cuda.synchronize()

N = 300
ev = {k: [] for k in routes}
host = {k: [] for k in routes}
for _ in range(N):
    for k, f in routes.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(); f(); e1.record()
        host[k].append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
        ev[k].append(e0.elapsed_time(e1) * 1e3)

# library calls per step of (a) and (b)
L = _lib.lib()
calls = []
names = ("d3_grad_sumsq", "d3_grad_clip_finish", "d3_adamw", "d3_adamw_clipped")
orig = {n: getattr(L, n) for n in names}
for n in names:
    setattr(L, n, (lambda n: lambda *a: (calls.append(n), orig[n](*a))[1])(n))
counts = {}
for k in ("a_off", "b_native_clip"):
    del calls[:]
    routes[k]()
    counts[k] = list(calls)
for n in names:
    setattr(L, n, orig[n])
torch.cuda.synchronize()

out = {"tensors": len(base), "elements": sum(p.numel() for p in base), "max_norm": V,
       "norm_b": float(ob.last_grad_norm()), "nonfinite_b": ob.nonfinite_steps(),
       "event_us": {k: {"median": statistics.median(v), "p10": sorted(v)[N // 10], "p90": sorted(v)[9 * N // 10]} for k, v in ev.items()},
       "host_enqueue_us": {k: statistics.median(v) for k, v in host.items()}, "library_calls": counts, "steps": N}
print(json.dumps(out))
