#!/usr/bin/env python3
"""Host and device time of the optimizer step (no profiler), one line per optimizer: the single-launch classes of d3net_amd.optim
beside torch.optim.X(fused=True), over the detector's ~300 parameter tensors with the gradients of one real step.
host: wall time of `step()` alone (launches queued, not waited for).  device: N steps queued behind a few large matmuls that keep
the GPU busy while the host enqueues them, timed between two events -- the kernels' time with no host gap in it.
usage: python tools/opt_host.py"""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3net_amd import pointgroup as PG, synthetic as S
from d3net_amd.config import default_conf
from d3net_amd.optim import FusedAdam, FusedAdamW, FusedSGD
dev = torch.device("cuda", 0)
cfg = default_conf(); torch.manual_seed(123)
model = PG.PointGroup(cfg).to(dev).train(); model.teacher = True
params = [p for p in model.parameters() if p.requires_grad]
occ, sem, inst, _ = S.occupancy_grid((100, 75, 50), 4, (8, 30), (8, 25), 0)
batch = S.make_batch([S.scene_from_grid(occ, sem, inst)], dev)
model.zero_grad(set_to_none=True)
loss, _ = model.training_step(dict(batch)); loss.backward(); torch.cuda.synchronize()
live = [p for p in params if p.grad is not None]
print("%d tensors with a gradient, %.2f M elements" % (len(live), sum(p.numel() for p in live) / 1e6))
N = 20
blocker = torch.randn(8192, 8192, device=dev)
rows = (("FusedAdamW", lambda: FusedAdamW(params, lr=2e-5)), ("torch AdamW fused", lambda: torch.optim.AdamW(params, lr=2e-5, fused=True)),
        ("FusedAdam", lambda: FusedAdam(params, lr=2e-5)), ("torch Adam fused", lambda: torch.optim.Adam(params, lr=2e-5, fused=True)),
        ("FusedSGD", lambda: FusedSGD(params, lr=2e-5, momentum=0.9)), ("torch SGD fused", lambda: torch.optim.SGD(params, lr=2e-5, momentum=0.9, fused=True)))
for name, make in rows:
    opt = make()
    for _ in range(4):
        opt.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(N):
        opt.step()
    host = (time.perf_counter() - t0) / N
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(6):
        blocker @ blocker
    e0.record()
    for _ in range(N):
        opt.step()
    e1.record()
    drained = torch.cuda.current_stream().query()         # True: the queue drained while the host was still enqueueing
    torch.cuda.synchronize()
    print("%-18s host %7.1f us  device %7.1f us per step%s" % (name, host * 1e6, e0.elapsed_time(e1) * 1e3 / N,
                                                              "  (device figure includes host gaps)" if drained else ""))
