#!/usr/bin/env python3
"""Milliseconds per validation batch of caption_eval.assign_dense_caption at the workload's shape (8 scenes, K = 128 proposals,
G = 128 GT slots, 10..60 valid GT boxes per scene, boxes from d3net_amd.synthetic.occupancy_grid): the host path
(device_assign=False: batched GIoU launches, cost matrix to the host, scipy per scene) against the device path
(device_assign=True: csrc/assign.hip), same GPU inputs, alternating, wall clock between two torch.cuda.synchronize() calls (the
host path's cost is a synchronisation that events do not see).  Also the kernel alone (HIP events around back-to-back launches) with
all 128 GT slots valid, its worst case, and the assignment step by itself (boxes -> per_gt on the device) in both forms.
Warm-up first, median of the repeats.  Nothing asserts on the times.  Run under `timeout`; prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3net_amd import _lib, caption_eval as ce, synthetic   # noqa: E402

B, K, G, L, V = 8, 128, 128, 31, 60
SGN = np.array([[1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1], [1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1]], np.float32)


def scene_boxes(n, seed):
    """n GT boxes of a synthetic room and K proposals: jittered copies of them plus random boxes, shuffled"""
    rng = np.random.default_rng(seed)
    boxes = np.array(synthetic.occupancy_grid(n_boxes=n, seed=seed)[3], np.float32) * synthetic.VOXEL
    gs = boxes[:, 3:6]
    gc = boxes[:, 0:3] + gs / 2
    m = min(n, K)
    pc = np.concatenate([gc[:m] + rng.normal(0, 0.1, (m, 3)), rng.random((K - m, 3)) * np.array([4, 3, 2])]).astype(np.float32)
    ps = np.concatenate([gs[:m] * rng.uniform(0.7, 1.3, (m, 3)), rng.random((K - m, 3)) * 0.9 + 0.3]).astype(np.float32)
    perm = rng.permutation(K)
    gt = np.zeros((G, 8, 3), np.float32)
    gt[:n] = gc[:, None] + SGN[None] * gs[:, None] / 2
    return (pc[:, None] + SGN[None] * ps[:, None] / 2)[perm], gt


def batch(nactual, dev, seed=0):
    rng = np.random.default_rng(seed)
    pg = [scene_boxes(int(n), seed + b) for b, n in enumerate(nactual)]
    words = ["pad_", "unk", "sos", "eos"] + ["w%d" % i for i in range(V - 4)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    masks = (np.arange(G)[None] < np.asarray(nactual)[:, None]).astype(np.float32)
    return dict(caps=t(rng.integers(3, V, (B, K, L)).astype(np.int64)), pred=t(np.stack([p for p, _ in pg])), gt=t(np.stack([g for _, g in pg])),
                ids=t(np.stack([rng.permutation(300)[:G] for _ in range(B)]).astype(np.int64)), masks=t(masks),
                scenes=["scene%04d_00" % b for b in range(B)], idx2word={str(i): w for i, w in enumerate(words)},
                special={"bos_token": "sos", "eos_token": "eos", "unk_token": "unk", "pad_token": "pad_"})


def run(d, device_assign):
    return ce.assign_dense_caption(d["caps"], d["pred"], d["gt"], d["ids"], d["masks"], d["scenes"], d["idx2word"], d["special"],
                                   device_assign=device_assign)


def host_assign(d, nactual):
    """the assignment step of the host path by itself, as assign_dense_caption(device_assign=False) runs it"""
    from scipy.optimize import linear_sum_assignment
    cost = (-ce.generalized_box3d_iou(d["pred"], d["gt"], nactual)).detach().cpu().numpy()
    per_gt = torch.zeros((B, G), dtype=torch.int64)
    for b in range(B):
        n = int(nactual[b])
        if n > 0:
            rows, cols = linear_sum_assignment(cost[b, :, :n])
            per_gt[b, torch.from_numpy(cols)] = torch.from_numpy(rows)
    return per_gt.to(d["pred"].device)


def main(reps=30, warm=5, chain=20):
    dev = torch.device("cuda", 0)
    nactual = np.random.default_rng(0).integers(10, 61, B)
    d = batch(nactual, dev)
    host_ms, dev_ms = [], []
    same = True
    for rep in range(reps + warm):
        out = []
        for arm, sink in ((False, host_ms), (True, dev_ms)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out.append(run(d, arm))
            torch.cuda.synchronize()
            if rep >= warm:
                sink.append((time.perf_counter() - t0) * 1e3)
        same = same and out[0] == out[1]
    # the assignment step by itself: boxes -> per_gt on the device
    na_dev = d["masks"].sum(1).long()
    step_host_ms, step_dev_ms = [], []
    for rep in range(reps + warm):
        got = []
        for fn, sink in ((lambda: host_assign(d, na_dev), step_host_ms), (lambda: ce.assign_boxes_device(d["pred"], d["gt"], na_dev), step_dev_ms)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got.append(fn())
            torch.cuda.synchronize()
            if rep >= warm:
                sink.append((time.perf_counter() - t0) * 1e3)
        same = same and torch.equal(got[0], got[1])
    # the kernel alone, all G slots valid
    w = batch([G] * B, dev, seed=100)
    na = torch.full((B,), G, dtype=torch.int32, device=dev)
    per_gt = torch.empty((B, G), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    launch = lambda: _lib.check(_lib.lib().d3_dense_caption_assign(p(w["pred"]), p(w["gt"]), p(na), B, K, G, p(per_gt), p(status), None, stream),
                                "dense_caption_assign")
    kern_ms = []
    for rep in range(reps + warm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(chain):
            launch()
        b.record()
        b.synchronize()
        if rep >= warm:
            kern_ms.append(a.elapsed_time(b) / chain)
    stat = lambda ms: {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}
    print(json.dumps({"scenes": B, "K": K, "G": G, "nactual": [int(n) for n in nactual], "reps": reps, "candidates_equal": bool(same),
                      "host_path_ms_per_batch": stat(host_ms), "device_path_ms_per_batch": stat(dev_ms),
                      "speedup_median": float(np.median(host_ms) / np.median(dev_ms)),
                      "assignment_only_host_ms": stat(step_host_ms), "assignment_only_device_ms": stat(step_dev_ms),
                      "kernel_ms_nactual_128": stat(kern_ms), "kernel_status": status.cpu().tolist()}))


if __name__ == "__main__":
    main()
