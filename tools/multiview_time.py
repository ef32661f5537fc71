#!/usr/bin/env python3
"""Milliseconds per scene of d3net_amd.multiview.project_multiview_features at ScanNet size (200 k points x 300 frames of
32 x 41 depth / 128-channel ENet maps), both fusion modes, timed with HIP events on the current stream.  The span includes the
host's float32 torch.inverse of the poses and its upload; points, depths and features start on the device.  The synthetic
room (points on walls and boxes, inward-looking cameras, z-buffered depth) is built on the host before timing.  Run under
`timeout`; prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3net_amd import multiview as MV             # noqa: E402

INTR, W, H = MV.INTRINSICS, 41, 32


def room(seed, n, F, ext=(7.0, 6.0, 2.8)):
    r = np.random.RandomState(seed)
    ext = np.asarray(ext)
    q = r.uniform(0, 1, (n, 3)) * ext
    axis = r.randint(0, 3, n)
    q[np.arange(n), axis] = np.where(r.rand(n) < 0.5, 0.0, ext[axis])
    poses = []
    for _ in range(F):
        eye, tgt = r.uniform(0.2, 0.8, 3) * ext, r.uniform(0.1, 0.9, 3) * ext
        z = (tgt - eye) / np.linalg.norm(tgt - eye)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, eye
        poses.append(m)
    depths = []
    for m in poses:
        w = np.linalg.inv(m)
        cam = q @ w[:3, :3].T + w[:3, 3]
        cam = cam[cam[:, 2] > 1e-3]
        u = np.rint(cam[:, 0] * INTR[0][0] / cam[:, 2] + INTR[0][2]).astype(np.int64)
        v = np.rint(cam[:, 1] * INTR[1][1] / cam[:, 2] + INTR[1][2]).astype(np.int64)
        ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
        zb = np.full(H * W, np.inf)
        np.minimum.at(zb, v[ok] * W + u[ok], cam[ok, 2])
        zb[~np.isfinite(zb)] = 0
        depths.append(zb.reshape(H, W))
    return q.astype(np.float32), np.stack(depths).astype(np.float32), np.stack(poses).astype(np.float32)


def main(n=200_000, F=300, reps=5):
    dev = torch.device("cuda", 0)
    pts, dep, poses = room(0, n, F)
    g = torch.Generator(device=dev).manual_seed(0)
    feats = torch.randn((F, 128, H, W), device=dev, generator=g).clamp_(min=0)     # ENet maps are post-ReLU
    pts_d, dep_d = torch.from_numpy(pts).to(dev), torch.from_numpy(dep).to(dev)
    res = {"points": n, "frames": F}
    for maxpool in (True, False):
        out, counts = MV.project_multiview_features(pts_d, dep_d, poses, feats, maxpool=maxpool, return_counts=True)   # warm-up
        torch.cuda.synchronize()
        res["mapped_per_frame"] = float(counts.float().mean())
        res["covered_points"] = float((out != 0).any(1).float().mean())
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            MV.project_multiview_features(pts_d, dep_d, poses, feats, maxpool=maxpool)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        res["%s_ms_per_scene" % ("maxpool" if maxpool else "first")] = {"median": float(np.median(ms)), "min": float(min(ms)),
                                                                         "max": float(max(ms))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
