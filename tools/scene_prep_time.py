#!/usr/bin/env python3
"""Milliseconds per 4-scene batch of d3net_amd.scene_prep.prepare_batch at ScanNet size (150 k - 280 k points, detector
config: augmentation, two elastic distortions, crop of the scenes over max_num_point), in both noise modes.  Timed with HIP
events on the preparing stream; the span includes the host's control-flow synchronisations (grid sizes, crop iterations, output
shapes) and, in host mode, the numpy draws of the noise grids and their upload.  Inputs start on the device.  Run under
`timeout`; prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3net_amd import scene_prep as SP            # noqa: E402
from d3net_amd.config import default_conf         # noqa: E402


def scene(seed, n, extent=(9.0, 7.0, 2.8), n_inst=40):
    r = np.random.RandomState(seed)
    pts = (r.rand(n, 3) * np.array(extent)).astype(np.float32)
    centers = r.rand(n_inst, 3) * np.array(extent)
    d = np.linalg.norm(pts[:, None, :] - centers[None], axis=2)
    ids = np.where(d.min(1) < 0.8, d.argmin(1), -1).astype(np.int32)
    return dict(points=pts, feats=(r.rand(n, 3) * 2 - 1).astype(np.float32), sem_labels=r.randint(-1, 20, n).astype(np.int32),
                instance_ids=ids)


def main(reps=5):
    dev = torch.device("cuda", 0)
    cfg = default_conf()
    msa = np.abs(np.random.RandomState(0).randn(18, 3)) + 0.5
    scenes = [{k: torch.from_numpy(v).to(dev) for k, v in scene(s, n).items()}
              for s, n in ((1, 150_000), (2, 200_000), (3, 260_000), (4, 280_000))]
    res = {"scenes": 4, "points": [int(s["points"].shape[0]) for s in scenes]}
    for mode in ("device", "host"):
        rng = np.random.RandomState(0)
        SP.prepare_batch(scenes, cfg, msa, rng=rng, noise=mode, device=dev)          # warm-up (allocator, code objects)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            SP.prepare_batch(scenes, cfg, msa, rng=rng, noise=mode, device=dev)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        res["%s_noise_ms_per_batch" % mode] = {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
