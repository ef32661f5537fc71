#!/usr/bin/env python3
"""Seconds to write n box-wireframe PLY files (default 2048 random boxes, both modes) into a directory (default: a temporary
directory under /dev/shm, so that the disk is not what is measured):
  device path  d3net_amd.visualize.write_box_plys: per chunk one d3_box_wire_text launch and one read-back, then header + the box's
               bytes + the face block per file.  Its split into launch + read-back and file writing is reported too.
  host path    tests/visualize_restate.py's box_ply per box (vectorised numpy geometry, Python's "{:f}" per coordinate) and the
               same file writes.  The reference's own write_bbox builds every vertex in a Python loop and is slower still.
Wall clock, the boxes in host memory at the start of both paths, the two paths alternating, one warm-up round and the median of
three timed rounds each.  Also whether the two paths' files are equal.  Nothing asserts on the times.  Run under `timeout`;
prints one JSON line."""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from d3net_amd import visualize as V   # noqa: E402
import visualize_restate as VR   # noqa: E402


def boxes(n, seed=5):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-5, 5, (n, 3))
    hi = lo + rng.uniform(0.05, 3, (n, 3))
    sgn = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], bool)
    return np.where(sgn[None], hi[:, None], lo[:, None]).astype(np.float32), rng.integers(0, 2, n).astype(np.int32)


def device_path(corners, modes, paths, dev):
    split = {}
    V.write_box_plys(corners, modes, paths, device=dev, timings=split)
    return split


def host_path(corners, modes, paths, dev):
    for c, m, p in zip(corners, modes.tolist(), paths):
        with open(p, "wb") as f:
            f.write(VR.box_ply(c, m))
    return None


def main(n=2048, rounds=3, warm=1, base=None):
    dev = torch.device("cuda", 0)
    corners, modes = boxes(n)
    base = base or ("/dev/shm" if os.path.isdir("/dev/shm") else None)
    root = tempfile.mkdtemp(prefix="visualize_time_", dir=base)
    try:
        dirs = {k: os.path.join(root, k) for k in ("host", "device")}
        for d in dirs.values():
            os.makedirs(d)
        paths = {k: [os.path.join(d, "%05d.ply" % i) for i in range(n)] for k, d in dirs.items()}
        times, split = {"host": [], "device": []}, {"device_s": [], "files_s": []}
        for rnd in range(rounds + warm):
            for name, fn in (("host", host_path), ("device", device_path)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                extra = fn(corners, modes, paths[name], dev)
                if rnd >= warm:
                    times[name].append(time.perf_counter() - t0)
                    if extra:
                        for k in split:
                            split[k].append(extra[k])
        equal = all(open(a, "rb").read() == open(b, "rb").read() for a, b in zip(paths["host"], paths["device"]))
        size = sum(os.path.getsize(p) for p in paths["device"])
    finally:
        shutil.rmtree(root)
    stat = lambda s: {"median": float(np.median(s)), "min": float(min(s)), "max": float(max(s))}
    print(json.dumps({"boxes": n, "bytes": size, "directory": os.path.dirname(root), "rounds": rounds, "host_path_s": stat(times["host"]),
                      "device_path_s": stat(times["device"]), "device_launch_readback_s": stat(split["device_s"]),
                      "device_file_writing_s": stat(split["files_s"]), "speedup_median": float(np.median(times["host"]) / np.median(times["device"])),
                      "host_ms_per_box": 1e3 * float(np.median(times["host"])) / n, "device_ms_per_box": 1e3 * float(np.median(times["device"])) / n,
                      "files_equal": bool(equal)}))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
