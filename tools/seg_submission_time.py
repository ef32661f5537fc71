#!/usr/bin/env python3
"""Seconds to write the ScanNet segmentation submission files of one batch into a directory (default: a temporary directory under
/dev/shm, so that the disk is not what is measured).  Workload: bench.py's four scenes' point counts (188 780, 188 092, 186 892 and
182 692 points) with 50 synthetic picked proposals of 2 000 points per scene -- 12 scene files and 200 mask files, about 77 MB.
  host path    d3net_amd.seg_eval.write_predictions: every array copied to the host, np.savetxt per file.
  device path  d3net_amd.seg_submission.SegmentationSubmission.add_batch: the text made by csrc/seg_submission.hip, read back into
               pinned buffers, slices written to the files.  Its split into device work + read-back and file writing is reported too.
Wall clock around each call, the inputs on the device at the start of both paths, the clock stopped after the last file is closed;
the two trees are written and compared equal first (that round is the warm-up), then the two paths alternate: the median of the timed rounds (default
5).  Nothing asserts on the times.  Run under `timeout`; prints one JSON line.  usage: seg_submission_time.py [rounds [picks]]"""
import json
import os
import pathlib
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3net_amd import seg_eval as SE   # noqa: E402
from d3net_amd import seg_submission as SS   # noqa: E402

POINTS = (188780, 188092, 186892, 182692)      # len(scene["locs"]) of the four scenes of bench.py's default configuration (make_scenes)


def batch(dev, picks=50, members=2000, seed=11):
    rng = np.random.default_rng(seed)
    bo = np.concatenate([[0], np.cumsum(POINTS)]).astype(np.int64)
    N = int(bo[-1])
    lists = [bo[b] + rng.choice(POINTS[b], members, replace=False) for b in range(len(POINTS)) for _ in range(picks)]
    idx = np.stack([np.repeat(np.arange(len(lists)), members), np.concatenate(lists)], 1).astype(np.int32)
    off = (np.arange(len(lists) + 1) * members).astype(np.int32)
    pick = rng.permutation(len(lists))
    pred = dict(pick=torch.from_numpy(pick), scores=torch.from_numpy(rng.random(len(pick)).astype(np.float32)),
                proposals_idx=torch.from_numpy(idx), proposals_offset=torch.from_numpy(off), semantic_pred=torch.from_numpy(rng.integers(0, 20, N)))
    pred = {k: v.to(dev) for k, v in pred.items()}
    return pred, dict(batch_offsets=torch.from_numpy(bo.astype(np.int32)).to(dev)), ["scene%04d_00" % b for b in range(len(POINTS))]


def tree(root):
    root = pathlib.Path(root)
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def main(rounds=5, picks=50, warm=0, base=None):
    dev = torch.device("cuda", 0)
    pred, data, names = batch(dev, picks)
    base = base or ("/dev/shm" if os.path.isdir("/dev/shm") else None)
    root = tempfile.mkdtemp(prefix="seg_submission_time_", dir=base)
    try:
        dirs = {k: os.path.join(root, k) for k in ("host", "device")}

        def host_path():
            SE.write_predictions(pred, data, dirs["host"], names)

        def device_path():
            split = {}
            SS.SegmentationSubmission(dirs["device"], device=dev, timings=split).add_batch(pred, data, names)
            return split
        host_path(); device_path()
        a, b = tree(dirs["host"]), tree(dirs["device"])
        equal = sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
        files, size = len(b), sum(len(v) for v in b.values())
        del a, b
        times, split = {"host": [], "device": []}, {"device_s": [], "files_s": []}
        for rnd in range(rounds + warm):
            for name, fn in (("host", host_path), ("device", device_path)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                extra = fn()
                if rnd >= warm:
                    times[name].append(time.perf_counter() - t0)
                    if extra:
                        for k in split:
                            split[k].append(extra[k])
    finally:
        shutil.rmtree(root)
    stat = lambda s: {"median": float(np.median(s)), "min": float(min(s)), "max": float(max(s))}
    print(json.dumps({"scenes": len(POINTS), "points": int(sum(POINTS)), "picks_per_scene": picks, "files": files, "bytes": size,
                      "directory": os.path.dirname(root), "rounds": rounds, "host_path_s": stat(times["host"]), "device_path_s": stat(times["device"]),
                      "device_work_readback_s": stat(split["device_s"]), "device_file_writing_s": stat(split["files_s"]),
                      "speedup_median": float(np.median(times["host"]) / np.median(times["device"])), "trees_equal": bool(equal)}))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
