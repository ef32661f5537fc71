"""Time the construction of one batch's scene half by `scene_prep.prepare_points_store` (the label-free path of the test split)
against `scene_prep.prepare_batch_store` (the labelled path, is_augment=False) on the same resident store and scenes, after DESIGN
§3.17's protocol: the four scenes of bench.py's captioning step (182-189 k points each, 131 feature columns), HIP events around
the call only, 5 warm-up calls then 20 timed ones, the two paths alternating in one process; the median and the spread (min, max,
interquartile range) of each, the same with the shared voxelisation's own median taken out, the one-off extents-table build time,
and whether the seven label-free keys are equal.  Prints one JSON line (and writes it to --out).  Needs a GPU.

    python tools/points_prep_time.py [--out FILE] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from batch_prep_time import scenes                                   # noqa: E402
from d3net_amd import dataset as D                                   # noqa: E402
from d3net_amd import pointgroup_ops                                 # noqa: E402
from d3net_amd import scene_prep as SP                               # noqa: E402
from d3net_amd.config import CONF_DIR, load_conf                     # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (t1 - t0) * 1e3


def spread(x):
    q1, med, q3 = np.percentile(x, [25, 50, 75])
    return {"median_ms": float(med), "min_ms": float(np.min(x)), "max_ms": float(np.max(x)), "iqr_ms": float(q3 - q1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="quarter-size scenes (a dry run of the tool)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("points_prep_time needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = load_conf(os.path.join(CONF_DIR, "path.yaml"), os.path.join(CONF_DIR, "pointgroup_captioning.yaml"), overrides={"data": {"batch_size": 4}})
    msa = torch.from_numpy(np.abs(np.random.RandomState(0).randn(18, 3)) + 0.3).to(dev)
    store = D.SceneStore.from_scenes(scenes(args.small), device=dev)
    sids, mode = list(store.scene_ids), int(cfg.data.mode)
    store.instance_index()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    store.extents(cfg.data.scale)
    torch.cuda.synchronize()
    extents_ms = (time.perf_counter() - t0) * 1e3
    paths = {"labelled": lambda: SP.prepare_batch_store(store, sids, cfg, msa, is_augment=False, device=dev, mode=mode),
             "label_free": lambda: SP.prepare_points_store(store, sids, cfg, device=dev, mode=mode)}
    a, b = paths["labelled"](), paths["label_free"]()
    equal = all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in SP._LABEL_FREE_KEYS) and set(b) == set(SP._LABEL_FREE_KEYS)
    vox = lambda: pointgroup_ops.voxelization_idx(b["locs_scaled"], len(sids), mode)
    ev = {k: [] for k in list(paths) + ["voxelisation"]}
    wall = {k: [] for k in paths}
    for rep in range(args.warmup + args.reps):
        for k, fn in paths.items():
            dt, host = timed(fn)
            if rep >= args.warmup:
                ev[k].append(dt); wall[k].append(host)
        dt, _ = timed(vox)
        if rep >= args.warmup:
            ev["voxelisation"].append(dt)
    vox_med = float(np.median(ev["voxelisation"]))
    n, Cf = int(store.points.shape[0]), int(store.feats.shape[1])
    res = {"points": [store.num_points(s) for s in sids], "feature_columns": Cf, "keys_equal": bool(equal),
           "labelled": spread(ev["labelled"]), "label_free": spread(ev["label_free"]), "voxelisation": spread(ev["voxelisation"]),
           "labelled_less_voxelisation_ms": float(np.median(ev["labelled"])) - vox_med,
           "label_free_less_voxelisation_ms": float(np.median(ev["label_free"])) - vox_med,
           "labelled_host_ms": float(np.median(wall["labelled"])), "label_free_host_ms": float(np.median(wall["label_free"])),
           # what d3_points_batch must move: xyz read, locs + locs_scaled written, the feature words read and written
           "label_free_kernel_bytes": n * (12 + 12 + 32 + 8 * Cf),
           "extents_build_ms": extents_ms, "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
