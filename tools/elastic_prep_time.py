"""Time the construction of one augmented detector-only batch (elastic distortion and crop) by `dataset.PipelineLoader`: the
per-scene path (`prepare_scene` per scene + `collate_scenes_device`) against fused_elastic=True
(`scene_prep.prepare_batch_store_elastic`), after DESIGN §3.16's protocol: one process, the four scenes of bench.py's step in one
resident store, HIP events around `PipelineLoader.build` only, 5 warm-up constructions then the median of 20, the two loaders
alternating, their batches compared first.  Also: the time until `build` returns to the host, the device operations of both paths
(torch profiler), the voxelisation both share, and the bytes the new path must move (the store rows it reads and the batch tensors it
writes, each once) beside the workspace it works in.  Prints one JSON line (and writes it to --out).

    python tools/elastic_prep_time.py [--out FILE] [--small] [--max-num-point N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from d3net_amd import _lib                                            # noqa: E402
from d3net_amd import dataset as D                                   # noqa: E402
from d3net_amd import pointgroup_ops                                 # noqa: E402
from d3net_amd import scene_prep as SP                               # noqa: E402
from d3net_amd.config import CONF_DIR, load_conf                     # noqa: E402
from batch_prep_time import device_ops, scenes                       # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="quarter-size scenes (a dry run of the tool)")
    ap.add_argument("--max-num-point", type=int, default=None, help="override data.max_num_point (a value below the scenes' sizes "
                    "makes slots crop; the batches are then compared by shape only, since the crop draws differ)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    data = {"batch_size": 4}
    if args.max_num_point is not None:
        data["max_num_point"] = args.max_num_point
    cfg = load_conf(os.path.join(CONF_DIR, "path.yaml"), os.path.join(CONF_DIR, "pointgroup.yaml"), overrides={"data": data})
    assert SP.elastic_enabled(cfg, True)
    msa = np.abs(np.random.RandomState(0).randn(18, 3)) + 0.3
    sc = scenes(args.small)
    store = D.SceneStore.from_scenes(sc, device=dev)
    mk = lambda f: D.PipelineLoader(cfg, store, None, "train", "detector", seed=1, mean_size_arr=msa, device=dev, is_augment=True, fused=f,
                                    fused_elastic=f)
    loaders = {f: mk(f) for f in (False, True)}
    assert loaders[True].fused_elastic_active() and not loaders[False].fused_elastic_active()
    store.instance_index(), store.absmax()
    idxs = list(range(4))
    gens = {f: loaders[f].generators(0) for f in loaders}
    build = lambda f: loaders[f].build(idxs, *gens[f])
    a, b = build(False), build(True)
    cropped = int(a["locs"].shape[0]) < sum(store.num_points(s) for s in store.scene_ids)
    equal = set(a) == set(b) and all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a) if not cropped else None
    ev, wall = {f: [] for f in loaders}, {f: [] for f in loaders}
    for rep in range(args.warmup + args.reps):
        for f in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            build(f)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                ev[f].append(e0.elapsed_time(e1))
                wall[f].append((t1 - t0) * 1e3)
    ops = {f: device_ops(lambda: build(f)) for f in loaders}
    mode = int(cfg.data.mode)
    vox = device_ops(lambda: pointgroup_ops.voxelization_idx(b["locs_scaled"], 4, mode))
    info = {}
    SP.prepare_batch_store_elastic(store, [store.scene_ids[i] for i in idxs], cfg, loaders[True].mean_sizes(), rng=gens[True][0], device=dev,
                                   mode=mode, info=info)
    n, Cf = np.diff(store.offsets), int(store.feats.shape[1])
    slots = np.ascontiguousarray(np.concatenate([n[:, None], (np.maximum(store.instance_index().scalars[:, 1], 0) + 1)[:, None], info["bounds"]],
                                                1).astype(np.int32))
    T = SP.crop_max_iters(cfg.data.full_scale[1])
    ws_bytes = int(_lib.lib().d3_batch_elastic_ws_bytes(slots.ctypes.data, 4, Cf, T))
    read = int(n.sum()) * (12 + 4 * Cf + 4 + 4)
    written = sum(t.numel() * t.element_size() for k, t in b.items() if torch.is_tensor(t) and k not in ("voxel_locs", "p2v_map", "v2p_map"))
    res = {"points": [int(v) for v in n], "feature_columns": Cf, "max_num_point": int(cfg.data.max_num_point), "batches_equal": equal,
           "kept_points": int(b["locs"].shape[0]),
           "plain_ms": float(np.median(ev[False])), "fused_elastic_ms": float(np.median(ev[True])),
           "plain_host_ms": float(np.median(wall[False])), "fused_elastic_host_ms": float(np.median(wall[True])),
           "plain_ops": {"kernels": ops[False][0], "copies_memsets": ops[False][1]},
           "fused_elastic_ops": {"kernels": ops[True][0], "copies_memsets": ops[True][1]},
           "voxelisation_ops": {"kernels": vox[0], "copies_memsets": vox[1]},
           "readback": {k: info["readback"][:, i].tolist() for i, k in enumerate(SP.READBACK_COLUMNS)}, "grid_bounds": info["bounds"].tolist(),
           "must_move_bytes": {"store_rows_read": read, "batch_written": int(written)}, "workspace_bytes": ws_bytes,
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
