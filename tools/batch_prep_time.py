"""Time the construction of one captioning batch by `dataset.PipelineLoader`, fused=False against fused=True, after DESIGN §3.15's
protocol: the four scenes of bench.py's captioning step (182-189 k points each, 131 feature columns, 8 descriptions per scene) in
one resident store, HIP events around the batch construction only, 5 warm-up constructions then the median of 20, the two
loaders alternating in one process; plus the device operations per batch (torch profiler; for the whole batch, and for the scene
half alone with the shared voxelisation taken out), the voxelisation's own time, the one-off instance-index build time and the
index's bytes.  Prints one JSON line (and writes it to --out).

    python tools/batch_prep_time.py [--out FILE] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from d3net_amd import dataset as D                                   # noqa: E402
from d3net_amd import lang_prep as LP                                # noqa: E402
from d3net_amd import pointgroup_ops                                 # noqa: E402
from d3net_amd import scene_prep as SP                               # noqa: E402
from d3net_amd import synthetic as S                                 # noqa: E402
from d3net_amd.config import CONF_DIR, load_conf                     # noqa: E402

VOCAB = 3004


def scenes(small):
    """bench.py:make_scenes("captioning", rank 0)"""
    out = {}
    for g in range(4):
        dims, nb, side = ((100, 75, 50), 10, (6, 16)) if small else ((200, 150, 100), 40, (8, 30))
        occ, sem, inst, _ = S.occupancy_grid(dims, nb, side, side, seed=g)
        sc = S.scene_from_grid(occ, sem, inst, seed=1 + g % 4, feat_seed=2 + g)
        out["scene%04d_00" % g] = dict(points=sc["locs"], feats=sc["feats"], sem_labels=sc["sem_labels"], instance_ids=sc["instance_ids"])
    return out


def annotations(scene_ids, per_scene):
    r = np.random.RandomState(2)
    return [{"scene_id": sid, "object_id": str(j % 3), "object_name": "chair", "ann_id": str(j // 3), "description": "d",
             "token": ["w%d" % w for w in r.randint(0, VOCAB - 4, r.randint(5, 28))]} for sid in scene_ids for j in range(per_scene)]


def device_ops(build):
    """(kernels, copies and memsets) of one construction, from the profiler's device-side events"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        build()
        torch.cuda.synchronize()
    kernels = copies = 0
    for e in prof.events():
        if str(getattr(e, "device_type", "")).endswith("CUDA"):
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                copies += 1
            else:
                kernels += 1
    return kernels, copies


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="quarter-size scenes (a dry run of the tool)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = load_conf(os.path.join(CONF_DIR, "path.yaml"), os.path.join(CONF_DIR, "pointgroup_captioning.yaml"), overrides={"data": {"batch_size": 4}})
    msa = np.abs(np.random.RandomState(0).randn(18, 3)) + 0.3
    sc = scenes(args.small)
    store = D.SceneStore.from_scenes(sc, device=dev)
    glove = np.random.default_rng(3).standard_normal((VOCAB, 300)).astype(np.float32)
    index = LP.DescriptionIndex(annotations(list(sc), cfg.data.num_des_per_scene), S.make_vocabulary(VOCAB), glove, cfg.data.max_spk_len,
                                cfg.data.num_des_per_scene, {"chair": 2}, device=dev)
    loaders = {f: D.PipelineLoader(cfg, store, index, "train", "speaker", seed=1, mean_size_arr=msa, device=dev, fused=f) for f in (False, True)}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ix = store.instance_index()
    torch.cuda.synchronize()
    index_ms = (time.perf_counter() - t0) * 1e3
    assert loaders[True].fused_active() and len(index) == 4
    idxs = list(range(4))
    gens = {f: loaders[f].generators(0) for f in loaders}
    build = lambda f: loaders[f].build(idxs, *gens[f])
    a, b = build(False), build(True)
    equal = set(a) == set(b) and all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)
    ev = {f: [] for f in loaders}
    wall = {f: [] for f in loaders}
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
    # the scene half alone (no descriptions), and the voxelisation both paths share, to take out of it
    sids, mode = [index.scene_id(c) for c in idxs], int(cfg.data.mode)
    per_scene = lambda: SP.collate_scenes_device([SP.prepare_scene(store.scene(s), cfg, msa, rng=gens[False][0], is_augment=False, device=dev)
                                                  for s in sids], dev, mode)
    from_store = lambda: SP.prepare_batch_store(store, sids, cfg, loaders[True].mean_sizes(), is_augment=False, device=dev, mode=mode)
    vox = device_ops(lambda: pointgroup_ops.voxelization_idx(b["locs_scaled"], 4, mode))
    half = {False: device_ops(per_scene), True: device_ops(from_store)}
    vox_ms = []
    for rep in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        pointgroup_ops.voxelization_idx(b["locs_scaled"], 4, mode)
        e1.record()
        torch.cuda.synchronize()
        vox_ms.append(e0.elapsed_time(e1))
    res = {"points": [store.num_points(s) for s in store.scene_ids], "feature_columns": int(store.feats.shape[1]),
           "store_mib": store.bytes() / 2 ** 20, "index_bytes": ix.bytes(), "index_build_ms": index_ms, "batches_equal": bool(equal),
           "plain_ms": float(np.median(ev[False])), "fused_ms": float(np.median(ev[True])),
           "voxelisation_ms": float(np.median(vox_ms[args.warmup:])),
           "plain_host_ms": float(np.median(wall[False])), "fused_host_ms": float(np.median(wall[True])),
           "plain_ops": {"kernels": ops[False][0], "copies_memsets": ops[False][1]},
           "fused_ops": {"kernels": ops[True][0], "copies_memsets": ops[True][1]},
           "voxelisation_ops": {"kernels": vox[0], "copies_memsets": vox[1]},
           "plain_scene_half_ops": {"kernels": half[False][0] - vox[0], "copies_memsets": half[False][1] - vox[1]},
           "fused_scene_half_ops": {"kernels": half[True][0] - vox[0], "copies_memsets": half[True][1] - vox[1]},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
