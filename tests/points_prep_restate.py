"""Host restatement of the reference's label-free sample and its stacking, written from the behaviour of
lib/dataset/pipeline.py:352-380 (the `else:` branch of `__getitem__`: points * scale, minus points.min(0), nothing read from the
label arrays) and of the point keys of `sparse_collate_fn` (:937-976, :992).  Plain numpy on float32 arrays with a Python-int
scale; the cast to int64 truncates toward zero, as `torch.Tensor.long()` does.  The voxelisation is not restated: it is
`pointgroup_ops.voxelization_idx` on every path and has its own tests.

`write_split` writes scene files the way data/scannet/prepare_scannet.py leaves a split's and `write_dataset` the tree around them
(annotation file, vocabulary, GloVe table, meta data), for the tests that load them."""
import os

import numpy as np


def sample(points, feats, scale):
    """one scene -> (locs, locs_scaled, feats) as `__getitem__` returns them"""
    points = np.asarray(points, np.float32)
    assert points.dtype == np.float32 and isinstance(scale, int)
    points_augment = points.copy()
    scaled = points_augment * scale                   # float32 * python int stays float32
    assert scaled.dtype == np.float32
    scaled -= scaled.min(0)
    return points_augment.astype(np.float32), scaled.astype(np.float32), np.asarray(feats, np.float32)


def collate(samples):
    """the stacked point keys of a batch of `sample` results: locs (N,3) float32, locs_scaled (N,4) int64 = (slot, truncated
    coordinates), feats (N,C) float32, batch_offsets (B+1) int32"""
    locs, scaled, feats, offsets = [], [], [], [0]
    for slot, (l, s, f) in enumerate(samples):
        n = l.shape[0]
        locs.append(l)
        scaled.append(np.concatenate([np.full((n, 1), slot, np.int64), np.trunc(s).astype(np.int64)], 1))
        feats.append(f.reshape(n, -1))
        offsets.append(offsets[-1] + n)
    return {"locs": np.concatenate(locs, 0), "locs_scaled": np.concatenate(scaled, 0), "feats": np.concatenate(feats, 0),
            "batch_offsets": np.asarray(offsets, np.int32)}


def batch(scenes, scene_ids, scale):
    """scenes: {scene_id: {"points", "feats", ...}}; a scene may fill several slots"""
    return collate([sample(scenes[s]["points"], scenes[s]["feats"], scale) for s in scene_ids])


def extents(points, scale):
    """(3,) float32: what `sample` subtracts"""
    return (np.asarray(points, np.float32) * np.float32(scale)).min(0)


def write_split(split_dir, meshes, labels=None):
    """meshes: {scene_id: (N,9) float32 aligned mesh}.  labels: {scene_id: (sem_labels, instance_ids)}; a scene missing from it
    (or labels=None) gets the placeholders prepare_scannet.py writes on the test split, labels="absent" leaves the keys out"""
    import torch
    os.makedirs(split_dir, exist_ok=True)
    for sid, mesh in meshes.items():
        n = mesh.shape[0]
        d = {"aligned_mesh": mesh}
        if labels != "absent":
            sem, ids = (labels or {}).get(sid, (np.zeros(n), np.zeros(n)))
            d.update(sem_labels=np.asarray(sem, np.float64), instance_ids=np.asarray(ids, np.float64))
        torch.save(d, os.path.join(split_dir, sid + ".pth"))


# ---- the dataset tree the loader and CLI tests read (host files only)
HERE = os.path.dirname(os.path.abspath(__file__))
MSA = np.load(os.path.join(HERE, "golden", "lang_prep_golden.npz"))["mean_size_arr"]
TSV = os.path.join(HERE, "golden", "lang_prep_labels.tsv")
V = 200
SEEDS = (8, 9)
# colours and normals as features (no multiview file is written), no pretrained weights
OVER = {"data": {"batch_size": 2}, "model": {"use_multiview": False, "use_color": True, "pretrained_detector": None}}


def _annotations(scene_ids, per_scene):
    r = np.random.RandomState(2)
    return [{"scene_id": sid, "object_id": str(j % 3), "object_name": "chair", "ann_id": str(j // 3), "description": "d",
             "token": ["w%d" % w for w in r.randint(0, V - 4, r.randint(5, 40))]}
            for sid, n in zip(scene_ids, per_scene) for j in range(n)]


def write_dataset(root, splits=("test",), per_scene=(9, 3)):
    """two scenes per split as the reference's preparation leaves them -- `<split>` with the placeholder labels of the test split,
    `<split>_labelled` the same meshes with their real labels -- the split's annotation file, vocabulary, GloVe table and meta data
    -> (DATA_PATH, {split: annotations})"""
    import json
    import shutil
    from d3net_amd import synthetic
    data = os.path.join(root, "data")
    meta = os.path.join(data, "scannet", "meta_data")
    os.makedirs(meta)
    shutil.copy(TSV, os.path.join(meta, "scannetv2-labels.combined.tsv"))
    np.savez(os.path.join(meta, "scannet_reference_means.npz"), MSA)
    r = np.random.RandomState(0)
    raw = {}
    for split in splits:
        meshes, labels = {}, {}
        for seed in SEEDS:
            sc = synthetic.small_scene(dims=(40, 32, 20), n_boxes=3, seed=seed)
            n = len(sc["locs"])
            sid = "scene%04d_00" % seed
            meshes[sid] = np.concatenate([sc["locs"], r.randint(0, 255, (n, 3)).astype(np.float32), r.randn(n, 3).astype(np.float32)], 1)
            labels[sid] = (sc["sem_labels"], sc["instance_ids"])
        write_split(os.path.join(data, "scannet", "split_data", split), meshes)
        write_split(os.path.join(data, "scannet", "split_data", split + "_labelled"), meshes, labels)
        raw[split] = _annotations(list(meshes)[::-1], per_scene)              # the file names the later scene first
        json.dump(raw[split], open(os.path.join(data, "ScanRefer_filtered_%s.json" % split), "w"))
    json.dump(synthetic.make_vocabulary(V), open(os.path.join(data, "ScanRefer_vocabulary.json"), "w"))
    np.save(os.path.join(data, "glove_trimmed_ScanRefer.npy"), np.random.default_rng(0).standard_normal((V, 300)))
    return data, raw
