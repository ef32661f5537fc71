"""dataset.PipelineLoader(fused=True) against fused=False on one store: every batch of every pass equal key by key, in the listener
and the detector mode, with the fall-back of the augmented detector mode, and `python -m d3net_amd.train --data --fused-prep` end
to end on files written the way the reference's preparation writes them."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from d3net_amd import dataset as D
from d3net_amd import lang_prep as LP
from d3net_amd import synthetic as S
from d3net_amd.config import default_conf

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MSA = np.load(os.path.join(HERE, "golden", "lang_prep_golden.npz"))["mean_size_arr"]
TSV = os.path.join(HERE, "golden", "lang_prep_labels.tsv")
V = 200


def _raw_scenes(n):
    out = {}
    for k in range(n):
        sc = S.small_scene(dims=(40, 32, 20), n_boxes=3, seed=3 + k, n_feat=6)
        out["scene%04d_00" % k] = dict(points=sc["locs"], feats=sc["feats"], sem_labels=sc["sem_labels"], instance_ids=sc["instance_ids"])
    return out


def _annotations(scene_ids, per_scene=(4, 3, 2, 1, 2)):
    r = np.random.RandomState(2)
    return [{"scene_id": sid, "object_id": str(j % 3), "object_name": "chair", "ann_id": str(j // 3), "description": "d",
             "token": ["w%d" % w for w in r.randint(0, V - 4, r.randint(5, 40))]}
            for sid, n in zip(scene_ids, per_scene) for j in range(n)]


def _cfg(grounding, **data):
    model = {"no_captioning": True, "no_grounding": not grounding}
    return default_conf(overrides={"model": model, "data": dict({"num_des_per_scene": 4, "batch_size": 2, "requires_gt_mask": True}, **data)})


def _assert_batches_equal(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
            assert torch.equal(g, w), k
        else:
            assert g == w, k


@pytest.fixture(scope="module")
def store(dev):
    return D.SceneStore.from_scenes(_raw_scenes(5), device=dev)


def _pair(cfg, store, index, mode, dev, **kw):
    return [D.PipelineLoader(cfg, store, index, "train", mode, seed=5, mean_size_arr=MSA, device=dev, fused=f, **kw) for f in (True, False)]


def _compare_passes(fused, plain, passes=2):
    n = 0
    for _ in range(passes):
        got, want = list(fused), list(plain)
        assert len(got) == len(want) == len(plain)
        for g, w in zip(got, want):
            _assert_batches_equal(g, w)
            n += 1
    return n


@pytest.mark.parametrize("is_augment", [False, True])
@pytest.mark.parametrize("rank", [0, 1])
def test_listener_passes(dev, store, rank, is_augment):
    cfg = _cfg(True)
    glove = np.random.default_rng(0).standard_normal((V, 300)).astype(np.float32)
    index = LP.DescriptionIndex(_annotations(store.scene_ids), S.make_vocabulary(V), glove, cfg.data.max_lis_len, cfg.data.num_des_per_scene,
                                {"chair": 2}, scan2cad_rotation={"scene0000_00": {"0": np.eye(3).tolist()}}, device=dev)
    fused, plain = _pair(cfg, store, index, "listener", dev, rank=rank, world=2, is_augment=is_augment)
    assert fused.fused_active() and not plain.fused_active()
    assert _compare_passes(fused, plain) == 4                # 3 samples per rank in batches of 2, two passes


@pytest.mark.parametrize("rank", [0, 1])
def test_detector_passes(dev, store, rank):
    cfg = _cfg(False)
    fused, plain = _pair(cfg, store, None, "detector", dev, rank=rank, world=2, is_augment=False)
    assert fused.fused_active()
    assert _compare_passes(fused, plain) == 4


def test_augmented_detector_falls_back(dev, store):
    cfg = _cfg(False, batch_size=3)
    fused, plain = _pair(cfg, store, None, "detector", dev, is_augment=True)
    assert not fused.fused_active()                          # elastic distortion and crop: today's path, silently
    assert _compare_passes(fused, plain, passes=1) == 2


def test_pinned_store_falls_back(dev):
    pinned = D.SceneStore.from_scenes(_raw_scenes(2), device="cpu")
    loader = D.PipelineLoader(_cfg(False), pinned, None, "train", "detector", seed=5, mean_size_arr=MSA, device=dev, fused=True)
    assert not loader.fused_active() and len(list(loader)) == 1
    host = D.PipelineLoader(_cfg(False), pinned, None, "train", "detector", seed=5, mean_size_arr=MSA, device=dev, fused=True, noise="host")
    assert not host.fused_active()


def _write_dataset(root):
    """three training scenes and two validation scenes as the reference's preparation leaves them, and the annotation files"""
    data = os.path.join(root, "data")
    meta = os.path.join(data, "scannet", "meta_data")
    os.makedirs(meta)
    shutil.copy(TSV, os.path.join(meta, "scannetv2-labels.combined.tsv"))
    np.savez(os.path.join(meta, "scannet_reference_means.npz"), MSA)
    r = np.random.RandomState(0)
    for split, seeds in (("train", (3, 4, 5)), ("val", (6, 7))):
        os.makedirs(os.path.join(data, "scannet", "split_data", split))
        ids = []
        for seed in seeds:
            sc = S.small_scene(dims=(40, 32, 20), n_boxes=3, seed=seed)
            n = len(sc["locs"])
            mesh = np.concatenate([sc["locs"], r.randint(0, 255, (n, 3)).astype(np.float32), r.randn(n, 3).astype(np.float32)], 1)
            sid = "scene%04d_00" % seed
            torch.save({"aligned_mesh": mesh, "sem_labels": sc["sem_labels"].astype(np.float64),
                        "instance_ids": sc["instance_ids"].astype(np.float64)}, os.path.join(data, "scannet", "split_data", split, sid + ".pth"))
            ids.append(sid)
        json.dump(_annotations(ids, per_scene=(9, 3, 5)), open(os.path.join(data, "ScanRefer_filtered_%s.json" % split), "w"))
    json.dump(S.make_vocabulary(V), open(os.path.join(data, "ScanRefer_vocabulary.json"), "w"))
    np.save(os.path.join(data, "glove_trimmed_ScanRefer.npy"), np.random.default_rng(0).standard_normal((V, 300)))
    return data


def test_train_data_fused_prep_end_to_end(dev, tmp_path, capsys):
    from d3net_amd import train
    data = _write_dataset(str(tmp_path))
    root = str(tmp_path / "run")
    over = {"DATA_PATH": data, "data": {"batch_size": 2}, "train": {"log_every_n_steps": 1},
            "model": {"use_multiview": False, "use_color": True, "pretrained_detector": None}}
    tr = train.main(["-c", "pointgroup_captioning.yaml", "--data", "--fused-prep", "--teacher", "--epochs", "1", "--root", root], overrides=over)
    assert tr.global_step == 2
    assert "fused batch preparation: in use by 2 of 2 loaders" in capsys.readouterr().out
    with open(os.path.join(root, "logs", "metrics.jsonl")) as f:
        records = [json.loads(line) for line in f]
    epochs = [r for r in records if r["kind"] == "epoch"]
    assert len(epochs) == 1 and epochs[0]["global_step"] == 2 and np.isfinite(epochs[0]["train_loss/loss"])
