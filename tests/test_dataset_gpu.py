"""d3net_amd.dataset on the device: a PipelineLoader batch over a SceneStore against lang_prep.prepare_pipeline_batch /
scene_prep.prepare_batch over the host-dict scenes (the same generators, samples and switches: every key equal), the pinned-host
store against the resident one, the passes of a sharded loader, and `python -m d3net_amd.train --data` end to end on files written
the way the reference's preparation writes them."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from d3net_amd import dataset as D
from d3net_amd import lang_prep as LP
from d3net_amd import scene_prep as SP
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


def _annotations(scene_ids, per_scene=(4, 3, 5, 1, 2)):
    r = np.random.RandomState(2)
    return [{"scene_id": sid, "object_id": str(j % 3), "object_name": "chair", "ann_id": str(j // 3), "description": "d",
             "token": ["w%d" % w for w in r.randint(0, V - 4, r.randint(5, 40))]}
            for sid, n in zip(scene_ids, per_scene) for j in range(n)]


def _cfg(grounding, **data):
    model = {"no_captioning": True, "no_grounding": not grounding}
    return default_conf(overrides={"model": model, "data": dict({"num_des_per_scene": 4, "batch_size": 2, "requires_gt_mask": True}, **data)})


def _index(raw, cfg, dev):
    glove = np.random.default_rng(0).standard_normal((V, 300)).astype(np.float32)
    return LP.DescriptionIndex(raw, S.make_vocabulary(V), glove, cfg.data.max_lis_len, cfg.data.num_des_per_scene, {"chair": 2},
                               scan2cad_rotation={"scene0000_00": {"0": np.eye(3).tolist()}}, device=dev)


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
def scenes():
    return _raw_scenes(3)


@pytest.mark.parametrize("is_augment", [True, False])
def test_language_batch_equals_prepare_pipeline_batch(dev, scenes, is_augment):
    cfg = _cfg(True)
    index = _index(_annotations(list(scenes)), cfg, dev)
    store = D.SceneStore.from_scenes(scenes, device=dev)
    loader = D.PipelineLoader(cfg, store, index, "train", "listener", seed=5, is_augment=is_augment, mean_size_arr=MSA, device=dev)
    rng, pyrng = loader.generators(0)
    order = loader.order(0)
    assert sorted(order) == list(range(len(index))) == [0, 1, 2, 3]
    it = iter(loader)
    for i in range(0, 4, 2):
        want = LP.prepare_pipeline_batch(index, order[i:i + 2], scenes, cfg, MSA, rng=rng, pyrng=pyrng, is_augment=is_augment,
                                         apply_word_erase=cfg.train.apply_word_erase, noise="device", device=dev)
        _assert_batches_equal(next(it), want)
    assert want["lang_feat"].shape[:2] == (2, 4) and "gt_proposals_idx" in want


@pytest.mark.parametrize("is_augment", [True, False])
def test_detector_batch_equals_prepare_batch(dev, scenes, is_augment):
    cfg = _cfg(False, batch_size=3)
    store = D.SceneStore.from_scenes(scenes, device=dev)
    loader = D.PipelineLoader(cfg, store, None, "train", "detector", seed=9, is_augment=is_augment, mean_size_arr=MSA, device=dev)
    rng, _ = loader.generators(0)
    order = loader.order(0)
    want = SP.prepare_batch([scenes[store.scene_ids[i]] for i in order], cfg, MSA, rng=rng, is_augment=is_augment, noise="device", device=dev,
                            mode=cfg.data.mode)
    got = list(loader)
    assert len(got) == len(loader) == 1
    _assert_batches_equal(got[0], want)
    # the views were read, not written
    for sid, sc in scenes.items():
        for k, v in store.scene(sid).items():
            assert np.array_equal(v.cpu().numpy(), np.asarray(sc[k]).astype(v.cpu().numpy().dtype)), (sid, k)


def test_pinned_store_gives_the_same_batch(dev, scenes):
    cfg = _cfg(True)
    index = _index(_annotations(list(scenes)), cfg, dev)
    on_device, pinned = D.SceneStore.from_scenes(scenes, device=dev), D.SceneStore.from_scenes(scenes, device="cpu")
    assert pinned.points.is_pinned() and not pinned.points.is_cuda and on_device.points.is_cuda and pinned.bytes() == on_device.bytes()
    view = on_device.scene("scene0001_00")["feats"]
    assert view.data_ptr() == on_device.feats[int(on_device.offsets[1])].data_ptr()
    batches = [next(iter(D.PipelineLoader(cfg, st, index, "train", "listener", seed=5, is_augment=True, mean_size_arr=MSA, device=dev)))
               for st in (on_device, pinned)]
    _assert_batches_equal(batches[1], batches[0])


def test_two_passes_over_both_ranks(dev):
    scenes = _raw_scenes(5)
    cfg = _cfg(True)
    index = _index(_annotations(list(scenes), per_scene=(4, 3, 2, 1, 2)), cfg, dev)
    assert len(index) == 5
    store = D.SceneStore.from_scenes(scenes, device=dev)
    passes = {}
    for rank in (0, 1):
        loader = D.PipelineLoader(cfg, store, index, "train", "listener", rank=rank, world=2, seed=5, mean_size_arr=MSA, device=dev)
        assert len(loader) == 2                                                          # 3 samples per rank in batches of 2
        passes[rank] = [list(loader), list(loader)]
        assert [len(p) for p in passes[rank]] == [2, 2] and [b["id"].numel() for b in passes[rank][0]] == [2, 1]
        loader.set_epoch(0)
        for again, first in zip(loader, passes[rank][0]):
            _assert_batches_equal(again, first)
    ids = lambda e: [int(i) for rank in (0, 1) for b in passes[rank][e] for i in b["id"]]
    assert set(ids(0)) == set(ids(1)) == set(range(5)) and len(ids(0)) == 6              # every sample, one wrapped around
    assert ids(0) != ids(1)


def _write_dataset(root):
    """three training scenes and two validation scenes as the reference's preparation leaves them, and the annotation files"""
    data = os.path.join(root, "data")
    meta = os.path.join(data, "scannet", "meta_data")
    os.makedirs(meta)
    shutil.copy(TSV, os.path.join(meta, "scannetv2-labels.combined.tsv"))
    np.savez(os.path.join(meta, "scannet_reference_means.npz"), MSA)
    r = np.random.RandomState(0)
    raw = {}
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
        raw[split] = _annotations(ids, per_scene=(9, 3, 5))
        json.dump(raw[split], open(os.path.join(data, "ScanRefer_filtered_%s.json" % split), "w"))
    json.dump(S.make_vocabulary(V), open(os.path.join(data, "ScanRefer_vocabulary.json"), "w"))
    np.save(os.path.join(data, "glove_trimmed_ScanRefer.npy"), np.random.default_rng(0).standard_normal((V, 300)))
    return data, raw


def test_train_data_end_to_end(dev, tmp_path):
    """`train.main(["-c", "pointgroup_captioning.yaml", "--data", "--epochs", "1", "--root", tmp])` with the path configuration
    pointed at files in tmp_path; `--teacher` because the detector's weights are random here (the reference starts from a
    pretrained detector), colours and normals as features (no multiview file is written), and one log record per step so that
    the steps can be counted"""
    from d3net_amd import train
    data, raw = _write_dataset(str(tmp_path))
    root = str(tmp_path / "run")
    over = {"DATA_PATH": data, "data": {"batch_size": 2}, "train": {"log_every_n_steps": 1},
            "model": {"use_multiview": False, "use_color": True, "pretrained_detector": None}}
    tr = train.main(["-c", "pointgroup_captioning.yaml", "--data", "--teacher", "--epochs", "1", "--root", root], overrides=over)
    chunks = sum(-(-n // 8) for n in (9, 3, 5))             # 9 + 3 + 5 descriptions in chunks of 8
    n_batches = -(-chunks // 2)
    assert tr.global_step == n_batches == 2
    assert os.path.exists(os.path.join(root, "last.ckpt"))
    with open(os.path.join(root, "logs", "metrics.jsonl")) as f:
        records = [json.loads(line) for line in f]
    steps, epochs = [r for r in records if r["kind"] == "step"], [r for r in records if r["kind"] == "epoch"]
    # the epoch record counts the steps; a step line is the snapshot taken one step earlier (MetricLog.snapshot never waits), so
    # n steps leave n - 1 of them
    assert len(epochs) == 1 and epochs[0]["global_step"] == n_batches
    assert [s["global_step"] for s in steps] == list(range(1, n_batches))
    assert np.isfinite(epochs[0]["train_loss/loss"]) and "nonfinite" not in epochs[0]
    assert all(np.isfinite(s["train_loss/loss"]) for s in steps)
    assert "val_score/cider" in epochs[0]
