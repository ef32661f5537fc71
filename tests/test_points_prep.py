"""The host side of the label-free path: `SceneStore(labels=False)` packing on host arrays, scene files without label keys, the
refusal of an empty scene, `build_test_loader`'s entry lists and chunks against tests/dataset_restate.py, `predict.main`'s
refusals, and the restatement's own arithmetic.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

import dataset_restate as DR
import points_prep_restate as PR
from d3net_amd import dataset as D
from d3net_amd import predict
from d3net_amd.config import default_conf

OVER, V = PR.OVER, PR.V


def _scene(n, width=3, seed=0, labels=True):
    r = np.random.RandomState(seed)
    sc = {"points": ((r.rand(n, 3) - 0.3) * 4).astype(np.float32), "feats": r.randn(n, width).astype(np.float32)}
    if labels:
        sc.update(sem_labels=r.randint(-1, 20, n).astype(np.int32), instance_ids=r.randint(-1, 4, n).astype(np.int32))
    return sc


def test_label_free_store_is_packed_as_specified():
    scenes = {"a": _scene(5, seed=1), "b": _scene(1, seed=2, labels=False), "c": _scene(7, seed=3)}
    store = D.SceneStore.from_scenes(scenes, device="cpu", labels=False)
    assert store.labels is False and list(store.offsets) == [0, 5, 6, 13] and store.scene_ids == ["a", "b", "c"]
    assert store.points.shape == (13, 3) and store.feats.shape == (13, 3)
    for k in ("sem_labels", "instance_ids"):
        assert getattr(store, k).shape == (0,) and getattr(store, k).dtype == torch.int32
    assert store.bytes() == 13 * (12 + 12)
    for i, (sid, sc) in enumerate(scenes.items()):
        a, b = int(store.offsets[i]), int(store.offsets[i + 1])
        assert np.array_equal(store.points[a:b].numpy(), sc["points"]) and np.array_equal(store.feats[a:b].numpy(), sc["feats"])
        assert store.num_points(sid) == b - a and store.row_of(sid) == i
    if not torch.cuda.is_available():                       # (with a GPU the pinned store's scene() returns device copies)
        assert set(store.scene("a")) == {"points", "feats"}
    with pytest.raises(ValueError, match="labels=False"):
        store.instance_index()
    with pytest.raises(ValueError, match="pinned host"):
        store.extents(50)
    # the labelled store of the same scenes is what it was
    labelled = D.SceneStore.from_scenes({k: v for k, v in scenes.items() if k != "b"}, device="cpu")
    assert labelled.labels is True and labelled.sem_labels.shape == (12,) and labelled.bytes() == 12 * (12 + 12 + 4 + 4)
    with pytest.raises(KeyError):
        D.SceneStore.from_scenes(scenes, device="cpu")     # "b" has no labels


def test_empty_scene_is_refused_by_name():
    scenes = {"fine": _scene(4), "hollow_scene": _scene(0)}
    with pytest.raises(ValueError, match="hollow_scene"):
        D.SceneStore.from_scenes(scenes, device="cpu", labels=False)


def test_scene_file_without_label_keys_loads(tmp_path):
    cfg = default_conf(overrides=dict(OVER, DATA_PATH=str(tmp_path)))
    r = np.random.RandomState(0)
    meshes = {"scene0001_00": r.rand(6, 9).astype(np.float32), "scene0002_00": r.rand(3, 9).astype(np.float32)}
    PR.write_split(str(tmp_path / "scannet" / "split_data" / "test"), meshes, labels="absent")
    store = D.SceneStore.load(cfg, "test", list(meshes), device="cpu", labels=False)
    assert list(store.offsets) == [0, 6, 9] and store.sem_labels.numel() == 0
    want = np.concatenate([DR.mesh_columns(m, cfg.model.use_color, cfg.model.use_normal, None)[1] for m in meshes.values()])
    assert np.array_equal(store.feats.numpy(), want) and np.array_equal(store.points.numpy(), np.concatenate([m[:, :3] for m in meshes.values()]))
    with pytest.raises(KeyError):
        D.SceneStore.load(cfg, "test", list(meshes), device="cpu")


@pytest.mark.parametrize("task,split", [("captioning", "test"), ("grounding", "test"), ("captioning", "val")])
def test_build_test_loader_lists_and_chunks(tmp_path, task, split):
    data, raw = PR.write_dataset(str(tmp_path), splits=(split,))
    cfg = predict.task_conf("pointgroup_captioning.yaml" if task == "captioning" else "pointgroup_grounding.yaml", task,
                            dict(OVER, DATA_PATH=data))
    size = cfg.data.num_des_per_scene
    assert size == (8 if task == "captioning" else 1) and cfg.cluster.prepare_epochs == -1
    loader, dataset, store = D.build_test_loader(cfg, "cpu", task, split)
    listed = DR.speaker([], raw[split], [], 0.0, 0)["val"] if (task, split) == ("captioning", "test") else DR.listener([], raw[split])["val"]
    entries, scans = listed
    assert D.prediction_entries(raw[split], split, task) == (entries, scans)
    assert store.scene_ids == scans and store.labels is False and store.sem_labels.numel() == 0
    assert set(dataset) == {"train", split} and not hasattr(dataset["train"], "chunked_data")
    assert dataset[split].chunked_data == DR.chunked(entries, size) and dataset[split].raw_data == entries
    assert len(dataset["train"].vocabulary["word2idx"]) == V and dataset["train"].glove.shape == (V, 300)
    assert loader.label_free and not loader.shuffle and loader.mode == ("speaker" if task == "captioning" else "listener")
    assert loader.index.max_des_len == (cfg.data.max_spk_len if task == "captioning" else cfg.data.max_lis_len)
    assert loader.num_samples() == len(DR.chunked(entries, size)) and loader.order(0) == list(range(loader.num_samples()))
    assert [loader.sample_scene(i) for i in range(loader.num_samples())] == [c[0]["scene_id"] for c in DR.chunked(entries, size)]
    if (task, split) == ("captioning", "test"):
        assert len(entries) == len(scans) == 2 and all(e["object_id"] == raw[split][0]["object_id"] for e in entries)
    else:
        assert len(entries) == len(raw[split]) > len(scans)
    with pytest.raises(ValueError):
        D.build_test_loader(cfg, "cpu", "detection", split)


def test_label_free_loader_switches():
    store = D.SceneStore.from_scenes({"a": _scene(5, labels=False)}, device="cpu", labels=False)
    cfg = default_conf()
    with pytest.raises(ValueError, match="augment"):
        D.PipelineLoader(cfg, store, None, "test", "detector", is_augment=True)
    with pytest.raises(ValueError, match="augment"):
        D.PipelineLoader(cfg, store, None, "val", "detector", is_augment=True, label_free=True)
    assert D.PipelineLoader(cfg, store, None, "test", "detector").label_free
    assert not D.PipelineLoader(cfg, store, None, "test", "detector", label_free=False).label_free
    on_train = D.PipelineLoader(cfg, store, None, "train", "detector", label_free=True)
    assert on_train.label_free and not on_train.shuffle and not on_train.fused_active("cpu")
    plain = D.PipelineLoader(cfg, store, None, "train", "detector")
    assert not plain.label_free and plain.shuffle
    assert D.PipelineLoader(cfg, store, None, "test", "detector", shuffle=True).shuffle


def test_predict_refusals(monkeypatch, tmp_path):
    argv = ["-c", "pointgroup_captioning.yaml", "--task", "captioning", "--root", str(tmp_path)]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no checkpoint at .*model.ckpt"):     # before anything is loaded or built
        predict.main(argv)
    with pytest.raises(SystemExit, match="no checkpoint at .*other.ckpt"):
        predict.main(argv + ["--ckpt", str(tmp_path / "other.ckpt")])
    (tmp_path / "model.ckpt").write_bytes(b"")
    with pytest.raises(SystemExit, match="needs a GPU"):
        predict.main(argv)
    with pytest.raises(SystemExit, match="requires_gt_mask"):
        predict.main(argv, overrides={"data": {"requires_gt_mask": True}})
    with pytest.raises(SystemExit, match="needs the detector and the listener"):
        predict.main(["-c", "pointgroup_captioning.yaml", "--task", "grounding"])
    with pytest.raises(SystemExit, match="needs the detector and the speaker"):
        predict.main(["-c", "pointgroup_grounding.yaml", "--task", "captioning"])
    with pytest.raises(SystemExit, match="needs the detector"):
        predict.main(argv, overrides={"model": {"no_detection": True}})
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single-process"):
        predict.main(argv)
    assert predict.default_output("r", "captioning", "val") == os.path.join("r", "benchmark_val.nms.json")
    assert predict.default_output("r", "grounding", "test") == os.path.join("r", "pred.json")


def test_restatement_arithmetic():
    pts = np.array([[-1.5, 0.25, 3.0], [2.0, -0.75, 3.0], [0.5, 0.5, 3.5]], np.float32)
    feats = np.arange(6, dtype=np.float32).reshape(3, 2)
    out = PR.batch({"s": {"points": pts, "feats": feats}}, ["s", "s"], 50)
    assert out["locs"].dtype == np.float32 and out["locs_scaled"].dtype == np.int64 and out["batch_offsets"].tolist() == [0, 3, 6]
    assert out["locs_scaled"].tolist() == [[0, 0, 50, 0], [0, 175, 0, 0], [0, 100, 62, 25]] + [[1, 0, 50, 0], [1, 175, 0, 0], [1, 100, 62, 25]]
    assert np.array_equal(out["locs"][:3], pts) and np.array_equal(out["feats"][3:], feats)
    assert PR.extents(pts, 50).tolist() == [-75.0, -37.5, 150.0]
    # truncation toward zero on the fractional part (all values are >= 0 after the shift)
    assert PR.collate([PR.sample(np.array([[0, 0, 0], [0.999, 0.019, 0.021]], np.float32), np.zeros((2, 0)), 50)])["locs_scaled"][1].tolist() == [0, 49, 0, 1]
