"""d3net_amd.dataset on the host: the annotation lists against the restated reference bookkeeping (tests/dataset_restate.py), the
per-rank pass order against torch's DistributedSampler, the joint mode's pairing, and SceneStore's packing on host arrays."""
import random

import numpy as np
import pytest
import torch
from torch.utils.data import DistributedSampler

import dataset_restate as DR
from d3net_amd import dataset as D
from d3net_amd import lang_prep as LP
from d3net_amd.config import default_conf

CHUNK = 3


def _entry(scene, obj, ann, n_tok=4):
    return {"scene_id": scene, "object_id": str(obj), "object_name": "chair", "ann_id": str(ann), "description": "d",
            "token": ["w%d" % ((obj + ann + t) % 5) for t in range(n_tok)]}


def _annotations():
    """scenes of 1, CHUNK, CHUNK + 1 and 2 * CHUNK descriptions, interleaved, and a SYNTHETIC entry"""
    sizes = {"scene0001_00": 1, "scene0002_00": CHUNK, "scene0003_00": CHUNK + 1, "scene0004_00": 2 * CHUNK}
    raw = [_entry(s, j % 4, j // 4) for s, n in sizes.items() for j in range(n)]
    random.Random(0).shuffle(raw)
    raw.insert(5, D.synthetic_entry("scene0005_00"))
    return raw


def _vocabulary():
    words = ["pad_", "unk", "sos", "eos"] + ["w%d" % i for i in range(5)]
    return {"word2idx": {w: i for i, w in enumerate(words)}, "idx2word": {str(i): w for i, w in enumerate(words)}}


def _index(raw, chunk=CHUNK):
    voc = _vocabulary()
    return LP.DescriptionIndex(raw, voc, np.zeros((len(voc["word2idx"]), 4), np.float32), 30, chunk, {"chair": 2})


def test_chunk_list_and_order():
    raw = _annotations()
    index = _index(raw)
    want = DR.chunked(raw, CHUNK)
    got = [[raw[n] for n in chunk] for chunk in index.chunks]
    assert got == want
    assert sorted(len(c) for c in got) == [1, 1, 1, CHUNK, CHUNK, CHUNK, CHUNK]          # 1 | SYNTHETIC | 3+1 -> 3, 1 | 3 | 6 -> 3, 3
    assert D._namespace(index, _vocabulary(), None).chunked_data == want
    assert [index.scene_id(i) for i in range(len(index))] == [c[0]["scene_id"] for c in want]
    org = D.organize(raw)
    assert "scene0005_00" not in org and sum(len(v) for objs in org.values() for v in objs.values()) == len(raw) - 1


def test_detector_speaker_listener_lists():
    raw_train, raw_val = _annotations()[:9], [e for e in _annotations()[9:] if e["object_id"] != D.SYNTHETIC]
    train_scans, val_scans = ["scene%04d_00" % i for i in (9, 3, 1)], ["scene0007_00", "scene0002_00"]
    want = DR.detector(train_scans, val_scans)
    assert D.detector_entries(train_scans) == want["train"][0] and D.detector_entries(val_scans) == want["val"][0]
    want = DR.speaker(raw_train, raw_val, [], 0.0, 1)
    assert (D.speaker_train_entries(raw_train, [], 0.0, random.Random(1)) == want["train"])
    assert D.speaker_val_entries(raw_val) == want["val"][0] and D.scan_list_of(raw_val) == want["val"][1]
    assert len(want["val"][0]) == len(set(e["scene_id"] for e in raw_val)) > 1
    assert all(e["token"] == raw_val[0]["token"] and e["object_id"] == raw_val[0]["object_id"] for e in want["val"][0])
    want = DR.listener(raw_train, raw_val)
    assert D.scan_list_of(raw_train) == want["train"][1] and D.scan_list_of(raw_val) == want["val"][1]


@pytest.mark.parametrize("ratio", [0.3, 1.5])
def test_extra_ratio_fill_under_a_fixed_seed(ratio):
    """ratio 1.5: more fill entries than unannotated scans, so the fill draws scans at random"""
    raw_train = [e for e in _annotations() if e["object_id"] != D.SYNTHETIC]
    all_scans = ["scene%04d_00" % i for i in range(1, 9)]
    for seed in (3, 4):
        want = DR.speaker(raw_train, raw_train[:1], all_scans, ratio, seed)["train"]
        got = D.speaker_train_entries(raw_train, all_scans, ratio, random.Random(seed))
        assert got[0] == want[0] and got[1] == want[1]
    n_fill = sum(e["object_id"] == D.SYNTHETIC for e in got[0])
    assert n_fill == int(len(raw_train) * ratio) and len(got[0]) == len(raw_train) + n_fill
    assert got[0][:len(raw_train)] != raw_train                                         # shuffled
    assert D.speaker_train_entries(raw_train, all_scans, ratio, random.Random(3))[0] != got[0]


def _detector_loader(n, world, rank, shuffle, seed=7, batch_size=2):
    scenes = {"s%d" % i: {"points": np.zeros((1, 3), np.float32), "feats": np.zeros((1, 3), np.float32),
                          "sem_labels": np.zeros(1), "instance_ids": np.zeros(1)} for i in range(n)}
    cfg = default_conf(overrides={"data": {"batch_size": batch_size}})
    return D.PipelineLoader(cfg, D.SceneStore.from_scenes(scenes, device="cpu"), None, "train", "detector", rank, world, seed, shuffle)


@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 5, 8])
def test_pass_order_is_the_distributed_samplers(n, world, shuffle):
    seed = 7
    per_epoch = []
    for epoch in (0, 1):
        seen = []
        for r in range(world):
            sampler = DistributedSampler(range(n), num_replicas=world, rank=r, shuffle=shuffle, seed=seed)
            sampler.set_epoch(epoch)
            loader = _detector_loader(n, world, r, shuffle, seed)
            assert loader.order(epoch) == list(sampler) == D.sampler_indices(n, world, r, shuffle, seed, epoch)
            assert len(loader) == -(-len(sampler) // 2)
            seen += loader.order(epoch)
        assert set(seen) == set(range(n))                                               # every index at least once across ranks
        per_epoch.append(seen)
    if shuffle and n > 1:
        assert per_epoch[0] != per_epoch[1]
    if not shuffle:
        assert per_epoch[0] == per_epoch[1]


def test_epoch_advances_per_pass_and_set_epoch_rewinds():
    loader = _detector_loader(8, 2, 1, True)
    loader.build = lambda idxs, rng, pyrng: list(idxs)                                   # (no device on this side)
    first, second = list(loader), list(loader)
    assert [i for b in first for i in b] == loader.order(0) and [i for b in second for i in b] == loader.order(1)
    assert first != second and len(first) == len(loader) == 2 and [len(b) for b in first] == [2, 2]
    loader.set_epoch(0)
    assert list(loader) == first and list(loader) == second
    a, b = loader.generators(0), loader.generators(0)
    assert a[0].rand() == b[0].rand() and a[1].random() == b[1].random()
    assert loader.generators(1)[0].rand() != loader.generators(0)[0].rand()
    assert _detector_loader(8, 2, 0, True).generators(0)[1].random() != loader.generators(0)[1].random()


def test_joint_pairing_cycles_the_shorter_source():
    short, long_ = ["a0", "a1", "a2"], ["b0", "b1", "b2", "b3", "b4"]
    pairs = list(D.PairedLoader(short, long_))
    assert len(pairs) == len(D.PairedLoader(short, long_)) == 5
    want = [[short[k] for _p, k in [step[0]]] + [long_[k] for _p, k in [step[1]]] for step in DR.max_size_cycle([3, 5])]
    assert pairs == want and pairs[3] == ["a0", "b3"]
    # loaders: the restarted one repeats its epoch's order, and the next epoch moves both on
    la, lb = _detector_loader(3, 1, 0, True, batch_size=1), _detector_loader(5, 1, 0, True, batch_size=1)
    for l in (la, lb):
        l.build = lambda idxs, rng, pyrng: idxs[0]
    joint = D.PairedLoader(la, lb)
    for epoch in (0, 1):
        joint.set_epoch(epoch)
        got = list(joint)
        assert [p[0] for p in got] == (la.order(epoch) * 2)[:5] and [p[1] for p in got] == lb.order(epoch)


# ------------------------------------------------------------------------------------------------ SceneStore on host arrays
def _meshes(cols=9):
    r = np.random.RandomState(0)
    out = {}
    for k, n in enumerate((5, 1, 17)):
        out["scene%04d_00" % k] = {"aligned_mesh": r.randn(n, cols).astype(np.float32), "sem_labels": r.randint(-1, 20, n).astype(np.float64),
                                   "instance_ids": r.randint(-1, 4, n).astype(np.float64)}
    return out


@pytest.mark.parametrize("color,normal,mv", [(False, True, True), (True, True, False), (True, False, False), (True, True, True)])
def test_store_packs_scenes_and_selects_feature_columns(color, normal, mv):
    meshes = _meshes()
    cfg = default_conf(overrides={"model": {"use_color": color, "use_normal": normal, "use_multiview": mv}})
    multiview = {"scene0000_00": np.random.RandomState(1).randn(5, 128), "scene0002_00": torch.ones(17, 128)}     # scene 1 is missing
    store = D.SceneStore.from_scenes(meshes, cfg, device="cpu", multiview=multiview)
    C = 3 * color + 3 * normal + 128 * mv
    assert store.scene_ids == list(meshes) and store.offsets.tolist() == [0, 5, 6, 23] and len(store) == 3
    assert store.bytes() == 23 * (3 + C + 2) * 4 and store.num_points("scene0001_00") == 1
    for sid, m in meshes.items():
        n = len(m["aligned_mesh"])
        row = None
        if mv:
            row = np.asarray(multiview[sid], np.float64) if sid in multiview else np.zeros((n, 128))
        pts, feats = DR.mesh_columns(m["aligned_mesh"].astype(np.float64), color, normal, row)
        sc = store.scene(sid)
        assert sc["points"].dtype == sc["feats"].dtype == torch.float32 and sc["sem_labels"].dtype == sc["instance_ids"].dtype == torch.int32
        np.testing.assert_array_equal(sc["points"].numpy(), pts.astype(np.float32))
        np.testing.assert_array_equal(sc["feats"].numpy(), feats.astype(np.float32))
        assert sc["feats"].shape == (n, C)
        np.testing.assert_array_equal(sc["sem_labels"].numpy(), m["sem_labels"].astype(np.int32))
        np.testing.assert_array_equal(sc["instance_ids"].numpy(), m["instance_ids"].astype(np.int32))
        assert sc["points"].data_ptr() == store.points[int(store.offsets[store.scene_ids.index(sid)])].data_ptr()       # a view, no copy
    if mv:
        assert not store.scene("scene0001_00")["feats"][:, -128:].any()                 # the placeholder of the missing scene


def test_store_takes_raw_scene_dicts_as_they_are():
    r = np.random.RandomState(2)
    scenes = {s: {"points": r.randn(n, 3).astype(np.float32), "feats": torch.from_numpy(r.randn(n, 4).astype(np.float32)),
                  "sem_labels": r.randint(-1, 20, n), "instance_ids": r.randint(-1, 3, n)} for s, n in (("a", 3), ("b", 9))}
    store = D.SceneStore.from_scenes(scenes, device="cpu")
    for sid, sc in scenes.items():
        got = store.scene(sid)
        for k in ("points", "feats", "sem_labels", "instance_ids"):
            np.testing.assert_array_equal(got[k].numpy(), np.asarray(sc[k]))
    assert "a" in store and "c" not in store
    with pytest.raises(ValueError, match="feature columns"):
        D.SceneStore.from_scenes(dict(scenes, c={"points": np.zeros((1, 3)), "feats": np.zeros((1, 5)), "sem_labels": [0], "instance_ids": [0]}),
                                 device="cpu")


def test_six_column_mesh_with_normals_is_an_error():
    cfg = default_conf(overrides={"model": {"use_color": True, "use_normal": True, "use_multiview": False}})
    with pytest.raises(ValueError, match="9"):
        D.SceneStore.from_scenes(_meshes(cols=6), cfg, device="cpu")
    cfg = default_conf(overrides={"model": {"use_color": True, "use_normal": False, "use_multiview": False}})
    assert D.SceneStore.from_scenes(_meshes(cols=6), cfg, device="cpu").feats.shape == (23, 3)


def test_loader_refuses_scenes_outside_the_store():
    raw = _annotations()
    scenes = {"scene0001_00": {"points": np.zeros((1, 3)), "feats": np.zeros((1, 3)), "sem_labels": [0], "instance_ids": [0]}}
    with pytest.raises(ValueError, match="not in the store"):
        D.PipelineLoader(default_conf(), D.SceneStore.from_scenes(scenes, device="cpu"), _index(raw), "train", "speaker")
