"""The test-split path end to end on files written the way the reference's preparation leaves them: the label-free loader's
batches against the labelled loader's over a labelled copy of the same scenes (every label-free key and every description key
equal), and `python -m d3net_amd.predict` for both tasks against an in-process `predict_captioning` / `predict_grounding` over
`dataset.build_test_loader`'s own loader with the same weights and seed."""
import json
import os

import numpy as np
import pytest
import torch

import points_prep_restate as PR
from d3net_amd import dataset as D
from d3net_amd import predict

MSA, SEEDS, OVER = PR.MSA, PR.SEEDS, PR.OVER
POINT_KEYS = {"locs", "locs_scaled", "feats", "batch_offsets", "voxel_locs", "p2v_map", "v2p_map"}
LANG_KEYS = {"lang_feat", "lang_len", "lang_ids", "annotated", "chunk_ids", "object_id", "ann_id", "object_cat", "unique_multiple", "id",
             "istrain", "scene_id"}
CONF = {"captioning": "pointgroup_captioning.yaml", "grounding": "pointgroup_grounding.yaml"}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("predict"))
    data, raw = PR.write_dataset(root)
    return root, data, raw


@pytest.mark.gpu
@pytest.mark.parametrize("task", ["captioning", "grounding"])
def test_label_free_batches_equal_the_labelled_loaders(dev, tree, task):
    """(a) a whole pass: every key of a label-free batch equals the labelled loader's over the labelled copy of the split"""
    _, data, raw = tree
    cfg = predict.task_conf(CONF[task], task, dict(OVER, DATA_PATH=data))
    loader, dataset, store = D.build_test_loader(cfg, dev, task)
    assert store.labels is False and store.sem_labels.numel() == 0 and loader.label_free
    labelled = D.SceneStore.load(cfg, "test_labelled", store.scene_ids, dev)
    assert labelled.labels and int(labelled.instance_ids.max()) > 0 and torch.equal(labelled.points, store.points)
    plain = D.PipelineLoader(cfg, labelled, loader.index, "test_labelled", loader.mode, seed=loader.seed, mean_size_arr=MSA, device=dev,
                             label_free=False)
    assert not plain.label_free and not plain.shuffle
    got, want = list(loader), list(plain)
    assert len(got) == len(want) == len(loader) == (1 if task == "captioning" else 6)
    for g, w in zip(got, want):
        assert set(g) == POINT_KEYS | LANG_KEYS and "center_label" in w and "sem_labels" in w
        for k in g:
            if torch.is_tensor(g[k]):
                assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, (k, g[k].dtype, w[k].dtype, g[k].shape, w[k].shape)
                assert torch.equal(g[k], w[k]), k
            else:
                assert g[k] == w[k], k
    assert [s for g in got for s in g["scene_id"]] == [loader.sample_scene(i) for i in range(loader.num_samples())]


def _in_process(cfg, dev, task, ckpt):
    """what `predict.main` does, spelled out: seed, loader, model, weights, submission"""
    from d3net_amd.checkpoint import load_lightning_checkpoint
    from d3net_amd.pipeline import PipelineNet
    from d3net_amd.submission import CaptionSubmission, GroundingSubmission
    torch.manual_seed(cfg.general.manual_seed)
    loader, dataset, store = D.build_test_loader(cfg, dev, task)
    net = PipelineNet(cfg, dataset).to(dev)
    if ckpt is None:
        return net
    load_lightning_checkpoint(net, ckpt, strict=False)
    chunked = dataset["test"].chunked_data
    if task == "captioning":
        sub = CaptionSubmission(chunked, net.vocabulary, max_proposals=cfg.model.max_num_proposal, max_len=cfg.data.max_spk_len + 1, device=dev)
        return net.predict_captioning(loader, sub).results(), loader
    return net.predict_grounding(loader, GroundingSubmission(chunked, device=dev)).results(), loader


def _cli(dev, tree, task, run):
    root, data, raw = tree
    over = dict(OVER, DATA_PATH=data)
    cfg = predict.task_conf(CONF[task], task, over)
    run = os.path.join(root, run)
    os.makedirs(run)
    ckpt = os.path.join(run, "model.ckpt")
    torch.save({"state_dict": _in_process(cfg, dev, task, None).state_dict()}, ckpt)       # seeded random-init weights
    want, loader = _in_process(cfg, dev, task, ckpt)
    sub = predict.main(["-c", CONF[task], "--task", task, "--root", run], overrides=over)
    path = predict.default_output(run, task, "test")
    assert os.path.exists(path)
    return json.load(open(path)), want, sub, loader, raw["test"]


@pytest.mark.gpu
def test_captioning_cli_writes_the_in_process_file(dev, tree):
    """(b) `predict.main --task captioning` with `<root>/model.ckpt` from a seeded random-init PipelineNet: the file equals
    `CaptionSubmission.results()` of the in-process run after the same seed, its scenes are the test scenes in loader order, and
    the in-process run keeps at least one proposal per scene (with these random-init weights, no teacher switch)"""
    got, want, sub, loader, raw = _cli(dev, tree, "captioning", "cap")
    assert all(len(v) > 0 for v in want.values())
    assert got == json.loads(json.dumps(want)) and sub.results() == want
    assert list(got) == [loader.sample_scene(i) for i in range(loader.num_samples())] == sorted("scene%04d_00" % s for s in SEEDS)
    assert all(set(rec) == {"caption", "box", "sem_prob", "obj_prob"} for v in got.values() for rec in v)


@pytest.mark.gpu
def test_grounding_cli_writes_the_in_process_file(dev, tree):
    """(c) the same for `--task grounding`: pred.json equals the in-process `GroundingSubmission.results()` and lists every
    annotation of the split exactly once"""
    got, want, sub, loader, raw = _cli(dev, tree, "grounding", "ground")
    assert got == json.loads(json.dumps(want)) and sub.results() == want
    keys = [(g["scene_id"], g["object_id"], g["ann_id"]) for g in got]
    assert len(keys) == len(set(keys)) == len(raw) and set(keys) == {(a["scene_id"], a["object_id"], a["ann_id"]) for a in raw}
    boxes = np.asarray([g["bbox"] for g in got], np.float32)
    assert boxes.shape == (len(raw), 8, 3) and np.isfinite(boxes).all() and np.abs(boxes).max() > 0        # some proposal exists
