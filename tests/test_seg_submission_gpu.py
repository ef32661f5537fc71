"""seg_submission.SegmentationSubmission on the GPU: every file it writes is byte-equal to `seg_eval.write_predictions` /
`write_gt` over the same inputs -- synthetic predict_instances-shaped dicts at the sizes where the line kernels change path, the
model's own predictions, and `python -m d3net_amd.predict --task segmentation` against the in-process run."""
import os
import pathlib

import numpy as np
import pytest
import torch

import points_prep_restate as PR
from d3net_amd import _lib, predict
from d3net_amd import seg_eval as SE
from d3net_amd import seg_submission as SS

pytestmark = pytest.mark.gpu
T = SS.TILE_LINES
SCORES = (0.91234, 0.5, 0.123449, 0.99995, 1e-5, 1.0)
# scene sizes and picks per scene (0, 1, 11 and 101 picks: scene-local ids of 1, 2 and 3 digits)
CASES = {"one_point": ([1], [1]), "wave": ([64, 65], [11, 0]), "block": ([255, 256, 257], [1, 101, 11]),
         "multi_tile": ([2500, 300, 2049], [11, 1, 101]), "empty_scene": ([300, 0, 200], [11, 0, 1]),
         "tile_edges": ([T - 1, T, T + 1], [0, 11, 101]), "no_picks": ([64, 65], [0, 0])}


def _tree(root):
    root = pathlib.Path(root)
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def _synthetic(sizes, picks, seed=0):
    """a predict_instances-shaped dict on the host: proposals of a few points each, picked and unpicked, in shuffled order over the
    scenes; the picks interleave scenes; one picked proposal is empty; where a scene has three picks and eight points its first
    three share a point and the first two another; the predicted classes cover the whole LUT"""
    rng = np.random.default_rng(seed)
    bo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(bo[-1])
    sp = (np.arange(N) + seed) % 20
    rng.shuffle(sp)
    members, picked = [], []
    for b, (n, k) in enumerate(zip(sizes, picks)):
        mine = []
        for j in range(k + 2 if n else 0):                 # two unpicked proposals per scene with points
            m = bo[b] + rng.choice(n, size=min(n, int(rng.integers(1, 6))), replace=False)
            mine.append(m)
            if j < k:
                picked.append(len(members) + j)
        if k >= 3 and n >= 8:
            x, y = bo[b] + rng.choice(n, size=2, replace=False)
            for j in range(3):
                mine[j] = np.concatenate([mine[j][:1], [x], mine[j][1:]])
            for j in range(2):
                mine[j] = np.concatenate([mine[j], [y]])
        members += mine
    members.append(np.zeros(0, np.int64))                  # the empty proposal, picked
    picked.append(len(members) - 1)
    order = rng.permutation(len(members))                  # proposal numbers do not follow the scenes
    rank = np.argsort(order)
    members = [members[i] for i in order]
    pick = rank[np.asarray(picked, np.int64)]
    rng.shuffle(pick)
    idx = np.concatenate([np.stack([np.full(len(m), j), m], 1) for j, m in enumerate(members)] + [np.zeros((0, 2), np.int64)]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
    scores = np.asarray([SCORES[i % len(SCORES)] for i in range(len(pick))], np.float32)
    pred = dict(pick=torch.from_numpy(pick), scores=torch.from_numpy(scores), proposals_idx=torch.from_numpy(idx),
                proposals_offset=torch.from_numpy(off), semantic_pred=torch.from_numpy(sp))
    return pred, dict(batch_offsets=torch.from_numpy(bo.astype(np.int32))), ["scene%04d_00" % (7 * b) for b in range(len(sizes))]


_reference = {}


def _reference_tree(case, tmp_path_factory):
    """the case's inputs and the tree `seg_eval.write_predictions` writes for them, made once"""
    if case not in _reference:
        pred, data, names = _synthetic(*CASES[case], seed=list(CASES).index(case))
        root = tmp_path_factory.mktemp("host_" + case)
        SE.write_predictions(pred, data, str(root), names)
        _reference[case] = (pred, data, names, _tree(root))
    return _reference[case]


def _on(dev, d):
    return {k: v.to(dev) if torch.is_tensor(v) else v for k, v in d.items()}


def _assert_same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k


@pytest.mark.parametrize("case", list(CASES))
def test_files_equal_write_predictions(dev, case, tmp_path, tmp_path_factory):
    pred, data, names, want = _reference_tree(case, tmp_path_factory)
    sizes, picks = CASES[case]
    # what the case is there for: ids of every digit count, overlaps of two and three picks, the empty pick, all classes
    assert len(want) == 3 * len(sizes) + sum(picks) and len(pred["pick"]) == sum(picks) + 1
    if max(picks) == 101:
        assert any(k.endswith("_100.txt") for k in want)
        cid = np.array(want["split_pred/val/instance/%s.cluster_ids.txt" % names[picks.index(101)]].split(), np.int64)
        assert cid.max() >= 2 and (cid == -1).any()
    timings = {}
    sub = SS.SegmentationSubmission(str(tmp_path), device=dev, timings=timings)
    sub.add_batch(_on(dev, pred), _on(dev, data), names)
    _assert_same(_tree(tmp_path), want)
    assert sorted(sub.files()) == sorted(want) and len(set(sub.files())) == len(sub.files())
    assert timings["device_s"] > 0 and timings["files_s"] > 0


def test_overlaps_and_classes_are_exercised():
    """the synthetic case holds what the issue asks for: points in two and in three picked proposals, every LUT entry predicted"""
    pred, data, names = _synthetic(*CASES["multi_tile"], seed=3)
    idx, off, pick = (pred[k].numpy() for k in ("proposals_idx", "proposals_offset", "pick"))
    hits = np.zeros(len(pred["semantic_pred"]), np.int64)
    for c in pick:
        np.add.at(hits, np.unique(idx[off[c]:off[c + 1], 1]), 1)
    assert (hits == 2).any() and (hits >= 3).any()
    assert set(pred["semantic_pred"].numpy().tolist()) == set(range(20))
    assert any(off[c] == off[c + 1] for c in pick) and len(pick) < len(off) - 1
    first_scene = np.searchsorted(data["batch_offsets"].numpy(), [idx[off[c], 1] for c in pick if off[c] < off[c + 1]], side="right")
    assert (np.diff(first_scene) < 0).any()                # the picks interleave the scenes


def test_small_chunks_write_the_same_files(dev, tmp_path, tmp_path_factory):
    """chunk_bytes=4096: six mask files of the 300-point scene per chunk, every mask of the 2500- and 2049-point scenes (5000 and
    4098 bytes, larger than a chunk) alone"""
    pred, data, names, want = _reference_tree("multi_tile", tmp_path_factory)
    assert SS.plan_chunks(11, 2500, 4096) == [(c, 1) for c in range(11)] and SS.plan_chunks(101, 2049, 4096)[-1] == (100, 1)
    sub = SS.SegmentationSubmission(str(tmp_path), chunk_bytes=4096, device=dev)
    sub.add_batch(_on(dev, pred), _on(dev, data), names)
    _assert_same(_tree(tmp_path), want)
    # a chunk between the two: several proposals of every scene per chunk, the last chunk of a scene short
    sub = SS.SegmentationSubmission(str(tmp_path / "again"), chunk_bytes=30000, device=dev)
    sub.add_batch(_on(dev, pred), _on(dev, data), names)
    _assert_same(_tree(tmp_path / "again"), want)


def test_a_second_batch_and_a_rewritten_scene(dev, tmp_path, tmp_path_factory):
    """two batches into one tree as the host route writes them; a scene written again is replaced and its older mask files stay"""
    a = _reference_tree("block", tmp_path_factory)
    b = _reference_tree("wave", tmp_path_factory)
    host = tmp_path / "host"
    sub = SS.SegmentationSubmission(str(tmp_path / "dev"), device=dev)
    for pred, data, names, _ in (a, b):                    # "wave" names scene0000_00 and scene0007_00 again, with fewer picks
        SE.write_predictions(pred, data, str(host), names)
        sub.add_batch(_on(dev, pred), _on(dev, data), names)
    _assert_same(_tree(tmp_path / "dev"), _tree(host))
    assert "split_pred/val/instance/predicted_masks/scene0007_00_100.txt" in _tree(host)


def _labelled(sizes, with_offsets, seed):
    rng = np.random.default_rng(seed)
    bo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(bo[-1])
    sem = rng.integers(0, 20, N)
    sem[rng.random(N) < 0.2] = -1                          # the ignore label
    sem[rng.random(N) < 0.05] = -100
    inst = np.full(N, -1, np.int64)
    ioff, base = [0], 0
    for b, n in enumerate(sizes):
        local = np.full(n, -1, np.int64)
        if n and b != 1:                                   # scene 1 has no instance; the others ids with gaps (1, 4, 5 .. never 0, 2, 3)
            local = rng.choice(np.array([-1, 1, 4, 5, 12]), n)
            local[0] = 1                                   # (the smallest id is present: without instance_offsets it is the base)
        inst[bo[b]:bo[b + 1]] = np.where(local >= 0, local + base, -1)
        base += 13 if n and b != 1 else 0
        ioff.append(base)
    data = dict(sem_labels=torch.from_numpy(sem), instance_ids=torch.from_numpy(inst), batch_offsets=torch.from_numpy(bo.astype(np.int32)))
    if with_offsets:
        data["instance_offsets"] = torch.tensor(ioff, dtype=torch.int32)
    return data, ["scene%04d_01" % b for b in range(len(sizes))]


@pytest.mark.parametrize("with_offsets", [True, False])
def test_gt_files_equal_write_gt(dev, tmp_path, with_offsets):
    data, names = _labelled([T + 1, 300, 0, 65], with_offsets, seed=5)
    data = _on(dev, data)
    SE.write_gt(data, str(tmp_path / "host"), names)
    sub = SS.SegmentationSubmission(str(tmp_path / "dev"), device=dev)
    sub.add_gt(data, names)
    want = _tree(tmp_path / "host")
    _assert_same(_tree(tmp_path / "dev"), want)
    assert sub.files() == ["split_gt/val/%s.txt" % n for n in names]
    values = np.concatenate([np.loadtxt(tmp_path / "dev" / f, dtype=np.int64, ndmin=1) for f in sub.files() if want[f]])
    assert (values == 0).any() and (values % 1000 == 0).any() and (values // 1000 == 39).any() and (values % 1000 > 4).any()
    assert want["split_gt/val/%s.txt" % names[2]] == b"" and set(np.unique(values % 1000)) <= ({0, 2, 5, 6, 13} if with_offsets else {0, 1, 4, 5, 12})


def test_a_class_outside_the_lut_raises(dev, tmp_path, tmp_path_factory):
    pred, data, names, _ = _reference_tree("wave", tmp_path_factory)
    pred = _on(dev, pred)
    pred["semantic_pred"] = pred["semantic_pred"].clone()
    pred["semantic_pred"][70] = 20
    sub = SS.SegmentationSubmission(str(tmp_path), device=dev)
    with pytest.raises(_lib.D3Error, match="semantic_pred outside"):
        sub.add_batch(pred, _on(dev, data), names)
    assert sub.files() == [] and not _tree(tmp_path)


# ------------------------------------------------------------------------------------------------ the model's own predictions
def _model_and_batch(dev, n_scenes):
    from d3net_amd import synthetic as S
    from d3net_amd.config import default_conf
    from d3net_amd.pointgroup import PointGroup
    cfg = default_conf(overrides={"model": {"blocks": [1, 2, 3]}})
    torch.manual_seed(0)
    model = PointGroup(cfg).to(dev).eval()
    model.teacher = True
    with torch.no_grad():
        model.score_linear.bias.fill_(4.0)
    scenes = [S.small_scene(dims=(44, 36, 20), n_boxes=4, seed=3), S.small_scene(dims=(40, 40, 20), n_boxes=3, seed=5)][:n_scenes]
    return model, S.make_batch(scenes, dev)


@pytest.mark.parametrize("n_scenes", [1, 2])
def test_predict_segmentation_writes_the_recorded_predictions(dev, tmp_path, n_scenes):
    model, batch = _model_and_batch(dev, n_scenes)
    gt = {k: batch[k].clone() for k in ("sem_labels", "instance_ids", "batch_offsets", "instance_offsets") if k in batch}
    recorded, orig = [], model.predict_instances
    model.predict_instances = lambda b: recorded.append(orig(b)) or recorded[-1]
    model.train()
    if n_scenes == 1:                                      # names from the batch's scene_id
        names = batch["scene_id"] = ["scene0042_00"]
    else:                                                  # or from scene_names, one list per batch
        names = ["scene_a", "scene_b"]
        with pytest.raises(ValueError, match="scene_names"):
            model.predict_segmentation([batch], SS.SegmentationSubmission(str(tmp_path / "none"), device=dev))
        assert not recorded and model.training
    sub = SS.SegmentationSubmission(str(tmp_path / "dev"), device=dev)
    assert model.predict_segmentation([batch], sub, scene_names=[names] if n_scenes == 2 else None, with_gt=True) is sub
    assert model.training and len(recorded) == 1 and model.cfg.general.task != "test"
    pred = recorded[0]
    assert len(pred["pick"]) >= 1
    SE.write_predictions(pred, gt, str(tmp_path / "host"), names)
    SE.write_gt(gt, str(tmp_path / "host"), names)
    want = _tree(tmp_path / "host")
    _assert_same(_tree(tmp_path / "dev"), want)
    assert sorted(sub.files()) == sorted(want)
    # the new files through the file evaluator equal the in-memory evaluator on the recorded predictions
    ev = SE.SegmentationEvaluator()
    ev.add_batch(pred, gt)
    ap = ev.instance_results()[1]
    base = tmp_path / "dev" / "split_pred" / "val" / "instance"
    _, f_ap = SE.evaluate_instance_files([str(base / (n + ".txt")) for n in names],
                                         [str(tmp_path / "dev" / "split_gt" / "val" / (n + ".txt")) for n in names], device=dev)
    assert np.array_equal(np.isnan(f_ap), np.isnan(ap)) and np.array_equal(f_ap[~np.isnan(f_ap)], ap[~np.isnan(ap)])


# ------------------------------------------------------------------------------------------------ the command
def test_segmentation_cli_writes_the_in_process_tree(dev, tmp_path):
    from d3net_amd.checkpoint import load_lightning_checkpoint
    from d3net_amd.pipeline import PipelineNet
    data, _ = PR.write_dataset(str(tmp_path))
    from d3net_amd import synthetic
    scenes = sorted("scene%04d_00" % s for s in PR.SEEDS)
    points = {"scene%04d_00" % s: len(synthetic.small_scene(dims=(40, 32, 20), n_boxes=3, seed=s)["locs"]) for s in PR.SEEDS}
    with open(os.path.join(data, "scannet", "meta_data", "scannetv2_test.txt"), "w") as f:
        f.write("".join(s + "\n" for s in scenes[::-1]))   # the list names the later scene first
    over = dict(PR.OVER, DATA_PATH=data)
    over["data"] = dict(over["data"], batch_size=1)        # two batches
    cfg = predict.task_conf("pointgroup.yaml", "segmentation", over)
    run = tmp_path / "run"
    run.mkdir()
    torch.manual_seed(cfg.general.manual_seed)
    torch.save({"state_dict": PipelineNet(cfg).to(dev).state_dict()}, str(run / "model.ckpt"))      # seeded random-init weights

    torch.manual_seed(cfg.general.manual_seed)
    loader, store = predict.segmentation_loader(cfg, dev)
    assert store.labels is False and loader.label_free and len(loader) == 2
    net = PipelineNet(cfg).to(dev)
    load_lightning_checkpoint(net, str(run / "model.ckpt"), strict=False)
    want_sub = SS.SegmentationSubmission(str(tmp_path / "in_process"), split="test", device=dev)
    batches = iter(loader)
    names = predict.batch_scene_names(loader)
    assert names == [[s] for s in scenes[::-1]]
    net.predict_segmentation(batches, want_sub, scene_names=names)

    sub = predict.main(["--task", "segmentation", "--root", str(run)], overrides=over)
    want = _tree(tmp_path / "in_process")
    got = {k: v for k, v in _tree(run).items() if k != "model.ckpt"}
    _assert_same(got, want)
    assert sub.files() == want_sub.files() and sorted(sub.files()) == sorted(want)
    for s in scenes:                                       # every scene of the split, whether anything was picked or not
        assert "split_pred/test/semantic/%s.txt" % s in got and "split_pred/test/instance/%s.cluster_ids.txt" % s in got
        lines = got["split_pred/test/semantic/%s.txt" % s].splitlines()
        assert len(lines) == len(got["split_pred/test/instance/%s.cluster_ids.txt" % s].splitlines()) == points[s]
        assert set(int(x) for x in lines) <= set(SE.SEM_CLASS_IDX)
    out = tmp_path / "elsewhere"
    predict.main(["--task", "segmentation", "--root", str(run), "--out", str(out)], overrides=over)
    _assert_same(_tree(out), want)
