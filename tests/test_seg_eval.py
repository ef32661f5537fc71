"""d3net_amd.seg_eval's host matching / AP / IoU against the reference's own segmentation evaluators (golden:
tests/golden/seg_eval_golden.npz from lib/evaluation/instance_segmentation.py + semantic_segmentation.py), fed with counts
computed here in numpy; and its file writers / readers against the reference's formats."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))


def numpy_counts(sc, round_scores=True):
    """the per-scene counts of assign_instances_for_scene / get_instances / build_confusion_for_scene, restated with dense numpy
    masks: the same dict SegmentationEvaluator keeps per scene (+ the scene's confusion)"""
    from d3net_amd import seg_eval as SE
    gs, gi, ps = sc["gt_sem"], sc["gt_inst"], sc["pred_sem"]
    G = int(gi.max()) if len(gi) else 0
    gt_vert = np.array([(gi == k).sum() for k in range(1, G + 1)], np.int64)
    gt_cls = np.array([np.argmax(np.bincount(gs[gi == k])) if (gi == k).any() else 0 for k in range(1, G + 1)], np.int64)
    void = ~np.isin(gs, SE.INST_CLASS_IDX)
    masks = []
    for m in sc["members"]:
        mk = np.zeros(len(gs), bool)
        mk[m] = True
        masks.append(mk)
    inter = np.array([[np.count_nonzero(mk & (gi == k)) for k in range(1, G + 1)] for mk in masks], np.int64).reshape(len(masks), G)
    conf = np.zeros((SE.NUM_IDS, SE.NUM_IDS), np.int64)
    np.add.at(conf, (gs, ps), 1)
    return dict(gt_vert=gt_vert, gt_cls=gt_cls, pred_vert=np.array([mk.sum() for mk in masks], np.int64),
                pred_void=np.array([np.count_nonzero(mk & void) for mk in masks], np.int64), pred_cls=np.asarray(sc["classes"]),
                pred_conf=[SE.round_score(s) if round_scores else float(s) for s in sc["scores"]], inter=inter, confusion=conf)


def check_against_golden(avgs, ap, ious, confusion):
    from d3net_amd import seg_eval as SE
    g = np.load(os.path.join(HERE, "golden", "seg_eval_golden.npz"))
    assert ap.shape == g["ap"].shape == (1, len(SE.INST_CLASS_IDX), 10)
    assert np.array_equal(np.isnan(ap), np.isnan(g["ap"]))
    ok = ~np.isnan(ap)
    assert np.abs(ap[ok] - g["ap"][ok]).max() <= 1e-12
    for k, gk in (("all_ap", "all_ap"), ("all_ap_50%", "all_ap_50"), ("all_ap_25%", "all_ap_25")):
        assert abs(avgs[k] - float(g[gk])) <= 1e-12, k
    cls = np.array([[avgs["classes"][n][k] for k in ("ap", "ap50%", "ap25%")] for n in SE.INST_CLASS_NAME])
    assert np.array_equal(np.isnan(cls), np.isnan(g["class_ap"]))
    assert np.abs(cls[~np.isnan(cls)] - g["class_ap"][~np.isnan(cls)]).max() <= 1e-12
    assert np.array_equal(confusion, g["confusion"])
    for i, name in enumerate(SE.SEM_CLASS_NAME):
        r = ious[name]
        if np.isnan(g["iou"][i]):
            assert isinstance(r, float) and np.isnan(r), name
        else:
            assert abs(r[0] - g["iou"][i]) <= 1e-12 and [int(r[1]), int(r[2])] == g["iou_tp_denom"][i].tolist(), name


def test_golden_reaches_every_branch():
    """the golden case is not degenerate: NaN classes (no GT), a 0.0 class (GT, no prediction), a NaN IoU, AP@50 != AP@25"""
    from d3net_amd import seg_eval as SE
    g = np.load(os.path.join(HERE, "golden", "seg_eval_golden.npz"))
    assert np.isnan(g["class_ap"][:, 0]).any() and (g["class_ap"][SE.INST_CLASS_IDX.index(39)] == 0).all()
    assert np.isnan(g["iou"][SE.SEM_CLASS_IDX.index(36)]) and 0.1 < float(g["all_ap"]) < 0.9
    assert float(g["all_ap_50"]) != float(g["all_ap_25"])


def test_host_matching_ap_iou_match_reference():
    from gen_seg_eval_golden import seg_eval_inputs
    from d3net_amd import seg_eval as SE
    scenes = [numpy_counts(sc) for sc in seg_eval_inputs()]
    ap = SE.evaluate_matches(scenes)
    confusion = sum(s["confusion"] for s in scenes)
    check_against_golden(SE.compute_averages(ap), ap, SE.semantic_iou(confusion), confusion)


def test_average_precision_steps():
    """two true positives above one false positive, one hard false negative: precision / recall curve integrated by hand"""
    from d3net_amd import seg_eval as SE
    ap = SE._average_precision(np.array([1., 1., 0.]), np.array([0.9, 0.8, 0.7]), 1)
    # thresholds 0.7 / 0.8 / 0.9: (p, r) = (2/3, 2/3), (1, 2/3), (1, 1/3), then (1, 0); step widths 0, 1/6, 1/3, 1/6
    assert abs(ap - (2 / 3 * 0 + 1 * (1 / 6) + 1 * (1 / 3) + 1 * (1 / 6))) < 1e-15
    assert SE._average_precision(np.zeros(0), np.zeros(0), 2) == 0.0


def _batch_and_pred():
    """a 2-scene collated batch and a predict_instances-shaped output, on the CPU"""
    rng = np.random.default_rng(3)
    n0, n1 = 300, 250
    sem = rng.integers(-1, 20, n0 + n1)
    inst = np.full(n0 + n1, -1)
    inst[10:60], inst[100:220], inst[n0 + 5:n0 + 140] = 0, 1, 2      # collated ids run on across scenes
    data = dict(sem_labels=torch.from_numpy(sem), instance_ids=torch.from_numpy(inst),
                batch_offsets=torch.tensor([0, n0, n0 + n1], dtype=torch.int32), instance_offsets=torch.tensor([0, 2, 3]))
    members = [np.arange(100, 210), np.arange(n0 + 5, n0 + 150), np.arange(5, 40)]
    idx = np.concatenate([np.stack([np.full(len(m), j), m], 1) for j, m in enumerate(members)]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
    sp = rng.integers(0, 20, n0 + n1)
    for m in members:
        sp[m] = sp[m[0]]
    pred = dict(pick=torch.tensor([1, 0, 2]), scores=torch.tensor([0.91234, 0.5, 0.123449], dtype=torch.float32),
                proposals_idx=torch.from_numpy(idx), proposals_offset=torch.from_numpy(off), semantic_pred=torch.from_numpy(sp))
    return data, pred, members, sem, inst, sp


def test_writers_produce_reference_formats(tmp_path):
    from d3net_amd import seg_eval as SE
    data, pred, members, sem, inst, sp = _batch_and_pred()
    SE.write_predictions(pred, data, str(tmp_path), ["sceneA", "sceneB"])
    SE.write_gt(data, str(tmp_path), ["sceneA", "sceneB"])
    base = tmp_path / "split_pred" / "val"
    lut = np.array(SE.SEM_CLASS_IDX)
    # semantic: one raw class id per point of the scene
    assert (base / "semantic" / "sceneA.txt").read_text().split("\n")[:3] == [str(v) for v in lut[sp[:3]]]
    assert np.array_equal(SE.read_ids(str(base / "semantic" / "sceneB.txt")), lut[sp[300:]])
    # instance list: pick order within each scene, class of the cluster, score with 4 decimals
    la = (base / "instance" / "sceneA.txt").read_text().splitlines()
    lb = (base / "instance" / "sceneB.txt").read_text().splitlines()
    assert la == ["predicted_masks/sceneA_000.txt %d 0.5000" % lut[sp[100]], "predicted_masks/sceneA_001.txt %d 0.1234" % lut[sp[5]]]
    assert lb == ["predicted_masks/sceneB_000.txt %d 0.9123" % lut[sp[305]]]
    m0 = SE.read_ids(str(base / "instance" / "predicted_masks" / "sceneA_000.txt"))
    assert len(m0) == 300 and np.array_equal(np.nonzero(m0)[0], members[0])
    cid = SE.read_ids(str(base / "instance" / "sceneA.cluster_ids.txt"))
    exp = np.full(300, -1); exp[members[0]] = 0; exp[members[2]] = 1
    assert np.array_equal(cid, exp)
    parsed = SE.read_instance_predictions(str(base / "instance" / "sceneA.txt"))
    assert [(os.path.basename(p), c, s) for p, c, s in parsed] == [("sceneA_000.txt", int(lut[sp[100]]), 0.5),
                                                                  ("sceneA_001.txt", int(lut[sp[5]]), 0.1234)]
    # GT: NYU20 class id of the label (0 for the ignore label) * 1000 + 1-based scene-local instance id
    gsem, ginst = SE.read_gt(str(tmp_path / "split_gt" / "val" / "sceneB.txt"))
    s = sem[300:]
    assert np.array_equal(gsem, np.where(s >= 0, lut[np.clip(s, 0, 19)], 0))
    assert np.array_equal(ginst, np.where(inst[300:] >= 0, inst[300:] - 2 + 1, 0))
    assert set(np.unique(SE.read_gt(str(tmp_path / "split_gt" / "val" / "sceneA.txt"))[1]).tolist()) == {0, 1, 2}


def test_gt_ids_without_instance_offsets():
    """a batch without instance_offsets (the synthetic collate) numbers each scene's instances from its smallest id"""
    from d3net_amd import seg_eval as SE
    data, _, _, _, inst, _ = _batch_and_pred()
    del data["instance_offsets"]
    _, local = SE.gt_ids(data)
    assert np.array_equal(local.numpy(), np.where(inst >= 0, inst - np.where(np.arange(len(inst)) < 300, 0, 2) + 1, 0))
