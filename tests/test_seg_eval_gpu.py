"""csrc/seg_eval.hip (d3_seg_eval) on the device: counts bit-equal to numpy on the golden scenes, edge scenes and a bench-sized
batch; the LDS bound; the full evaluator and the file route against the reference's golden numbers; and
PointGroup.evaluate_segmentation against a dense-mask numpy restatement."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu


def _batch(scenes):
    """scenes (golden-style dicts) -> one concatenated batch: per-point arrays, offsets, proposal lists, pick (all proposals,
    in order)"""
    bo = np.concatenate([[0], np.cumsum([len(s["gt_sem"]) for s in scenes])]).astype(np.int64)
    members = [np.asarray(m, np.int64) + bo[b] for b, s in enumerate(scenes) for m in s["members"]]
    off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
    idx = np.zeros((int(off[-1]), 2), np.int64)
    for j, m in enumerate(members):
        idx[off[j]:off[j + 1], 0], idx[off[j]:off[j + 1], 1] = j, m
    cat = lambda k: np.concatenate([s[k] for s in scenes]) if bo[-1] else np.zeros(0, np.int64)
    return dict(gt_sem=cat("gt_sem"), gt_inst=cat("gt_inst"), pred_sem=cat("pred_sem"), bo=bo, members=members, idx=idx, off=off)


def _numpy_counts(bt):
    """vectorised numpy restatement of every output of d3_seg_eval for a batch"""
    from d3net_amd import seg_eval as SE
    gs, gi, ps, bo = bt["gt_sem"], bt["gt_inst"], bt["pred_sem"], bt["bo"]
    B, G = len(bo) - 1, (int(bt["gt_inst"].max()) if len(gi) else 0)
    scene = np.repeat(np.arange(B), np.diff(bo))
    conf = np.zeros((SE.NUM_IDS, SE.NUM_IDS), np.int64)
    np.add.at(conf, (gs, ps), 1)
    h = np.zeros((B, G + 1, SE.NUM_IDS), np.int64)
    np.add.at(h, (scene, gi, gs), 1)
    h = h[:, 1:]
    gt_vert, gt_cls = h.sum(2), h.argmax(2)
    n = len(bt["members"])
    pred = np.zeros((n, 5), np.int64)
    inter = np.zeros((n, G + 1), np.int64)
    void = ~np.isin(gs, SE.INST_CLASS_IDX)
    for j, m in enumerate(bt["members"]):
        pred[j, 0] = len(m)
        if len(m) == 0:
            pred[j, 2:4] = -1
            continue
        pred[j, 1] = void[m].sum()
        pred[j, 2], pred[j, 3] = ps[m[0]], scene[m[0]]
        pred[j, 4] = int((ps[m] != ps[m[0]]).any())
        np.add.at(inter[j], gi[m], 1)
    return dict(confusion=conf, gt_vert=gt_vert, gt_cls=gt_cls, pred=pred, inter=inter[:, 1:])


def _device_counts(bt, dev, pick=None):
    from d3net_amd import seg_eval as SE
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = len(bt["members"])
    return SE.count(t(bt["gt_sem"]), t(bt["gt_inst"]), t(bt["pred_sem"]), bt["bo"], t(np.arange(n) if pick is None else pick),
                    t(bt["idx"]), t(bt["off"]))


def _assert_equal_counts(got, exp):
    for k in ("confusion", "gt_vert", "gt_cls", "pred", "inter"):
        assert got[k].shape == exp[k].shape and np.array_equal(got[k], exp[k]), k


def _golden_check(*a):
    from test_seg_eval import check_against_golden
    check_against_golden(*a)


def test_device_counts_golden_scenes(dev):
    from gen_seg_eval_golden import seg_eval_inputs
    scenes = seg_eval_inputs()
    bt = _batch(scenes)
    got = _device_counts(bt, dev)
    _assert_equal_counts(got, _numpy_counts(bt))
    assert (got["pred"][:, 4] == 1).any() and got["inter"].max() > 0      # mixed-class members are flagged, not an error


def _edge_scene(rng, N, G, n_pred, two=False):
    gt_sem = rng.choice([0, 1, 2, 3, 5, 39], size=N)
    gt_inst = np.zeros(N, np.int64)
    if G:
        gt_inst[:] = rng.integers(0, G + 1, N)
        gt_inst[rng.permutation(N)[:G]] = np.arange(1, G + 1)            # every id present
    pred_sem = rng.choice([1, 3, 5, 39], size=N)
    members = [rng.permutation(N)[:int(rng.integers(1, max(2, N // 3)))] for _ in range(n_pred)]
    if two and n_pred >= 2:
        members[1] = np.concatenate([members[1], members[0][:5]])       # points in two predictions
        members[1] = np.unique(members[1])
    return dict(gt_sem=gt_sem, gt_inst=gt_inst, pred_sem=pred_sem, members=members)


def test_device_counts_edge_scenes(dev):
    from d3net_amd import _lib
    rng = np.random.default_rng(11)
    gmax = _lib.lib().d3_seg_eval_max_inst()
    cases = [
        [_edge_scene(rng, 500, 4, 0)],                                           # no picks
        [_edge_scene(rng, 300, 3, 2), _edge_scene(rng, 0, 0, 0), _edge_scene(rng, 400, 5, 3, two=True)],   # an empty scene
        [_edge_scene(rng, 2000, 7, 4, two=True)],                                # a point in two picks
        [_edge_scene(rng, 3000, gmax, 5), _edge_scene(rng, 1000, 10, 2)],        # GT count at the LDS bound
        [_edge_scene(rng, 800, 0, 3)],                                           # no GT instances at all
    ]
    for scenes in cases:
        bt = _batch(scenes)
        _assert_equal_counts(_device_counts(bt, dev), _numpy_counts(bt))


def test_device_counts_bench_sized_batch(dev):
    """4 scenes of 150 k points (the bench's size), ~100 instances and ~150 predictions each, pick order shuffled"""
    rng = np.random.default_rng(12)
    scenes = []
    for _ in range(4):
        N, G = 150_000 + int(rng.integers(0, 5000)), int(rng.integers(80, 120))
        inst = rng.integers(0, G + 1, N)
        sem = np.where(inst > 0, rng.choice([3, 4, 5, 7, 14, 39], size=N), rng.choice([0, 1, 2], size=N))
        members = []
        for _ in range(int(rng.integers(120, 180))):                      # cliques: most members inside one instance
            k = int(rng.integers(1, G + 1))
            core = np.nonzero(inst == k)[0]
            m = np.unique(np.concatenate([core[rng.random(len(core)) < 0.8], rng.integers(0, N, int(rng.integers(0, 200)))]))
            members.append(rng.permutation(m))
        scenes.append(dict(gt_sem=sem, gt_inst=inst, pred_sem=np.where(rng.random(N) < 0.9, np.maximum(sem, 1), 5), members=members))
    bt = _batch(scenes)
    assert bt["bo"][-1] >= 600_000
    pick = rng.permutation(len(bt["members"]))
    got = _device_counts(bt, dev, pick)
    exp = _numpy_counts(dict(bt, members=[bt["members"][j] for j in pick]))
    _assert_equal_counts(got, exp)
    got2 = _device_counts(bt, dev, pick)
    _assert_equal_counts(got2, got)                                        # deterministic


def test_over_the_lds_bound_raises_range(dev):
    from d3net_amd import _lib
    rng = np.random.default_rng(13)
    g = _lib.lib().d3_seg_eval_max_inst() + 1
    bt = _batch([_edge_scene(rng, 2000, g, 3)])
    with pytest.raises(_lib.D3Error, match="D3_ERR_RANGE"):
        _device_counts(bt, dev)
    # and the library is still usable afterwards
    bt = _batch([_edge_scene(rng, 200, 3, 1)])
    _assert_equal_counts(_device_counts(bt, dev), _numpy_counts(bt))


def test_evaluator_on_golden_inputs_matches_reference(dev):
    from gen_seg_eval_golden import seg_eval_inputs
    from d3net_amd import seg_eval as SE
    ev = SE.SegmentationEvaluator()
    for sc in seg_eval_inputs():
        ev.add_scene(sc["gt_sem"], sc["gt_inst"], sc["pred_sem"], sc["members"], sc["scores"], sc["classes"], device=dev)
    avgs, ap = ev.instance_results()
    ious, confusion = ev.semantic_results()
    _golden_check(avgs, ap, ious, confusion)
    ev.reset()
    assert ev.scenes == [] and not ev.confusion.any()


def test_files_in_reference_format_match_reference(dev, tmp_path):
    """files in the reference's layout (as its test() writes them) scored by evaluate_*_files give the golden numbers"""
    from gen_seg_eval_golden import seg_eval_inputs, write_reference_files
    from d3net_amd import seg_eval as SE
    gt_files, sem_files, inst_files = write_reference_files(seg_eval_inputs(), str(tmp_path))
    avgs, ap = SE.evaluate_instance_files(inst_files, gt_files, device=dev)
    ious, confusion = SE.evaluate_semantic_files(sem_files, gt_files, device=dev)
    _golden_check(avgs, ap, ious, confusion)


def _model_and_batch(dev):
    from d3net_amd import synthetic as S
    from d3net_amd.config import default_conf
    from d3net_amd.pointgroup import PointGroup
    cfg = default_conf(overrides={"model": {"blocks": [1, 2, 3]}})
    torch.manual_seed(0)
    model = PointGroup(cfg).to(dev).eval()
    model.teacher = True
    with torch.no_grad():
        model.score_linear.bias.fill_(4.0)
    scenes = [S.small_scene(dims=(44, 36, 20), n_boxes=4, seed=3), S.small_scene(dims=(40, 40, 20), n_boxes=3, seed=5)]
    return model, S.make_batch(scenes, dev)


def _dense_restatement(pred, gt):
    """the evaluator's inputs rebuilt from predict_instances' output with dense (N,) masks per picked proposal, in numpy"""
    from d3net_amd import seg_eval as SE
    from test_seg_eval import numpy_counts
    lut = np.array(SE.SEM_CLASS_IDX)
    bo = gt["batch_offsets"].cpu().numpy().astype(np.int64)
    sem, ins = gt["sem_labels"].cpu().numpy(), gt["instance_ids"].cpu().numpy()
    sp = lut[pred["semantic_pred"].cpu().numpy()]
    idx, off = pred["proposals_idx"].cpu().numpy(), pred["proposals_offset"].cpu().numpy()
    pick, scores = pred["pick"].cpu().numpy(), pred["scores"].cpu().numpy()
    scenes, confusion = [], np.zeros((40, 40), np.int64)
    for b in range(len(bo) - 1):
        lo, hi = bo[b], bo[b + 1]
        s, i = sem[lo:hi], ins[lo:hi]
        gsem = np.where((s >= 0) & (s < 20), lut[np.clip(s, 0, 19)], 0)
        ginst = np.where(i >= 0, i - (i[i >= 0].min() if (i >= 0).any() else 0) + 1, 0)
        mine = [j for j in range(len(pick)) if lo <= idx[off[pick[j]], 1] < hi]
        masks = []
        for j in mine:
            mk = np.zeros(hi - lo, bool)
            mk[idx[off[pick[j]]:off[pick[j] + 1], 1] - lo] = True
            masks.append(np.nonzero(mk)[0])
        c = numpy_counts(dict(gt_sem=gsem, gt_inst=ginst, pred_sem=sp[lo:hi], members=masks,
                              classes=[sp[idx[off[pick[j]], 1]] for j in mine], scores=scores[mine]))
        confusion += c.pop("confusion")
        scenes.append(c)
    return scenes, confusion


def test_pointgroup_evaluate_segmentation(dev, tmp_path):
    from d3net_amd import seg_eval as SE
    model, batch = _model_and_batch(dev)
    gt = {k: batch[k].clone() for k in ("sem_labels", "instance_ids", "batch_offsets")}
    recorded, orig = [], model.predict_instances
    model.predict_instances = lambda b: recorded.append(orig(b)) or recorded[-1]
    model.train()
    ev = SE.SegmentationEvaluator()
    avgs, ious = model.evaluate_segmentation([batch], evaluator=ev)
    assert model.training                                                 # mode restored
    pred = recorded[0]
    assert len(pred["pick"]) >= 2
    sp, idx, off = (pred[k].cpu().numpy() for k in ("semantic_pred", "proposals_idx", "proposals_offset"))
    mixed = [np.unique(sp[idx[off[c]:off[c + 1], 1]]).size > 1 for c in pred["pick"].cpu().numpy()]
    assert ev.mixed_class_predictions == sum(mixed)                       # flagged and counted, the first member's class kept
    scenes, confusion = _dense_restatement(pred, gt)
    ap = SE.evaluate_matches(scenes)
    exp_avgs, exp_ious = SE.compute_averages(ap), SE.semantic_iou(confusion)
    got_ap = ev.instance_results()[1]
    assert np.array_equal(np.isnan(got_ap), np.isnan(ap)) and np.array_equal(got_ap[~np.isnan(ap)], ap[~np.isnan(ap)])
    assert np.array_equal(ev.confusion, confusion)
    for k in ("all_ap", "all_ap_50%", "all_ap_25%"):
        assert (np.isnan(avgs[k]) and np.isnan(exp_avgs[k])) or avgs[k] == exp_avgs[k], k
    for name in SE.SEM_CLASS_NAME:
        a, e = ious[name], exp_ious[name]
        assert (isinstance(a, float) and isinstance(e, float) and np.isnan(a) and np.isnan(e)) or a == e, name

    # the file route on what write_predictions / write_gt produced equals the in-memory result
    names = ["scene_a", "scene_b"]
    SE.write_predictions(pred, gt, str(tmp_path), names)
    SE.write_gt(gt, str(tmp_path), names)
    base = tmp_path / "split_pred" / "val"
    gtf = [str(tmp_path / "split_gt" / "val" / (n + ".txt")) for n in names]
    f_avgs, f_ap = SE.evaluate_instance_files([str(base / "instance" / (n + ".txt")) for n in names], gtf, device=dev)
    f_ious, f_conf = SE.evaluate_semantic_files([str(base / "semantic" / (n + ".txt")) for n in names], gtf, device=dev)
    assert np.array_equal(np.isnan(f_ap), np.isnan(got_ap)) and np.array_equal(f_ap[~np.isnan(f_ap)], got_ap[~np.isnan(got_ap)])
    assert np.array_equal(f_conf, ev.confusion)
    for name in SE.SEM_CLASS_NAME:
        a, e = f_ious[name], ious[name]
        assert (isinstance(a, float) and np.isnan(a) and np.isnan(e)) or a == e, name
