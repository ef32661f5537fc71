"""The specification of csrc/det_eval.hip, pinned on the CPU: the order-free true-positive rule and the AP pass as restated in
tests/det_eval_restate.py give eval_det's curves bit for bit on tie-free streams and the reference's own numbers on the golden
inputs; DetectionEvaluator refuses what the kernels cannot take before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import det_eval_restate as R  # noqa: E402

THRESHOLDS = (0.25, 0.5)


def _host(batches, thr):
    """parse_predictions (host NMS) + parse_groundtruths + eval_det over the stream -> rec, prec, ap per class, the NMS masks"""
    from d3net_amd import evaluator as ev
    pred_all, gt_all, picks, n = {}, {}, [], 0
    for d in batches:
        t = {k: torch.from_numpy(v) for k, v in d.items()}
        preds, gts = ev.parse_predictions(t, device_nms=False), ev.parse_groundtruths(t)
        picks.append(np.asarray(t["pred_mask"]))
        for p, g in zip(preds, gts):
            pred_all[n], gt_all[n] = p, g
            n += 1
    return ev.eval_det(pred_all, gt_all, ovthresh=thr), picks


@pytest.mark.parametrize("family", R.FAMILIES)
def test_restatement_equals_eval_det_on_tie_free_streams(family):
    from d3net_amd import evaluator as ev
    for seed, shapes in ((1, [(3, 33, 12)]), (2, [(3, 8, 5), (2, 128, 40)]), (3, [(1, 1, 1), (3, 65, 0)])):
        batches = R.stream(100 * seed + R.FAMILIES.index(family), shapes, family)
        classes_seen = 0
        for q, thr in enumerate(THRESHOLDS):
            (rec, prec, ap), picks = _host(batches, thr)
            recs = [R.batch_records(d, p, ev.POST_DICT["conf_thresh"], THRESHOLDS) for d, p in zip(batches, picks)]
            tab = R.table(recs, len(THRESHOLDS))
            assert sorted(int(c) for c in ap) == [c for c in range(18) if tab[q, c, 3] == 1]
            flat = {k: np.concatenate([r[k].reshape(-1) for r in recs]) for k in ("kept", "cls", "score", "tp")}
            gt_count = np.concatenate([r["gt_count"] for r in recs])
            for c in ap:
                r, p, a, _ = R.curves(flat["kept"], flat["cls"], flat["score"], flat["tp"], gt_count, q, int(c))
                assert np.array_equal(r, rec[c]) and np.array_equal(p, prec[c]) and a == ap[c], (family, seed, thr, c)
                assert tab[q, int(c), 0] == ap[c] and tab[q, int(c), 2] == len(rec[c])
                classes_seen += 1
        assert classes_seen > 0


def test_stream_families_hold_the_cases_they_name():
    d = R.stream(7, [(3, 33, 12)], "empty_scenes")[0]
    assert d["proposal_batch_mask"][0].sum() == 0 and d["gt_bbox_label"][1].sum() == 0
    d = R.stream(7, [(3, 33, 12)], "duplicated_proposals")[0]
    assert np.array_equal(d["proposal_bbox_batched"][:, 1], d["proposal_bbox_batched"][:, 0])
    d = R.stream(7, [(3, 64, 12)], "random")[0]
    assert (R.map_classes(d["proposal_sem_cls_batched"]) == 16).any() and not (d["sem_cls_label"] == 16).any()   # prediction-only
    s = np.concatenate([b["proposal_scores_batched"].ravel() for b in R.stream(7, [(3, 33, 12), (2, 128, 4)], "random")])
    assert len(np.unique(s)) == s.size
    s = R.stream(7, [(3, 33, 12)], "random", tie_free=False)[0]["proposal_scores_batched"]
    assert len(np.unique(s)) <= 8


def test_restatement_reproduces_the_reference_golden():
    from gen_evaluator_golden import evaluator_inputs
    from d3net_amd import evaluator as ev
    g = np.load(os.path.join(HERE, "golden", "evaluator_golden.npz"))
    d = evaluator_inputs()
    rec = R.batch_records(d, g["pred_mask"].astype(np.float64), ev.POST_DICT["conf_thresh"], THRESHOLDS)
    assert rec["kept"].sum(1).tolist() == g["n_pred"].tolist() and rec["gt_count"].sum(1).tolist() == g["n_gt"].tolist()
    kept_scores = d["proposal_scores_batched"][rec["kept"] == 1]
    assert len(np.unique(kept_scores)) == kept_scores.size                # no ties among the kept detections
    tab = R.table([rec], 2)
    for q, thr in enumerate(THRESHOLDS):
        m = R.metrics(tab)[q]
        present = tab[q, :, 3] == 1
        assert np.array_equal(tab[q, present, 0], g["AP@%s" % thr])
        assert abs(m["mAP"] - float(g["mAP@%s" % thr])) <= 1e-12 and abs(m["AR"] - float(g["AR@%s" % thr])) <= 1e-12


def test_add_batch_refuses_host_tensors_and_k_257_before_any_launch(monkeypatch):
    from d3net_amd import evaluator as ev, _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("a launch was attempted"))
    d = {k: torch.from_numpy(v) for k, v in R.stream(5, [(2, 8, 4)])[0].items()}
    e = ev.DetectionEvaluator()
    with pytest.raises(ValueError):
        e.add_batch(d)
    with pytest.raises(ValueError):
        e.add_batch({k: torch.from_numpy(v) for k, v in R.stream(5, [(2, 257, 4)])[0].items()})
    # K = 257 is refused for its size, not only for where it lives
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    ok = {k: torch.from_numpy(v) for k, v in R.stream(5, [(2, 256, 4)])[0].items()}
    e._checked(ok)
    with pytest.raises(ValueError, match="K <= 256"):
        e._checked({k: torch.from_numpy(v) for k, v in R.stream(5, [(2, 257, 4)])[0].items()})
    with pytest.raises(ValueError, match="dtype"):
        e._checked(dict(ok, proposal_scores_batched=ok["proposal_scores_batched"].double()))
    with pytest.raises(ValueError):
        ev.DetectionEvaluator(post_dict={"cls_nms": False})
    with pytest.raises(ValueError):
        ev.DetectionEvaluator(thresholds=(0.1, 0.2, 0.3, 0.4, 0.5))


def test_new_symbols_are_bound():
    from d3net_amd import _lib
    assert {"d3_det_match", "d3_det_ap"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["d3_det_match"][1]) == 23 and len(_lib.SIGNATURES["d3_det_ap"][1]) == 9


def test_pipeline_delegates_to_its_detector():
    import types
    from d3net_amd.pipeline import PipelineNet
    calls = []
    det = types.SimpleNamespace(evaluate_detection=lambda batches, evaluator=None: calls.append((batches, evaluator)) or "metrics")
    assert PipelineNet.evaluate_detection(types.SimpleNamespace(no_detection=False, detector=det), [1, 2], "ev") == "metrics"
    assert calls == [([1, 2], "ev")]
    with pytest.raises(NotImplementedError):
        PipelineNet.evaluate_detection(types.SimpleNamespace(no_detection=True, detector=det), [])
