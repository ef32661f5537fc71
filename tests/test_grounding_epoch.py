"""The grounding validation's specification, pinned on the CPU: the numpy restatement of csrc/grounding_eval.hip's per-row rule and
of the Acc@kIoU table (tests/grounding_epoch_restate.py) gives the numbers the reference's own get_eval + eval_grounding printed
(tests/golden/grounding_epoch_golden.npz, made by gen_grounding_epoch_golden.py); the host half of GroundingEvaluator.compute, fed the
golden integer tables, is bit-equal to them; GroundingEvaluator and PipelineNet.evaluate_grounding refuse what they cannot take
before any launch.  Counts and scores compare with ==: that needs every IoU but the two constructed ones away from 0.25 and 0.5
by more than 1e-5, asserted here on the stored IoUs.  Per-row IoUs compare within rtol 1e-5, atol 1e-6, the bounds of
tests/test_grounding_eval.py (the reference adds 1e-8 to a numpy float32 scalar: float64 under numpy 1.x, float32 under numpy 2)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import grounding_epoch_restate as R  # noqa: E402

ROWS, COLS = ("unique", "multiple", "overall"), ("not_in_others", "in_others", "overall")


@pytest.fixture(scope="module")
def golden():
    from gen_grounding_epoch_golden import epoch_inputs
    return np.load(os.path.join(HERE, "golden", "grounding_epoch_golden.npz")), epoch_inputs()


def assert_result_equals_golden(res, g, where):
    """stats, every score and lang_acc of a compute()-shaped result == the reference's printed numbers"""
    for i, k in enumerate(ROWS):
        for j, k_o in enumerate(COLS):
            assert res["stats"][k][k_o] == g["stats"][i, j], (where, k, k_o)
            for q, metric in enumerate(R.METRICS):
                assert np.float64(res["scores"][k][k_o][metric]) == g["scores"][i, j, q], (where, k, k_o, metric)
    assert np.float64(res["lang_acc"]) == g["lang_acc"], where


def test_golden_ious_stay_clear_of_the_thresholds(golden):
    g, _ = golden
    ious, exact = g["ious"].astype(np.float64), g["exact"]
    assert exact.sum() == 2 and sorted(g["ious"][exact].tolist()) == [0.25, 0.5]
    for thr in (0.25, 0.5):
        assert (np.abs(ious[~exact] - thr) > 1e-5).all()
    assert 0 < (ious >= 0.5).sum() < (ious >= 0.25).sum() < ious.size            # both outcomes at both thresholds
    assert (g["masks"] == 2).any() and g["tables"][:, 2].sum() > 0              # the "other" bucket is populated


def test_restatement_equals_the_reference(golden):
    g, inputs = golden
    res = R.epoch(inputs)
    assert np.array_equal(res["tables"], g["tables"])
    assert_result_equals_golden(res, g, "restatement")
    assert res["status"] == 0
    for r, rows in enumerate(res["rows"]):
        cat = lambda k: np.concatenate([b[k] for b in rows])
        assert np.allclose(cat("iou"), g["ious"][r], rtol=1e-5, atol=1e-6) and np.allclose(cat("best_iou"), g["best_ious"][r], rtol=1e-5, atol=1e-6)
        assert np.array_equal(cat("ref_acc"), g["ref_acc"][r].astype(np.int64)) and np.array_equal(cat("o"), g["others"][r])
        assert np.array_equal(cat("unique_multiple"), g["masks"][r])
        assert np.array_equal(cat("pred_bbox"), g["pred_bboxes"][r]) and np.array_equal(cat("gt_bbox"), g["gt_bboxes"][r])
    # the planted rows do what they were planted for
    r00, r02, r10, r11 = res["rows"][0][0], res["rows"][0][2], res["rows"][1][0], res["rows"][1][1]
    assert r00["pred_ref"][0] == 2 and r00["gt_ref"][2] == 0 and r00["top"][3] == 20 and r00["pred_ref"][3] == 20      # zero tie, no label, tie
    assert r00["pred_ref"][[4, 6, 7]].tolist() == [0, 0, 0] and r00["pred_ref"][5] == 62 and r00["top"][5] == 62    # empty mask, NaN
    assert r02["pred_ref"][:3].tolist() == [5, 6, 40] and r02["iou"][0] == 0.5 and r02["iou"][1] == 0.25
    assert r10["pred_ref"][0] == 33 and r10["top"][1] == 64 and r10["pred_ref"][1] != 64 and r10["top"][2] == 0
    assert r11["pred_ref"][2] == 70 and r11["pred_ref"][3] == 0 and r11["gt_ref"][4] == 0


def test_host_half_of_compute_is_bit_equal(golden):
    from gen_grounding_epoch_golden import SHAPES
    from d3net_amd.grounding_eval import grounding_scores
    g, _ = golden
    rows = [B * Cn for rep in SHAPES for B, Cn, _ in rep]
    acc = g["lang_acc_batches"].reshape(-1)
    correct = [int(round(a * n)) for a, n in zip(acc, rows)]
    assert all(float(np.float32(c) / np.float32(n)) == a for c, n, a in zip(correct, rows, acc))
    stats, scores, lang_acc = grounding_scores(g["tables"], correct, rows)
    assert_result_equals_golden({"stats": stats, "scores": scores, "lang_acc": lang_acc}, g, "host half")
    # repeat 0 alone: the stats stay, the scores become that repeat's own ratios; an empty cell scores 0; the classifier off: 0
    stats0, scores0, off = grounding_scores(g["tables"][:1])
    assert stats0 == stats and off == 0.0
    t = g["tables"][0]
    assert scores0["multiple"]["in_others"]["acc@0.25iou"] == t[1, 1, 2] / t[1, 1, 0]
    assert scores0["overall"]["overall"]["ref_acc"] == t[:, :, 1].sum() / t[:, :, 0].sum()
    empty = np.zeros((1, 3, 2, 4), np.int64)
    empty[0, 2, 0] = [3, 1, 2, 1]                                                # only "other" rows: they count in the overall rows alone
    s, sc, _ = grounding_scores(empty)
    assert s["unique"]["overall"] == 0 and sc["unique"]["overall"]["ref_acc"] == 0 and s["overall"]["not_in_others"] == 3
    assert sc["overall"]["overall"]["acc@0.25iou"] == 2 / 3 and sc["overall"]["in_others"]["acc@0.5iou"] == 0


def test_bad_input_is_refused_before_any_launch(golden, monkeypatch):
    from d3net_amd import _lib, grounding_eval as ge

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)
    _, inputs = golden
    good = {k: torch.from_numpy(v.copy()) for k, v in inputs[0][0].items()}
    ev = ge.GroundingEvaluator(keep_predictions=True)

    def refused(match, **change):
        d = dict(good)
        d.update(change)
        for k in [k for k, v in change.items() if v is None]:
            del d[k]
        with pytest.raises(ValueError, match=match):
            ev.add_batch(d)

    refused("missing", cluster_labels=None)
    refused("missing", lang_scores=None)
    refused("missing", chunk_ids=None)
    refused("must be a tensor", object_cat=inputs[0][0]["object_cat"])
    refused("dtype", cluster_ref=good["cluster_ref"].double())
    refused("dtype", proposal_bbox_batched=good["proposal_bbox_batched"].half())
    refused("dtype", unique_multiple=good["unique_multiple"].float())
    refused("shape", cluster_labels=good["cluster_labels"][:, :-1])
    refused("shape", ref_box_corner_label=good["ref_box_corner_label"][:, :3])
    refused("shape", chunk_ids=good["chunk_ids"].reshape(-1))
    refused("expected", proposal_bbox_batched=good["proposal_bbox_batched"].reshape(2, 63, 24))
    refused("1 <= K", cluster_ref=torch.zeros(8, 4097), cluster_labels=torch.zeros(8, 4097), proposal_batch_mask=torch.zeros(2, 4097),
            proposal_bbox_batched=torch.zeros(2, 4097, 8, 3))
    refused("N = B", cluster_ref=good["cluster_ref"][:7], cluster_labels=good["cluster_labels"][:7])
    refused("lang_scores", lang_scores=torch.zeros(8, 65))
    refused("lang_scores", lang_scores=torch.zeros(7, 18))
    refused("GPU", **{})                                                          # a well-formed batch in host memory
    off = ge.GroundingEvaluator(use_lang_classifier=False)
    with pytest.raises(ValueError, match="GPU"):                                  # without the classifier lang_scores is not asked for
        off.add_batch({k: v for k, v in good.items() if k not in ("lang_scores", "id", "chunk_ids")})
    with pytest.raises(ValueError, match="no batch"):
        ev.compute()
    with pytest.raises(ValueError, match="keep_predictions"):
        off.predictions([])


def _cfg(**model):
    from d3net_amd.config import default_conf
    base = {"model": {"blocks": [1, 2, 3], "num_graph_steps": 2, "num_locals": 10, "use_relation": True, "use_orientation": True,
                      "match_type": "Transformer", "use_lang_classifier": True, "use_bidir": False, "num_bbox_class": 18,
                      "loss_type": "cross_entropy"},
            "data": {"num_des_per_scene": 4, "max_spk_len": 30, "max_lis_len": 126, "min_iou_threshold": 0.25, "num_ori_bins": 6},
            "train": {"use_rl": False, "sample_topn": 1}}
    base["model"].update(model)
    return default_conf(overrides=base)


def test_evaluate_grounding_refuses_other_modes_and_one_shot_iterators():
    from d3net_amd import synthetic as S
    from d3net_amd.pipeline import PipelineNet
    V = 50
    ds = {"train": types.SimpleNamespace(vocabulary=S.make_vocabulary(V), glove=np.zeros((V, 300), np.float32))}
    net0 = PipelineNet(_cfg(no_captioning=True, no_grounding=True), ds)
    with pytest.raises(NotImplementedError, match="modes 2 and 3"):
        net0.evaluate_grounding([])
    net2 = PipelineNet(_cfg(no_captioning=True, no_grounding=False), ds).train()
    assert net2.mode == 2
    with pytest.raises(TypeError, match="one-shot"):
        net2.evaluate_grounding(iter([]), seeds=[1, 2])
    with pytest.raises(TypeError, match="one-shot"):
        net2.evaluate_grounding((b for b in []), seeds=[1, 2])
    assert net2.training                                                        # refused before any work: the flag was not touched
    assert net2.cfg.eval.repeat == 1                                            # the default seed list is [general.manual_seed]


def test_binding_table_entry(built_lib):
    import ctypes as C
    from d3net_amd import _lib
    res, args = _lib.SIGNATURES["d3_ground_eval_batch"]
    assert res is C.c_int and len(args) == 27 and args[14] is C.c_longlong and args[8] is C.c_int
    l = _lib.lib()
    # the range checks come before any launch and before any pointer is looked at: no device needed
    null = [None] * 27
    def call(B, Cn, K, n_lang=0, lang=None):
        a = list(null)
        a[7], a[8], a[11], a[12], a[13], a[14] = lang, n_lang, B, Cn, K, 0
        return l.d3_ground_eval_batch(*a)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 4097), (65536, 65536, 8)):
        assert call(*bad) == -2, bad
    assert call(1, 1, 8, 0, C.c_void_p(64)) == -2 and call(1, 1, 8, 65, C.c_void_p(64)) == -2
    assert call(1, 1, 8) == -3 and call(1, 1, 4096, 65) == -3                   # in range (n_lang is not read without lang_scores): D3_ERR_ARG
