"""The grounding validation on the device (csrc/grounding_eval.hip, grounding_eval.GroundingEvaluator,
PipelineNet.evaluate_grounding): on the golden inputs the evaluator's integer tables, stats, every score and lang_acc equal the
numbers the reference's own get_eval + eval_grounding printed (tests/golden/grounding_epoch_golden.npz) with ==; random epochs equal
the numpy restatement (tests/grounding_epoch_restate.py, pinned to the golden on the CPU); add_batch reads nothing back; the
prediction records round-trip; evaluate_grounding agrees with get_eval run batch by batch and aggregated on the host.
Tolerances: counts are integers and the scores are one float64 division of them per repeat, then np.mean -> ==.  The per-row IoU
against the reference's record: rtol 1e-5, atol 1e-6, the bounds of tests/test_grounding_eval.py (the reference adds its 1e-8 in
float64 under numpy 1.x).  Against the restatement, which does the kernel's float32 operations one by one (IEEE add, multiply and
divide, no contraction): bit-equal."""
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import grounding_epoch_restate as R  # noqa: E402
from test_grounding_epoch import _cfg, assert_result_equals_golden  # noqa: E402

REC_INT = ("pred_ref", "gt_ref", "ref_acc")


def _to(dev, d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _add(ev, batch):
    """add_batch under sync-debug "error": it reads nothing back"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.add_batch(batch)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _assert_records_equal_restatement(rec, rows, where):
    cat = lambda k: np.concatenate([b[k] for b in rows])
    for k in REC_INT:
        assert np.array_equal(rec[k], cat(k)), (where, k)
    for k in ("iou", "best_iou", "pred_bbox", "gt_bbox"):
        assert np.array_equal(rec[k].view(np.int32), cat(k).view(np.int32)), (where, k)         # bit-equal float32 (NaN included)
    if rows[0]["ids"] is not None:
        assert np.array_equal(rec["ids"], cat("ids")), where


def _assert_result_equals_restatement(got, want, where):
    assert got["stats"] == want["stats"], where
    for k, by_o in want["scores"].items():
        for k_o, by_m in by_o.items():
            for metric, v in by_m.items():
                assert np.float64(got["scores"][k][k_o][metric]) == np.float64(v), (where, k, k_o, metric)
    assert got["lang_acc"] == want["lang_acc"] and got["status"] == want["status"], where


def test_golden_epoch_equals_the_reference(dev):
    from gen_grounding_epoch_golden import epoch_inputs
    from d3net_amd import grounding_eval as ge
    g = np.load(os.path.join(HERE, "golden", "grounding_epoch_golden.npz"))
    inputs = epoch_inputs()
    want = R.epoch(inputs)
    ev = ge.GroundingEvaluator(keep_predictions=True, device=dev)
    for r, rep in enumerate(inputs):
        if r:
            ev.begin_repeat()                              # the first repeat is implicit
        for d in rep:
            batch = _to(dev, d)
            before = {k: v.clone() for k, v in batch.items()}
            _add(ev, batch)
            assert list(batch) == list(before) and all(_same_bits(batch[k], before[k]) for k in before)      # data_dict is left as it is
        rec = ev.records()                                 # this repeat's rows: the records are the last repeat's
        print("repeat", r, "max |iou - reference|", np.abs(rec["iou"] - g["ious"][r]).max())
        assert np.allclose(rec["iou"], g["ious"][r], rtol=1e-5, atol=1e-6) and np.allclose(rec["best_iou"], g["best_ious"][r], rtol=1e-5, atol=1e-6)
        assert np.array_equal(rec["ref_acc"], g["ref_acc"][r].astype(np.int32))
        assert np.array_equal(rec["pred_bbox"], g["pred_bboxes"][r]) and np.array_equal(rec["gt_bbox"], g["gt_bboxes"][r])
        _assert_records_equal_restatement(rec, want["rows"][r], ("golden", r))
    res = ev.compute()
    print(ev.tables.reshape(-1, 6, 4), res["scores"]["overall"], res["lang_acc"])
    assert np.array_equal(ev.tables, g["tables"]) and ev.tables.dtype == np.int64
    assert_result_equals_golden(res, g, "evaluator")
    assert res["status"] == 0
    ev.reset()
    for d in inputs[1]:
        ev.add_batch(_to(dev, d))
    assert np.array_equal(ev.compute()["stats"]["overall"]["overall"], 17) and np.array_equal(ev.tables, g["tables"][1:])


@pytest.mark.parametrize("use_lang", [True, False], ids=["lang", "nolang"])
def test_random_epochs_equal_the_restatement(dev, use_lang):
    from gen_grounding_epoch_golden import SHAPES
    from d3net_amd import grounding_eval as ge
    inputs = R.random_epoch(101 + use_lang, SHAPES)
    want = R.epoch(inputs, use_lang)
    ev = ge.GroundingEvaluator(use_lang_classifier=use_lang, keep_predictions=use_lang, device=dev)
    for rep in inputs:
        ev.begin_repeat()                                  # an explicit first begin_repeat is repeat 0 as well
        for d in rep:
            batch = _to(dev, d)
            if not use_lang:
                for k in ("lang_scores", "id", "chunk_ids"):
                    del batch[k]                           # not asked for without the classifier / the records
                batch["proposal_batch_mask"] = batch["proposal_batch_mask"].bool()          # the dtypes that are converted
                batch["unique_multiple"], batch["cluster_labels"] = batch["unique_multiple"].int(), batch["cluster_labels"].long()
            _add(ev, batch)
    got = ev.compute()
    assert np.array_equal(ev.tables, want["tables"])
    _assert_result_equals_restatement(got, want, ("random", use_lang))
    assert want["tables"][:, :, :, 2].sum() > want["tables"][:, :, :, 3].sum() > 0 and want["tables"][:, 2].sum() > 0
    if use_lang:
        _assert_records_equal_restatement(ev.records(), want["rows"][-1], "random")
        assert 0 < got["lang_acc"] < 1
    else:
        assert got["lang_acc"] == 0.0


def test_storage_grows_and_predictions_round_trip(dev):
    """3 repeats (the table storage starts at 2), 10 batches per repeat (the language counters at 8), 1076 rows (the records at
    1024): every growth happens inside add_batch under sync-debug "error" """
    from d3net_amd import grounding_eval as ge
    shapes = (((2, 2, 5),) * 9 + ((260, 4, 3),),) * 3
    inputs = R.random_epoch(7, shapes, nan_rate=0.0)
    want = R.epoch(inputs)
    ev = ge.GroundingEvaluator(keep_predictions=True, device=dev)
    for rep in inputs:
        ev.begin_repeat()
        for d in rep:
            _add(ev, _to(dev, d))
    got = ev.compute()
    assert ev.tables.shape == (3, 3, 2, 4) and np.array_equal(ev.tables, want["tables"])
    _assert_result_equals_restatement(got, want, "growth")
    rows = want["rows"][-1]
    _assert_records_equal_restatement(ev.records(), rows, "growth")
    chunked = [[{"scene_id": "scene%04d_00" % (s % 7), "object_id": str(c % 3), "ann_id": str((s + c) % 2)} for c in range(9)] for s in range(50)]
    pred = ev.predictions(chunked)
    host = {}
    for b in rows:
        for i, (s, c) in enumerate(b["ids"].tolist()):
            a = chunked[s][c]
            host.setdefault(a["scene_id"], {}).setdefault(a["object_id"], {})[a["ann_id"]] = (b["pred_bbox"][i], b["gt_bbox"][i], b["iou"][i])
    assert set(pred) == set(host) and len(host) == 7
    n = 0
    for s in host:
        assert set(pred[s]) == set(host[s])
        for o in host[s]:
            assert set(pred[s][o]) == set(host[s][o])
            for a, (pb, gb, iou) in host[s][o].items():
                p = pred[s][o][a]
                assert set(p) == {"pred_bbox", "gt_bbox", "iou"} and p["pred_bbox"].shape == (8, 3)
                assert np.array_equal(p["pred_bbox"], pb) and np.array_equal(p["gt_bbox"], gb) and p["iou"] == iou
                n += 1
    assert n < sum(len(b["iou"]) for b in rows)            # annotations collide: later rows overwrote earlier ones


def test_non_finite_boxes_set_the_status(dev):
    from d3net_amd import grounding_eval as ge
    d = R.random_epoch(3, (((2, 4, 65),),), nan_rate=0.0)[0][0]
    rows = R.batch_rows(d)
    scored = set(zip((np.arange(8) // 4).tolist(), rows["pred_ref"].tolist())) | set(zip((np.arange(8) // 4).tolist(), rows["gt_ref"].tolist()))
    unscored = next(k for k in range(65) if (0, k) not in scored)

    def status(dd):
        ev = ge.GroundingEvaluator(device=dev)
        ev.add_batch(_to(dev, dd))
        return ev.compute()["status"]

    assert status(d) == 0
    harmless = {k: v.copy() for k, v in d.items()}
    harmless["proposal_bbox_batched"][0, unscored, 3, 1] = np.inf
    assert status(harmless) == 0
    for key, idx in (("proposal_bbox_batched", (1, int(rows["pred_ref"][5]), 0, 2)), ("proposal_bbox_batched", (0, int(rows["gt_ref"][2]), 7, 0)),
                     ("ref_box_corner_label", (1, 3, 4, 1))):
        bad = {k: v.copy() for k, v in d.items()}
        bad[key][idx] = np.nan if key.startswith("ref") else np.inf
        assert status(bad) == 1 and R.epoch([[bad]])["status"] == 1, (key, idx)


def test_evaluate_grounding_equals_get_eval_batch_by_batch(dev):
    from d3net_amd import synthetic as S, grounding_eval as ge
    from d3net_amd.pipeline import PipelineNet
    V = 200
    ds = {"train": types.SimpleNamespace(vocabulary=S.make_vocabulary(V), glove=np.random.default_rng(0).standard_normal((V, 300)).astype(np.float32))}
    torch.manual_seed(2)
    net = PipelineNet(_cfg(no_captioning=True, no_grounding=False), ds).to(dev).train()
    net.detector.teacher = True
    scenes = [S.small_scene(dims=(40, 32, 20), n_boxes=3, seed=s) for s in (3, 4)]
    batches = [S.add_language(S.make_batch(scenes[i:i + n], dev), dev, chunk=4, vocab=V) for i, n in ((0, 2), (1, 1))]
    for i, b in enumerate(batches):                         # (the synthetic loader has no unique / multiple lookup)
        b["unique_multiple"] = torch.from_numpy(np.random.default_rng(i).integers(0, 2, tuple(b["object_cat"].shape))).to(dev)
        b["object_cat"][:, 1] = 17
    keys =("cluster_ref", "cluster_labels", "proposal_batch_mask", "proposal_bbox_batched", "ref_box_corner_label", "unique_multiple",
            "object_cat", "lang_scores", "id", "chunk_ids")

    class Recording(ge.GroundingEvaluator):
        def add_batch(self, data_dict):
            self.seen.setdefault(self._repeat, []).append({k: data_dict[k].detach().clone() for k in keys})
            super().add_batch(data_dict)

    rec = Recording(keep_predictions=True, device=dev)
    rec.seen = {}
    got = net.evaluate_grounding(batches, rec, seeds=[5, 0])
    assert net.training and sorted(rec.seen) == [0, 1] and [len(v) for v in rec.seen.values()] == [2, 2]
    lists = {k: [] for k in ("masks", "others", "ref_acc", "ious", "lang_acc")}
    for r in (0, 1):
        row = {k: [] for k in lists}
        for seen in rec.seen[r]:
            d = ge.get_eval(dict(seen), grounding=True, use_lang_classifier=True)
            row["masks"] += d["ref_multiple_mask"]; row["others"] += d["ref_others_mask"]; row["ref_acc"] += d["ref_acc"]
            row["ious"] += d["ref_iou"].cpu().numpy().tolist(); row["lang_acc"].append(d["lang_acc"].item())
            if r == 1:
                row.setdefault("pred", []).append(d["pred_bboxes"].cpu().numpy()); row.setdefault("best", []).append(d["best_ious"].cpu().numpy())
        for k in lists:
            lists[k].append(row[k])
    ious = np.array(lists["ious"], np.float32)
    assert min(np.abs(ious.astype(np.float64) - 0.25).min(), np.abs(ious.astype(np.float64) - 0.5).min()) > 1e-5   # the == below needs it
    stats, scores, lang_acc = R.aggregate(lists["masks"], lists["others"], lists["ref_acc"], ious, lists["lang_acc"])
    _assert_result_equals_restatement(got, dict(stats=stats, scores=scores, lang_acc=lang_acc, status=0), "evaluate_grounding")
    assert got["stats"]["overall"]["overall"] == 12
    records = rec.records()                                # every row of the last repeat
    assert np.allclose(records["iou"], ious[1], rtol=1e-5, atol=1e-6) and np.allclose(records["best_iou"], np.concatenate(row["best"]), rtol=1e-5, atol=1e-6)
    assert np.array_equal(records["pred_bbox"], np.concatenate(row["pred"])) and np.array_equal(records["ref_acc"], np.array(lists["ref_acc"][1], np.int32))
    # the default evaluator and seed list: one repeat, the module's own language-classifier switch; eval() stays eval()
    net.eval()
    one = net.evaluate_grounding(lambda: iter(batches))
    assert not net.training and one["stats"] == got["stats"] and one["status"] == 0
