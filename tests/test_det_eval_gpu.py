"""csrc/det_eval.hip on the GPU: d3_det_match against the numpy restatement (tests/det_eval_restate.py, pinned to eval_det on the
CPU) and the reference's golden numbers, d3_det_ap on synthesised segments, DetectionEvaluator against the host APCalculator,
PointGroup.evaluate_detection against the host path on the same feed() outputs.
Tolerances (derived, not tuned): recall is one correctly rounded float64 division of exact integers -> bit-equal; AP is a sum of
n non-negative terms totalling <= 1 whose summation order alone differs from numpy's -> |dAP| <= n 2^-53 < 6e-13 for n <= 5000,
1e-12 required; mAP and AR are means of <= 18 such values -> 1e-12."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import det_eval_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.25, 0.5)
CONF = 0.09
OUTS = (("kept", torch.int32), ("cls", torch.int32), ("score", torch.float32), ("ovmax", torch.float64), ("jmax", torch.int32),
        ("tp", torch.int32))
TOL = 1e-12


def _to(dev, d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}


def _raw_match(dev, d, pick, thresholds, T=None, num_class=18):
    """d3_det_match straight through the ABI on sentinel-filled outputs -> rc, dict of numpy outputs"""
    from d3net_amd import _lib, evaluator as ev
    t = _to(dev, d)
    B, K = d["proposal_scores_batched"].shape
    G = d["gt_bbox_label"].shape[1]
    cls = ev.map_pred_classes(t["proposal_sem_cls_batched"])
    pk = torch.from_numpy(np.ascontiguousarray(pick, np.float32)).to(dev)
    gm, gc = (t["gt_bbox_label"] == 1).float().contiguous(), t["sem_cls_label"].to(torch.int32).contiguous()
    out = {k: torch.full((B, K), -7, dtype=dt, device=dev) for k, dt in OUTS}
    out["gt_count"] = torch.full((B, num_class), -7, dtype=torch.int32, device=dev)
    out["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
    thr = (C.c_double * 8)(*[float(x) for x in thresholds])
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = _lib.lib().d3_det_match(p(t["proposal_bbox_batched"]), p(cls), p(t["proposal_scores_batched"]), p(pk), CONF, p(t["gt_bbox"]), p(gm), p(gc),
                                 B, K, G, num_class, thr, len(thresholds) if T is None else T, p(out["kept"]), p(out["cls"]), p(out["score"]),
                                 p(out["ovmax"]), p(out["jmax"]), p(out["tp"]), p(out["gt_count"]), p(out["status"]),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def _assert_records_equal(got, want, where):
    for k in ("kept", "cls", "jmax", "tp", "gt_count"):
        assert np.array_equal(got[k], want[k]), (where, k)
    assert np.array_equal(got["score"].view(np.int32), want["score"].view(np.int32)), where
    assert np.array_equal(got["ovmax"].view(np.int64), want["ovmax"].view(np.int64)), where        # bit-equal float64 IoU


def _device_table(dev, recs, T, num_class=18):
    """numpy records (one dict per batch) -> d3_det_ap's table as numpy"""
    from d3net_amd import evaluator as ev
    flat = {k: torch.from_numpy(np.concatenate([r[k].reshape(-1) for r in recs])).to(dev) for k in ("kept", "cls", "score", "tp")}
    gt_count = torch.from_numpy(np.concatenate([r["gt_count"] for r in recs]).astype(np.int32)).to(dev)
    tab = ev.det_ap_device(flat["kept"].to(torch.int32), flat["cls"].to(torch.int32), flat["score"], flat["tp"].to(torch.int32), gt_count, T, num_class)
    return tab.cpu().numpy()


def _assert_tables_close(got, want, where):
    print(where, "max |dAP| %.3e" % np.abs(got[..., 0] - want[..., 0]).max())
    assert np.array_equal(got[..., 2:], want[..., 2:]), where                      # detections, present: exact
    assert np.array_equal(got[..., 1].view(np.int64), want[..., 1].view(np.int64)), where      # last recall: bit-equal
    assert np.abs(got[..., 0] - want[..., 0]).max() <= TOL, where


def _assert_metrics_close(got, want, where):
    assert list(got) == list(want), where
    for k in want:
        print(where, k, got[k], want[k])
        if k.endswith("Recall"):
            assert np.float64(got[k]) == np.float64(want[k]), (where, k)
        else:
            assert abs(got[k] - want[k]) <= TOL, (where, k)


def _host_metrics(batches, thresholds, device_nms=False):
    """parse_predictions + parse_groundtruths + one APCalculator per threshold over CPU copies of the batches"""
    from d3net_amd import evaluator as ev
    calcs = [ev.APCalculator(t) for t in thresholds]
    for d in batches:
        t = {k: (v.detach().cpu() if torch.is_tensor(v) else torch.from_numpy(v)) for k, v in d.items() if k in R.KEYS}
        preds, gts = ev.parse_predictions(t, device_nms=device_nms), ev.parse_groundtruths(t)
        for c in calcs:
            c.step(preds, gts)
    return [c.compute_metrics() for c in calcs]


def test_golden_through_the_match_kernel_with_the_reference_pick(dev):
    from gen_evaluator_golden import evaluator_inputs
    from d3net_amd import evaluator as ev
    g = np.load(os.path.join(HERE, "golden", "evaluator_golden.npz"))
    d = evaluator_inputs()
    rc, out = _raw_match(dev, d, g["pred_mask"], THRESHOLDS)
    assert rc == 0 and out["status"][0] == 0
    assert out["kept"].sum(1).tolist() == g["n_pred"].tolist() and out["gt_count"].sum(1).tolist() == g["n_gt"].tolist()
    tab = _device_table(dev, [out], 2)
    ours = ev.DetectionEvaluator(THRESHOLDS)
    ours.add_batch(_to(dev, d))                    # device NMS: the tied scores are all 0.05, below conf_thresh
    m = ours.compute_metrics()
    for q, thr in enumerate(THRESHOLDS):
        present = tab[q, :, 3] == 1
        assert np.abs(tab[q, present, 0] - g["AP@%s" % thr]).max() <= TOL
        for res in (R.metrics(tab)[q], m[q]):
            assert abs(res["mAP"] - float(g["mAP@%s" % thr])) <= TOL and abs(res["AR"] - float(g["AR@%s" % thr])) <= TOL
        assert np.abs(np.array([m[q]["%d Average Precision" % c] for c in np.where(present)[0]]) - g["AP@%s" % thr]).max() <= TOL
    assert np.array_equal(ours.table, tab)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("KG", [(1, 1), (8, 0), (64, 5), (65, 128), (128, 128), (256, 256)], ids=lambda s: "%dx%d" % s)
def test_match_kernel_equals_the_host(dev, KG, family):
    K, G = KG
    seed = 1000 * K + G + R.FAMILIES.index(family)
    d = R.stream(seed, [(3, K, G)], family)[0]
    pick = ((np.random.default_rng(seed).random((3, K)) < 0.8) & (d["proposal_batch_mask"] == 1)).astype(np.float32)
    rc, out = _raw_match(dev, d, pick, THRESHOLDS)
    assert rc == 0 and out["status"][0] == 0
    _assert_records_equal(out, R.batch_records(d, pick, CONF, THRESHOLDS), (KG, family))
    if family == "empty_scenes":
        assert out["kept"][0].sum() == 0 and out["gt_count"][1].sum() == 0


@pytest.mark.parametrize("shape", [(3, 64, 12), (2, 256, 40)], ids=lambda s: "%dx%dx%d" % s)
def test_tied_scores_follow_the_stable_order(dev, shape):
    batches = R.stream(77 + shape[1], [shape, shape], "duplicated_proposals", tie_free=False)
    recs, outs = [], []
    for i, d in enumerate(batches):
        pick = d["proposal_batch_mask"].copy()
        rc, out = _raw_match(dev, d, pick, (0.1, 0.25, 0.5, 0.75))
        assert rc == 0
        want = R.batch_records(d, pick, CONF, (0.1, 0.25, 0.5, 0.75))
        _assert_records_equal(out, want, ("ties", shape, i))
        recs.append(want); outs.append(out)
    kept_scores = np.concatenate([r["score"][r["kept"] == 1] for r in recs])
    assert len(np.unique(kept_scores)) < kept_scores.size                          # there are ties among the kept detections
    _assert_tables_close(_device_table(dev, outs, 4), R.table(recs, 4), ("ties", shape))


@pytest.mark.parametrize("T", [1, 4])
def test_ap_kernel_on_synthesised_records(dev, T):
    """no match launch: segments of 0 (a GT-only class), 1, 64, 65, 1024, 1025 and 5000 records (the carried scan forward and
    backward over up to 20 passes), a prediction-only class, unkept slots in between, tied scores"""
    rng = np.random.default_rng(40 + T)
    lengths = {0: 0, 1: 1, 2: 64, 3: 65, 4: 1024, 5: 1025, 6: 5000, 9: 7}     # class 9: only predicted; classes 7, 8, 10.. absent
    cls = np.concatenate([np.full(n, c) for c, n in lengths.items()] + [np.full(300, -1)])
    n = cls.size
    kept = (cls >= 0).astype(np.int64)
    tp = np.where(cls == 9, 0, rng.integers(0, 1 << T, n) & np.where(rng.random(n) < 0.6, (1 << T) - 1, 0)) * kept
    score = (rng.integers(1, 2000, n) / np.float32(2000)).astype(np.float32)
    perm = rng.permutation(n)
    rec = dict(kept=kept[perm], cls=cls[perm], score=score[perm], tp=tp[perm])
    gt_count = np.zeros((3, 18), np.int64)
    for c in lengths:
        if c != 9:
            most = max(int((((tp >> q) & 1)[cls == c]).sum()) for q in range(T))
            gt_count[:, c] = [most // 3 + 1, most // 3 + 1, most // 3 + 2]
    rec["gt_count"] = gt_count
    got, want = _device_table(dev, [rec], T), R.table([rec], T)
    assert want[0, 0].tolist() == [0, 0, 0, 1] and want[0, 9].tolist() == [0, 0, 7, 1] and want[0, 7, 3] == 0 and want[0, 6, 2] == 5000
    assert 0 < want[0, 6, 0] < 1
    _assert_tables_close(got, want, ("synth", T))


def test_accumulation_equals_the_host_calculators_and_reset(dev):
    from d3net_amd import evaluator as ev
    batches = R.stream(9, [(3, 33, 12), (2, 128, 40), (1, 256, 128)], "random")
    want = _host_metrics(batches, THRESHOLDS)
    ours = ev.DetectionEvaluator(THRESHOLDS)
    torch.cuda.synchronize()
    for d in batches:
        t = _to(dev, d)
        torch.cuda.set_sync_debug_mode("error")             # add_batch reads nothing back
        try:
            ours.add_batch(t)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    got = ours.compute_metrics()
    assert len(got) == 2
    for q in range(2):
        _assert_metrics_close(got[q], want[q], ("accumulate", THRESHOLDS[q]))
    assert want[0]["mAP"] > 0.05 and want[1]["mAP"] > 0          # a non-degenerate stream
    ours.reset()
    ours.add_batch(_to(dev, batches[1]))
    fresh = ev.DetectionEvaluator(THRESHOLDS)
    fresh.add_batch(_to(dev, batches[1]))
    again, first = ours.compute_metrics(), fresh.compute_metrics()
    assert all(list(a) == list(f) and all(a[k] == f[k] for k in f) for a, f in zip(again, first))
    _assert_metrics_close(again[1], _host_metrics(batches[1:2], (0.5,))[0], "after reset")


def test_range_violations_leave_the_outputs_untouched(dev):
    from d3net_amd import _lib
    untouched = lambda out: all((out[k] == -7).all() for k in ("kept", "cls", "score", "ovmax", "jmax", "tp", "gt_count"))
    for shape, thr, T in (((1, 257, 4), THRESHOLDS, None), ((1, 4, 257), THRESHOLDS, None), ((1, 4, 4), THRESHOLDS, 0), ((1, 4, 4), THRESHOLDS, 5)):
        d = R.stream(3, [shape])[0]
        rc, out = _raw_match(dev, d, d["proposal_batch_mask"], thr, T=T)
        assert rc == -2 and untouched(out) and out["status"][0] == 0, (shape, T)          # D3_ERR_RANGE before any launch
    rc, out = _raw_match(dev, R.stream(3, [(1, 4, 4)])[0], np.ones((1, 4), np.float32), THRESHOLDS)
    assert rc == 0 and not untouched(out)
    tp = torch.zeros(4, dtype=torch.int32, device=dev)
    off = torch.zeros(19, dtype=torch.int32, device=dev)
    cnt = torch.zeros((1, 18), dtype=torch.int32, device=dev)
    table = torch.full((4, 18, 4), -7.0, dtype=torch.float64, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    for T in (0, 5):
        assert _lib.lib().d3_det_ap(p(tp), p(off), p(cnt), 1, 4, 18, T, p(table), None) == -2
    torch.cuda.synchronize()
    assert (table == -7).all()


def test_non_finite_coordinates(dev):
    from d3net_amd import evaluator as ev, _lib
    d = R.stream(11, [(2, 64, 12)], "random")[0]
    d["gt_bbox_label"][0, -1] = 0                                                  # a masked GT slot
    host = {k: torch.from_numpy(v.copy()) for k, v in d.items()}
    ev.parse_predictions(host, device_nms=False)
    rec = R.batch_records(d, np.asarray(host["pred_mask"]), CONF, THRESHOLDS)
    kb, kk = [int(x[0]) for x in np.where(rec["kept"] == 1)]
    unpicked = int(np.where(d["proposal_batch_mask"][0] == 0)[0][0])
    low = int(np.where((d["proposal_scores_batched"][1] < CONF) & (d["proposal_batch_mask"][1] == 1))[0][0])

    def run(dd):
        e = ev.DetectionEvaluator(THRESHOLDS)
        e.add_batch(_to(dev, dd))
        return e.compute_metrics()

    clean = run(d)
    harmless = {k: v.copy() for k, v in d.items()}
    harmless["proposal_bbox_batched"][0, unpicked, 3, 1] = np.nan                  # not a valid proposal: never picked
    harmless["proposal_bbox_batched"][1, low, 0, 0] = np.inf                       # below conf_thresh
    harmless["gt_bbox"][0, -1, 5, 2] = np.nan                                      # masked GT slot
    got = run(harmless)
    assert all(list(a) == list(b) and all(a[k] == b[k] for k in b) for a, b in zip(got, clean))
    bad = {k: v.copy() for k, v in d.items()}
    bad["proposal_bbox_batched"][kb, kk, 2, 0] = np.nan
    with pytest.raises(_lib.D3Error):
        run(bad)
    bad = {k: v.copy() for k, v in d.items()}
    bad["gt_bbox"][1, 0, 0, 0] = np.inf                                            # a valid GT box
    with pytest.raises(_lib.D3Error):
        run(bad)


SGN = R.SGN


def _with_gt(batch, dev):
    c, s = batch["center_label"].cpu().numpy(), batch["size_label"].cpu().numpy()
    cls = batch["sem_cls_label"].cpu().numpy() - 2
    cls[cls < 0] = 17
    batch.update(gt_bbox=torch.from_numpy((c[:, :, None] + SGN[None, None] * s[:, :, None] / 2).astype(np.float32)).to(dev),
                 gt_bbox_label=batch["box_label_mask"].to(dev), sem_cls_label=torch.from_numpy(cls).to(dev))
    return batch


def test_evaluate_detection_equals_the_host_path_on_the_same_feed_outputs(dev):
    from d3net_amd import synthetic as S, evaluator as ev
    from d3net_amd.config import default_conf
    from d3net_amd.pointgroup import PointGroup
    cfg = default_conf(overrides={"model": {"blocks": [1, 2, 3]}})
    torch.manual_seed(1)
    model = PointGroup(cfg).to(dev).train()
    model.teacher = True
    with torch.no_grad():   # confident objectness so that proposals pass TEST_SCORE_THRESH whatever the random ScoreNet says
        model.score_linear.bias.fill_(3.0)
    batches = [_with_gt(S.make_batch([S.small_scene(dims=(44, 36, 20), n_boxes=4, seed=seed)], dev), dev) for seed in (3, 4)]

    class Recording(ev.DetectionEvaluator):
        seen = []

        def add_batch(self, data_dict):
            self.seen.append({k: data_dict[k].detach().cpu().clone() for k in R.KEYS})
            super().add_batch(data_dict)

    rec = Recording(THRESHOLDS)
    got = model.evaluate_detection(batches, rec)
    assert model.training and len(rec.seen) == 2
    want = _host_metrics(rec.seen, THRESHOLDS)
    assert rec.table[:, :, 2].sum() > 0                    # there are detections to score
    for q in range(2):
        _assert_metrics_close(got[q], want[q], ("evaluate_detection", THRESHOLDS[q]))
    model.eval()
    model.evaluate_detection(batches[:1])
    assert not model.training
