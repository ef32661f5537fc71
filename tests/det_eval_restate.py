"""Plain numpy restatement of csrc/det_eval.hip: the order-free true-positive rule of d3_det_match and the AP pass of d3_det_ap,
with exactly tied scores in the stable order the device defines (descending score, scene sequence number, proposal index).
A test helper: tests/test_det_eval.py pins it against d3net_amd.evaluator.eval_det and the reference's golden numbers, the GPU
tests compare the kernels with it.  Also the seeded input streams both test files share."""
import numpy as np

from d3net_amd import evaluator as ev

SGN = np.array([[1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1], [1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1]], np.float32)
KEYS = ("proposal_bbox_batched", "proposal_sem_cls_batched", "proposal_batch_mask", "proposal_scores_batched",
        "gt_bbox", "gt_bbox_label", "sem_cls_label")
FAMILIES = ("random", "integer_grid", "duplicated_proposals", "identical_gt", "empty_scenes")


def map_classes(sem):
    cls = np.asarray(sem, np.float64) - 2
    cls[cls < 0] = 17
    ci = cls.astype(np.int64)
    return np.where(ci == cls, ci, -1)


def match(boxes, cls, scores, pick, conf, gt, gt_mask, gt_cls, thresholds, num_class=18):
    """one batch: boxes (B,K,8,3), cls (B,K) mapped ints, scores (B,K) float32, pick (B,K), gt (B,G,8,3), gt_mask, gt_cls (B,G)
    -> dict kept, cls, ovmax (float64), jmax, tp (bit q per threshold) (B,K); gt_count (B,num_class)"""
    B, K = scores.shape
    G = gt_mask.shape[1]
    kept = (pick == 1) & (scores > np.float32(conf)) & (cls >= 0) & (cls < num_class)
    ovmax, jmax = np.full((B, K), -np.inf), np.full((B, K), -1, np.int64)
    tp, gt_count = np.zeros((B, K), np.int64), np.zeros((B, num_class), np.int64)
    for b in range(B):
        valid = gt_mask[b] == 1
        for c in range(num_class):
            gt_count[b, c] = int((valid & (gt_cls[b] == c)).sum())
        for d in np.where(kept[b])[0]:
            bb = boxes[b, d].astype(float)
            for j in range(G):
                if valid[j] and gt_cls[b, j] == cls[b, d]:
                    iou = ev.box3d_iou(bb, gt[b, j].astype(float))
                    if iou > ovmax[b, d]:
                        ovmax[b, d], jmax[b, d] = iou, j
        for d in np.where(kept[b] & (jmax[b] >= 0))[0]:
            s = scores[b, d]
            earlier = kept[b] & (cls[b] == cls[b, d]) & (jmax[b] == jmax[b, d]) & ((scores[b] > s) | ((scores[b] == s) & (np.arange(K) < d)))
            for q, thr in enumerate(thresholds):
                if ovmax[b, d] > thr and not (ovmax[b][earlier] > thr).any():
                    tp[b, d] |= 1 << q
    return dict(kept=kept.astype(np.int64), cls=np.where(kept, cls, -1), ovmax=ovmax, jmax=jmax, tp=tp, gt_count=gt_count,
                score=scores + np.float32(0))


def curves(kept, cls, score, tp, gt_count, q, c):
    """flat records in record order -> rec, prec, ap, npos of class c at threshold index q (eval_det.py:138-158)"""
    idx = np.where((kept == 1) & (cls == c))[0]
    idx = idx[np.argsort(-score[idx], kind="stable")]
    npos = int(gt_count[:, c].sum()) if len(gt_count) else 0
    t = ((tp[idx] >> q) & 1).astype(np.float64)
    f = 1.0 - t
    f, t = np.cumsum(f), np.cumsum(t)
    rec = t / float(npos + 1e-8)
    prec = t / np.maximum(t + f, np.finfo(np.float64).eps)
    return rec, prec, ev.voc_ap(rec, prec), npos


def table(records, T, num_class=18):
    """records: list of match() dicts (one per batch, in order) -> (T,num_class,4) = AP, last recall, detections, present"""
    flat = {k: np.concatenate([r[k].reshape(-1) for r in records]) for k in ("kept", "cls", "score", "tp")}
    gt_count = np.concatenate([r["gt_count"] for r in records])
    out = np.zeros((T, num_class, 4))
    for q in range(T):
        for c in range(num_class):
            rec, _, ap, npos = curves(flat["kept"], flat["cls"], flat["score"], flat["tp"], gt_count, q, c)
            out[q, c] = ap, (rec[-1] if len(rec) else 0.0), len(rec), float(npos > 0 or len(rec) > 0)
    return out


def metrics(tab):
    """table -> the dicts APCalculator.compute_metrics returns, one per threshold"""
    out = []
    for t in tab:
        present = [c for c in range(t.shape[0]) if t[c, 3] == 1]
        ret = {"%d Average Precision" % c: t[c, 0] for c in present}
        ret["mAP"] = np.mean([t[c, 0] for c in present])
        ret.update({"%d Recall" % c: t[c, 1] for c in present})
        ret["AR"] = np.mean([t[c, 1] for c in present])
        out.append(ret)
    return out


def batch_records(d, pick, conf, thresholds, num_class=18):
    """match() of one batch given as the seven numpy arrays of KEYS and the NMS mask"""
    return match(d[KEYS[0]], map_classes(d[KEYS[1]]), d[KEYS[3]], pick, conf, d[KEYS[4]], d[KEYS[5]], d[KEYS[6]], thresholds, num_class)


# ------------------------------------------------------------------------------------------------- seeded inputs
def stream(seed, shapes, family="random", tie_free=True):
    """-> one dict of the seven numpy arrays per (B, K, G) in `shapes`.  Scores are distinct float32 values over the WHOLE stream
    when tie_free (numpy's argsort leaves tied scores to its sort), else drawn from eight values.  GT classes 0..5; proposals
    carry their GT box's class, some a random one, some class 16 that no GT box has (a prediction-only class)."""
    rng = np.random.default_rng(seed)
    total = sum(B * K for B, K, _ in shapes)
    pool = ((rng.permutation(total) + 1) / np.float64(total + 1)).astype(np.float32)
    assert not tie_free or len(np.unique(pool)) == total
    if not tie_free:
        pool = (rng.integers(1, 9, total) / np.float32(8)).astype(np.float32)
    room, out, at = np.array([4, 3, 2], np.float32), [], 0
    for B, K, G in shapes:
        if family == "integer_grid":
            gc, gs = rng.integers(0, 4, (B, G, 3)).astype(np.float32), rng.integers(1, 3, (B, G, 3)).astype(np.float32) * 2
            pc, ps = rng.integers(0, 4, (B, K, 3)).astype(np.float32), rng.integers(1, 3, (B, K, 3)).astype(np.float32) * 2
        else:
            gc, gs = rng.random((B, G, 3)).astype(np.float32) * room, rng.random((B, G, 3)).astype(np.float32) * 0.9 + 0.3
            pc, ps = rng.random((B, K, 3)).astype(np.float32) * room, rng.random((B, K, 3)).astype(np.float32) * 0.9 + 0.3
        gt_cls = rng.integers(0, 6, (B, G)).astype(np.int64)
        sem = rng.integers(0, 9, (B, K)).astype(np.float32)            # 0 / 1 -> class 17
        m = min(K, G)
        for b in range(B if family != "integer_grid" else 0):          # some proposals are jittered GT boxes, in shuffled slots
            slots = rng.permutation(K)[:m]
            pc[b, slots] = gc[b, :m] + rng.normal(0, 0.1, (m, 3)).astype(np.float32)
            ps[b, slots] = gs[b, :m] * rng.uniform(0.8, 1.25, (m, 3)).astype(np.float32)
            sem[b, slots] = np.where(rng.random(m) > 0.15, gt_cls[b, :m] + 2, rng.integers(0, 20, m)).astype(np.float32)
        if family == "integer_grid":
            sem = rng.integers(2, 6, (B, K)).astype(np.float32)
            gt_cls = rng.integers(0, 4, (B, G)).astype(np.int64)
        sem[rng.random((B, K)) < 0.05] = 18                            # class 16: only ever predicted
        gt = gc[:, :, None] + SGN[None, None] * gs[:, :, None] / 2
        pred = pc[:, :, None] + SGN[None, None] * ps[:, :, None] / 2
        nvalid = [G, max(G - 2, 0), G // 2]
        gt_mask = (np.arange(G)[None] < np.array([nvalid[b % 3] for b in range(B)])[:, None]).astype(np.float32)
        pmask = (rng.random((B, K)) < 0.9).astype(np.float32)
        if family == "duplicated_proposals":                           # PointGroup's two clusterings: copies that all claim one GT box
            h = K // 2
            pred[:, 1:2 * h:2], sem[:, 1:2 * h:2] = pred[:, 0:2 * h:2], sem[:, 0:2 * h:2]
        elif family == "identical_gt" and G > 1:
            gt[:, 1], gt_cls[:, 1] = gt[:, 0], gt_cls[:, 0]
        elif family == "empty_scenes":                                 # scene 0 has no valid proposal, scene 1 no GT box
            pmask[0] = 0
            if B > 1:
                gt_mask[1] = 0
        out.append(dict(zip(KEYS, (pred.astype(np.float32), sem, pmask, pool[at:at + B * K].reshape(B, K).copy(),
                                   gt.astype(np.float32), gt_mask, gt_cls))))
        at += B * K
    return out
