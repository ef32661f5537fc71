"""Plain numpy restatement of csrc/grounding_eval.hip's per-row rule and of the table scripts/eval.py:305-426 forms from the rows.
A test helper that shares no code with d3net_amd.grounding_eval: tests/test_grounding_epoch.py pins it against the reference's own
numbers (tests/golden/grounding_epoch_golden.npz), the GPU tests compare the kernel and the evaluator with it on random epochs."""
import numpy as np

F = np.float32
SGN = np.array([[1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1], [1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1]], np.float32)
MULTIPLE = {"unique": 0, "multiple": 1}
OTHERS = {"not_in_others": 0, "in_others": 1}
METRICS = ("ref_acc", "acc@0.25iou", "acc@0.5iou")


def argmax(x):
    """torch.argmax on the CPU: the lowest NaN if there is one, else the lowest index of the maximum (+0 == -0)"""
    x = np.asarray(x, np.float32)
    nan = np.flatnonzero(x != x)
    if nan.size:
        return int(nan[0])
    best = 0
    for i in range(1, x.size):
        if x[i] > x[best]:
            best = i
    return best


def aabb_iou(c1, c2):
    """lib/utils/bbox.py:221-244 in float32, one operation at a time"""
    c1, c2 = np.asarray(c1, np.float32), np.asarray(c2, np.float32)
    lo1, hi1, lo2, hi2 = c1.min(0), c1.max(0), c2.min(0), c2.max(0)
    with np.errstate(all="ignore"):
        d = np.maximum(np.minimum(hi1, hi2) - np.maximum(lo1, lo2), F(0))
        inter = F(F(d[0] * d[1]) * d[2])
        e1, e2 = hi1 - lo1, hi2 - lo2
        v1, v2 = F(F(e1[0] * e1[1]) * e1[2]), F(F(e2[0] * e2[1]) * e2[2])
        return F(inter / F(F(F(v1 + v2) - inter) + F(1e-8)))


def batch_rows(d, use_lang=True):
    """one batch (numpy arrays under the evaluator's keys) -> per-row dict of arrays"""
    ref, labels = np.asarray(d["cluster_ref"], np.float32), np.asarray(d["cluster_labels"], np.float32)
    boxes = np.asarray(d["proposal_bbox_batched"], np.float32)
    N, K = ref.shape
    B = boxes.shape[0]
    Cn = N // B
    valid = (np.asarray(d["proposal_batch_mask"]).astype(np.int64) == 1).astype(np.float32)
    gt = np.asarray(d["ref_box_corner_label"], np.float32).reshape(N, 8, 3)
    um, cat = np.asarray(d["unique_multiple"]).reshape(-1), np.asarray(d["object_cat"]).reshape(-1)
    out = {k: np.zeros(N, np.int64) for k in ("top", "pred_ref", "gt_ref", "ref_acc", "lang_ok", "m", "o")}
    out.update(iou=np.zeros(N, np.float32), best_iou=np.zeros(N, np.float32), pred_bbox=np.zeros((N, 8, 3), np.float32), gt_bbox=gt.copy(),
               bad=np.zeros(N, bool))
    for n in range(N):
        b = n // Cn
        with np.errstate(invalid="ignore"):
            masked = (ref[n] * valid[b]).astype(np.float32)
        top, pr, gr = argmax(ref[n]), argmax(masked), argmax(labels[n])
        out["top"][n], out["pred_ref"][n], out["gt_ref"][n] = top, pr, gr
        out["ref_acc"][n] = int(labels[n, top] == 1)
        out["iou"][n], out["best_iou"][n] = aabb_iou(boxes[b, pr], gt[n]), aabb_iou(boxes[b, gr], gt[n])
        out["pred_bbox"][n] = boxes[b, pr]
        out["bad"][n] = not (np.isfinite(boxes[b, pr]).all() and np.isfinite(boxes[b, gr]).all() and np.isfinite(gt[n]).all())
        out["m"][n] = um[n] if um[n] in (0, 1) else 2
        out["o"][n] = int(cat[n] == 17)
        if use_lang:
            out["lang_ok"][n] = int(argmax(d["lang_scores"][n]) == cat[n])
    out["unique_multiple"], out["ids"] = um.astype(np.int64), None
    if "id" in d and "chunk_ids" in d:
        out["ids"] = np.stack([np.repeat(np.asarray(d["id"]), Cn), np.asarray(d["chunk_ids"]).reshape(-1)], 1).astype(np.int64)
    return out


def table(rows):
    """(3,2,4) int64 cell counts {rows, ref_acc, iou >= 0.25, iou >= 0.5} of per-row arrays"""
    t = np.zeros((3, 2, 4), np.int64)
    for m, o, a, iou in zip(rows["m"], rows["o"], rows["ref_acc"], rows["iou"]):
        t[m, o] += [1, int(a), int(iou >= F(0.25)), int(iou >= F(0.5))]         # a NaN compares false
    return t


def aggregate(masks, others, ref_acc, ious, lang_acc):
    """scripts/eval.py:305-426 on the (repeat, row) arrays it unpacks, by boolean selections as the reference writes them
    -> stats, scores, mean language accuracy"""
    masks, others, ref_acc, ious = (np.asarray(x) for x in (masks, others, ref_acc, ious))
    R = masks.shape[0]
    sel_m = {k: [masks[i] == v for i in range(R)] for k, v in MULTIPLE.items()}
    sel_m["overall"] = [np.ones(masks.shape[1], bool) for _ in range(R)]
    sel_o = {k: [others[i] == v for i in range(R)] for k, v in OTHERS.items()}
    sel_o["overall"] = sel_m["overall"]
    stats, scores = {}, {}
    for k in ("unique", "multiple", "overall"):
        stats[k], scores[k] = {}, {}
        for k_o in ("not_in_others", "in_others", "overall"):
            accs = {m: [] for m in METRICS}
            for i in range(R):
                s = sel_m[k][i] & sel_o[k_o][i]
                n = int(s.sum())
                accs["ref_acc"].append(np.mean(ref_acc[i][s].astype(np.float64)) if n else 0)
                accs["acc@0.25iou"].append(int((ious[i][s] >= 0.25).sum()) / n if n else 0)
                accs["acc@0.5iou"].append(int((ious[i][s] >= 0.5).sum()) / n if n else 0)
            stats[k][k_o] = int((sel_m[k][0] & sel_o[k_o][0]).sum())
            scores[k][k_o] = {m: np.mean(accs[m]) for m in METRICS}
    return stats, scores, float(np.mean(np.asarray(lang_acc, np.float64))) if np.size(lang_acc) else 0.0


def epoch(repeats, use_lang=True):
    """[repeat][batch] input dicts -> dict(tables (R,3,2,4), lang_correct, lang_rows, rows [repeat][batch], stats, scores, lang_acc,
    status)"""
    tables, rows_all, lang_correct, lang_rows, lang_acc, lists, bad = [], [], [], [], [], [], False
    for rep in repeats:
        rows = [batch_rows(d, use_lang) for d in rep]
        rows_all.append(rows)
        tables.append(sum(table(r) for r in rows))
        cat = lambda k: np.concatenate([r[k] for r in rows])
        lists.append((cat("unique_multiple"), cat("o"), cat("ref_acc"), cat("iou")))
        for r in rows:
            lang_correct.append(int(r["lang_ok"].sum())); lang_rows.append(len(r["lang_ok"]))
            lang_acc.append(float(F(r["lang_ok"].sum()) / F(len(r["lang_ok"]))) if use_lang else 0.0)
            bad = bad or bool(r["bad"].any())
    stats, scores, la = aggregate(*[[l[i] for l in lists] for i in range(4)], lang_acc)
    return dict(tables=np.stack(tables), lang_correct=lang_correct, lang_rows=lang_rows, rows=rows_all, stats=stats, scores=scores,
                lang_acc=la, status=int(bad))


def random_epoch(seed, shapes, L=18, nan_rate=0.02):
    """[repeat][batch] dicts at `shapes` = ((B, C, K), ...) per repeat: quantised scores (many exact ties), sparse masks, some
    all-negative rows, NaN scores, all-zero label rows, unique_multiple in {0, 1, 2}, IoUs away from the thresholds by rejection"""
    rng = np.random.default_rng(seed)
    out = []
    for rep in shapes:
        batches = []
        for B, Cn, K in rep:
            N = B * Cn
            while True:
                mask = (rng.random((B, K)) < 0.5).astype(np.float32)
                c = rng.random((B, K, 3)).astype(np.float32) * np.array([2, 2, 1], np.float32)
                s = rng.random((B, K, 3)).astype(np.float32) * 0.9 + 0.3
                corners = (c[:, :, None] + SGN[None, None] * s[:, :, None] / 2).astype(np.float32)
                ref = (rng.integers(-6, 7, (N, K)) / 4).astype(np.float32)
                ref[rng.random((N, K)) < nan_rate] = np.nan
                neg = rng.random(N) < 0.25
                ref[neg] = -np.abs(ref[neg]) - 0.25
                labels = np.zeros((N, K), np.float32)
                labels[np.arange(N), rng.integers(0, K, N)] = 1
                labels[rng.random(N) < 0.15] = 0
                gt = np.stack([corners[n // Cn, rng.integers(K)] + rng.normal(0, 0.1, (1, 3)).astype(np.float32) for n in range(N)])
                cat = rng.integers(0, L, (B, Cn)).astype(np.int64)
                cat[rng.random((B, Cn)) < 0.3] = 17
                lang = (rng.integers(-4, 5, (N, L)) / 2).astype(np.float32)
                d = dict(proposal_batch_mask=mask, proposal_bbox_batched=corners, cluster_ref=ref, cluster_labels=labels,
                         ref_box_corner_label=gt.reshape(B, Cn, 8, 3).astype(np.float32), unique_multiple=rng.integers(0, 3, (B, Cn)).astype(np.int64),
                         object_cat=cat, lang_scores=lang, id=rng.integers(0, 50, B).astype(np.int64),
                         chunk_ids=rng.integers(0, 9, (B, Cn)).astype(np.int64))
                iou = batch_rows(d)["iou"].astype(np.float64)
                if min(np.abs(iou - 0.25).min(), np.abs(iou - 0.5).min()) > 1e-5:
                    break
            batches.append(d)
        out.append(batches)
    return out
