"""ScanNet segmentation evaluation of PointGroup's predictions: instance AP over overlaps 0.50:0.95 (+ AP@50 / AP@25), per class
and averaged, and semantic per-class IoU from a confusion matrix -- the numbers of the reference's two evaluators
(lib/evaluation/instance_segmentation.py, lib/evaluation/semantic_segmentation.py, lib/utils/eval.py), without their
per-scene text files.

Split as `evaluator.py` splits the detection metric:
  * the per-point counting (confusion, GT instance sizes / classes, prediction sizes / void / intersections) runs on the device,
    one `d3_seg_eval` call per batch (csrc/seg_eval.hip; integer counts, bit-exact);
  * the matching and AP (assign_instances_for_scene :219-274, evaluate_matches :55-196, compute_averages :199-216,
    get_semantic_iou :28-44) run on the host in float64 numpy over those counts -- an epoch-end metric.
File interop: `write_predictions` / `write_gt` produce the reference's file layout and formats (model/pointgroup.py:603-625,
lib/utils/eval.py:14-56), `evaluate_*_files` score such files (ours or the reference's) through the same device counting."""
import math
import os

import numpy as np

# data/scannet/model_util_scannet.py:13-15
NYU20_CLASS_IDX = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]
NYU20_CLASS_NAME = ['unannotated', 'wall', 'floor', 'cabinet', 'bed', 'chair', 'sofa', 'table', 'door', 'window', 'bookshelf',
                    'picture', 'counter', 'desk', 'curtain', 'refrigerator', 'shower curtain', 'toilet', 'sink', 'bathtub',
                    'otherfurniture']
NUM_IDS = 40                                   # raw class ids 0..39; the reference's confusion is (max id + 1)^2
# semantic IoU: every class but 'unannotated' (semantic_segmentation.py:107-108); instance AP: wall and floor excluded as well
# (instance_segmentation.py:363-369 "for scannet temporarily") -- their GT points count as void there
SEM_CLASS_IDX, SEM_CLASS_NAME = NYU20_CLASS_IDX[1:], NYU20_CLASS_NAME[1:]
INST_CLASS_IDX, INST_CLASS_NAME = NYU20_CLASS_IDX[3:], NYU20_CLASS_NAME[3:]
INST_CLASS_MASK = sum(1 << c for c in INST_CLASS_IDX)

OVERLAPS = np.append(np.arange(0.5, 0.95, 0.05), 0.25)     # instance_segmentation.py:45-52
MIN_REGION_SIZE = 100


# ------------------------------------------------------------------------------------------------ device counting
def count(gt_sem, gt_inst, pred_sem, batch_offsets, pick=None, proposals_idx=None, proposals_offset=None):
    """One d3_seg_eval call over a batch.  gt_sem / gt_inst / pred_sem: (N,) device int tensors (raw class ids; gt_inst 1-based per
    scene, 0 = none); batch_offsets (B+1,) scene boundaries; pick (n,) proposal ids into proposals_offset / proposals_idx (S,2), in
    pick order.  -> dict of numpy int arrays: confusion (40,40), gt_vert / gt_cls (B,G), pred (n,5) = [vert, void, class, scene,
    flags], inter (n,G).  Raises D3Error (D3_ERR_RANGE) when a scene has more instances than the kernel's LDS bound."""
    import torch
    from . import _lib
    from ._call import call, on, ptr, stream
    dev = gt_sem.device
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    gs, gi, ps = i32(gt_sem), i32(gt_inst), i32(pred_sem)
    N = gs.numel()
    if not (gi.numel() == N and ps.numel() == N):
        raise ValueError("gt_sem / gt_inst / pred_sem differ in length")
    bo_h = np.asarray(batch_offsets.cpu() if torch.is_tensor(batch_offsets) else batch_offsets, dtype=np.int64).reshape(-1)
    B = len(bo_h) - 1
    if B < 1 or bo_h[0] < 0 or bo_h[-1] > N or (np.diff(bo_h) < 0).any():
        raise ValueError("batch_offsets must be nondecreasing within [0, N]: %s" % bo_h)
    G = int(gi.max()) if N else 0
    if pick is None:
        pick = torch.zeros(0, dtype=torch.int32, device=dev)
        proposals_idx = torch.zeros((0, 2), dtype=torch.int32, device=dev)
        proposals_offset = torch.zeros(1, dtype=torch.int32, device=dev)
    pk, pidx, poff = i32(pick), i32(proposals_idx), i32(proposals_offset)
    n, P, S = pk.numel(), poff.numel() - 1, pidx.shape[0]
    bo = torch.from_numpy(bo_h.astype(np.int32)).to(dev)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    conf, gts, pst, inter, status = z(NUM_IDS, NUM_IDS), z(B, max(G, 1), 2), z(max(n, 1), 5), z(max(n, 1), max(G, 1)), z(1)
    ws = torch.empty(max(int(_lib.lib().d3_seg_eval_ws_bytes(B, G)), 4), dtype=torch.uint8, device=dev)
    with on(dev):
        call("seg_eval", ptr(gs), ptr(gi), ptr(ps), ptr(bo), B, N, int(np.diff(bo_h).max()), G, ptr(pk), n, ptr(pidx), ptr(poff),
             P, S, INST_CLASS_MASK, ptr(conf), ptr(gts), ptr(pst), ptr(inter), ptr(status), ptr(ws), ws.numel(), stream())
    if int(status.item()):
        raise ValueError("seg_eval: point labels outside [0, 40) or instance ids outside [0, G]")
    gts = gts.cpu().numpy()[:, :G]
    return dict(confusion=conf.cpu().numpy().astype(np.int64), gt_vert=gts[..., 0], gt_cls=gts[..., 1],
                pred=pst.cpu().numpy()[:n], inter=inter.cpu().numpy()[:n, :G])


def round_score(s):
    """the reference's file round trip of a confidence: f"{score:.4f}" written, float() read back (model/pointgroup.py:623)"""
    return float("%.4f" % float(s))


# ------------------------------------------------------------------------------------------------ host matching and AP
def evaluate_matches(scenes, overlaps=OVERLAPS, min_region_size=MIN_REGION_SIZE):
    """AP (1, C, len(overlaps)) over the per-scene counts (instance_segmentation.py:55-196).  A scene is a dict of gt_vert /
    gt_cls (G,), pred_vert / pred_void / pred_cls / pred_conf (n,) in pick order and inter (n, G).  Greedy assignment per
    overlap: GT instances in id order take the first unvisited same-class prediction (pick order) above the overlap; a second
    such prediction turns the lower of the two scores into a false positive; unmatched predictions are false positives unless
    their void + small-GT share is above the overlap; NaN for a class without GT, 0 with GT but no prediction."""
    per_class = []                         # [class][scene] -> (gt_vert, pred_vert, pred_void, pred_conf, inter) of that class
    for c in INST_CLASS_IDX:
        rows = []
        for sc in scenes:
            g = np.nonzero((sc["gt_vert"] > 0) & (sc["gt_cls"] == c))[0]
            p = np.nonzero((sc["pred_cls"] == c) & (sc["pred_vert"] >= min_region_size))[0]
            rows.append((sc["gt_vert"][g].tolist(), sc["pred_vert"][p].tolist(), sc["pred_void"][p].tolist(),
                         [sc["pred_conf"][q] for q in p], sc["inter"][np.ix_(p, g)].tolist()))
        per_class.append(rows)
    ap = np.zeros((1, len(INST_CLASS_IDX), len(overlaps)), np.float64)
    for oi, th in enumerate(overlaps):
        for ci in range(len(INST_CLASS_IDX)):
            y_true, y_score, hard_fn, has_gt, has_pred = [], [], 0, False, False
            for gv, pv, pvoid, pconf, inter in per_class[ci]:
                big = [k for k in range(len(gv)) if gv[k] >= min_region_size]
                has_gt |= bool(big)
                has_pred |= bool(pv)
                visited = [False] * len(pv)
                for k in big:
                    matched, score = False, -math.inf
                    for q in range(len(pv)):
                        i = inter[q][k]
                        if i == 0 or visited[q]:
                            continue
                        if float(i) / (gv[k] + pv[q] - i) > th:
                            if matched:
                                y_true.append(0.); y_score.append(min(score, pconf[q]))
                                score = max(score, pconf[q])
                            else:
                                matched, score, visited[q] = True, pconf[q], True
                    if matched:
                        y_true.append(1.); y_score.append(score)
                    else:
                        hard_fn += 1
                for q in range(len(pv)):
                    hits = [k for k in range(len(gv)) if inter[q][k] > 0]
                    if any(float(inter[q][k]) / (gv[k] + pv[q] - inter[q][k]) > th for k in hits):
                        continue
                    ignore = pvoid[q] + sum(inter[q][k] for k in hits if gv[k] < min_region_size)
                    if float(ignore) / pv[q] <= th:
                        y_true.append(0.); y_score.append(pconf[q])
            if has_gt and has_pred:
                ap[0, ci, oi] = _average_precision(np.array(y_true, np.float64), np.array(y_score, np.float64), hard_fn)
            elif has_gt:
                ap[0, ci, oi] = 0.0
            else:
                ap[0, ci, oi] = float("nan")
    return ap


def _average_precision(y_true, y_score, hard_fn):
    """precision / recall at every distinct score, integrated with the reference's step widths (instance_segmentation.py:153-190)
    -- only the order of the scores matters, not the order the pairs were collected in.  (No scored pair at all: the reference
    fails on an empty cumsum there; the curve is then the artificial point alone and the AP 0.)"""
    if y_score.size == 0:
        return 0.0
    o = np.argsort(y_score)
    ys, cs = y_score[o], np.cumsum(y_true[o])
    _, first = np.unique(ys, return_index=True)
    below = np.append(cs, 0.)[first - 1]           # true examples strictly below each threshold (index -1 -> the appended 0)
    tp = cs[-1] - below
    fp = ys.size - first - tp
    precision = np.append(tp / (tp + fp), 1.)
    recall = np.append(tp / (tp + below + hard_fn), 0.)
    r = np.concatenate([recall[:1], recall, [0.]])
    steps = np.convolve(r, [-0.5, 0, 0.5], "valid")
    return float(np.dot(precision, steps))


def compute_averages(aps):
    """instance_segmentation.py:199-216: AP over 0.50:0.95, AP@50, AP@25, averaged over classes (NaN ignored) and per class"""
    o50, o25 = np.where(np.isclose(OVERLAPS, 0.5)), np.where(np.isclose(OVERLAPS, 0.25))
    rest = np.where(np.logical_not(np.isclose(OVERLAPS, 0.25)))
    out = {"all_ap": np.nanmean(aps[0, :, rest]), "all_ap_50%": np.nanmean(aps[0, :, o50]),
           "all_ap_25%": np.nanmean(aps[0, :, o25]), "classes": {}}
    for ci, name in enumerate(INST_CLASS_NAME):
        out["classes"][name] = {"ap": np.average(aps[0, ci, rest]), "ap50%": np.average(aps[0, ci, o50]),
                                "ap25%": np.average(aps[0, ci, o25])}
    return out


def semantic_iou(confusion):
    """semantic_segmentation.py:28-44 for every class but 'unannotated': name -> (iou, tp, tp + fp + fn), or NaN when that is 0;
    false positives count only predictions on points of the other evaluated classes"""
    out = {}
    for c, name in zip(SEM_CLASS_IDX, SEM_CLASS_NAME):
        tp = np.longlong(confusion[c, c])
        fn = np.longlong(confusion[c, :].sum()) - tp
        fp = np.longlong(confusion[[k for k in SEM_CLASS_IDX if k != c], c].sum())
        denom = tp + fp + fn
        out[name] = float("nan") if denom == 0 else (float(tp) / denom, tp, denom)
    return out


# ------------------------------------------------------------------------------------------------ evaluator
class SegmentationEvaluator:
    """Accumulates scenes; `instance_results()` / `semantic_results()` at the end.  round_scores: confidences rounded to 4
    decimals as the reference's prediction files carry them, so the in-memory and the file route agree."""

    def __init__(self, round_scores=True):
        self.round_scores = round_scores
        self.reset()

    def reset(self):
        self.scenes = []
        self.confusion = np.zeros((NUM_IDS, NUM_IDS), np.int64)
        self.mixed_class_predictions = 0

    def _conf(self, scores):
        # (device scores are float32 and print as the reference prints them; file confidences are already the parsed float64)
        return [round_score(s) if self.round_scores else float(s) for s in np.asarray(scores).reshape(-1)]

    def _add(self, counts, scores, classes=None, semantic=True, instance=True):
        if semantic:
            self.confusion += counts["confusion"]
        if not instance:
            return
        pred, inter = counts["pred"], counts["inter"]
        if (pred[:, 4] & 2).any():
            raise ValueError("seg_eval: a prediction has members outside its scene (or a malformed pick)")
        conf = self._conf(scores)
        cls = pred[:, 2] if classes is None else np.asarray(classes, np.int64).reshape(-1)
        for b in range(counts["gt_vert"].shape[0]):
            sel = np.nonzero(pred[:, 3] == b)[0]
            self.scenes.append(dict(gt_vert=counts["gt_vert"][b], gt_cls=counts["gt_cls"][b], pred_vert=pred[sel, 0],
                                    pred_void=pred[sel, 1], pred_cls=cls[sel], pred_conf=[conf[j] for j in sel], inter=inter[sel]))

    def add_batch(self, pred, data_dict):
        """pred: PointGroup.predict_instances' output for the collated batch `data_dict` (its sem_labels / instance_ids /
        batch_offsets are the GT).  One device call for the whole batch."""
        gt_sem, gt_inst = gt_ids(data_dict)
        counts = count(gt_sem, gt_inst, pred_class_ids(pred["semantic_pred"]), data_dict["batch_offsets"], pred["pick"],
                       pred["proposals_idx"], pred["proposals_offset"])
        # model/pointgroup.py:620 asserts one class per picked cluster; here the first member's class stands and the
        # disagreeing predictions are counted
        self.mixed_class_predictions += int((counts["pred"][:, 4] & 1).sum())
        self._add(counts, pred["scores"].detach().cpu().numpy())

    def add_scene(self, gt_sem, gt_inst, pred_sem=None, pred_members=(), pred_scores=(), pred_classes=None, device=None):
        """One scene from raw per-point arrays: gt_sem (N,) raw GT class ids, gt_inst (N,) 1-based instance ids (0 = none),
        pred_sem (N,) raw predicted class ids (None: instance evaluation only), pred_members: one index array (or (N,) mask)
        per prediction in pick order, pred_scores their confidences, pred_classes their class ids (None: each prediction's
        first member's pred_sem)."""
        import torch
        dev = device or torch.device("cuda", torch.cuda.current_device())
        t = lambda a: torch.as_tensor(np.asarray(a, np.int64)).to(dev)
        N = len(gt_sem)
        members = [np.nonzero(m)[0] if (np.asarray(m).dtype == bool and len(m) == N) else np.asarray(m, np.int64).reshape(-1)
                   for m in pred_members]
        off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
        idx = np.zeros((int(off[-1]), 2), np.int64)
        for j, m in enumerate(members):
            idx[off[j]:off[j + 1], 0], idx[off[j]:off[j + 1], 1] = j, m
        semantic = pred_sem is not None
        counts = count(t(gt_sem), t(gt_inst), t(pred_sem if semantic else np.zeros(N, np.int64)), [0, N],
                       t(np.arange(len(members))), t(idx), t(off))
        self._add(counts, pred_scores, pred_classes, semantic=semantic, instance=True)

    def instance_results(self):
        """-> (compute_averages dict, raw AP array (1, C, 10))"""
        ap = evaluate_matches(self.scenes)
        return compute_averages(ap), ap

    def semantic_results(self):
        """-> ({class name: (iou, tp, denom) or NaN}, confusion (40, 40) [gt][pred])"""
        return semantic_iou(self.confusion), self.confusion.copy()


# ------------------------------------------------------------------------------------------------ label encodings
def pred_class_ids(semantic_pred):
    """per-point argmax over the 20 classes -> raw class id NYU20_CLASS_IDX[1:][argmax] (model/pointgroup.py:561-566)"""
    import torch
    lut = torch.tensor(SEM_CLASS_IDX, dtype=torch.int32, device=semantic_pred.device)
    return lut[semantic_pred.long()]


def gt_ids(data_dict):
    """GT of a collated batch in the reference's GT-file encoding (lib/utils/eval.py:14-56, value = sem * 1000 + inst), as two
    (N,) int32 tensors: class = NYU20_CLASS_IDX[1:][sem_label], 0 for the ignore label; instance = 1 + the scene-local id, 0 for
    none.  Scene-local ids: instance_ids minus the scene's instance_offsets entry (the collated ids run on across scenes); a
    batch without instance_offsets takes the scene's smallest id."""
    import torch
    sem, ins, bo = data_dict["sem_labels"], data_dict["instance_ids"], data_dict["batch_offsets"]
    dev = sem.device
    lut = torch.tensor(SEM_CLASS_IDX, dtype=torch.int32, device=dev)
    valid = (sem >= 0) & (sem < len(SEM_CLASS_IDX))
    gsem = torch.where(valid, lut[sem.clamp(0, len(SEM_CLASS_IDX) - 1)], torch.zeros_like(sem, dtype=torch.int32))
    counts = (bo[1:] - bo[:-1]).long().to(dev)
    scene = torch.repeat_interleave(torch.arange(counts.numel(), device=dev), counts)
    has = ins >= 0
    if "instance_offsets" in data_dict:
        base = data_dict["instance_offsets"].long().to(dev)[:-1]
    else:
        big = torch.full((counts.numel(),), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
        base = big.scatter_reduce(0, scene[has], ins[has].long(), "amin")
    local = torch.where(has, ins.long() - base[scene] + 1, torch.zeros_like(ins, dtype=torch.int64))
    return gsem, local.to(torch.int32)


# ------------------------------------------------------------------------------------------------ file interop
def _scene_arrays(pred, data_dict):
    bo = data_dict["batch_offsets"].cpu().numpy().astype(np.int64)
    sem = pred_class_ids(pred["semantic_pred"]).cpu().numpy()
    pick = pred["pick"].cpu().numpy().astype(np.int64)
    idx, off = pred["proposals_idx"].cpu().numpy(), pred["proposals_offset"].cpu().numpy().astype(np.int64)
    members = [idx[off[c]:off[c + 1], 1].astype(np.int64) for c in pick]
    scores = pred["scores"].detach().cpu().numpy().astype(np.float32)
    return bo, sem, members, scores


def write_predictions(pred, data_dict, root, scene_names, split="val"):
    """predict_instances' output as PointGroup.test writes it (model/pointgroup.py:603-625): <root>/split_pred/<split>/
    semantic/<scene>.txt (raw class id per point), instance/<scene>.txt ("predicted_masks/<scene>_<id:03d>.txt <class>
    <score:.4f>" per picked proposal, pick order), instance/predicted_masks/<scene>_<id:03d>.txt (0/1 per point) and
    instance/<scene>.cluster_ids.txt (the last picked proposal containing the point, -1 for none).  A prediction belongs to
    the scene of its first member."""
    bo, sem, members, scores = _scene_arrays(pred, data_dict)
    base = os.path.join(root, "split_pred", split)
    sem_dir, inst_dir = os.path.join(base, "semantic"), os.path.join(base, "instance")
    mask_dir = os.path.join(inst_dir, "predicted_masks")
    for d in (sem_dir, mask_dir):
        os.makedirs(d, exist_ok=True)
    for b, name in enumerate(scene_names):
        lo, hi = int(bo[b]), int(bo[b + 1])
        np.savetxt(os.path.join(sem_dir, "%s.txt" % name), sem[lo:hi], fmt="%d")
        mine = [j for j, m in enumerate(members) if len(m) and lo <= m[0] < hi]
        cluster_ids = np.full(hi - lo, -1, np.int64)
        with open(os.path.join(inst_dir, "%s.txt" % name), "w") as f:
            for c_id, j in enumerate(mine):
                mask = np.zeros(hi - lo, np.int64)
                mask[members[j] - lo] = 1
                cluster_ids[mask == 1] = c_id
                cls = sem[members[j][0]]     # the first member's class, as the in-memory route takes it (the reference takes the
                                             # first point of the mask; the same wherever the members agree, which it asserts)
                f.write("predicted_masks/%s_%03d.txt %d %.4f\n" % (name, c_id, cls, float(scores[j])))
                np.savetxt(os.path.join(mask_dir, "%s_%03d.txt" % (name, c_id)), mask, fmt="%d")
        np.savetxt(os.path.join(inst_dir, "%s.cluster_ids.txt" % name), cluster_ids, fmt="%d")


def write_gt(data_dict, root, scene_names, split="val"):
    """<root>/split_gt/<split>/<scene>.txt: sem * 1000 + inst per point (lib/utils/eval.py:14-56 encoding, see gt_ids)"""
    gsem, ginst = gt_ids(data_dict)
    enc = (gsem.long() * 1000 + ginst.long()).cpu().numpy()
    bo = data_dict["batch_offsets"].cpu().numpy().astype(np.int64)
    d = os.path.join(root, "split_gt", split)
    os.makedirs(d, exist_ok=True)
    for b, name in enumerate(scene_names):
        np.savetxt(os.path.join(d, "%s.txt" % name), enc[bo[b]:bo[b + 1]], fmt="%d")


def read_ids(path):
    """one integer per line (lib/utils/eval.py:37-56)"""
    return np.loadtxt(path, dtype=np.int64, ndmin=1)


def read_gt(path):
    """-> (class ids, instance ids) of a GT file: value // 1000, value % 1000"""
    v = read_ids(path)
    return v // 1000, v % 1000


def read_instance_predictions(path):
    """an instance prediction file (lib/utils/eval.py:59-72) -> [(mask file, class id, confidence)] in file order"""
    out = []
    for line in open(path).read().splitlines():
        rel, cls, conf = line.split(" ")
        out.append((os.path.join(os.path.dirname(path), rel), int(cls), float(conf)))
    return out


def evaluate_instance_files(pred_files, gt_files, evaluator=None, device=None):
    """instance AP of per-scene prediction / GT files (the reference's or ours), counted on the device -> instance_results()"""
    ev = evaluator or SegmentationEvaluator(round_scores=False)
    for pf, gf in zip(pred_files, gt_files):
        gsem, ginst = read_gt(gf)
        preds = read_instance_predictions(pf)
        masks = [read_ids(m) != 0 for m, _, _ in preds]
        if any(len(m) != len(gsem) for m in masks):
            raise ValueError("a mask of %s differs in length from %s" % (pf, gf))
        ev.add_scene(gsem, ginst, None, masks, [c for _, _, c in preds], [c for _, c, _ in preds], device=device)
    return ev.instance_results()


def evaluate_semantic_files(pred_files, gt_files, evaluator=None, device=None):
    """semantic IoU of per-scene prediction / GT files, counted on the device -> semantic_results()"""
    import torch
    ev = evaluator or SegmentationEvaluator()
    dev = device or torch.device("cuda", torch.cuda.current_device())
    for pf, gf in zip(pred_files, gt_files):
        gsem, ginst = read_gt(gf)
        psem = read_ids(pf)
        if len(psem) != len(gsem):
            raise ValueError("%s and %s differ in length" % (pf, gf))
        t = lambda a: torch.from_numpy(a).to(dev)
        ev._add(count(t(gsem), t(np.zeros_like(ginst)), t(psem), [0, len(gsem)]), [], semantic=True, instance=False)
    return ev.semantic_results()
