"""Grounding evaluation: the reference's `lib/grounding/eval_helper.py:28-137 get_eval`
on batched tensors -- the referred-box prediction, its AABB IoU with the GT box, the pseudo-GT ("best") IoU, Acc@0.25 /
Acc@0.5, the unique / multiple and "others" masks and the language-classification accuracy -- without the reference's
per-sample python loop and per-sample device->host copies (eval_helper.py:92-116: one `.cpu().numpy()` IoU per
description).  Pinned to golden vectors produced by the reference's own function (tests/golden/gen_grounding_eval_golden.py).

The epoch form runs on the device (`GroundingEvaluator`): scripts/eval.py:168-426 `eval_grounding` -- the
Acc@kIoU / ref_acc table over unique / multiple / overall x in_others / not_in_others / overall, averaged over the repeats, the
language-classification accuracy and the per-annotation predictions.  Per batch csrc/grounding_eval.hip's d3_ground_eval_batch adds
every description to integer cell counters with no read-back and without the (N, K) IoU matrix `get_eval` builds; the floating
point of the table stays on the host (`grounding_scores`), in the reference's float64 operations, so the scores equal the numbers
the reference prints (tests/golden/gen_grounding_epoch_golden.py).  `get_eval` stays as it is: the per-batch form with the
reference's return keys.
"""
import torch

from .listener import aabb_iou_to_gt


def get_eval(data_dict, grounding=True, use_lang_classifier=False):
    mask = (data_dict["proposal_batch_mask"].long() == 1).float()                  # (B, K)
    cluster_ref = data_dict["cluster_ref"]                                        # (B*C, K)
    N, K = cluster_ref.shape
    chunk = N // mask.shape[0]
    pred_masks = mask.unsqueeze(1).repeat(1, chunk, 1).reshape(N, K)
    labels = data_dict["cluster_labels"].float()

    # classification accuracy of the arg-max proposal (over ALL slots, as the reference: eval_helper.py:51-60)
    top = torch.argmax(cluster_ref, 1)
    corrects = (labels.gather(1, top.unsqueeze(1)).squeeze(1) == 1).float()
    ref_acc = corrects / (1.0 + 1e-8)
    data_dict["ref_acc"] = ref_acc.cpu().numpy().tolist()
    data_dict["ref_acc_mean"] = ref_acc.mean()

    # localisation: arg-max over the valid proposals, IoU with the referred box; pseudo-GT IoU
    masked = cluster_ref * pred_masks
    pred_ref = torch.argmax(masked, 1)
    data_dict["cluster_ref"] = masked
    corners = data_dict["proposal_bbox_batched"].unsqueeze(1).repeat(1, chunk, 1, 1, 1).reshape(N, K, 8, 3)
    gt = data_dict["ref_box_corner_label"].reshape(N, 8, 3)
    all_ious = aabb_iou_to_gt(corners, gt)                                         # (N, K)
    ious = all_ious.gather(1, pred_ref.unsqueeze(1)).squeeze(1)
    gt_ref = torch.argmax(labels, 1)
    best_ious = all_ious.gather(1, gt_ref.unsqueeze(1)).squeeze(1)
    rows = torch.arange(N, device=corners.device)
    object_cat = data_dict["object_cat"].reshape(-1)

    if grounding and use_lang_classifier:
        data_dict["lang_acc"] = (torch.argmax(data_dict["lang_scores"], 1) == object_cat).float().mean()
    else:
        data_dict["lang_acc"] = torch.zeros(1)[0].type_as(ious)

    data_dict["ref_iou"] = ious
    data_dict["best_ious"] = best_ious
    data_dict["ref_iou_mean"] = ious.mean()
    data_dict["best_ious_mean"] = best_ious.mean()
    data_dict["ref_iou_rate_0.25"] = float((ious >= 0.25).sum()) / N
    data_dict["ref_iou_rate_0.5"] = float((ious >= 0.5).sum()) / N
    data_dict["ref_multiple_mask"] = data_dict["unique_multiple"].reshape(-1).cpu().tolist()
    data_dict["ref_others_mask"] = (object_cat == 17).long().cpu().tolist()
    data_dict["pred_bboxes"] = corners[rows, pred_ref]
    data_dict["gt_bboxes"] = gt
    return data_dict


# ---------------------------------------------------------------------------------------------------- the device form
GROUND_MAX_K, GROUND_MAX_LANG = 4096, 64             # proposal slots per scene / language classes of csrc/grounding_eval.hip
_MULTIPLE = (("unique", 0), ("multiple", 1))          # scripts/eval.py:305-312
_OTHERS = (("not_in_others", 0), ("in_others", 1))
_METRICS = ("ref_acc", "acc@0.25iou", "acc@0.5iou")
_GROUND_KEYS = ("cluster_ref", "cluster_labels", "proposal_batch_mask", "proposal_bbox_batched", "ref_box_corner_label",
                "unique_multiple", "object_cat")
_INTS = (torch.int32, torch.int64)


def grounding_scores(tables, lang_correct=(), lang_rows=()):
    """The host half of `GroundingEvaluator.compute`, scripts/eval.py:305-426 from integers: tables (R,3,2,4) = per repeat and cell
    [unique_multiple 0 / 1 / other][object_cat == 17] the counts {rows, ref_acc, iou >= 0.25, iou >= 0.5}; lang_correct / lang_rows:
    per (repeat, batch) the correct language classifications and the batch's rows -> (stats, scores, lang_acc).  float64 where the
    reference is: a score is the np.mean over the repeats of count / rows (0 for an empty cell), stats are repeat 0's row counts."""
    import numpy as np
    tables = np.asarray(tables, np.int64).reshape(-1, 3, 2, 4)
    if tables.shape[0] < 1:
        raise ValueError("grounding_scores: no repeat")
    picks = {k: [v] for k, v in _MULTIPLE}
    picks["overall"] = [0, 1, 2]                       # every row: a unique_multiple outside {0, 1} counts only here
    opicks = {k: [v] for k, v in _OTHERS}
    opicks["overall"] = [0, 1]
    stats, scores = {}, {}
    for k, ms in picks.items():
        stats[k], scores[k] = {}, {}
        for k_o, os_ in opicks.items():
            cells = tables[:, ms][:, :, os_].sum(axis=(1, 2))          # (R, 4) integer margins
            stats[k][k_o] = int(cells[0, 0])
            scores[k][k_o] = {}
            for q, metric in enumerate(_METRICS):
                per_repeat = [int(c[q + 1]) / int(c[0]) if c[0] > 0 else 0 for c in cells]
                scores[k][k_o][metric] = np.mean(per_repeat)
    if len(lang_rows):
        per_batch = [float(np.float32(c) / np.float32(n)) for c, n in zip(lang_correct, lang_rows)]      # the batch's float32 mean
        lang_acc = float(np.mean(np.array(per_batch)))
    else:
        lang_acc = 0.0
    return stats, scores, lang_acc


class GroundingEvaluator:
    """scripts/eval.py:168-426 (eval_grounding) on the device: `add_batch` takes the dict as it leaves
    `PipelineNet._ground(self.listener(...), False)` and runs one d3_ground_eval_batch launch (csrc/grounding_eval.hip) that adds the
    batch to the repeat's (3,2,4) integer table -- nothing is read back, the (N,K) IoU matrix and the repeated boxes of `get_eval` are
    never built; `begin_repeat` starts the table of the next seed (the first repeat is implicit); `compute` reads the tables, the
    per-batch language counts and the status back once and forms Acc@kIoU / ref_acc, unique / multiple / overall x in_others /
    not_in_others / overall, averaged over the repeats, with the reference's key names.  keep_predictions: the per-description
    records of the last repeat stay on the device (storage doubles, device-to-device) and `predictions` reads them back once."""

    def __init__(self, use_lang_classifier=True, keep_predictions=False, device="cuda"):
        self.use_lang_classifier, self.keep_predictions, self.device = bool(use_lang_classifier), bool(keep_predictions), torch.device(device)
        self.reset()

    def reset(self):
        self._tables = self._lang = self._status = self._rec = None
        self._repeat, self._lang_rows, self._rows, self.tables = -1, [], 0, None

    def begin_repeat(self):
        self._repeat += 1
        self._rows = 0                                  # the records are the last repeat's (scripts/eval.py:196, 264-266)

    def _checked(self, d):
        name = "GroundingEvaluator.add_batch"
        keys = _GROUND_KEYS + (("lang_scores",) if self.use_lang_classifier else ()) + (("id", "chunk_ids") if self.keep_predictions else ())
        missing = [k for k in keys if k not in d]
        if missing:
            raise ValueError("%s: missing %s" % (name, missing))
        for k in keys:
            if not torch.is_tensor(d[k]):
                raise ValueError("%s: %s must be a tensor" % (name, k))
        ref, labels, mask, boxes, gt = (d[k] for k in _GROUND_KEYS[:5])
        if ref.dim() != 2 or boxes.dim() != 4 or tuple(boxes.shape[2:]) != (8, 3) or mask.dim() != 2:
            raise ValueError("%s: cluster_ref (N,K), proposal_batch_mask (B,K) and proposal_bbox_batched (B,K,8,3) expected" % name)
        (N, K), B = ref.shape, boxes.shape[0]
        if B < 1 or N < 1 or N % B or not 1 <= K <= GROUND_MAX_K:
            raise ValueError("%s: B >= 1, N = B * C >= 1 and 1 <= K <= %d (got B %d, N %d, K %d)" % (name, GROUND_MAX_K, B, N, K))
        Cn = N // B
        want = {"cluster_labels": ((N, K),), "proposal_batch_mask": ((B, K),), "proposal_bbox_batched": ((B, K, 8, 3),),
                "ref_box_corner_label": ((B, Cn, 8, 3), (N, 8, 3)), "unique_multiple": ((B, Cn), (N,)), "object_cat": ((B, Cn), (N,)),
                "id": ((B,),), "chunk_ids": ((B, Cn),)}
        for k in keys:
            if k in want and tuple(d[k].shape) not in want[k]:
                raise ValueError("%s: %s has shape %s, expected %s" % (name, k, tuple(d[k].shape), " or ".join(map(str, want[k]))))
        floats, flags = (torch.float32,), (torch.float32, torch.bool, torch.uint8) + _INTS
        ok = {"cluster_ref": floats, "cluster_labels": flags, "proposal_batch_mask": flags, "proposal_bbox_batched": floats,
              "ref_box_corner_label": floats, "unique_multiple": _INTS, "object_cat": _INTS, "lang_scores": floats, "id": _INTS,
              "chunk_ids": _INTS}
        for k in keys:
            if d[k].dtype not in ok[k]:
                raise ValueError("%s: %s has dtype %s, expected one of %s" % (name, k, d[k].dtype, ok[k]))
        L = 0
        if self.use_lang_classifier:
            ls = d["lang_scores"]
            if ls.dim() != 2 or ls.shape[0] != N or not 1 <= ls.shape[1] <= GROUND_MAX_LANG:
                raise ValueError("%s: lang_scores must be (%d, L) with 1 <= L <= %d, got %s" % (name, N, GROUND_MAX_LANG, tuple(ls.shape)))
            L = ls.shape[1]
        for k in keys:
            t = d[k]
            if not t.is_cuda or (self.device.index is not None and t.device != self.device):
                raise ValueError("%s: %s must be on the evaluator's GPU (%s), it is on %s" % (name, k, self.device, t.device))
            if t.device != ref.device or (self._status is not None and t.device != self._status.device):
                raise ValueError("%s: the batches of one evaluation live on one device" % name)
        return B, Cn, K, N, L

    @staticmethod
    def _grown(t, need):
        """t with room for `need` leading entries: capacity doubles, the old entries are copied on the device, the rest is zero"""
        if t.shape[0] >= need:
            return t
        cap = t.shape[0]
        while cap < need:
            cap *= 2
        new = torch.zeros((cap,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        new[:t.shape[0]].copy_(t)
        return new

    def add_batch(self, data_dict):
        """one launch, nothing read back; `data_dict` is left as it is"""
        import ctypes as C
        from . import _lib
        d = data_dict
        B, Cn, K, N, L = self._checked(d)
        dev = d["cluster_ref"].device
        if self._repeat < 0:
            self._repeat = 0
        if self._status is None:
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
            self._tables = torch.zeros((2, 3, 2, 4), dtype=torch.int64, device=dev)
            self._lang = torch.zeros(8, dtype=torch.int64, device=dev)
        self._tables = self._grown(self._tables, self._repeat + 1)
        # the dtypes the dict leaves `_ground` with pass through untouched (float32 scores / labels / mask, int64 ids)
        f32 = lambda t: t.detach().contiguous() if t.dtype == torch.float32 else t.detach().float().contiguous()
        i64 = lambda t: t.detach().contiguous() if t.dtype == torch.int64 else t.detach().long().contiguous()
        ref, labels, boxes, gt = f32(d["cluster_ref"]), f32(d["cluster_labels"]), f32(d["proposal_bbox_batched"]), f32(d["ref_box_corner_label"])
        mask = d["proposal_batch_mask"]
        mask = mask.detach().contiguous() if mask.dtype == torch.float32 else (mask.detach().long() == 1).float().contiguous()
        um, cat = i64(d["unique_multiple"]), i64(d["object_cat"])
        slot = len(self._lang_rows)
        lang = ids = chunks = None
        if self.use_lang_classifier:
            lang = f32(d["lang_scores"])
            self._lang = self._grown(self._lang, slot + 1)
        rec = None
        if self.keep_predictions:
            ids, chunks = i64(d["id"]), i64(d["chunk_ids"])
            if self._rec is None:
                z = lambda shape, dt: torch.zeros((1024,) + shape, dtype=dt, device=dev)
                self._rec = dict(iou=z((), torch.float32), best_iou=z((), torch.float32), pred_ref=z((), torch.int32), gt_ref=z((), torch.int32),
                                 ref_acc=z((), torch.int32), pred_bbox=z((8, 3), torch.float32), gt_bbox=z((8, 3), torch.float32),
                                 ids=z((2,), torch.int64))
            self._rec = {k: self._grown(t, self._rows + N) for k, t in self._rec.items()}
            rec = self._rec
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        r = (lambda k: p(rec[k])) if rec is not None else (lambda k: None)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().d3_ground_eval_batch(
                p(ref), p(labels), p(mask), p(boxes), p(gt), p(um), p(cat), p(lang), L, p(ids), p(chunks), B, Cn, K, self._rows,
                p(self._tables[self._repeat]), p(self._lang[slot:]) if lang is not None else None, r("iou"), r("best_iou"), r("pred_ref"),
                r("gt_ref"), r("ref_acc"), r("pred_bbox"), r("gt_bbox"), r("ids"), p(self._status),
                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ground_eval_batch")
        self._lang_rows.append(N)
        if rec is not None:
            self._rows += N

    def compute(self):
        """-> {"stats", "scores", "lang_acc", "status"} as scripts/eval.py:305-426 forms and prints them; sets self.tables (R,3,2,4)"""
        if self._status is None:
            raise ValueError("GroundingEvaluator.compute: no batch was added")
        R, nb = self._repeat + 1, len(self._lang_rows)
        host = torch.cat([self._tables[:R].reshape(-1), self._lang[:nb], self._status.long()]).cpu().numpy()       # the one read-back
        self.tables = host[:R * 24].reshape(R, 3, 2, 4).copy()
        lang = host[R * 24:R * 24 + nb]
        stats, scores, lang_acc = grounding_scores(self.tables, lang if self.use_lang_classifier else (),
                                                   self._lang_rows if self.use_lang_classifier else ())
        return {"stats": stats, "scores": scores, "lang_acc": lang_acc, "status": int(host[-1])}

    def records(self):
        """the last repeat's per-description records read back once -> dict of numpy arrays (keep_predictions only)"""
        if not self.keep_predictions:
            raise ValueError("GroundingEvaluator: constructed without keep_predictions")
        if self._rec is None:
            raise ValueError("GroundingEvaluator: no batch was added")
        return {k: t[:self._rows].cpu().numpy() for k, t in self._rec.items()}

    def device_predictions(self, chunked_data):
        """`predictions` for the box writer (d3net_amd.visualize.visualize_grounding): the same tree, but "pred_bbox" / "gt_bbox" are
        rows of the device records (views, (8,3) float32) and there is no "iou"; only the (rows, 2) ids are read back"""
        if not self.keep_predictions:
            raise ValueError("GroundingEvaluator: constructed without keep_predictions")
        if self._rec is None:
            raise ValueError("GroundingEvaluator: no batch was added")
        pred, gt = self._rec["pred_bbox"][:self._rows], self._rec["gt_bbox"][:self._rows]
        out = {}
        for i, (scene, chunk) in enumerate(self._rec["ids"][:self._rows].cpu().tolist()):
            ann = chunked_data[scene][chunk]
            out.setdefault(ann["scene_id"], {}).setdefault(ann["object_id"], {})[ann["ann_id"]] = {"pred_bbox": pred[i], "gt_bbox": gt[i]}
        return out

    def predictions(self, chunked_data):
        """{scene_id: {object_id: {ann_id: {"pred_bbox", "gt_bbox", "iou"}}}} of the last repeat as scripts/eval.py:243-266 leaves it:
        `chunked_data[id][chunk_id]` names a row's annotation, later rows overwrite earlier ones"""
        rec = self.records()
        out = {}
        for i, (scene, chunk) in enumerate(rec["ids"].tolist()):
            ann = chunked_data[scene][chunk]
            out.setdefault(ann["scene_id"], {}).setdefault(ann["object_id"], {})[ann["ann_id"]] = {
                "pred_bbox": rec["pred_bbox"][i], "gt_bbox": rec["gt_bbox"][i], "iou": rec["iou"][i]}
        return out
