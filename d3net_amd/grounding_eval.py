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

from ._call import call, on, ptr, stream
from .devstate import FLAGS, FLOATS, GROUND_MAX_K, INTS, RecordStore, as_f32, as_i64, check_batch, read_back
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
GROUND_MAX_LANG = 64                                  # language classes of csrc/grounding_eval.hip
_MULTIPLE = (("unique", 0), ("multiple", 1))          # scripts/eval.py:305-312
_OTHERS = (("not_in_others", 0), ("in_others", 1))
_METRICS = ("ref_acc", "acc@0.25iou", "acc@0.5iou")
_ROWS = (("B", "C"), ("N",))                          # one value per description, batched or flat
_TABLE = {"cluster_ref": (FLOATS, None), "cluster_labels": (FLAGS, (("N", "K"),)), "proposal_batch_mask": (FLAGS, (("B", "K"),)),
          "proposal_bbox_batched": (FLOATS, (("B", "K", 8, 3),)), "ref_box_corner_label": (FLOATS, (("B", "C", 8, 3), ("N", 8, 3))),
          "unique_multiple": (INTS, _ROWS), "object_cat": (INTS, _ROWS),
          "lang_scores": (FLOATS, (("N", "L"),)),                             # use_lang_classifier
          "id": (INTS, (("B",),)), "chunk_ids": (INTS, (("B", "C"),))}        # keep_predictions
_REC = dict(iou=((), torch.float32), best_iou=((), torch.float32), pred_ref=((), torch.int32), gt_ref=((), torch.int32),
            ref_acc=((), torch.int32), pred_bbox=((8, 3), torch.float32), gt_bbox=((8, 3), torch.float32), ids=((2,), torch.int64))


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
        self._repeat, self._lang_rows, self.tables = -1, [], None

    def begin_repeat(self):
        self._repeat += 1
        if self._rec is not None:
            self._rec.rows = 0                          # the records are the last repeat's (scripts/eval.py:196, 264-266)

    def _geometry(self, d):
        name = "GroundingEvaluator.add_batch"
        ref, mask, boxes = d["cluster_ref"], d["proposal_batch_mask"], d["proposal_bbox_batched"]
        if ref.dim() != 2 or boxes.dim() != 4 or tuple(boxes.shape[2:]) != (8, 3) or mask.dim() != 2:
            raise ValueError("%s: cluster_ref (N,K), proposal_batch_mask (B,K) and proposal_bbox_batched (B,K,8,3) expected" % name)
        (N, K), B = ref.shape, boxes.shape[0]
        if B < 1 or N < 1 or N % B or not 1 <= K <= GROUND_MAX_K:
            raise ValueError("%s: B >= 1, N = B * C >= 1 and 1 <= K <= %d (got B %d, N %d, K %d)" % (name, GROUND_MAX_K, B, N, K))
        L = 0
        if self.use_lang_classifier:
            ls = d["lang_scores"]
            if ls.dim() != 2 or not 1 <= ls.shape[1] <= GROUND_MAX_LANG:
                raise ValueError("%s: lang_scores must be (%d, L) with 1 <= L <= %d, got %s" % (name, N, GROUND_MAX_LANG, tuple(ls.shape)))
            L = ls.shape[1]
        return dict(B=B, C=N // B, K=K, N=N, L=L)

    def _checked(self, d):
        skip = (() if self.use_lang_classifier else ("lang_scores",)) + (() if self.keep_predictions else ("id", "chunk_ids"))
        dims = check_batch("GroundingEvaluator.add_batch", d, {k: v for k, v in _TABLE.items() if k not in skip}, self._geometry,
                           self.device, self._status)
        return tuple(dims[k] for k in "BCKNL")

    def add_batch(self, data_dict):
        """one launch, nothing read back; `data_dict` is left as it is"""
        d = data_dict
        B, Cn, K, N, L = self._checked(d)
        dev = d["cluster_ref"].device
        if self._repeat < 0:
            self._repeat = 0
        if self._status is None:
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
            self._tables = RecordStore(dev, 2, t=((3, 2, 4), torch.int64))
            self._lang = RecordStore(dev, 8, n=((), torch.int64))
        self._tables.reserve(self._repeat + 1)
        # the dtypes the dict leaves `_ground` with pass through untouched (float32 scores / labels / mask, int64 ids)
        ref, labels, boxes, gt = (as_f32(d[k]) for k in ("cluster_ref", "cluster_labels", "proposal_bbox_batched", "ref_box_corner_label"))
        mask = d["proposal_batch_mask"]
        mask = mask.detach().contiguous() if mask.dtype == torch.float32 else (mask.detach().long() == 1).float().contiguous()
        um, cat = as_i64(d["unique_multiple"]), as_i64(d["object_cat"])
        slot = len(self._lang_rows)
        lang = lang_out = ids = chunks = None
        if self.use_lang_classifier:
            lang = as_f32(d["lang_scores"])
            self._lang.reserve(slot + 1)
            lang_out = self._lang["n"][slot:]
        rec = [None] * len(_REC)
        if self.keep_predictions:
            ids, chunks = as_i64(d["id"]), as_i64(d["chunk_ids"])
            if self._rec is None:
                self._rec = RecordStore(dev, **_REC)
            self._rec.reserve(self._rec.rows + N)
            rec = [self._rec[k] for k in _REC]
        with on(dev):
            call("ground_eval_batch", ptr(ref), ptr(labels), ptr(mask), ptr(boxes), ptr(gt), ptr(um), ptr(cat), ptr(lang), L, ptr(ids),
                 ptr(chunks), B, Cn, K, self._rec.rows if self.keep_predictions else 0, ptr(self._tables["t"][self._repeat]), ptr(lang_out),
                 *[ptr(t) for t in rec], ptr(self._status), stream())
        self._lang_rows.append(N)
        if self.keep_predictions:
            self._rec.rows += N

    def compute(self):
        """-> {"stats", "scores", "lang_acc", "status"} as scripts/eval.py:305-426 forms and prints them; sets self.tables (R,3,2,4)"""
        if self._status is None:
            raise ValueError("GroundingEvaluator.compute: no batch was added")
        R, nb = self._repeat + 1, len(self._lang_rows)
        tables, lang, status = read_back([self._tables["t"][:R], self._lang["n"][:nb], self._status])       # the one read-back
        self.tables = tables.copy()
        stats, scores, lang_acc = grounding_scores(self.tables, lang if self.use_lang_classifier else (),
                                                   self._lang_rows if self.use_lang_classifier else ())
        return {"stats": stats, "scores": scores, "lang_acc": lang_acc, "status": int(status[0])}

    def _filled(self):
        if not self.keep_predictions:
            raise ValueError("GroundingEvaluator: constructed without keep_predictions")
        if self._rec is None:
            raise ValueError("GroundingEvaluator: no batch was added")
        return self._rec.filled()

    def records(self):
        """the last repeat's per-description records read back once -> dict of numpy arrays (keep_predictions only)"""
        self._filled()
        return self._rec.read_back()[0]

    @staticmethod
    def _tree(ids, chunked_data, entry):
        out = {}
        for i, (scene, chunk) in enumerate(ids):
            ann = chunked_data[scene][chunk]
            out.setdefault(ann["scene_id"], {}).setdefault(ann["object_id"], {})[ann["ann_id"]] = entry(i)
        return out

    def device_predictions(self, chunked_data):
        """`predictions` for the box writer (d3net_amd.visualize.visualize_grounding): the same tree, but "pred_bbox" / "gt_bbox" are
        rows of the device records (views, (8,3) float32) and there is no "iou"; only the (rows, 2) ids are read back"""
        rec = self._filled()
        return self._tree(rec["ids"].cpu().tolist(), chunked_data, lambda i: {"pred_bbox": rec["pred_bbox"][i], "gt_bbox": rec["gt_bbox"][i]})

    def predictions(self, chunked_data):
        """{scene_id: {object_id: {ann_id: {"pred_bbox", "gt_bbox", "iou"}}}} of the last repeat as scripts/eval.py:243-266 leaves it:
        `chunked_data[id][chunk_id]` names a row's annotation, later rows overwrite earlier ones"""
        rec = self.records()
        return self._tree(rec["ids"].tolist(), chunked_data, lambda i: {k: rec[k][i] for k in ("pred_bbox", "gt_bbox", "iou")})
