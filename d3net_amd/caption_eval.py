"""Dense-captioning evaluation: assignment of the per-proposal captions to the GT boxes and
CIDEr@kIoU corpus scoring -- the reference's `lib/captioning/eval_helper.py:102-307` (`assign_dense_caption`,
`eval_caption_step`, the candidate filtering of `eval_caption_epoch`) and `lib/utils/bbox.py:571-757`
(`generalized_box3d_iou` for axis-aligned boxes, `box3d_iou_batch_tensor`).

The assignment has two forms that give the same pairs.  On the device (`assign_boxes_device`, csrc/assign.hip): one launch, one
workgroup per scene, computes the -GIoU cost from the boxes and solves the assignment with scipy's algorithm and tie order; the
cost matrix is never stored and nothing is read back.  On the host (the reference's form, `device_assign=False`): the
(B, K1, K2) generalised-IoU cost matrix is computed batched on whatever device the boxes live on (the reference loops over the
batch in python to mask the padded GT columns), copied to the host and handed to scipy scene by scene.  `device_assign=None`
takes the device form when the boxes are on a GPU and K, G <= 256 (DESIGN.md section 3.6 has the measurement behind that
default).  CIDEr is d3net_amd.cider (bit-identical to lib/capeval/cider).  BLEU / ROUGE / METEOR are not restated (METEOR
needs a Java runtime).  Pinned to golden vectors produced by the reference's own functions
(tests/golden/gen_caption_eval_golden.py).

Quirk kept on purpose: the reference's "footprint" rectangle of a box is read from corner columns (x, z) of corners 2 and 0
and the height from the z of corners 0 and 4 -- conventions inherited from a y-up code base -- so for this repo's z-up corner
order the intersection term is usually zero and the cost is dominated by the enclosing-volume term.  Assignments must match
the reference's, so the arithmetic is restated as it is, not as it was presumably meant.
"""
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from .cider import cider_scores

_EPS = 1e-8


def _edge_volume(c):
    """box volume from three edge lengths (bbox.py:571-592), (..., 8, 3) -> (...)"""
    def edge(i, j):
        return torch.sqrt((c[..., i, :] - c[..., j, :]).pow(2).sum(-1).clamp(min=1e-6))
    return edge(0, 1) * edge(1, 2) * edge(0, 4)


def generalized_box3d_iou(corners1, corners2, nums_k2=None):
    """(B,K1,8,3), (B,K2,8,3) -> (B,K1,K2) generalised IoU, axis-aligned path of bbox.py:645-757 (rotated_boxes=False)"""
    a, b = corners1.float(), corners2.float()
    B, K1, K2 = a.shape[0], a.shape[1], b.shape[1]
    height = (torch.minimum(a[:, :, 0, 2].unsqueeze(2), b[:, :, 0, 2].unsqueeze(1)) -
              torch.maximum(a[:, :, 4, 2].unsqueeze(2), b[:, :, 4, 2].unsqueeze(1))).clamp(min=0)
    cols = [0, 2]
    lt = torch.maximum(a[:, :, 2][..., cols].unsqueeze(2), b[:, :, 2][..., cols].unsqueeze(1))
    rb = torch.minimum(a[:, :, 0][..., cols].unsqueeze(2), b[:, :, 0][..., cols].unsqueeze(1))
    wh = (rb - lt).clamp(min=0)
    valid = torch.ones((B, 1, K2), dtype=a.dtype, device=a.device)
    if nums_k2 is not None:
        valid = (torch.arange(K2, device=a.device).view(1, 1, K2) < nums_k2.view(B, 1, 1)).to(a.dtype)
    inter_vol = wh[..., 0] * wh[..., 1] * valid * height
    lo = torch.minimum(a.min(2).values.unsqueeze(2), b.min(2).values.unsqueeze(1))
    hi = torch.maximum(a.max(2).values.unsqueeze(2), b.max(2).values.unsqueeze(1))
    enclosing = (hi - lo).abs().prod(-1)
    v1, v2 = _edge_volume(a).clamp(min=_EPS), _edge_volume(b).clamp(min=_EPS)
    sum_vols = v1.unsqueeze(2) + v2.unsqueeze(1)
    good = ((enclosing > 2 * _EPS) & (sum_vols > 4 * _EPS)).to(a.dtype)
    union = (sum_vols - inter_vol).clamp(min=_EPS)
    giou = (inter_vol / union - (1 - union / enclosing)) * good
    return giou * valid


def box3d_iou(c1, c2):
    """AABB IoU of paired boxes (N,8,3) x (N,8,3) -> (N) (bbox.py:273-305)"""
    c1, c2 = c1.float(), c2.float()
    lo1, hi1, lo2, hi2 = c1.min(1).values, c1.max(1).values, c2.min(1).values, c2.max(1).values
    inter = (torch.minimum(hi1, hi2) - torch.maximum(lo1, lo2)).clamp(min=0).prod(-1)
    return inter / ((hi1 - lo1).prod(-1) + (hi2 - lo2).prod(-1) - inter + 1e-8)


def decode_caption(tokens, idx2word, special_tokens):
    out = [special_tokens["bos_token"]]
    for t in tokens.tolist():
        w = idx2word[str(t)]
        out.append(w)
        if w == special_tokens["eos_token"]:
            break
    if special_tokens["eos_token"] not in out:
        out.append(special_tokens["eos_token"])
    return " ".join(out)


DEVICE_ASSIGN_MAX = 256          # rows / columns per scene of csrc/assign.hip
_ASSIGN_ERRORS = {1: "matrix contains invalid numeric entries", 2: "cost matrix is infeasible"}   # scipy's messages


def _center_cost(pred_boxes, gt_boxes):
    return torch.cdist(pred_boxes.mean(2).float(), gt_boxes.mean(2).float())


def _assign_launch(pred_boxes, gt_boxes, nactual, strategy, return_cost):
    """-> per_gt (B, G) int32, status (B) int32, cost (B, K, G) or None; stream-ordered, nothing read back"""
    import ctypes as C
    from . import _lib
    if strategy not in ("giou", "center"):
        raise ValueError("invalid strategy.")
    if not pred_boxes.is_cuda:
        raise ValueError("assign_boxes_device needs the boxes on a GPU (device_assign=False is the host path)")
    B, K, G = pred_boxes.shape[0], pred_boxes.shape[1], gt_boxes.shape[1]
    if K > DEVICE_ASSIGN_MAX or G > DEVICE_ASSIGN_MAX:
        raise ValueError("assign_boxes_device: K = %d, G = %d exceed the kernel's %d" % (K, G, DEVICE_ASSIGN_MAX))
    dev = pred_boxes.device
    per_gt = torch.empty((B, G), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0 or K == 0 or G == 0:
        return per_gt.zero_(), status.zero_(), (torch.zeros((B, K, G), device=dev) if return_cost else None)
    na = nactual.to(device=dev, dtype=torch.int32).contiguous()
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if strategy == "giou":
            pb, gb = pred_boxes.detach().float().contiguous(), gt_boxes.detach().float().contiguous()
            cost = torch.empty((B, K, G), dtype=torch.float32, device=dev) if return_cost else None
            _lib.check(_lib.lib().d3_dense_caption_assign(p(pb), p(gb), p(na), B, K, G, p(per_gt), p(status),
                                                          p(cost) if cost is not None else None, stream), "dense_caption_assign")
        else:
            cost = _center_cost(pred_boxes.detach(), gt_boxes.detach()).contiguous()
            _lib.check(_lib.lib().d3_lsap_batched(p(cost), p(na), B, K, G, p(per_gt), p(status), stream), "lsap_batched")
    return per_gt, status, (cost if return_cost else None)


def _raise_on_status(status_host):
    for st in status_host.tolist():
        if st != 0:
            raise ValueError(_ASSIGN_ERRORS.get(st, "assignment failed (status %d)" % st))


def assign_boxes_device(pred_boxes, gt_boxes, nactual, strategy="giou", return_cost=False):
    """Hungarian assignment of proposals (B,K,8,3) to the first nactual[b] GT boxes (B,G,8,3) in one launch (csrc/assign.hip)
    -> per_gt (B,G) int64 on the device: per_gt[b, g] = the proposal assigned to GT box g, 0 where none (with return_cost:
    also the (B,K,G) cost the kernel solved).  "giou": the cost is computed inside the kernel; "center": torch.cdist, the host
    path's own bits, handed to the solver.  Raises scipy's ValueError for a non-finite cost in a valid column."""
    per_gt, status, cost = _assign_launch(pred_boxes, gt_boxes, nactual, strategy, return_cost)
    _raise_on_status(status.cpu())
    return (per_gt.long(), cost) if return_cost else per_gt.long()


def assign_dense_caption(pred_captions, pred_boxes, gt_boxes, gt_box_ids, gt_box_masks, gt_scene_list, idx2word,
                         special_tokens, strategy="giou", device_assign=None):
    """eval_helper.py:102-246: Hungarian assignment of proposals to GT boxes, the matched proposal's caption per GT box.
    device_assign (default: when the boxes live on the GPU and K, G <= 256): cost and assignment run as one kernel and stay on
    the device; False: the reference's form, cost matrix to the host and scipy scene by scene."""
    B, ngt = gt_box_ids.shape
    nactual = gt_box_masks.sum(1).long()
    if strategy not in ("giou", "center"):
        raise ValueError("invalid strategy.")
    if device_assign is None:
        device_assign = bool(pred_boxes.is_cuda) and max(pred_boxes.shape[1], ngt) <= DEVICE_ASSIGN_MAX
    status = None
    if device_assign:
        per_gt, status, _ = _assign_launch(pred_boxes, gt_boxes, nactual, strategy, False)
        per_gt = per_gt.long()
    else:
        if strategy == "giou":
            cost = -generalized_box3d_iou(pred_boxes, gt_boxes, nactual)
        else:
            cost = _center_cost(pred_boxes, gt_boxes)
        cost = cost.detach().cpu().numpy()
        per_gt = torch.zeros((B, ngt), dtype=torch.int64)
        for b in range(B):
            n = int(nactual[b])
            if n > 0:
                rows, cols = linear_sum_assignment(cost[b, :, :n])
                per_gt[b, torch.from_numpy(cols)] = torch.from_numpy(rows)
        per_gt = per_gt.to(pred_boxes.device)
    matched = torch.gather(pred_boxes, 1, per_gt[:, :, None, None].expand(B, ngt, 8, 3))
    ious = box3d_iou(matched.reshape(-1, 8, 3), gt_boxes.reshape(-1, 8, 3)).reshape(B, ngt).cpu()
    caps = torch.gather(pred_captions, 1, per_gt[:, :, None].expand(B, ngt, pred_captions.shape[2])).cpu()
    matched_h, gt_h, masks, ids = matched.cpu(), gt_boxes.cpu(), gt_box_masks.cpu(), gt_box_ids.cpu()
    if status is not None:
        _raise_on_status(status.cpu())      # after the copies above: the device path adds no synchronisation of its own
    candidates = {}
    for b in range(B):
        for g in range(ngt):
            if masks[b, g] == 0:
                continue
            key = "{}|{}".format(gt_scene_list[b], str(ids[b, g].item()))
            candidates[key] = {"caption": decode_caption(caps[b, g], idx2word, special_tokens), "iou": ious[b, g].item(),
                               "box": matched_h[b, g].numpy().tolist(), "gt_box": gt_h[b, g].numpy().tolist()}
    return candidates


def eval_caption_step(data_dict, dataset_vocabulary):
    """eval_helper.py:248-262"""
    return assign_dense_caption(data_dict["lang_cap"], data_dict["proposal_bbox_batched"], data_dict["gt_bbox"],
                                data_dict["gt_bbox_object_id"], data_dict["gt_bbox_label"], data_dict["scene_id"],
                                dataset_vocabulary["idx2word"], dataset_vocabulary["special_tokens"])


def prepare_corpus(raw_data, candidates, max_len=30):
    """eval_helper.py:35-62: reference descriptions ("sos ... eos") of the scenes that have candidates"""
    scenes = {k.split("|")[0] for k in candidates}
    corpus = {}
    for d in raw_data:
        if d["scene_id"] not in scenes:
            continue
        corpus.setdefault("{}|{}".format(d["scene_id"], d["object_id"]), []).append("sos " + " ".join(d["token"][:max_len]) + " eos")
    return corpus


def score_captions(candidates, raw_data, max_len=30, min_iou=0.5):
    """CIDEr@min_iou as eval_caption_epoch computes it (eval_helper.py:264-296): captions whose matched box has IoU <
    min_iou, and undetected objects, count as the empty caption "sos eos".  -> (mean, per-object scores, keys)"""
    corpus = prepare_corpus(raw_data, candidates, max_len)
    kept = {k: v["caption"] for k, v in candidates.items() if v["iou"] >= min_iou}
    keys = list(corpus.keys())
    mean, scores = cider_scores([corpus[k] for k in keys], [kept.get(k, "sos eos") for k in keys])
    return mean, scores, keys


def eval_caption_epoch(candidates, raw_data, max_len=30, min_iou=0.5):
    """Corpus scores of one validation epoch in the reference's return format (eval_helper.py:264-340):
    (bleu, cider, rouge, meteor) with bleu = ([BLEU-1..4], [per-entry lists]) and the others (mean, per-entry scores).
    Captions whose matched box has IoU < min_iou, and undetected objects, count as the empty caption "sos eos".  METEOR is a
    Java subprocess in the reference (lib/capeval/meteor) and no Java runtime exists here: it is reported as (0.0, zeros)."""
    from .caption_metrics import bleu_scores, rouge_l_scores
    corpus = prepare_corpus(raw_data, candidates, max_len)
    kept = {k: v["caption"] for k, v in candidates.items() if v["iou"] >= min_iou}
    keys = list(corpus.keys())
    refs, cands = [corpus[k] for k in keys], [kept.get(k, "sos eos") for k in keys]
    if not keys:
        z = (0.0, np.zeros(0))
        return ([0.0] * 4, [[] for _ in range(4)]), z, z, z
    bleu = bleu_scores(refs, cands, 4)
    cider = cider_scores(refs, cands)
    rouge = rouge_l_scores(refs, cands)
    return bleu, cider, rouge, (0.0, np.zeros(len(keys)))
