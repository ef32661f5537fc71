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
default).  CIDEr is d3net_amd.cider (bit-identical to lib/capeval/cider), BLEU-1..4 and ROUGE-L are d3net_amd.caption_metrics;
METEOR is not restated (it needs a Java runtime).  Pinned to golden vectors produced by the reference's own functions
(tests/golden/gen_caption_eval_golden.py).

The whole validation also runs on the device (`CaptionEvaluator`): per batch the assignment and
csrc/caption_eval.hip's d3_caption_collect keep the winning caption (token ids) and IoU of every described object on the GPU under
the host's merge rule, and at the end of the epoch d3_cider_scores and d3_caption_stats score them against `EvalCorpus`, the
token-id twin of `prepare_corpus`.  BLEU and ROUGE need only integers from the sentences (clipped n-gram counts, lengths, LCS
lengths), so they equal the host's bit for bit; CIDEr is within the 1e-12 the device scorer is held to.  The host functions
below stay as they are: they are the reference form, and they keep the box lists the visualisers read.

Quirk kept on purpose: the reference's "footprint" rectangle of a box is read from corner columns (x, z) of corners 2 and 0
and the height from the z of corners 0 and 4 -- conventions inherited from a y-up code base -- so for this repo's z-up corner
order the intersection term is usually zero and the cost is dominated by the enclosing-volume term.  Assignments must match
the reference's, so the arithmetic is restated as it is, not as it was presumably meant.
"""
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import _lib
from ._call import call, on, ptr, stream
from .cider import cider_scores
from .devstate import FLAGS, FLOATS, INTS, check_batch, read_back

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
    with on(dev):
        if strategy == "giou":
            pb, gb = pred_boxes.detach().float().contiguous(), gt_boxes.detach().float().contiguous()
            cost = torch.empty((B, K, G), dtype=torch.float32, device=dev) if return_cost else None
            call("dense_caption_assign", ptr(pb), ptr(gb), ptr(na), B, K, G, ptr(per_gt), ptr(status), ptr(cost), stream())
        else:
            cost = _center_cost(pred_boxes.detach(), gt_boxes.detach()).contiguous()
            call("lsap_batched", ptr(cost), ptr(na), B, K, G, ptr(per_gt), ptr(status), stream())
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


# ---------------------------------------------------------------------------------------------------- the device form
EVAL_MAX_TOKENS = 64             # tokens per sentence of csrc/caption_eval.hip, sos and eos included
EVAL_MAX_OBJECT_ID = 4095        # columns of the per-scene slot table
EVAL_MAX_SLOTS_PER_BATCH = 1 << 20


class EvalCorpus:
    """`prepare_corpus` as token ids for csrc/caption_eval.hip and csrc/cider.hip, built once per split: one int32 row
    [sos] + token[:max_len] + [eos] per description, ids canonical as in captioning_loss.CiderCorpus (the lower id of two that spell
    one word, corpus-private ids >= V for words outside the vocabulary, so string equality == id equality).  Keys "scene|object" are
    numbered as slots in order of first appearance; the rows of a slot are contiguous, in order of appearance.  Data beyond the
    kernels' fixed sizes raises ValueError (the host path, eval_caption_step + eval_caption_epoch, takes it)."""
    MAX_SET_NGRAMS, MAX_ID = 2048, 65534

    def __init__(self, raw_data, idx2word, special_tokens, max_len=30, device="cuda"):
        from .captioning_loss import canonical_ids
        if special_tokens["bos_token"] != "sos" or special_tokens["eos_token"] != "eos":
            raise ValueError("EvalCorpus: prepare_corpus writes the literal words 'sos' / 'eos'; the vocabulary's are %r / %r"
                             % (special_tokens["bos_token"], special_tokens["eos_token"]))
        canon, V = canonical_ids(idx2word)
        one_word = lambda w: isinstance(w, str) and w.split() == [w]          # then split(), split(" ") and id equality agree
        for w in canon:
            if not one_word(w):
                raise ValueError("EvalCorpus: vocabulary word %r is empty or contains whitespace" % (w,))
        if "sos" not in canon or "eos" not in canon:
            raise ValueError("EvalCorpus: the vocabulary has no 'sos' / 'eos'")
        extra, per_slot, self.keys, self.scene_index, slot_scene, slot_obj = {}, [], [], {}, [], []
        slot_of_key = {}
        for d in raw_data:
            sid, oid = d["scene_id"], d["object_id"]
            key = "{}|{}".format(sid, oid)
            slot = slot_of_key.get(key)
            if slot is None:
                try:
                    o = int(oid)
                except (TypeError, ValueError):
                    raise ValueError("EvalCorpus: object id %r of %s is not an integer" % (oid, sid))
                if not 0 <= o <= EVAL_MAX_OBJECT_ID:
                    raise ValueError("EvalCorpus: object id %d of %s outside [0, %d]" % (o, sid, EVAL_MAX_OBJECT_ID))
                slot = slot_of_key[key] = len(self.keys)
                self.keys.append(key); per_slot.append([])
                slot_scene.append(self.scene_index.setdefault(sid, len(self.scene_index)))
                slot_obj.append(o if str(o) == str(oid) else -1)       # the candidates' keys are written with str(int)
            words = list(d["token"][:max_len])
            if len(words) + 2 > EVAL_MAX_TOKENS:
                raise ValueError("EvalCorpus: a description of %s has %d tokens with sos and eos, the kernels hold %d"
                                 % (key, len(words) + 2, EVAL_MAX_TOKENS))
            for w in words:
                if not one_word(w):
                    raise ValueError("EvalCorpus: word %r of %s is empty or contains whitespace" % (w, key))
            per_slot[slot].append([canon[w] if w in canon else extra.setdefault(w, V + len(extra)) for w in ["sos"] + words + ["eos"]])
        if not self.keys:
            raise ValueError("EvalCorpus: no descriptions")
        if V + len(extra) > self.MAX_ID:
            raise ValueError("EvalCorpus: %d distinct words, ids end at %d" % (V + len(extra), self.MAX_ID))
        rows, self.row_off = [], [0]
        for key, rs in zip(self.keys, per_slot):
            if 4 * sum(len(r) for r in rs) > self.MAX_SET_NGRAMS:
                raise ValueError("EvalCorpus: the references of %s hold %d n-gram positions, the per-set table %d"
                                 % (key, 4 * sum(len(r) for r in rs), self.MAX_SET_NGRAMS))
            rows.extend(rs); self.row_off.append(len(rows))
        self.row_len = [len(r) for r in rows]
        self.ldt = EVAL_MAX_TOKENS
        tok = np.zeros((len(rows), self.ldt), np.int32)
        for i, r in enumerate(rows):
            tok[i, :len(r)] = r
        self.V, self.sos, self.eos, self.device = V, canon["sos"], canon["eos"], torch.device(device)
        self.n_scenes, self.n_obj, self.slot_scene = len(self.scene_index), max(max(slot_obj), 0) + 1, slot_scene
        table = np.full((self.n_scenes, self.n_obj), -1, np.int32)
        for s, (sc, o) in enumerate(zip(slot_scene, slot_obj)):
            if o >= 0:
                table[sc, o] = s
        lut = np.full(V, -1, np.int32)
        for i, w in idx2word.items():
            lut[int(i)] = canon[w]
        self.words = {i: w for w, i in list(canon.items()) + list(extra.items())}          # canonical id -> word
        self.tokens = torch.from_numpy(tok).to(self.device)
        self.lens = torch.tensor(self.row_len, dtype=torch.int32, device=self.device)
        self.slot_of = torch.from_numpy(table).to(self.device)
        self.lut = torch.from_numpy(lut).to(self.device)

    def decode(self, ids):
        return " ".join(self.words[int(i)] for i in ids)


_CAP_TABLE = {"lang_cap": ((torch.int64,), (("B", "K", "T"),)), "proposal_bbox_batched": (FLOATS, None), "gt_bbox": (FLOATS, None),
              "gt_bbox_object_id": (INTS, (("B", "G"),)), "gt_bbox_label": (FLAGS, (("B", "G"),)), "scene_id": None}


class CaptionEvaluator:
    """eval_caption_step + the candidate merge of validation_epoch_end + eval_caption_epoch on the device: `add_batch` runs the
    Hungarian assignment (csrc/assign.hip) and d3_caption_collect, which keeps the epoch's winning caption and IoU per corpus slot
    on the GPU (state sized by the corpus, no read-back); `compute` reads the seen-scene flags, runs d3_cider_scores and
    d3_caption_stats over the entries and reads one block back -> what eval_caption_epoch returns, BLEU and ROUGE formed by
    caption_metrics' floating-point halves from the kernel's integers."""

    def __init__(self, raw_data, vocabulary, max_len=30, min_iou=0.5, device="cuda", strategy="giou"):
        if strategy not in ("giou", "center"):
            raise ValueError("invalid strategy.")
        self.corpus = EvalCorpus(raw_data, vocabulary["idx2word"], vocabulary["special_tokens"], max_len, device)
        self.min_iou, self.strategy, self.keys = float(min_iou), strategy, None
        self.reset()

    def reset(self):
        c, dev = self.corpus, self.corpus.device
        S = len(c.keys)
        self._owner = torch.full((S,), -1, dtype=torch.int64, device=dev)             # (uint64 all ones: unowned)
        self._cap = torch.zeros((S, EVAL_MAX_TOKENS), dtype=torch.int32, device=dev)
        self._cap_len = torch.zeros(S, dtype=torch.int32, device=dev)
        self._iou = torch.zeros(S, dtype=torch.float32, device=dev)
        self._seen = torch.zeros(c.n_scenes, dtype=torch.int32, device=dev)
        self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._seq, self._entries = 0, {}

    @staticmethod
    def _geometry(d):
        name = "CaptionEvaluator.add_batch"
        caps, pb, gb = d["lang_cap"], d["proposal_bbox_batched"], d["gt_bbox"]
        if pb.dim() != 4 or tuple(pb.shape[2:]) != (8, 3) or gb.dim() != 4 or tuple(gb.shape[2:]) != (8, 3) or gb.shape[0] != pb.shape[0]:
            raise ValueError("%s: corners (B,K,8,3) and (B,G,8,3) expected" % name)
        B, K, G = pb.shape[0], pb.shape[1], gb.shape[1]
        if B < 1 or K < 1 or G < 1 or K > DEVICE_ASSIGN_MAX or G > DEVICE_ASSIGN_MAX:
            raise ValueError("%s: B >= 1, 1 <= K, G <= %d (got B %d, K %d, G %d)" % (name, DEVICE_ASSIGN_MAX, B, K, G))
        if B * G > EVAL_MAX_SLOTS_PER_BATCH:
            raise ValueError("%s: B * G = %d exceeds %d" % (name, B * G, EVAL_MAX_SLOTS_PER_BATCH))
        if caps.dim() != 3:
            raise ValueError("%s: lang_cap must be (%d, %d, T)" % (name, B, K))
        T = caps.shape[2]
        if T > EVAL_MAX_TOKENS - 2:
            raise ValueError("%s: captions of T = %d tokens, the kernel holds %d" % (name, T, EVAL_MAX_TOKENS - 2))
        if len(d["scene_id"]) != B:
            raise ValueError("%s: scene_id must name the %d scenes" % (name, B))
        return dict(B=B, K=K, G=G, T=T)

    def _checked(self, d):
        dims = check_batch("CaptionEvaluator.add_batch", d, _CAP_TABLE, self._geometry, self.corpus.device, self._status)
        return tuple(d[k] for k in _CAP_TABLE) + tuple(dims[k] for k in "BKGT")

    def add_batch(self, data_dict):
        """the six keys eval_caption_step reads, tensors on the GPU; returns nothing and reads nothing back"""
        caps, pb, gb, ids, mask, scenes, B, K, G, T = self._checked(data_dict)
        c, dev = self.corpus, self.corpus.device
        nactual = mask.sum(1).long()
        pb, gb = pb.detach().contiguous(), gb.detach().contiguous()
        per_gt, astatus, _ = _assign_launch(pb, gb, nactual, self.strategy, False)
        scene_idx = torch.tensor([c.scene_index.get(s, -1) for s in scenes], dtype=torch.int32).to(dev, non_blocking=True)
        m32, ids64, caps = (mask != 0).to(torch.int32).contiguous(), ids.long().contiguous(), caps.detach().contiguous()
        with on(dev):
            call("caption_collect", ptr(per_gt), ptr(pb), ptr(gb), ptr(m32), ptr(ids64), ptr(caps) if T else None, ptr(c.lut), ptr(scene_idx),
                 ptr(c.slot_of), ptr(astatus), B, K, G, T, c.V, c.n_scenes, c.n_obj, len(c.keys), c.sos, c.eos, self._seq, ptr(self._owner),
                 ptr(self._cap), ptr(self._cap_len), ptr(self._iou), ptr(self._seen), ptr(self._status), stream())
        self._seq += 1

    def _entry_tables(self, seen):
        """the entries of a set of seen scenes: slots in slot order (prepare_corpus's keys) and the d3_cider_scores batch description"""
        ent = self._entries.get(seen)
        if ent is None:
            c = self.corpus
            slots = [s for s in range(len(c.keys)) if seen[c.slot_scene[s]]]
            slot_row, u_off = [], [0]
            for s in slots:
                slot_row.extend(range(c.row_off[s], c.row_off[s + 1])); u_off.append(len(slot_row))
            E, SR = len(slots), len(slot_row)
            ngrams = 4 * sum(c.row_len[r] for r in slot_row)
            hash_slots = 1024
            while hash_slots < 4 * ngrams:
                hash_slots *= 2
            meta = torch.tensor(slots + slot_row + u_off + [1] * E + list(range(E)), dtype=torch.int32).to(c.device)
            o = np.cumsum([0, E, SR, E + 1, E, E])
            self._entries = {seen: (slots, slot_row, u_off, hash_slots) + tuple(meta[o[i]:o[i + 1]] for i in range(5))}
            ent = self._entries[seen]
        return ent

    def compute(self, min_iou=None):
        """-> (bleu, cider, rouge, meteor) as eval_caption_epoch returns them for the epoch's merged candidates; sets self.keys"""
        from .caption_metrics import bleu_from_counts, rouge_from_lcs
        min_iou = self.min_iou if min_iou is None else float(min_iou)
        c, dev = self.corpus, self.corpus.device
        seen = tuple(bool(x) for x in self._seen.cpu().tolist())                    # read-back 1: decides the entry set
        slots, slot_row, u_off, hash_slots, d_slots, d_rows, d_uoff, d_mult, d_ent = self._entry_tables(seen)
        self.keys = [c.keys[s] for s in slots]
        E, SR = len(slots), len(slot_row)
        if E == 0:
            self._raise_on(int(self._status.cpu()[0]))
            z = (0.0, np.zeros(0))
            return ([0.0] * 4, [[] for _ in range(4)]), z, z, z
        sel = d_slots.long()
        keep = (self._owner[sel] != -1) & (self._iou[sel].double() >= min_iou)      # a NaN IoU compares false, as on the host
        empty = torch.zeros(EVAL_MAX_TOKENS, dtype=torch.int32, device=dev)
        empty[0], empty[1] = c.sos, c.eos
        cand = torch.where(keep[:, None], self._cap[sel], empty[None]).contiguous()
        clen = torch.where(keep, self._cap_len[sel], torch.full_like(self._cap_len[sel], 2)).contiguous()
        ws = torch.empty(_lib.lib().d3_cider_ws_bytes(SR, E, hash_slots), dtype=torch.uint8, device=dev)
        scores = torch.empty(E, dtype=torch.float64, device=dev)
        flag = torch.empty(1, dtype=torch.int32, device=dev)
        stats = torch.empty((E, 6), dtype=torch.int32, device=dev)
        lcs = torch.empty(SR, dtype=torch.int32, device=dev)
        with on(dev):
            call("cider_scores", ptr(c.tokens), c.ldt, ptr(c.lens), ptr(d_rows), ptr(d_uoff), ptr(d_mult), ptr(d_ent), E, SR, ptr(cand),
                 EVAL_MAX_TOKENS, ptr(clen), E, c.eos, 6.0, hash_slots, ptr(scores), ptr(flag), ptr(ws), ws.numel(), stream())
            call("caption_stats", ptr(cand), EVAL_MAX_TOKENS, ptr(clen), ptr(c.tokens), c.ldt, ptr(c.lens), ptr(d_rows), ptr(d_uoff), E, ptr(stats),
                 ptr(lcs), stream())
        counts, lcs_h, cider, flag, status = read_back([stats, lcs, scores, flag, self._status])                      # read-back 2
        if int(flag[0]):
            raise _lib.D3Error("CaptionEvaluator: a CIDEr hash table overflowed")
        self._raise_on(int(status[0]))
        counts, lcs_h, cider = counts.tolist(), lcs_h.tolist(), cider.copy()
        bleu = bleu_from_counts(counts, 4)
        rouge = rouge_from_lcs([(counts[e][4], [c.row_len[r] for r in slot_row[u_off[e]:u_off[e + 1]]], lcs_h[u_off[e]:u_off[e + 1]])
                                for e in range(E)])
        return bleu, (float(np.mean(cider)), cider), rouge, (0.0, np.zeros(E))

    @staticmethod
    def _raise_on(status):
        if status & 1:
            raise _lib.D3Error("CaptionEvaluator: a matched caption holds a token outside the vocabulary")
        if status & 6:
            raise ValueError(_ASSIGN_ERRORS[1 if status & 2 else 2])

    def candidates(self):
        """the debugging / parity view: the state read back -> {key: {"caption": str, "iou": float}} for the owned slots"""
        c = self.corpus
        owner, cap, n, iou = (t.cpu().numpy() for t in (self._owner, self._cap, self._cap_len, self._iou))
        return {c.keys[s]: {"caption": c.decode(cap[s, :n[s]]), "iou": float(iou[s])} for s in range(len(c.keys)) if owner[s] != -1}
