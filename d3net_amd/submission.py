"""The two leaderboard prediction writers: the files one uploads to the Scan2Cap and ScanRefer benchmark
servers, as the reference's `benchmark/benchmark_captioning.py:121-196` and `benchmark/benchmark_grounding.py:110-186` (`predict`)
write them, without the reference's per-proposal `.cpu()` copies, its numpy NMS loop and its (N, K, 8, 3) repeated corners on the host.

`CaptionSubmission` / `GroundingSubmission` follow the evaluators' pattern: `add_batch` takes the dict as it leaves the speaker's
evaluation decode / the listener and runs csrc/nms.hip's d3_nms3d_samecls + csrc/submission.hip's d3_caption_submit_batch / one
d3_ground_submit_batch into device state, nothing is read back; `results()` reads the state back once and forms the reference's
Python objects, `write(path)` is the reference's `json.dump(..., indent=4)`.  Two quirks of the reference are kept: the captioning
writer applies the class-aware NMS but NO confidence threshold, and a scene named again replaces its earlier list while keeping its
place in the file; the grounding writer takes `cluster_ref.argmax(-1)` over ALL slots (an invalid one can win) and drops a repeated
"scene-object-ann" only within a batch.  No CPU fallback: tensors in host memory are refused.
"""
import json

import numpy as np
import torch

from . import _lib
from ._call import call, on, ptr, stream
from .devstate import FLAGS, FLOATS, GROUND_MAX_K, INTS, RecordStore, as_i64, check_batch, read_back
from .evaluator import POST_DICT, nms_pred_mask_device

SUBMIT_MAX_K, SUBMIT_MAX_TOKENS, SUBMIT_MAX_ROWS = 256, 62, 1 << 20      # proposal slots / caption tokens / rows per batch of csrc/submission.hip
NUM_CLASS = 18
_ROWS = (("B", "C"), ("N",))                                              # one value per description, batched or flat
_CAP_TABLE = {"proposal_bbox_batched": (FLOATS, None), "proposal_sem_cls_batched": (FLOATS, (("B", "K"),)),
              "proposal_scores_batched": (FLOATS, (("B", "K"),)), "proposal_batch_mask": (FLAGS, (("B", "K"),)),
              "lang_cap": ((torch.int64,), (("B", "K", "T"),)), "id": (INTS, (("B",),))}
_CAP_STATE = ("box", "cls", "score", "ntok", "tok", "count", "first_seen", "status")         # the state `records` reads back
_GROUND_TABLE = {"cluster_ref": (FLOATS, None), "proposal_bbox_batched": (FLOATS, None), "unique_multiple": (INTS, _ROWS),
                 "object_cat": (INTS, _ROWS), "id": (INTS, (("B",),)), "chunk_ids": (INTS, (("B", "C"),))}
_GROUND_REC = dict(bbox=((8, 3), torch.float32), pred_ref=((), torch.int32), unique_multiple=((), torch.int64), others=((), torch.int32),
                   key=((), torch.int32), keep=((), torch.int32), ids=((2,), torch.int64))


class CaptionSubmission:
    """benchmark_captioning.py:121-196 (predict) on the device.  chunked_data[id][0]["scene_id"] names the scene of dataset index
    `id`; the scenes of the split are numbered in order of first appearance there and each owns room for `max_proposals` records
    of `max_len` tokens, allocated at the first batch.  `add_batch`: the NMS launch and the collect launch, no read-back.
    `results()` -> {scene_id: [{"caption", "box", "sem_prob", "obj_prob"}, ...]}, scenes in the order they first appeared in the
    batches, a scene's records in slot order; raises when a decoded token lies outside the vocabulary, a kept proposal's class
    outside [0, 18) or an `id` outside chunked_data."""

    def __init__(self, chunked_data, vocabulary, max_proposals=SUBMIT_MAX_K, max_len=SUBMIT_MAX_TOKENS, device="cuda", post_dict=POST_DICT):
        name = "CaptionSubmission"
        if not 1 <= max_proposals <= SUBMIT_MAX_K or not 1 <= max_len <= SUBMIT_MAX_TOKENS:
            raise ValueError("%s: 1 <= max_proposals <= %d and 1 <= max_len <= %d (got %d, %d)"
                             % (name, SUBMIT_MAX_K, SUBMIT_MAX_TOKENS, max_proposals, max_len))
        cfg = dict(POST_DICT); cfg.update(post_dict or {})
        if not (cfg["use_3d_nms"] and cfg["cls_nms"]) or cfg["remove_empty_box"]:
            raise ValueError("%s: only the class-aware 3-D NMS the reference configures" % name)
        self.nms_iou, self.old_type = float(cfg["nms_iou"]), bool(cfg["use_old_type_nms"])
        idx2word = vocabulary["idx2word"]
        self.V = len(idx2word)
        if sorted(int(i) for i in idx2word) != list(range(self.V)):
            raise ValueError("%s: idx2word must number its words 0 .. V - 1" % name)
        self.words = [idx2word[str(i)] if str(i) in idx2word else idx2word[i] for i in range(self.V)]
        if self.words.count("eos") != 1:
            raise ValueError("%s: decode_caption stops at the literal word 'eos'; the vocabulary spells it %d times" % (name, self.words.count("eos")))
        self.eos = self.words.index("eos")
        self.scene_ids, index, table = [], {}, np.full(max(len(chunked_data), 1), -1, np.int32)
        for i, chunks in enumerate(chunked_data):
            if len(chunks):
                sid = chunks[0]["scene_id"]
                if sid not in index:
                    index[sid] = len(self.scene_ids); self.scene_ids.append(sid)
                table[i] = index[sid]
        if not self.scene_ids:
            raise ValueError("%s: chunked_data names no scene" % name)
        self._table, self.max_proposals, self.max_len, self.device = table, int(max_proposals), int(max_len), torch.device(device)
        self.reset()

    def reset(self):
        self._state, self._seq = None, 0

    def _geometry(self, d):
        name = "CaptionSubmission.add_batch"
        boxes, caps = d["proposal_bbox_batched"], d["lang_cap"]
        if boxes.dim() != 4 or tuple(boxes.shape[2:]) != (8, 3):
            raise ValueError("%s: proposal_bbox_batched (B,K,8,3) expected, got %s" % (name, tuple(boxes.shape)))
        B, K = boxes.shape[:2]
        if not 1 <= B <= SUBMIT_MAX_ROWS or not 1 <= K <= self.max_proposals:
            raise ValueError("%s: 1 <= B <= %d and 1 <= K <= %d (got B %d, K %d)" % (name, SUBMIT_MAX_ROWS, self.max_proposals, B, K))
        if caps.dim() != 3:
            raise ValueError("%s: lang_cap has shape %s, expected (%d, %d, T)" % (name, tuple(caps.shape), B, K))
        T = caps.shape[2]
        if not 1 <= T <= self.max_len:
            raise ValueError("%s: captions of T = %d tokens, the state holds 1 <= T <= %d" % (name, T, self.max_len))
        return dict(B=B, K=K, T=T)

    def _checked(self, d):
        dims = check_batch("CaptionSubmission.add_batch", d, _CAP_TABLE, self._geometry, self.device,
                           None if self._state is None else self._state["status"])
        return dims["B"], dims["K"], dims["T"]

    def add_batch(self, data_dict):
        """two launches (d3_nms3d_samecls, d3_caption_submit_batch), nothing read back; `data_dict` is left as it is"""
        d = data_dict
        B, K, T = self._checked(d)
        dev = d["lang_cap"].device
        if self._state is None:
            S, Kc, Tc = len(self.scene_ids), self.max_proposals, self.max_len
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            self._state = dict(box=z((S, Kc, 8, 3), torch.float32), cls=z((S, Kc), torch.int32), score=z((S, Kc), torch.float32),
                               ntok=z((S, Kc), torch.int32), tok=z((S, Kc, Tc), torch.int32), count=z((S,), torch.int32),
                               first_seen=torch.full((S,), -1, dtype=torch.int64, device=dev), status=z((1,), torch.int32),
                               table=torch.from_numpy(self._table).to(dev))
        st = self._state
        pick = nms_pred_mask_device(d, self.nms_iou, self.old_type)
        boxes, sem, scores, caps = (d[k].detach().contiguous() for k in ("proposal_bbox_batched", "proposal_sem_cls_batched",
                                                                         "proposal_scores_batched", "lang_cap"))
        ids = as_i64(d["id"])
        with on(dev):
            call("caption_submit_batch", ptr(boxes), ptr(sem), ptr(scores), ptr(pick), ptr(caps), ptr(ids), ptr(st["table"]),
                 st["table"].numel(), B, K, T, self.V, self.eos, self._seq, len(self.scene_ids), self.max_proposals, self.max_len,
                 *[ptr(st[k]) for k in _CAP_STATE], stream())
        self._seq += 1

    def records(self):
        """the state read back once -> dict of numpy arrays (box, cls, score, ntok, tok, count, first_seen, status)"""
        if self._state is None:
            raise ValueError("CaptionSubmission: no batch was added")
        return dict(zip(_CAP_STATE, read_back([self._state[k] for k in _CAP_STATE])))

    def results(self):
        rec = self.records()
        status = int(rec["status"][0])
        if status & 1:
            raise _lib.D3Error("CaptionSubmission: a kept caption holds a token outside the vocabulary")
        if status & 2:
            raise _lib.D3Error("CaptionSubmission: a kept proposal's class (sem - 2, negative -> 17) lies outside [0, %d)" % NUM_CLASS)
        if status & 4:
            raise _lib.D3Error("CaptionSubmission: a batch's `id` names no scene of chunked_data")
        return format_caption_results(rec, self.scene_ids, self.words)

    def write(self, path):
        with open(path, "w") as f:
            json.dump(self.results(), f, indent=4)


def format_caption_results(rec, scene_ids, words):
    """the host half of CaptionSubmission.results: per-scene record arrays -> benchmark_captioning.py:167-188's dict.  Floats are
    the float32 values as Python floats, as `.cpu().numpy().tolist()` gives them."""
    first = np.asarray(rec["first_seen"])
    seen = np.flatnonzero(first >= 0)
    out = {}
    for s in seen[np.argsort(first[seen], kind="stable")].tolist():
        scene = []
        for r in range(int(rec["count"][s])):
            decoded = ["sos"] + [words[t] for t in rec["tok"][s, r, :int(rec["ntok"][s, r])].tolist()]
            if "eos" not in decoded:
                decoded.append("eos")
            sem_prob = np.zeros(NUM_CLASS, np.float32)
            sem_prob[int(rec["cls"][s, r])] = 1
            scene.append({"caption": " ".join(decoded), "box": np.asarray(rec["box"][s, r], np.float32).tolist(), "sem_prob": sem_prob.tolist(),
                          "obj_prob": np.array([0, rec["score"][s, r]], np.float32).tolist()})
        out[scene_ids[s]] = scene
    return out


class GroundingSubmission:
    """benchmark_grounding.py:110-186 (predict) on the device.  `add_batch`: one d3_ground_submit_batch launch that writes one
    record per description row behind the earlier batches' (the record storage doubles on the device), no read-back.  `results()`
    -> [{"scene_id", "object_id", "ann_id", "bbox", "unique_multiple", "others"}, ...] over the rows whose annotation was not
    named by an earlier row of the same batch, in row order; raises on an `id` / `chunk_ids` pair without an annotation."""

    def __init__(self, chunked_data, device="cuda"):
        self.chunked_data = chunked_data
        D, Cmax = max(len(chunked_data), 1), max([len(c) for c in chunked_data] + [1])
        table, numbers = np.full((D, Cmax), -1, np.int32), {}
        for i, chunks in enumerate(chunked_data):
            for j, ann in enumerate(chunks):
                query = "{}-{}-{}".format(ann["scene_id"], ann["object_id"], ann["ann_id"])          # benchmark_grounding.py:168
                table[i, j] = numbers.setdefault(query, len(numbers))
        if not numbers:
            raise ValueError("GroundingSubmission: chunked_data holds no annotation")
        self._table, self.device = table, torch.device(device)
        self.reset()

    def reset(self):
        self._rec = self._status = self._key_of = None

    @staticmethod
    def _geometry(d):
        name = "GroundingSubmission.add_batch"
        ref, boxes = d["cluster_ref"], d["proposal_bbox_batched"]
        if ref.dim() != 2 or boxes.dim() != 4 or tuple(boxes.shape[2:]) != (8, 3):
            raise ValueError("%s: cluster_ref (N,K) and proposal_bbox_batched (B,K,8,3) expected" % name)
        (N, K), B = ref.shape, boxes.shape[0]
        if B < 1 or N < 1 or N % B or not 1 <= K <= GROUND_MAX_K or boxes.shape[1] != K:
            raise ValueError("%s: B >= 1, N = B * C >= 1 and 1 <= K <= %d, the same for scores and boxes (got B %d, N %d, K %d and %d)"
                             % (name, GROUND_MAX_K, B, N, K, boxes.shape[1]))
        return dict(B=B, C=N // B, K=K, N=N)

    def _checked(self, d):
        dims = check_batch("GroundingSubmission.add_batch", d, _GROUND_TABLE, self._geometry, self.device, self._status)
        return tuple(dims[k] for k in "BCKN")

    def add_batch(self, data_dict):
        """one launch, nothing read back; `data_dict` is left as it is"""
        d = data_dict
        B, Cn, K, N = self._checked(d)
        dev = d["cluster_ref"].device
        if self._status is None:
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
            self._key_of = torch.from_numpy(self._table).to(dev)
            self._rec = RecordStore(dev, **_GROUND_REC)
        r = self._rec
        r.reserve(r.rows + N)
        ref, boxes = d["cluster_ref"].detach().contiguous(), d["proposal_bbox_batched"].detach().contiguous()
        um, cat, ids, chunks = (as_i64(d[k]) for k in ("unique_multiple", "object_cat", "id", "chunk_ids"))
        with on(dev):
            call("ground_submit_batch", ptr(ref), ptr(boxes), ptr(um), ptr(cat), ptr(ids), ptr(chunks), ptr(self._key_of),
                 self._table.shape[0], self._table.shape[1], B, Cn, K, r.rows, *[ptr(r[k]) for k in _GROUND_REC], ptr(self._status), stream())
        r.rows += N

    def records(self):
        """the rows read back once -> dict of numpy arrays (bbox, pred_ref, unique_multiple, others, key, keep, ids, status)"""
        if self._rec is None:
            raise ValueError("GroundingSubmission: no batch was added")
        rec, (status,) = self._rec.read_back(self._status)
        return dict(rec, status=status)

    def results(self):
        rec = self.records()
        if int(rec["status"][0]) & 1:
            raise _lib.D3Error("GroundingSubmission: an `id` / `chunk_ids` pair names no annotation of chunked_data")
        return format_grounding_results(rec, self.chunked_data)

    def write(self, path):
        with open(path, "w") as f:
            json.dump(self.results(), f, indent=4)


def format_grounding_results(rec, chunked_data):
    """the host half of GroundingSubmission.results: the kept rows -> benchmark_grounding.py:155-178's list"""
    out = []
    for i in np.flatnonzero(np.asarray(rec["keep"]) != 0).tolist():
        scene, chunk = (int(x) for x in rec["ids"][i])
        ann = chunked_data[scene][chunk]
        out.append({"scene_id": ann["scene_id"], "object_id": ann["object_id"], "ann_id": ann["ann_id"],
                    "bbox": np.asarray(rec["bbox"][i], np.float32).tolist(), "unique_multiple": int(rec["unique_multiple"][i]),
                    "others": int(rec["others"][i])})
    return out
