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

from .evaluator import POST_DICT

SUBMIT_MAX_K, SUBMIT_MAX_TOKENS, SUBMIT_MAX_ROWS = 256, 62, 1 << 20      # proposal slots / caption tokens / rows per batch of csrc/submission.hip
GROUND_MAX_K = 4096
NUM_CLASS = 18
_INTS = (torch.int32, torch.int64)
_FLAGS = (torch.float32, torch.bool, torch.uint8) + _INTS
_CAP_KEYS = ("proposal_bbox_batched", "proposal_sem_cls_batched", "proposal_scores_batched", "proposal_batch_mask", "lang_cap", "id")
_GROUND_KEYS = ("cluster_ref", "proposal_bbox_batched", "unique_multiple", "object_cat", "id", "chunk_ids")


def _on_gpu(name, d, keys, device, state):
    for k in keys:
        t = d[k]
        if not t.is_cuda:
            raise ValueError("%s: %s is in host memory (%s); the writers run on the GPU, there is no CPU fallback" % (name, k, t.device))
        if (device.index is not None and t.device != device) or t.device != d[keys[0]].device or (state is not None and t.device != state.device):
            raise ValueError("%s: %s is on %s; the batches of one submission live on one GPU (%s)" % (name, k, t.device, device))


def _present(name, d, keys):
    missing = [k for k in keys if k not in d]
    if missing:
        raise ValueError("%s: missing %s" % (name, missing))
    for k in keys:
        if not torch.is_tensor(d[k]):
            raise ValueError("%s: %s must be a tensor" % (name, k))


def _bytes_back(tensors):
    """the one read-back: the tensors as one byte run -> numpy arrays of their dtypes and shapes"""
    flat = torch.cat([t.contiguous().view(-1).view(torch.uint8) for t in tensors]).cpu().numpy()
    out, pos = [], 0
    for t in tensors:
        n = t.numel() * t.element_size()
        out.append(flat[pos:pos + n].view(np.dtype(str(t.dtype).replace("torch.", ""))).reshape(tuple(t.shape)))
        pos += n
    return out


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

    def _checked(self, d):
        name = "CaptionSubmission.add_batch"
        _present(name, d, _CAP_KEYS)
        boxes, sem, scores, mask, caps, ids = (d[k] for k in _CAP_KEYS)
        if boxes.dim() != 4 or tuple(boxes.shape[2:]) != (8, 3):
            raise ValueError("%s: proposal_bbox_batched (B,K,8,3) expected, got %s" % (name, tuple(boxes.shape)))
        B, K = boxes.shape[:2]
        if not 1 <= B <= SUBMIT_MAX_ROWS or not 1 <= K <= self.max_proposals:
            raise ValueError("%s: 1 <= B <= %d and 1 <= K <= %d (got B %d, K %d)" % (name, SUBMIT_MAX_ROWS, self.max_proposals, B, K))
        for k in _CAP_KEYS[1:4]:
            if tuple(d[k].shape) != (B, K):
                raise ValueError("%s: %s has shape %s, expected %s" % (name, k, tuple(d[k].shape), (B, K)))
        if caps.dim() != 3 or tuple(caps.shape[:2]) != (B, K):
            raise ValueError("%s: lang_cap has shape %s, expected (%d, %d, T)" % (name, tuple(caps.shape), B, K))
        T = caps.shape[2]
        if not 1 <= T <= self.max_len:
            raise ValueError("%s: captions of T = %d tokens, the state holds 1 <= T <= %d" % (name, T, self.max_len))
        if tuple(ids.shape) != (B,):
            raise ValueError("%s: id has shape %s, expected %s" % (name, tuple(ids.shape), (B,)))
        floats = (torch.float32,)
        ok = dict(zip(_CAP_KEYS, (floats, floats, floats, _FLAGS, (torch.int64,), _INTS)))
        for k in _CAP_KEYS:
            if d[k].dtype not in ok[k]:
                raise ValueError("%s: %s has dtype %s, expected one of %s" % (name, k, d[k].dtype, ok[k]))
        _on_gpu(name, d, _CAP_KEYS, self.device, None if self._state is None else self._state["status"])
        return B, K, T

    def add_batch(self, data_dict):
        """two launches (d3_nms3d_samecls, d3_caption_submit_batch), nothing read back; `data_dict` is left as it is"""
        import ctypes as C
        from . import _lib
        from .evaluator import nms_pred_mask_device
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
        boxes, sem, scores = (d[k].detach().contiguous() for k in _CAP_KEYS[:3])
        caps, ids = d["lang_cap"].detach().contiguous(), d["id"].detach().long().contiguous()
        p = lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().d3_caption_submit_batch(
                p(boxes), p(sem), p(scores), p(pick), p(caps), p(ids), p(st["table"]), st["table"].numel(), B, K, T, self.V, self.eos, self._seq,
                len(self.scene_ids), self.max_proposals, self.max_len, p(st["box"]), p(st["cls"]), p(st["score"]), p(st["ntok"]), p(st["tok"]),
                p(st["count"]), p(st["first_seen"]), p(st["status"]), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "caption_submit_batch")
        self._seq += 1

    def records(self):
        """the state read back once -> dict of numpy arrays (box, cls, score, ntok, tok, count, first_seen, status)"""
        if self._state is None:
            raise ValueError("CaptionSubmission: no batch was added")
        keys = ("box", "cls", "score", "ntok", "tok", "count", "first_seen", "status")
        return dict(zip(keys, _bytes_back([self._state[k] for k in keys])))

    def results(self):
        from . import _lib
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
        self._rows = 0

    def _checked(self, d):
        name = "GroundingSubmission.add_batch"
        _present(name, d, _GROUND_KEYS)
        ref, boxes = d["cluster_ref"], d["proposal_bbox_batched"]
        if ref.dim() != 2 or boxes.dim() != 4 or tuple(boxes.shape[2:]) != (8, 3):
            raise ValueError("%s: cluster_ref (N,K) and proposal_bbox_batched (B,K,8,3) expected" % name)
        (N, K), B = ref.shape, boxes.shape[0]
        if B < 1 or N < 1 or N % B or not 1 <= K <= GROUND_MAX_K or boxes.shape[1] != K:
            raise ValueError("%s: B >= 1, N = B * C >= 1 and 1 <= K <= %d, the same for scores and boxes (got B %d, N %d, K %d and %d)"
                             % (name, GROUND_MAX_K, B, N, K, boxes.shape[1]))
        Cn = N // B
        want = {"unique_multiple": ((B, Cn), (N,)), "object_cat": ((B, Cn), (N,)), "id": ((B,),), "chunk_ids": ((B, Cn),)}
        for k, shapes in want.items():
            if tuple(d[k].shape) not in shapes:
                raise ValueError("%s: %s has shape %s, expected %s" % (name, k, tuple(d[k].shape), " or ".join(map(str, shapes))))
        floats = (torch.float32,)
        ok = dict(zip(_GROUND_KEYS, (floats, floats, _INTS, _INTS, _INTS, _INTS)))
        for k in _GROUND_KEYS:
            if d[k].dtype not in ok[k]:
                raise ValueError("%s: %s has dtype %s, expected one of %s" % (name, k, d[k].dtype, ok[k]))
        _on_gpu(name, d, _GROUND_KEYS, self.device, self._status)
        return B, Cn, K, N

    def add_batch(self, data_dict):
        """one launch, nothing read back; `data_dict` is left as it is"""
        import ctypes as C
        from . import _lib
        from .grounding_eval import GroundingEvaluator
        d = data_dict
        B, Cn, K, N = self._checked(d)
        dev = d["cluster_ref"].device
        if self._status is None:
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
            self._key_of = torch.from_numpy(self._table).to(dev)
            z = lambda shape, dt: torch.zeros((1024,) + shape, dtype=dt, device=dev)
            self._rec = dict(bbox=z((8, 3), torch.float32), pred_ref=z((), torch.int32), unique_multiple=z((), torch.int64),
                             others=z((), torch.int32), key=z((), torch.int32), keep=z((), torch.int32), ids=z((2,), torch.int64))
        self._rec = {k: GroundingEvaluator._grown(t, self._rows + N) for k, t in self._rec.items()}
        i64 = lambda t: t.detach().contiguous() if t.dtype == torch.int64 else t.detach().long().contiguous()
        ref, boxes = d["cluster_ref"].detach().contiguous(), d["proposal_bbox_batched"].detach().contiguous()
        um, cat, ids, chunks = (i64(d[k]) for k in _GROUND_KEYS[2:])
        p = lambda t: C.c_void_p(t.data_ptr())
        r = self._rec
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().d3_ground_submit_batch(
                p(ref), p(boxes), p(um), p(cat), p(ids), p(chunks), p(self._key_of), self._table.shape[0], self._table.shape[1], B, Cn, K,
                self._rows, p(r["bbox"]), p(r["pred_ref"]), p(r["unique_multiple"]), p(r["others"]), p(r["key"]), p(r["keep"]), p(r["ids"]),
                p(self._status), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ground_submit_batch")
        self._rows += N

    def records(self):
        """the rows read back once -> dict of numpy arrays (bbox, pred_ref, unique_multiple, others, key, keep, ids, status)"""
        if self._rec is None:
            raise ValueError("GroundingSubmission: no batch was added")
        keys = tuple(self._rec)
        back = _bytes_back([self._rec[k][:self._rows] for k in keys] + [self._status])
        return dict(zip(keys + ("status",), back))

    def results(self):
        from . import _lib
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
