"""Plain numpy restatement of csrc/submission.hip's per-row rules: what one batch row leaves in the Scan2Cap state and what one
description row leaves in the ScanRefer records.  A test helper that shares no code with d3net_amd.submission:
tests/test_submission.py pins it, through the library's host formatter, against the files the reference's own two `predict`
functions wrote (tests/golden/submission_golden.npz); the GPU tests compare the kernels with it field by field."""
import numpy as np

from grounding_epoch_restate import argmax

NUM_CLASS = 18
SEQ_BITS = 20


def scene_table(chunked_data):
    """-> (scene ids in order of first appearance, (D) int32 scene slot of every dataset index, -1: none)"""
    names, table = [], np.full(max(len(chunked_data), 1), -1, np.int32)
    for i, chunks in enumerate(chunked_data):
        if len(chunks):
            sid = chunks[0]["scene_id"]
            if sid not in names:
                names.append(sid)
            table[i] = names.index(sid)
    return names, table


def key_table(chunked_data):
    """-> (D, Cmax) int32: equal "scene-object-ann" strings, equal numbers; -1: no annotation"""
    Cmax = max([len(c) for c in chunked_data] + [1])
    table, seen = np.full((max(len(chunked_data), 1), Cmax), -1, np.int32), []
    for i, chunks in enumerate(chunked_data):
        for j, a in enumerate(chunks):
            q = "{}-{}-{}".format(a["scene_id"], a["object_id"], a["ann_id"])
            if q not in seen:
                seen.append(q)
            table[i, j] = seen.index(q)
    return table


def caption_state(S, Kcap, Tcap):
    return dict(box=np.zeros((S, Kcap, 8, 3), np.float32), cls=np.zeros((S, Kcap), np.int32), score=np.zeros((S, Kcap), np.float32),
                ntok=np.zeros((S, Kcap), np.int32), tok=np.zeros((S, Kcap, Tcap), np.int32), count=np.zeros(S, np.int32),
                first_seen=np.full(S, -1, np.int64), status=np.zeros(1, np.int32))


def caption_batch(state, d, pick, table, V, eos, seq):
    """one batch into `state`: d holds numpy arrays under the writer's keys, pick (B,K) is the NMS mask"""
    boxes, sem, scores, caps, ids = (np.asarray(d[k]) for k in ("proposal_bbox_batched", "proposal_sem_cls_batched",
                                                                "proposal_scores_batched", "lang_cap", "id"))
    B, K, T = caps.shape
    S = state["count"].shape[0]
    scene = []
    for b in range(B):
        i = int(ids[b])
        s = int(table[i]) if 0 <= i < len(table) else -1
        scene.append(s if 0 <= s < S else -1)
    for b in range(B):
        s = scene[b]
        if s < 0:
            state["status"][0] |= 4
            continue
        if s not in scene[:b] and state["first_seen"][s] < 0:
            state["first_seen"][s] = (seq << SEQ_BITS) + b
        if s in scene[b + 1:]:
            continue                                                    # a later row of the batch replaces this one
        kept = [k for k in range(K) if pick[b, k] == 1]
        for r, k in enumerate(kept):
            state["box"][s, r] = boxes[b, k]
            c = np.float32(sem[b, k]) - np.float32(2)
            if c < 0:
                c = np.float32(17)
            if not (c >= 0 and c < NUM_CLASS):
                state["status"][0] |= 2
                c = 0
            state["cls"][s, r] = int(c)
            state["score"][s, r] = scores[b, k]
            toks = caps[b, k].tolist()
            cut = toks.index(eos) + 1 if eos in toks else T
            if any(t < 0 or t >= V for t in toks[:cut]):
                state["status"][0] |= 1
            state["tok"][s, r, :T] = [t if 0 <= t < V else 0 for t in toks]
            state["ntok"][s, r] = cut
        state["count"][s] = len(kept)
    return state


def ground_batch(d, key_of):
    """one batch -> per-row records (bbox, pred_ref, unique_multiple, others, key, keep, ids) and the status"""
    ref, boxes = np.asarray(d["cluster_ref"], np.float32), np.asarray(d["proposal_bbox_batched"], np.float32)
    N, K = ref.shape
    B = boxes.shape[0]
    Cn = N // B
    um, cat = np.asarray(d["unique_multiple"]).reshape(-1), np.asarray(d["object_cat"]).reshape(-1)
    ids, chunks = np.repeat(np.asarray(d["id"]), Cn), np.asarray(d["chunk_ids"]).reshape(-1)
    D, Cmax = key_of.shape
    out = dict(bbox=np.zeros((N, 8, 3), np.float32), pred_ref=np.zeros(N, np.int32), unique_multiple=um.astype(np.int64),
               others=(cat == 17).astype(np.int32), key=np.zeros(N, np.int32), keep=np.zeros(N, np.int32),
               ids=np.stack([ids, chunks], 1).astype(np.int64))
    status = 0
    for n in range(N):
        p = argmax(ref[n])                                              # every slot, valid or not
        out["pred_ref"][n], out["bbox"][n] = p, boxes[n // Cn, p]
        key = int(key_of[ids[n], chunks[n]]) if 0 <= ids[n] < D and 0 <= chunks[n] < Cmax else -1
        out["key"][n] = key
        if key < 0:
            status |= 1
        out["keep"][n] = int(key >= 0 and key not in out["key"][:n].tolist())
    return out, status


def ground_epoch(batches, key_of):
    """-> the records of all batches, row after row, and the OR of their status"""
    parts, status = [], 0
    for d in batches:
        rec, st = ground_batch(d, key_of)
        parts.append(rec); status |= st
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    out["status"] = np.array([status], np.int32)
    return out
