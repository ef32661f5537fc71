#!/usr/bin/env python3
"""Milliseconds per batch of description features at the bench's shape (4 scenes x 8 descriptions, L = 128, V = 3004, D = 300):
d3net_amd.lang_prep.prepare_descriptions (HIP events on the preparing stream; includes the host draws and the row-index upload)
against the restatement of the reference's host path (tests/lang_prep_restate.py: deep copy of the per-description float64 arrays,
erase, stack, float32 cast; wall clock) plus the host-to-device copy of its (B, C, L, 300) float32 result.  Both take the same draws.
Warm-up first, median of the repeats.  Nothing asserts on the times.  Run under `timeout`; prints one JSON line."""
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lang_prep_restate as LR                     # noqa: E402
from d3net_amd import lang_prep as LP, synthetic   # noqa: E402

B, CHUNK, MAX_LEN, V, D = 4, 8, 126, 3004, 300


def annotations(seed=0):
    r = np.random.RandomState(seed)
    return [{"scene_id": "scene%04d_00" % b, "object_id": str(c), "object_name": "chair", "ann_id": "0",
             "token": ["w%d" % w for w in r.randint(0, V - 4, r.randint(10, MAX_LEN + 1))]} for b in range(B) for c in range(CHUNK)]


def host_path(index, store, glove, draws, dev):
    rows = np.concatenate([d["rows"] for d in draws])
    erase = [e for d in draws for e in d["erase"]]
    feat, ids, lens = LR.lang_features(store, index.token_len, glove, index.unk, rows, erase, index.L)
    return [torch.from_numpy(x).to(dev) for x in (feat.reshape(B, CHUNK, index.L, D), ids, lens)]


def main(reps=20):
    dev = torch.device("cuda", 0)
    glove = np.random.RandomState(1).randn(V, D).astype(np.float32)
    index = LP.DescriptionIndex(annotations(), synthetic.make_vocabulary(V), glove, MAX_LEN, CHUNK, {"chair": 2}, device=dev)
    store = LR.description_store(index.token_ids, index.token_len, glove)
    chunks = list(range(B))
    ours, theirs = index.table_bytes()
    res = {"scenes": B, "descriptions_per_scene": CHUNK, "L": index.L, "V": V, "D": D, "table_bytes": ours,
           "reference_store_bytes": theirs}
    dev_ms, host_ms = [], []
    for rep in range(reps + 3):
        rng, pyrng = np.random.RandomState(rep), random.Random(rep)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        LP.prepare_descriptions(index, chunks, rng=rng, pyrng=pyrng, is_augment=True, device=dev)
        b.record()
        b.synchronize()
        rng, pyrng = np.random.RandomState(rep), random.Random(rep)
        t0 = time.perf_counter()
        draws = [LP.draw_descriptions(index, c, rng, pyrng, is_augment=True) for c in chunks]
        host_path(index, store, glove, draws, dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if rep >= 3:                                # the first three are warm-up (allocator, code objects)
            dev_ms.append(a.elapsed_time(b))
            host_ms.append((t1 - t0) * 1e3)
    for name, ms in (("device_ms_per_batch", dev_ms), ("host_ms_per_batch", host_ms)):
        res[name] = {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
