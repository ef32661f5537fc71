#!/usr/bin/env python3
"""Seconds per validation-sized grounding evaluation (312 scenes: 26 batches of tests/golden's eval_inputs(B=12, Cn=8, K=128), one
seed per batch, 18 language classes, one repeat), inputs on the GPU as `PipelineNet._ground` leaves them:
  host path    grounding_eval.get_eval per batch and the list appends of scripts/eval.py:224-228 (the three `.tolist()` copies, the
               IoUs' `.cpu()`, `lang_acc.item()`), then the cell counts with numpy and grounding_scores;
  device path  GroundingEvaluator.add_batch per batch (csrc/grounding_eval.hip, one launch, no read-back), one compute.
Wall clock between two torch.cuda.synchronize() calls, the epoch-end table included, the two paths alternating, one warm-up round
and the median of three timed rounds each.  Also whether stats and scores of the two paths are equal, and both language accuracies:
the device forms a batch's float32 mean as correct / N, which is what torch's mean gives on the CPU (the golden's arithmetic);
torch's GPU mean multiplies by a rounded 1 / N and can differ in the last bit when N is no power of two.  Nothing asserts on the
times.  Run under `timeout`; prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from d3net_amd import grounding_eval as ge   # noqa: E402
from gen_grounding_eval_golden import eval_inputs   # noqa: E402


def host_path(batches):
    ref_acc, ious, masks, others, lang_acc, rows = [], [], [], [], [], []
    for d in batches:
        d = ge.get_eval(dict(d), grounding=True, use_lang_classifier=True)
        ref_acc += d["ref_acc"]
        ious += d["ref_iou"].cpu().numpy().tolist()
        masks += d["ref_multiple_mask"]
        others += d["ref_others_mask"]
        lang_acc.append(d["lang_acc"].item())
        rows.append(len(d["ref_acc"]))
    table = np.zeros((3, 2, 4), np.int64)
    mk = np.array(masks)
    m = np.where((mk == 0) | (mk == 1), mk, 2)
    hits = np.stack([np.ones(len(ious)), np.array(ref_acc) == 1, np.array(ious) >= 0.25, np.array(ious) >= 0.5], 1).astype(np.int64)
    np.add.at(table, (m, np.array(others)), hits)
    stats, scores, _ = ge.grounding_scores(table[None])
    return {"stats": stats, "scores": scores, "lang_acc": float(np.mean(np.array(lang_acc)))}, None


def device_path(batches):
    e = ge.GroundingEvaluator()
    t0 = time.perf_counter()
    for d in batches:
        e.add_batch(d)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return e.compute(), t1 - t0


def main(n_batches=26, B=12, Cn=8, K=128, rounds=3, warm=1):
    dev = torch.device("cuda", 0)
    batches = [{k: torch.from_numpy(v).to(dev) for k, v in eval_inputs(B=B, Cn=Cn, K=K, seed=21 + i).items()} for i in range(n_batches)]
    times, add_s, res = {"host": [], "device": []}, [], {}
    for rnd in range(rounds + warm):
        for name, fn in (("host", host_path), ("device", device_path)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[name], extra = fn(batches)
            torch.cuda.synchronize()
            if rnd >= warm:
                times[name].append(time.perf_counter() - t0)
                if extra is not None:
                    add_s.append(extra)
    same = all(res["host"][k] == res["device"][k] for k in ("stats", "scores"))
    stat = lambda s: {"median": float(np.median(s)), "min": float(min(s)), "max": float(max(s))}
    print(json.dumps({"scenes": n_batches * B, "rows": n_batches * B * Cn, "K": K, "rounds": rounds, "host_path_s": stat(times["host"]),
                      "device_path_s": stat(times["device"]), "device_add_batch_s": stat(add_s),
                      "speedup_median": float(np.median(times["host"]) / np.median(times["device"])), "equal_stats_and_scores": bool(same),
                      "overall": {k: float(v) for k, v in res["device"]["scores"]["overall"]["overall"].items()},
                      "lang_acc": {"host": res["host"]["lang_acc"], "device": res["device"]["lang_acc"]}}))


if __name__ == "__main__":
    main()
