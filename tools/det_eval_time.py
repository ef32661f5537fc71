#!/usr/bin/env python3
"""Seconds per validation-sized detection evaluation (312 scenes: 26 batches of tests/golden's evaluator_inputs(B=12, K=256), one
seed per batch, G = 128 GT slots, IoU thresholds 0.25 and 0.5), inputs on the GPU as `feed` leaves them:
  host path    parse_predictions(device_nms=False) + parse_groundtruths per batch, two APCalculators, compute_metrics of both;
  device path  DetectionEvaluator.add_batch per batch (csrc/nms.hip + csrc/det_eval.hip), one compute_metrics.
Wall clock between two torch.cuda.synchronize() calls, compute_metrics included, the two paths alternating, one warm-up round and
the median of three timed rounds each.  Also how far the two results are apart.  Nothing asserts on the times.  Run under
`timeout`; prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from d3net_amd import evaluator as ev   # noqa: E402
from gen_evaluator_golden import evaluator_inputs   # noqa: E402

THRESHOLDS = (0.25, 0.5)


def host_path(batches):
    calcs = [ev.APCalculator(t) for t in THRESHOLDS]
    for d in batches:
        d = dict(d)
        preds, gts = ev.parse_predictions(d, device_nms=False), ev.parse_groundtruths(d)
        for c in calcs:
            c.step(preds, gts)
    return [c.compute_metrics() for c in calcs], None


def device_path(batches):
    e = ev.DetectionEvaluator(THRESHOLDS)
    t0 = time.perf_counter()
    for d in batches:
        e.add_batch(d)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return e.compute_metrics(), t1 - t0


def main(n_batches=26, B=12, K=256, rounds=3, warm=1):
    dev = torch.device("cuda", 0)
    batches = [{k: torch.from_numpy(v).to(dev) for k, v in evaluator_inputs(B=B, K=K, seed=21 + i).items()} for i in range(n_batches)]
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
    diff = max(abs(res["host"][q][k] - res["device"][q][k]) for q in range(len(THRESHOLDS)) for k in res["host"][q])
    same_keys = all(list(res["host"][q]) == list(res["device"][q]) for q in range(len(THRESHOLDS)))
    stat = lambda s: {"median": float(np.median(s)), "min": float(min(s)), "max": float(max(s))}
    print(json.dumps({"scenes": n_batches * B, "K": K, "G": 128, "thresholds": THRESHOLDS, "rounds": rounds,
                      "host_path_s": stat(times["host"]), "device_path_s": stat(times["device"]),
                      "device_add_batch_s": stat(add_s), "speedup_median": float(np.median(times["host"]) / np.median(times["device"])),
                      "same_keys": same_keys, "max_abs_metric_difference": float(diff),
                      "mAP": {"host": [float(r["mAP"]) for r in res["host"]], "device": [float(r["mAP"]) for r in res["device"]]}}))


if __name__ == "__main__":
    main()
