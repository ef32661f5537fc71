#!/usr/bin/env python3
"""Seconds per captioning validation (n_batches batches of tests/golden's caption_inputs(B, K=128, G=24, L=31), one seed per
batch, scene names made distinct per batch so that every batch brings new keys; IoU threshold 0.5), inputs on the GPU as the
speaker's evaluation decode leaves them:
  host path    eval_caption_step per batch (device assignment, four copies to the host, the B x G decode loop), the setdefault
               merge, eval_caption_epoch (BLEU, CIDEr and ROUGE over strings);
  device path  CaptionEvaluator.add_batch per batch (csrc/assign.hip + csrc/caption_eval.hip), one compute (csrc/cider.hip +
               csrc/caption_eval.hip, two read-backs).  The EvalCorpus is built once, outside the timing, as once per split.
Wall clock between two torch.cuda.synchronize() calls, the epoch-end scoring included, the two paths alternating, one warm-up
round and the median of three timed rounds each.  Also how far the two results are apart.  Nothing asserts on the times.  Run
under `timeout`; prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from d3net_amd import caption_eval as ce   # noqa: E402
from gen_caption_eval_golden import caption_inputs   # noqa: E402

MIN_IOU, MAX_LEN = 0.5, 30


def host_path(batches, raw, vocab, evaluator):
    candidates = {}
    for d in batches:
        for k, v in ce.eval_caption_step(dict(d), vocab).items():
            candidates.setdefault(k, v)
    return ce.eval_caption_epoch(candidates, raw, max_len=MAX_LEN, min_iou=MIN_IOU), None


def device_path(batches, raw, vocab, evaluator):
    evaluator.reset()
    t0 = time.perf_counter()
    for d in batches:
        evaluator.add_batch(d)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return evaluator.compute(MIN_IOU), t1 - t0


def main(n_batches=26, B=12, rounds=3, warm=1):
    dev = torch.device("cuda", 0)
    batches, raw, vocab = [], [], None
    for i in range(n_batches):
        inp = caption_inputs(B=B, seed=17 + i)
        rename = {s: "scene%04d_%02d" % (b, i) for b, s in enumerate(inp["scene_list"])}
        raw += [dict(d, scene_id=rename[d["scene_id"]]) for d in inp["raw"]]
        vocab = inp["vocab"]
        t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items() if isinstance(v, np.ndarray)}
        batches.append(dict(lang_cap=t["pred_captions"], proposal_bbox_batched=t["pred_boxes"], gt_bbox=t["gt_boxes"],
                            gt_bbox_object_id=t["gt_box_ids"], gt_bbox_label=t["gt_box_masks"],
                            scene_id=[rename[s] for s in inp["scene_list"]]))
    evaluator = ce.CaptionEvaluator(raw, vocab, max_len=MAX_LEN, min_iou=MIN_IOU, device=dev)
    times, add_s, res = {"host": [], "device": []}, [], {}
    for rnd in range(rounds + warm):
        for name, fn in (("host", host_path), ("device", device_path)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[name], extra = fn(batches, raw, vocab, evaluator)
            torch.cuda.synchronize()
            if rnd >= warm:
                times[name].append(time.perf_counter() - t0)
                if extra is not None:
                    add_s.append(extra)
    (hb, hc, hr, _), (db, dc, dr, _) = res["host"], res["device"]
    stat = lambda s: {"median": float(np.median(s)), "min": float(min(s)), "max": float(max(s))}
    print(json.dumps({"scenes": n_batches * B, "K": 128, "G": 24, "T": 31, "entries": len(dc[1]), "descriptions": len(raw), "min_iou": MIN_IOU,
                      "rounds": rounds, "host_path_s": stat(times["host"]), "device_path_s": stat(times["device"]),
                      "device_add_batch_s": stat(add_s), "speedup_median": float(np.median(times["host"]) / np.median(times["device"])),
                      "bleu_equal": bool(hb[0] == db[0] and hb[1] == db[1]), "rouge_equal": bool(hr[0] == dr[0] and hr[1].tolist() == dr[1].tolist()),
                      "cider_max_rel_difference": float(np.max(np.abs(hc[1] - dc[1]) / np.maximum(np.abs(hc[1]), 1e-300))),
                      "cider": {"host": hc[0], "device": dc[0]}, "bleu-4": {"host": hb[0][3], "device": db[0][3]},
                      "rouge": {"host": hr[0], "device": dr[0]}}))


if __name__ == "__main__":
    main()
