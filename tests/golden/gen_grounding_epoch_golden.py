#!/usr/bin/env python3
"""Generates tests/golden/grounding_epoch_golden.npz by RUNNING THE REFERENCE: per (repeat, batch) its own
`lib/grounding/eval_helper.get_eval` on the CPU, the lists `scripts/eval.py:224-228` appends pickled as `scores.p`, then its own
`eval_grounding` (scripts/eval.py:168-426) through the load branch (eval.repeat = 1, eval.force = False, the file present: the
generation loop cannot run, `batch_data` is undefined at :199, while the load branch aggregates however many repeat rows the file
holds) with stdout captured and the printed `a | b | c: value` lines parsed.  Run in the build container only (needs
/root/reference); the tests never run it.  Inputs are not stored: `epoch_inputs()` rebuilds them.  Stored: arrays, scalars and the
numpy version (the reference adds 1e-8 to numpy float32 scalars: a float64 sum under numpy 1.x, float32 under numpy 2)."""
import contextlib
import importlib.util
import io
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

SGN = np.array([[1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1], [1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1]], np.float32)
# (B, C, K) per batch; every repeat holds 17 rows.  K = 1, 63, 64, 65, 257 (below, at and above the wave; several strides), C = 1 and 4,
# a batch with B = 1, and N = 5 rows: no multiple of the 4 waves of a workgroup
SHAPES = (((2, 4, 63), (5, 1, 1), (1, 4, 64)), ((2, 4, 65), (5, 1, 257), (1, 4, 64)))
L = 18
KEYS = ("ref_acc", "acc@0.25iou", "acc@0.5iou")
ROWS = ("unique", "multiple", "overall")
COLS = ("not_in_others", "in_others", "overall")


def _cube(lo, hi):
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return ((lo + hi) / 2)[None] + SGN * ((hi - lo) / 2)[None]


def _batch(rng, B, Cn, K):
    N = B * Cn
    mask = (rng.random((B, K)) < 0.6).astype(np.float32)
    mask[:, 0] = 1 if K == 1 else mask[:, 0]
    c = rng.random((B, K, 3)).astype(np.float32) * np.array([4, 3, 2], np.float32)
    s = rng.random((B, K, 3)).astype(np.float32) * 0.9 + 0.2
    corners = (c[:, :, None] + SGN[None, None] * s[:, :, None] / 2).astype(np.float32)     # every slot holds a box, valid or not
    ref = np.zeros((B, Cn, 8, 3), np.float32)
    labels = np.zeros((N, K), np.float32)
    cluster_ref = rng.standard_normal((N, K)).astype(np.float32)
    for b in range(B):
        for ci in range(Cn):
            o = int(rng.integers(K))
            ref[b, ci] = corners[b, o] + rng.normal(0, 0.08, (1, 3)).astype(np.float32)
            labels[b * Cn + ci, o] = 1
            if rng.random() < 0.5:
                cluster_ref[b * Cn + ci, o] += 4.0
    cat = rng.integers(0, 18, (B, Cn)).astype(np.int64)
    cat[rng.random((B, Cn)) < 0.3] = 17
    return dict(proposal_batch_mask=mask, proposal_bbox_batched=corners, cluster_ref=cluster_ref, cluster_labels=labels,
                ref_box_corner_label=ref, unique_multiple=rng.integers(0, 2, (B, Cn)).astype(np.int64), object_cat=cat,
                lang_scores=rng.standard_normal((N, L)).astype(np.float32), id=np.arange(B, dtype=np.int64) + 10 * K,
                chunk_ids=np.tile(np.arange(Cn, dtype=np.int64), (B, 1)))


def epoch_inputs(seed=23):
    """-> [repeat][batch] dicts of numpy arrays, the special rows planted"""
    rng = np.random.default_rng(seed)
    epoch = [[_batch(rng, *shape) for shape in rep] for rep in SHAPES]
    # repeat 0, batch 0 (B 2, C 4, K 63)
    d = epoch[0][0]
    d["proposal_batch_mask"][0, :] = 1
    d["proposal_batch_mask"][0, [2, 7, 30]] = 0
    d["cluster_ref"][0] = -np.abs(d["cluster_ref"][0]) - 0.01       # row 0: every score negative -> the masked maximum is the -0 at slot 2
    d["cluster_labels"][2] = 0                                      # row 2: an all-zero label row
    d["cluster_ref"][3, 20] = d["cluster_ref"][3, 41] = 9.0         # row 3: an exact tie between two valid slots
    d["proposal_batch_mask"][1, :] = 0                              # scene 1: an all-zero mask
    d["cluster_ref"][5, 62] = np.nan                                # row 5 (scene 1): a NaN score
    d["unique_multiple"][1, 2] = 2
    # repeat 0, batch 2 (B 1, C 4, K 64): the two exact IoUs and a NaN in a valid slot
    d = epoch[0][2]
    d["proposal_batch_mask"][0, [5, 6, 63]] = 1
    d["proposal_bbox_batched"][0, 5] = _cube([0, 0, 0], [1, 1, 0.5])
    d["proposal_bbox_batched"][0, 6] = _cube([0, 0, 0], [1, 1, 0.25])
    d["ref_box_corner_label"][0, 0] = d["ref_box_corner_label"][0, 1] = _cube([0, 0, 0], [1, 1, 1])
    d["cluster_ref"][0, 5] = 20.0                                   # row 0: IoU exactly 0.5
    d["cluster_ref"][1, 6] = 20.0                                   # row 1: IoU exactly 0.25
    d["cluster_ref"][2, 63] = np.nan
    d["cluster_ref"][2, 40] = np.nan                                # row 2: two NaNs, the lower one wins (when valid)
    d["proposal_batch_mask"][0, 40] = 1
    d["unique_multiple"][0, 3] = 2
    # repeat 1, batch 0 (B 2, C 4, K 65): the slot beyond the wave wins; the zero tie at an invalid slot that is not slot 0
    d = epoch[1][0]
    d["proposal_batch_mask"][0, :] = 1
    d["proposal_batch_mask"][0, [33, 64]] = 0
    d["cluster_ref"][0] = -np.abs(d["cluster_ref"][0]) - 0.01       # row 0: the masked maximum is the -0 at slot 33
    d["cluster_ref"][1, 64] = 30.0                                  # row 1: top is the invalid slot 64, pred_ref another
    d["cluster_ref"][2, 0] = d["cluster_ref"][2, 64] = 11.0         # row 2: a tie of slot 0 with the last slot
    d["unique_multiple"][1, 0] = 2
    # repeat 1, batch 1 (B 5, C 1, K 257): a tie across the lanes' strides, an all-zero mask, an all-zero label row
    d = epoch[1][1]
    d["proposal_batch_mask"][2, [70, 134, 199]] = 1
    d["cluster_ref"][2, [70, 134, 199]] = 12.0
    d["proposal_batch_mask"][3, :] = 0
    d["cluster_labels"][4] = 0
    return epoch


def tables_from_rows(masks, others, ref_acc, ious):
    """the integer cell counts of one repeat's per-row lists"""
    t = np.zeros((3, 2, 4), np.int64)
    for m, o, a, iou in zip(masks, others, ref_acc, ious):
        c = t[m if m in (0, 1) else 2, o]
        c += [1, int(a == 1), int(iou >= 0.25), int(iou >= 0.5)]
    return t


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    for name in ("trimesh", "plyfile", "omegaconf"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = object
    sys.modules["omegaconf"].OmegaConf = object
    from lib.grounding.eval_helper import get_eval
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        spec = importlib.util.spec_from_file_location("ref_scripts_eval", os.path.join(REF, "scripts", "eval.py"))
        ref_eval = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref_eval)
    finally:
        os.chdir(cwd)

    lists = {k: [] for k in ("ref_acc", "ious", "masks", "others", "lang_acc")}
    extra = {k: [] for k in ("best_ious", "pred_bboxes", "gt_bboxes")}
    for rep in epoch_inputs():
        row = {k: [] for k in lists}
        ext = {k: [] for k in extra}
        for batch in rep:
            d = {k: torch.from_numpy(v.copy()) for k, v in batch.items()}
            d = get_eval(d, grounding=True, use_lang_classifier=True)
            row["ref_acc"] += d["ref_acc"]                                     # scripts/eval.py:224-228
            row["ious"] += d["ref_iou"].cpu().numpy().tolist()
            row["masks"] += d["ref_multiple_mask"]
            row["others"] += d["ref_others_mask"]
            row["lang_acc"].append(d["lang_acc"].item())
            ext["best_ious"].append(d["best_ious"].numpy())
            ext["pred_bboxes"].append(d["pred_bboxes"].numpy())
            ext["gt_bboxes"].append(d["gt_bboxes"].numpy())
        for k in lists:
            lists[k].append(row[k])
        for k in extra:
            extra[k].append(np.concatenate(ext[k]))

    ious = np.array(lists["ious"], np.float32)
    exact = np.zeros(ious.shape, bool)
    exact[0, 13], exact[0, 14] = True, True                                    # repeat 0, batch 2, rows 0 and 1
    assert ious[0, 13] == np.float32(0.5) and ious[0, 14] == np.float32(0.25), ious[0, 13:15]
    for thr in (0.25, 0.5):
        near = np.abs(ious.astype(np.float64) - thr) <= 1e-5
        assert not (near & ~exact).any(), ("an IoU within 1e-5 of a threshold", thr, ious[near & ~exact])

    with tempfile.TemporaryDirectory() as root:
        with open(os.path.join(root, "scores.p"), "wb") as f:
            pickle.dump(lists, f)
        ns = types.SimpleNamespace
        cfg = ns(general=ns(manual_seed=123, root=root), eval=ns(repeat=1, force=False))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            ref_eval.eval_grounding(cfg, None, None, None)
    stats = np.full((3, 3), -1, np.int64)
    scores = np.full((3, 3, 3), np.nan, np.float64)
    lang_acc = None
    for line in buf.getvalue().splitlines():
        if line.startswith("language classification accuracy:"):
            lang_acc = float(line.split(":")[1])
        elif " | " in line:
            head, value = line.rsplit(":", 1)
            parts = [x.strip() for x in head.split("|")]
            if len(parts) == 2:
                stats[ROWS.index(parts[0]), COLS.index(parts[1])] = int(value)
            else:
                scores[ROWS.index(parts[0]), COLS.index(parts[1]), KEYS.index(parts[2])] = float(value)
    assert (stats >= 0).all() and np.isfinite(scores).all() and lang_acc is not None, buf.getvalue()

    tables = np.stack([tables_from_rows(lists["masks"][r], lists["others"][r], lists["ref_acc"][r], lists["ious"][r]) for r in range(len(SHAPES))])
    out = {"stats": stats, "scores": scores, "lang_acc": np.float64(lang_acc), "tables": tables,
           "lang_acc_batches": np.array(lists["lang_acc"], np.float64), "ref_acc": np.array(lists["ref_acc"], np.float32), "ious": ious,
           "masks": np.array(lists["masks"], np.int64), "others": np.array(lists["others"], np.int64), "exact": exact,
           "best_ious": np.stack(extra["best_ious"]).astype(np.float32), "pred_bboxes": np.stack(extra["pred_bboxes"]),
           "gt_bboxes": np.stack(extra["gt_bboxes"]), "numpy_version": np.array(np.__version__)}
    np.savez_compressed(os.path.join(HERE, "grounding_epoch_golden.npz"), **out)
    print({k: np.asarray(v).shape for k, v in out.items()})
    print(buf.getvalue())
    print(tables.reshape(len(SHAPES), 6, 4))


if __name__ == "__main__":
    main()
