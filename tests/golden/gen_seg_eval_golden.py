#!/usr/bin/env python3
"""Generates tests/golden/seg_eval_golden.npz by RUNNING THE REFERENCE's own segmentation evaluators on files in its formats:
lib/evaluation/instance_segmentation.py (assign_instances_for_scene, evaluate_matches, compute_averages) and
lib/evaluation/semantic_segmentation.py (build_confusion_for_scene, get_semantic_iou).  Their imports need mesh I/O and a logger
this path never calls: `trimesh`, `plyfile` and `lib.utils.log` are registered as placeholders; the class tables the reference
sets from its config are set by hand; numpy 2's removed aliases (np.float / np.int / np.bool) are restored AFTER the imports
(before them they break numpy.ma).  Run where the reference is available; the tests rebuild the inputs from `seg_eval_inputs()`."""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

NYU20_CLASS_IDX = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]
INST = NYU20_CLASS_IDX[3:]
NO_PRED_CLASS, ABSENT_CLASS = 39, 36            # a class with GT but never predicted; a class with neither


def seg_eval_inputs(n_scenes=6, seed=7):
    """-> list of scenes: dict(gt_sem (N,) raw GT class ids, gt_inst (N,) 1-based ids (0 none), pred_sem (N,) raw predicted class
    ids, members [index arrays in pick order], classes, scores float32).  Reaches: GT instances under 100 points, void and
    wall/floor points inside predictions, duplicate predictions of one GT, wall/floor-class predictions, predictions under 100
    points, class ties in a GT instance's bincount, exactly tied 4-decimal scores, points in two predictions, an absent instance id."""
    rng = np.random.default_rng(seed)
    use = [c for c in INST if c != ABSENT_CLASS]
    scenes = []
    for s in range(n_scenes):
        N = int(rng.integers(2000, 20001))
        gt_sem = rng.choice([0, 1, 2], size=N, p=[0.2, 0.5, 0.3]).astype(np.int64)
        gt_inst = np.zeros(N, np.int64)
        perm = rng.permutation(N)
        n_inst = int(rng.integers(6, 13))
        cur, inst_pts, inst_cls = 0, {}, {}
        for k in range(1, n_inst + 1):
            if k == 3:
                continue                                 # an absent id
            size = int(rng.integers(30, 99)) if k % 4 == 0 else int(rng.integers(120, max(121, N // (n_inst + 3))))
            pts = perm[cur:cur + size]
            cur += size
            cls = int(rng.choice(use)) if k != 2 else NO_PRED_CLASS
            if k == n_inst:
                cls = int(rng.choice([1, 2]))            # a wall / floor instance: not an instance class
            gt_sem[pts] = cls
            noise = pts[rng.random(size) < 0.08]
            gt_sem[noise] = rng.choice([0, 1, 2, 5, 7], size=len(noise))
            if k == 1:                                   # exact bincount tie: the smaller class id wins
                other = cls + 1 if cls + 1 in INST else cls - 1
                gt_sem[pts] = cls
                gt_sem[pts[: size // 2]] = other
                if size % 2:
                    gt_sem[pts[-1]] = 0
            gt_inst[pts] = k
            inst_pts[k], inst_cls[k] = pts, cls
        bg = perm[cur:]
        pred_sem = np.where(rng.random(N) < 0.8, gt_sem, rng.choice([c for c in NYU20_CLASS_IDX[1:] if c != ABSENT_CLASS], size=N))
        pred_sem[pred_sem == 0] = 1
        members, classes, scores = [], [], []

        def add(m, c, sc):
            members.append(np.asarray(m, np.int64)); classes.append(int(c)); scores.append(np.float32(sc))

        for k, pts in inst_pts.items():
            cls = inst_cls[k]
            if cls == NO_PRED_CLASS:
                continue
            for r in range(int(rng.integers(1, 4))):     # duplicates of one GT share points
                take = pts[rng.random(len(pts)) < rng.uniform(0.45, 1.0)]
                extra = rng.choice(bg, size=int(rng.integers(0, max(1, len(pts) // 3))), replace=False)   # void / wall points
                m = rng.permutation(np.concatenate([take, extra]))
                c = cls if rng.random() < 0.85 else int(rng.choice(use))
                add(m, c, rng.random())
        add(rng.choice(bg, size=400, replace=False), 1, rng.random())                         # wall-class prediction
        add(rng.choice(bg, size=300, replace=False), int(rng.choice(use)), rng.random())      # mostly void: ignored or FP
        add(rng.choice(bg, size=60, replace=False), int(rng.choice(use)), rng.random())       # under 100 points
        small = [k for k in inst_pts if len(inst_pts[k]) < 100 and inst_cls[k] in use]
        if small:                                        # a prediction on a small GT instance (its points count as ignored)
            k = small[0]
            add(np.concatenate([inst_pts[k], rng.choice(bg, size=90, replace=False)]), inst_cls[k], rng.random())
        scores = np.array(scores, np.float32)
        scores[1] = scores[0]                            # exactly tied
        scores[3] = np.float32(round(float(scores[2]), 4) + 0.00002)   # tied after rounding to 4 decimals
        scores[2] = np.float32(round(float(scores[2]), 4) - 0.00002)
        if s == 0:
            scores[4] = np.float32(0.5)
        if s == 1:
            scores[0] = np.float32(0.5)                  # tied across scenes
        order = np.argsort(-scores, kind="stable")       # pick order: descending score
        scenes.append(dict(gt_sem=gt_sem, gt_inst=gt_inst, pred_sem=pred_sem.astype(np.int64),
                           members=[members[i] for i in order], classes=np.array(classes, np.int64)[order], scores=scores[order]))
    return scenes


def write_reference_files(scenes, root):
    """the reference's file formats: GT sem*1000+inst, semantic ids, instance list + 0/1 masks (model/pointgroup.py:603-625)"""
    gt_files, sem_files, inst_files = [], [], []
    for d in ("gt", "semantic", "instance/predicted_masks"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for s, sc in enumerate(scenes):
        name = "scene%04d_00" % s
        N = len(sc["gt_sem"])
        g = os.path.join(root, "gt", name + ".txt")
        np.savetxt(g, sc["gt_sem"] * 1000 + sc["gt_inst"], fmt="%d")
        p = os.path.join(root, "semantic", name + ".txt")
        np.savetxt(p, sc["pred_sem"], fmt="%d")
        f = os.path.join(root, "instance", name + ".txt")
        with open(f, "w") as fh:
            for c_id, (m, c, score) in enumerate(zip(sc["members"], sc["classes"], sc["scores"])):
                mask = np.zeros(N, np.int64)
                mask[m] = 1
                fh.write(f"predicted_masks/{name}_{c_id:03d}.txt {c} {score:.4f}\n")
                np.savetxt(os.path.join(root, "instance", "predicted_masks", f"{name}_{c_id:03d}.txt"), mask, fmt="%d")
        gt_files.append(g); sem_files.append(p); inst_files.append(f)
    return gt_files, sem_files, inst_files


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    for name in ("trimesh", "plyfile"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = object
    log = types.ModuleType("lib.utils.log"); log.Logger = object
    sys.modules["lib.utils.log"] = log
    import lib.evaluation.instance_segmentation as IS
    import lib.evaluation.semantic_segmentation as SS
    np.float, np.int, np.bool = float, int, bool
    names = ['unannotated', 'wall', 'floor', 'cabinet', 'bed', 'chair', 'sofa', 'table', 'door', 'window', 'bookshelf', 'picture',
             'counter', 'desk', 'curtain', 'refrigerator', 'shower curtain', 'toilet', 'sink', 'bathtub', 'otherfurniture']
    IS.CLASS_NAME, IS.CLASS_IDX = names[3:], np.array(NYU20_CLASS_IDX[3:])
    for n, i in zip(IS.CLASS_NAME, IS.CLASS_IDX):
        IS.NAME_TO_IDX[n], IS.IDX_TO_NAME[i] = i, n
    SS.CLASS_NAME, SS.CLASS_IDX = names[1:], np.array(NYU20_CLASS_IDX[1:])

    scenes = seg_eval_inputs()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        gt_files, sem_files, inst_files = write_reference_files(scenes, tmp)
        matches = {}
        for pf, gf in zip(inst_files, gt_files):
            gt2pred, pred2gt = IS.assign_instances_for_scene(pf, gf)
            matches[os.path.abspath(gf)] = {"gt": gt2pred, "pred": pred2gt}
        ap = IS.evaluate_matches(matches)
        avgs = IS.compute_averages(ap)
        confusion = np.zeros((40, 40), dtype=np.ulonglong)
        for pf, gf in zip(sem_files, gt_files):
            SS.build_confusion_for_scene(pf, gf, confusion)
        ious = [SS.get_semantic_iou(c, confusion) for c in SS.CLASS_IDX]
    out["ap"] = ap
    out["all_ap"], out["all_ap_50"], out["all_ap_25"] = (np.float64(avgs[k]) for k in ("all_ap", "all_ap_50%", "all_ap_25%"))
    out["class_ap"] = np.array([[avgs["classes"][n][k] for k in ("ap", "ap50%", "ap25%")] for n in IS.CLASS_NAME], np.float64)
    out["confusion"] = confusion.astype(np.int64)
    out["iou"] = np.array([np.nan if isinstance(r, float) else r[0] for r in ious], np.float64)
    out["iou_tp_denom"] = np.array([[-1, -1] if isinstance(r, float) else [int(r[1]), int(r[2])] for r in ious], np.int64)
    np.savez_compressed(os.path.join(HERE, "seg_eval_golden.npz"), **out)
    print("wrote seg_eval_golden.npz: all_ap %.6f ap50 %.6f ap25 %.6f, classes with NaN AP: %d, NaN IoU: %d" %
          (out["all_ap"], out["all_ap_50"], out["all_ap_25"], int(np.isnan(out["class_ap"][:, 0]).sum()), int(np.isnan(out["iou"]).sum())))


if __name__ == "__main__":
    main()
