#!/usr/bin/env python3
"""Generates tests/golden/scene_prep_golden.npz by RUNNING THE REFERENCE's own scene preparation: PipelineDataset._augment,
_croppedInstanceIds, _getInstanceInfo and _generate_gt_clusters (lib/dataset/pipeline.py:679-833) on a stub `self`, plus
lib/utils/transform.py:elastic, lib/utils/pc.py:crop and lib/utils/bbox.py:get_3d_box_batch, in the order of __getitem__ (:141-187),
under np.random.seed(seed).  The pipeline module's imports that this path never calls (h5py, MinkowskiEngine(.utils),
lib.pointgroup_ops.functions, plyfile, trimesh, matplotlib) are registered as placeholders.  Also stores the reference's
scannet_reference_means.npz (18,3) used for the size residuals.  Run where the reference is available."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _import_reference():
    for name in ("h5py", "plyfile", "trimesh", "matplotlib", "matplotlib.pyplot", "lib.pointgroup_ops",
                 "lib.pointgroup_ops.functions"):
        _stub(name, PlyData=None, PlyElement=None, pointgroup_ops=None)
    _stub("MinkowskiEngine")
    _stub("MinkowskiEngine.utils", batched_coordinates=None)
    sys.path.insert(0, REF)
    from lib.dataset import pipeline
    from lib.utils import transform, pc, bbox
    return pipeline, transform, pc, bbox


def ns(**kw):
    return types.SimpleNamespace(**kw)


def make_cfg(scale=50, full_scale=512, max_num_point=250000, max_num_instance=128, gt_mask=False, captioning=False):
    return ns(data=ns(scale=scale, full_scale=[128, full_scale], max_num_point=max_num_point, max_num_instance=max_num_instance,
                      requires_gt_mask=gt_mask, requires_bbox=True, transform=ns(jitter=True, flip=True, rot=True)),
              model=ns(no_detection=False, no_captioning=not captioning, no_grounding=True))


def make_scene(seed, n=3000, n_inst=9, extent=(8.0, 6.0, 2.5), unlabelled=True, far_instance=True):
    """points in metres; instances are blobs, the last one in the far +x+y corner (a crop can remove it whole); ids skip a value"""
    r = np.random.RandomState(seed)
    pts = (r.rand(n, 3) * np.array(extent)).astype(np.float32)
    ids = np.full(n, -1, np.int64)
    sem = r.randint(0, 20, size=n).astype(np.int64)
    sem[r.rand(n) < 0.05] = -1
    centers = r.rand(n_inst, 3) * np.array(extent) * 0.8 + 0.1 * np.array(extent)
    if far_instance:
        centers[-1] = np.array(extent) * np.array([0.97, 0.97, 0.5])
    d = np.linalg.norm(pts[:, None, :] - centers[None], axis=2)
    near = d.argmin(1)
    lab = d.min(1) < (0.9 if unlabelled else 1e9)
    id_values = [k if k < 3 else k + 1 for k in range(n_inst)]          # id 3 absent
    ids[lab] = np.array(id_values)[near[lab]]
    feats = r.rand(n, 3).astype(np.float32) * 2 - 1
    return dict(points=pts, feats=feats, sem_labels=sem, instance_ids=ids)


class Stub:
    """the attributes of `self` the four PipelineDataset methods read"""

    def __init__(self, cfg, mean_size_arr):
        self.cfg = cfg
        self.requires_bbox = True
        self.DC = ns(mean_size_arr=mean_size_arr)


def run_reference(P, T, PC, B, scene, cfg, mean_size_arr, seed, is_augment):
    """pipeline.py:141-187 + :236-247 for one scene under np.random.seed(seed); records the intermediate values tests compare"""
    self = Stub(cfg, mean_size_arr)
    D = P.PipelineDataset
    rec = {}
    np.random.seed(seed)
    points = scene["points"]
    feats, instance_ids, sem_labels = scene["feats"], scene["instance_ids"].copy(), scene["sem_labels"]
    if is_augment:
        points_augment, _, m = D._augment(self, points, return_mat=True)
    else:
        points_augment, m = points.copy(), np.eye(3)
    rec["M"] = m
    points = points_augment * cfg.data.scale
    elastic_on = is_augment and (not cfg.model.no_detection and cfg.model.no_captioning and cfg.model.no_grounding)
    bbs = []
    if elastic_on:
        for gran, mag in ((6 * cfg.data.scale // 50, 40 * cfg.data.scale / 50), (20 * cfg.data.scale // 50, 160 * cfg.data.scale / 50)):
            bbs.append(np.abs(points).max(0).astype(np.int32) // gran + 3)
            points = T.elastic(points, gran, mag)
    rec["bb"] = np.array(bbs, np.int64).reshape(-1, 3)
    points -= points.min(0)
    rec["precrop"] = points.copy()
    valid = np.ones(len(points), bool)
    iters = 0
    if elastic_on:
        calls = []
        orig_rand = np.random.rand

        def counting_rand(*a):
            calls.append(a)
            return orig_rand(*a)
        PC.np.random.rand = counting_rand
        try:
            points, valid = PC.crop(points, cfg.data.max_num_point, cfg.data.full_scale[1])
        finally:
            PC.np.random.rand = orig_rand
        iters = len(calls)
        rng_final = np.array([cfg.data.full_scale[1] - 32 * max(iters - 1, 0)] * 2 + [cfg.data.full_scale[1]], np.float64)
        nz = np.abs(points[points != 0])                 # exact zeros: the minimum point where the offset is 0
        rec["crop_margin"] = min(nz.min(), np.abs(points - rng_final).min()) if iters else np.inf
        points = points[valid]
        points_augment = points_augment[valid]
        feats = feats[valid]
        sem_labels = sem_labels[valid]
        instance_ids = D._croppedInstanceIds(self, instance_ids, valid)
    rec["valid"], rec["crop_iters"] = valid, np.int64(iters)
    (num_instance, instance_info, instance_num_point, instance_bboxes, instance_bboxes_semcls, instance_bbox_ids,
     angle_classes, angle_residuals, size_classes, size_residuals, bbox_label) = D._getInstanceInfo(self, points_augment, instance_ids,
                                                                                                      sem_labels)
    if cfg.data.requires_gt_mask:
        gi, go, _, _ = D._generate_gt_clusters(self, points, instance_ids)
        rec["gt_proposals_idx"], rec["gt_proposals_offset"] = gi, go
    rec["next_draw"] = np.random.rand()                  # the draw after the scene: same stream position
    rec.update(locs=points_augment.astype(np.float32), locs_scaled=points.astype(np.float32), feats=feats.astype(np.float32),
               sem_labels=sem_labels.astype(np.int32), instance_ids=instance_ids.astype(np.int32),
               num_instance=np.array(num_instance).astype(np.int32), instance_info=instance_info.astype(np.float32),
               instance_num_point=np.array(instance_num_point).astype(np.int32),
               center_label=instance_bboxes.astype(np.float32)[:, 0:3], sem_cls_label=instance_bboxes_semcls.astype(np.int64),
               heading_class_label=angle_classes.astype(np.int64), heading_residual_label=angle_residuals.astype(np.float32),
               size_class_label=size_classes.astype(np.int64), size_residual_label=size_residuals.astype(np.float32),
               gt_bbox_object_id=instance_bbox_ids.astype(np.int64), gt_bbox_label=bbox_label.astype(np.int64),
               gt_bbox=B.get_3d_box_batch(instance_bboxes[:, 0:3], instance_bboxes[:, 3:6], angle_classes).astype(np.float32))
    return rec


# name -> (scene kwargs, cfg kwargs, is_augment)
CASES = {
    "crop": (dict(seed=11), dict(max_num_point=1500, full_scale=512), True),
    "nolabel": (dict(seed=12, unlabelled=False, n=2500, n_inst=6), dict(max_num_point=1800, full_scale=512), True),
    "gtmask": (dict(seed=13), dict(max_num_point=2000, full_scale=512, gt_mask=True), True),
    "val": (dict(seed=14, far_instance=False), dict(gt_mask=True), False),
    "caption": (dict(seed=15), dict(captioning=True, gt_mask=True), True),
}


def check_margins(rec, cfg, elastic_on):
    """no point within 1e-9 of a crop boundary or of an integer in locs_scaled (the device's fp64 may differ in the last bits)"""
    v = rec["locs_scaled"].astype(np.float64)
    v = v[v != 0]                                        # the minimum point is exactly 0 in any arithmetic
    assert np.abs(v - np.round(v)).min() > 1e-9, "a point on an integer of locs_scaled"
    if elastic_on and rec["crop_iters"]:
        assert rec["crop_margin"] > 1e-9, "a point on a crop boundary"


def main():
    P, T, PC, B = _import_reference()
    mean_size_arr = np.load(os.path.join(REF, "data/scannet/meta_data/scannet_reference_means.npz"))["arr_0"]
    out = {"mean_size_arr": mean_size_arr, "cases": np.array(list(CASES))}
    for name, (skw, ckw, aug) in CASES.items():
        scene = make_scene(**skw)
        cfg = make_cfg(**ckw)
        seed = 100 + skw["seed"]
        rec = run_reference(P, T, PC, B, scene, cfg, mean_size_arr, seed, aug)
        elastic_on = aug and not ckw.get("captioning", False)
        check_margins(rec, cfg, elastic_on)
        if name == "crop":
            assert rec["crop_iters"] >= 2, rec["crop_iters"]
            kept = set(np.unique(scene["instance_ids"][rec["valid"]])) - {-1}
            assert len(kept) < len(set(np.unique(scene["instance_ids"])) - {-1}), "crop removed no whole instance"
        if name == "nolabel":
            assert (rec["instance_ids"] >= 0).all()
        for k, v in scene.items():
            out["%s/in_%s" % (name, k)] = v
        for k, v in rec.items():
            out["%s/%s" % (name, k)] = np.asarray(v)
        out["%s/seed" % name] = np.int64(seed)
        out["%s/cfg" % name] = np.array([ckw.get("max_num_point", 250000), ckw.get("full_scale", 512), int(ckw.get("gt_mask", False)),
                                         int(ckw.get("captioning", False)), int(aug)], np.int64)
    np.savez_compressed(os.path.join(HERE, "scene_prep_golden.npz"), **out)
    print("wrote scene_prep_golden.npz:", {n: int(out[n + "/num_instance"]) for n in CASES},
          "crop iterations", {n: int(out[n + "/crop_iters"]) for n in CASES})


if __name__ == "__main__":
    main()
