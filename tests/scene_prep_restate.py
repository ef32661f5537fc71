"""Host restatement of the reference's per-scene preparation (lib/dataset/pipeline.py:141-187, :679-833 with
lib/utils/transform.py:elastic on scipy.ndimage / RegularGridInterpolator and lib/utils/pc.py:crop) in numpy, for scenes too large
for a golden file.  Draws come from `rng` in the reference's order (host noise)."""
import numpy as np
import scipy.interpolate
import scipy.ndimage

from d3net_amd import scene_prep as SP


def elastic(x, gran, mag, rng):
    blur = [np.ones(s).astype("float32") / 3 for s in ((3, 1, 1), (1, 3, 1), (1, 1, 3))]
    bb = np.abs(x).max(0).astype(np.int32) // gran + 3
    noise = [rng.randn(bb[0], bb[1], bb[2]).astype("float32") for _ in range(3)]
    for k in (0, 1, 2, 0, 1, 2):
        noise = [scipy.ndimage.convolve(n, blur[k], mode="constant", cval=0) for n in noise]
    ax = [np.linspace(-(b - 1) * gran, (b - 1) * gran, b) for b in bb]
    interp = [scipy.interpolate.RegularGridInterpolator(ax, n, bounds_error=0, fill_value=0) for n in noise]
    return x + np.hstack([i(x)[:, None] for i in interp]) * mag


def prepare(scene, cfg, mean_size_arr, rng, is_augment=True):
    d = cfg.data
    points = np.asarray(scene["points"], np.float32)
    feats = np.asarray(scene["feats"], np.float32)
    sem = np.asarray(scene["sem_labels"])
    ids = np.asarray(scene["instance_ids"]).copy()
    pa = np.matmul(points, SP.augment_matrix(rng, d.transform)) if is_augment else points.copy()
    p = pa * d.scale
    on = SP.elastic_enabled(cfg, is_augment)
    if on:
        for gran, mag in SP.elastic_params(d.scale):
            p = elastic(p, gran, mag, rng)
    p -= p.min(0)
    valid = np.ones(len(p), bool)
    if on:
        mpr = np.array([d.full_scale[1]] * 3)
        rngp = p.max(0) - p.min(0)
        pc_off = p.copy()
        while valid.sum() > d.max_num_point:
            off = np.clip(mpr - rngp + 0.001, None, 0) * rng.rand(3)
            pc_off = p + off
            valid = (pc_off.min(1) >= 0) * ((pc_off < mpr).sum(1) == 3)
            mpr[:2] -= 32
        p, pa, feats, sem = pc_off[valid], pa[valid], feats[valid], sem[valid]
        ids = ids[valid]
        j = 0
        while j < ids.max():
            if len(np.where(ids == j)[0]) == 0:
                ids[ids == ids.max()] = j
            j += 1
    R = d.max_num_instance
    uniq = np.unique(ids)
    info = np.zeros((len(p), 12), np.float32)
    npt, boxes = [], np.zeros((R, 6))
    cls, bid, lab = np.zeros(R), np.zeros(R), np.zeros(R)
    res = np.zeros((R, 3))
    gi, go = [], [0]
    for k, i_ in enumerate(uniq, -1):
        if i_ < 0:
            continue
        w = np.where(ids == i_)[0]
        x = pa[w]
        mn, mx, mean = x.min(0), x.max(0), x.mean(0)
        c = (mn + mx) / 2
        info[w, 0:3], info[w, 3:6], info[w, 6:9], info[w, 9:12] = mean, c, mn, mx
        npt.append(len(w))
        gi.append(np.stack([np.full(len(w), k), w], 1).astype(np.int32))
        go.append(go[-1] + len(w))
        if k >= 128:
            continue
        boxes[k, :3], boxes[k, 3:] = c, mx - mn
        s = sem[w][0]
        s = s - 2 if s >= 2 else 17
        cls[k], bid[k], lab[k] = s, i_, 1
        res[k] = boxes[k, 3:] - mean_size_arr[int(s)]
    sgn = np.array([[1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1], [1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1]], np.float64)
    out = dict(locs=pa.astype(np.float32), locs_scaled=p.astype(np.float32), feats=feats, sem_labels=sem.astype(np.int32),
               instance_ids=ids.astype(np.int32), num_instance=np.array(len(npt), np.int32), instance_info=info,
               instance_num_point=np.array(npt, np.int32), valid=valid,
               center_label=boxes[:, :3].astype(np.float32), sem_cls_label=cls.astype(np.int64),
               heading_class_label=np.zeros(R, np.int64), heading_residual_label=np.zeros(R, np.float32),
               size_class_label=cls.astype(np.int64), size_residual_label=res.astype(np.float32),
               gt_bbox_object_id=bid.astype(np.int64), gt_bbox_label=lab.astype(np.int64),
               gt_bbox=(sgn[None] * (boxes[:, None, 3:] / 2) + boxes[:, None, :3]).astype(np.float32))
    if d.requires_gt_mask:
        out["gt_proposals_idx"] = np.concatenate(gi, 0)
        out["gt_proposals_offset"] = np.array(go, np.int32)
    return out
