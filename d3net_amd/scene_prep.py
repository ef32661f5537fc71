"""PointGroup scene preparation on the device: the per-scene half of the reference's `PipelineDataset.__getitem__`
(lib/dataset/pipeline.py:141-187) -- augmentation (:679-697), two elastic distortions (lib/utils/transform.py:elastic), offset,
crop (lib/utils/pc.py:crop), instance relabelling (:699-709), instance statistics and box labels (:711-772), GT proposal lists
(:804-833) -- followed by the batch stacking of `collate.sparse_collate_fn`, so `prepare_batch` hands `PointGroup.feed` a
device-resident batch without the host numpy / scipy pass.

The bulk work is HIP (csrc/scene_prep.hip).  The host keeps the reference's data-dependent control flow, and that is where it
synchronises with the device, per scene:
  * the |s| maxima that size each elastic's noise grids (one read per elastic, augmented detector path only);
  * the coordinate extent and instance-id range after the elastic (one read: crop range, workspace size);
  * each crop iteration's kept-point count (the reference's `while` loop);
  * the instance count and labelled-point count (output shapes).

`prepare_batch_store` (no elastic, no crop: no read-back at all) and `prepare_batch_store_elastic` (the augmented detector-only mode:
one read-back per batch) build the same batches straight from a resident `dataset.SceneStore` instead.

Random draws come from `rng` (a numpy RandomState, or None for numpy's global state as the reference's loader uses) in the
reference's order: randn(3,3) jitter, randint(0,2) flip, rand() rotation, then the noise grids, then one rand(3) per crop
iteration.  noise="host" draws the six noise grids with rng.randn in the reference's order and sizes, which reproduces the
reference wherever fp64 allows.  noise="device" instead takes ONE rng.randint draw in the grids' place and fills the grids on the
device (Philox4x32-10 + Box-Muller): the training path then pays no host RNG for the grids, but the host RNG stream -- and so
every later draw -- differs from the reference's.
"""
import collections
import ctypes as C
import threading

import numpy as np
import torch

from . import _lib, pointgroup_ops
from ._call import _on, _ptr, _stream, _workspace, call

_NOISE_MODES = ("host", "device")


# ------------------------------------------------------------------------------------------------ host control flow
def augment_matrix(rng, tcfg):
    """`_augment`'s matrix (pipeline.py:679-697, transform.py jitter / flip / rotz) with the same draws in the same order."""
    m = np.eye(3)
    if tcfg.jitter:
        m *= np.eye(3) + rng.randn(3, 3) * 0.1
    if tcfg.flip:
        f = np.eye(3)
        f[0][0] *= rng.randint(0, 2) * 2 - 1
        m *= f
    if tcfg.rot:
        t = rng.rand() * 2 * np.pi
        c, s = np.cos(t), np.sin(t)
        m = np.matmul(m, np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]))
    return m


def elastic_params(scale):
    """(gran, mag) of the two elastic calls (pipeline.py:152-153)"""
    return [(6 * scale // 50, 40 * scale / 50), (20 * scale // 50, 160 * scale / 50)]


def grid_shape(absmax, gran):
    """transform.py:elastic `bb = np.abs(x).max(0).astype(np.int32)//gran + 3`"""
    return np.asarray(absmax, dtype=np.float64).astype(np.int32) // gran + 3


def grid_axes(bb, gran):
    return [np.linspace(-(b - 1) * gran, (b - 1) * gran, b) for b in bb]


def host_noise(rng, bb):
    """the reference's three noise grids of one elastic call, in its draw order"""
    return [rng.randn(bb[0], bb[1], bb[2]).astype("float32") for _ in range(3)]


def crop_loop(count, n, pc_range, max_num_point, scale, rng):
    """pc.py:crop's loop with the kept-point count of a candidate offset supplied by `count(offset, max_pc_range)`.
    -> (offset or None when the loop never ran, number of kept points)"""
    max_pc_range = np.array([scale] * 3)
    valid, offset = n, None
    while valid > max_num_point:
        offset = np.clip(max_pc_range - pc_range + 0.001, None, 0) * rng.rand(3)
        valid = count(offset, max_pc_range.astype(np.float64))
        max_pc_range[:2] -= 32
    return offset, valid


def crop_max_iters(full_scale):
    """The hard bound of `crop_loop`'s iterations: once max_pc_range[:2] = full_scale - 32 j is <= 0 no point passes
    `0 <= p < max_pc_range`, the count is 0 and the loop ends; that happens at j = ceil(full_scale / 32), the (j + 1)-th iteration."""
    return int(-(-float(full_scale) // 32)) + 1


_NOISE_ABS_MAX = 6.67      # csrc/scene_prep.h:sp_noise_quad: |z| <= sqrt(-2 ln 2^-32) = 6.66; blur and interpolation are convex


def elastic_grid_bound(absmax_xyz, m, scale, call, slack=1):
    """An upper bound, from host data alone, of the noise-grid shape `grid_shape(|s|.max(0), gran)` of elastic call 0 or 1 for
    s = (xyz @ m) * scale: |s_d| <= scale * sum_j |m[j, d]| * absmax_xyz[j]; call 1 adds 6.67 * mag_0, the most the first
    distortion can move a point.  `slack` cells per axis cover the rounding of the float64 products (a relative 1e-15) and of
    the noise kernel's float32 arithmetic.  -> (3,) int64"""
    params = elastic_params(scale)
    gran = params[call][0]
    b = float(scale) * (np.abs(np.asarray(m, np.float64)).T @ np.asarray(absmax_xyz, np.float64))
    if call == 1:
        b = b + _NOISE_ABS_MAX * params[0][1]
    return (np.floor(b).astype(np.int64) // int(gran) + 3 + int(slack)).astype(np.int64)


def relabel_table(present):
    """`_croppedInstanceIds` (pipeline.py:699-709) as a map over id values, from the presence table of ids 0..V-1; the same walk
    as csrc/scene_prep.hip's sp_relabel_map_kernel.  -> val_of (V,) int: points with id v end with id val_of[v]."""
    present = np.asarray(present, dtype=bool)
    V = len(present)
    val_of = np.arange(V)
    orig_at = np.where(present, np.arange(V), -1)
    cur = int(np.nonzero(present)[0].max()) if present.any() else -1
    j = 0
    while j < cur:
        if orig_at[j] == -1:
            o = orig_at[cur]
            orig_at[j], val_of[o], orig_at[cur] = o, j, -1
            while cur > j and orig_at[cur] == -1:
                cur -= 1
        j += 1
    return val_of


def _decode(enc):
    """order-preserving u64 encodings of csrc/scene_prep.hip -> float64"""
    e = np.asarray(enc, dtype=np.uint64)
    neg = (e >> np.uint64(63)) != 0
    b = np.where(neg, e & np.uint64(0x7FFFFFFFFFFFFFFF), ~e)
    return b.view(np.float64)


def _range_error(what):
    _lib.check(-2, what)


def elastic_enabled(cfg, is_augment):
    """pipeline.py:150 / :158: elastic distortion and crop run on the augmented detector-only path"""
    m = cfg.model
    return bool(is_augment and (not m.no_detection and m.no_captioning and m.no_grounding))


# ------------------------------------------------------------------------------------------------ one scene
def _dev_tensor(x, dtype, device):
    t = torch.as_tensor(x) if isinstance(x, np.ndarray) else x
    return t.to(device=device, dtype=dtype).contiguous()


def prepare_scene(scene, cfg, mean_size_arr, rng=None, is_augment=True, noise="device", device=None):
    """One raw scene -> the per-scene sample dict of the reference's `__getitem__` (point keys, box labels, GT proposal lists
    when cfg.data.requires_gt_mask), as device tensors (num_instance a python int).  See the module docstring for the draws."""
    if noise not in _NOISE_MODES:
        raise ValueError("noise must be one of %s" % (_NOISE_MODES,))
    rng = np.random if rng is None else rng
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    L = _lib.lib()
    st = _stream()
    d = cfg.data
    scale, R = d.scale, int(d.max_num_instance)
    xyz = _dev_tensor(scene["points"], torch.float32, device)
    n = xyz.shape[0]
    feats = _dev_tensor(scene["feats"], torch.float32, device).reshape(n, -1)
    sem = _dev_tensor(scene["sem_labels"], torch.int32, device)
    ids = _dev_tensor(scene["instance_ids"], torch.int32, device)
    ms = _dev_tensor(np.asarray(mean_size_arr, dtype=np.float64), torch.float64, device)
    fp32 = 0 if is_augment else 1
    elastic = elastic_enabled(cfg, is_augment)

    y = torch.empty((n, 3), dtype=torch.float64, device=device)
    s = torch.empty((n, 3), dtype=torch.float64, device=device)
    stats = torch.empty(12, dtype=torch.int64, device=device)
    m = augment_matrix(rng, d.transform) if is_augment else np.eye(3)
    mh = np.ascontiguousarray(m, dtype=np.float64)
    call("scene_transform", _ptr(xyz), n, mh.ctypes.data_as(C.c_void_p), float(scale), fp32, _ptr(y), _ptr(s), st)

    if elastic:
        seed = None if noise == "host" else int(rng.randint(0, 2 ** 31 - 1))
        for e, (gran, mag) in enumerate(elastic_params(scale)):
            call("scene_reduce", _ptr(s), None, n, _ptr(stats), st)
            bb = grid_shape(_decode(stats[0:3].cpu().numpy()), gran)             # sync: grid sizes
            X, Y, Z = (int(b) for b in bb)
            nbytes = L.d3_scene_elastic_ws_bytes(X, Y, Z)
            if nbytes == 0:
                _range_error("scene_prep: noise grid %dx%dx%d" % (X, Y, Z))
            if noise == "host":
                grids = torch.from_numpy(np.stack(host_noise(rng, bb))).to(device)
            else:
                grids = torch.empty((3, X, Y, Z), dtype=torch.float32, device=device)
                call("scene_noise", _ptr(grids), 3 * X * Y * Z, (seed << 1) | e, st)
            axes = torch.from_numpy(np.concatenate(grid_axes(bb, gran))).to(device)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
            call("scene_elastic", _ptr(s), n, _ptr(grids), _ptr(axes), X, Y, Z, float(mag), _ptr(ws), nbytes, st)

    call("scene_reduce", _ptr(s), _ptr(ids), n, _ptr(stats), st)
    sh = stats.cpu().numpy().view(np.uint64)                                         # sync: extent, id range
    mn, mx = _decode(sh[3:6]), _decode(sh[6:9])
    id_lo, id_hi = (int(v) - 2 ** 31 for v in sh[9:11]) if n else (-1, -1)
    if id_lo < -1:
        _range_error("scene_prep: instance id %d < -1" % id_lo)
    nbytes = L.d3_scene_ws_bytes(n, id_hi)
    if nbytes == 0:
        _range_error("scene_prep: %d points / instance id %d" % (n, id_hi))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    call("scene_offset", _ptr(s), n, _ptr(stats), fp32, st)

    flags, off, keep = None, None, n
    if elastic:
        flags_t = torch.empty(n, dtype=torch.int32, device=device)
        cnt = torch.empty(1, dtype=torch.int32, device=device)

        def count(offset, rng_):
            o = np.ascontiguousarray(offset, dtype=np.float64)
            r = np.ascontiguousarray(rng_, dtype=np.float64)
            call("scene_crop_count", _ptr(s), n, o.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), _ptr(flags_t), _ptr(cnt), st)
            return int(cnt.item())                                               # sync: one per crop iteration

        off, keep = crop_loop(count, n, (mx - mn) - 0.0, d.max_num_point, d.full_scale[1], rng)
        if off is not None:
            flags = flags_t
            off = np.ascontiguousarray(off, dtype=np.float64)

    Cf = feats.shape[1]
    y2 = torch.empty((keep, 3), dtype=torch.float64, device=device)
    locs = torch.empty((keep, 3), dtype=torch.float32, device=device)
    locs_scaled = torch.empty((keep, 3), dtype=torch.float32, device=device)
    feats2 = torch.empty((keep, Cf), dtype=torch.float32, device=device)
    sem2 = torch.empty(keep, dtype=torch.int32, device=device)
    ids2 = torch.empty(keep, dtype=torch.int32, device=device)
    call("scene_emit", _ptr(y), _ptr(s), _ptr(feats), Cf, _ptr(sem), _ptr(ids), n, _ptr(flags),
         off.ctypes.data_as(C.c_void_p) if off is not None else None, fp32,
         _ptr(y2), _ptr(locs), _ptr(locs_scaled), _ptr(feats2), _ptr(sem2), _ptr(ids2), _ptr(ws), nbytes, st)
    if elastic:
        call("scene_relabel", _ptr(ids2), keep, id_hi, _ptr(ws), nbytes, st)

    V = max(id_hi, 0) + 1
    info = torch.empty((keep, 12), dtype=torch.float32, device=device)
    npt = torch.zeros(V, dtype=torch.int32, device=device)
    gt_idx = torch.empty((max(keep, 1), 2), dtype=torch.int32, device=device)
    gt_off = torch.zeros(V + 1, dtype=torch.int32, device=device)
    boxes = torch.zeros((R, 36), dtype=torch.float64, device=device)
    counts = torch.empty(4, dtype=torch.int32, device=device)
    call("scene_instances", _ptr(y2), _ptr(ids2), _ptr(sem2), keep, id_hi, fp32, R, _ptr(ms), _ptr(info), _ptr(npt),
         _ptr(gt_idx), _ptr(gt_off), _ptr(boxes), _ptr(counts), _ptr(ws), nbytes, st)
    K, Lp, _, _ = (int(v) for v in counts.cpu())                                    # sync: output shapes

    out = {"locs": locs, "locs_scaled": locs_scaled, "feats": feats2, "sem_labels": sem2, "instance_ids": ids2,
           "num_instance": K, "instance_info": info, "instance_num_point": npt[:K]}
    if d.requires_gt_mask:
        out["gt_proposals_idx"] = gt_idx[:Lp]
        out["gt_proposals_offset"] = gt_off[:K + 1]
    zeros = torch.zeros(R, dtype=torch.int64, device=device)
    out.update({
        "center_label": boxes[:, 0:3].float(),
        "sem_cls_label": boxes[:, 6].long(),
        "heading_class_label": zeros,
        "heading_residual_label": torch.zeros(R, dtype=torch.float32, device=device),
        "size_class_label": boxes[:, 6].long(),
        "size_residual_label": boxes[:, 9:12].float(),
        "gt_bbox_object_id": boxes[:, 7].long(),
        "gt_bbox_label": boxes[:, 8].long(),
        "gt_bbox": boxes[:, 12:36].reshape(R, 8, 3).float(),
    })
    return out


# ------------------------------------------------------------------------------------------------ the batch's output tensors
_Key = collections.namedtuple("_Key", "name dtype tail extent scene_dtype scene_tail gt")
_f32, _i32, _i64 = torch.float32, torch.int32, torch.int64


def _key(name, dtype, tail, extent, scene_dtype=None, scene_tail=None, gt=False):
    return _Key(name, dtype, tail, extent, dtype if scene_dtype is None else scene_dtype, tail if scene_tail is None else scene_tail, gt)


# The 20 tensors every labelled batch kernel writes, in the C ABI's order (`BpOut`, csrc/scene_prep.h; the `out_host` pointer
# array of d3_collate_scenes / d3_batch_prepare / d3_batch_elastic).  Per key: the batch dtype, the trailing shape ("C" the
# feature columns) and the leading extent -- "points", "instances", "instances+1", "entries" (GT proposal entries), "B+1" or "B,R"
# -- then what a per-scene sample of `prepare_scene` holds where it differs (32-bit labels and a three-column float locs_scaled:
# the kernels widen them and add the batch index), and whether the key exists only with data.requires_gt_mask (slot 0 otherwise).
_BATCH_KEYS = (
    _key("locs", _f32, (3,), "points"),
    _key("locs_scaled", _i64, (4,), "points", _f32, (3,)),
    _key("feats", _f32, ("C",), "points"),
    _key("sem_labels", _i64, (), "points", _i32),
    _key("instance_ids", _i64, (), "points", _i32),
    _key("instance_info", _f32, (12,), "points"),
    _key("instance_num_point", _i32, (), "instances"),
    _key("gt_proposals_idx", _i32, (2,), "entries", gt=True),
    _key("gt_proposals_offset", _i32, (), "instances+1", gt=True),
    _key("batch_offsets", _i32, (), "B+1"),
    _key("instance_offsets", _i32, (), "B+1"),
    _key("center_label", _f32, (3,), "B,R"),
    _key("sem_cls_label", _i64, (), "B,R"),
    _key("heading_class_label", _i64, (), "B,R"),
    _key("heading_residual_label", _f32, (), "B,R"),
    _key("size_class_label", _i64, (), "B,R"),
    _key("size_residual_label", _f32, (3,), "B,R"),
    _key("gt_bbox_object_id", _i64, (), "B,R"),
    _key("gt_bbox_label", _i64, (), "B,R"),
    _key("gt_bbox", _f32, (8, 3), "B,R"),
)
_SCENE_KEYS = tuple(k for k in _BATCH_KEYS if k.extent != "B+1")       # a per-scene sample's tensors: d3_collate_scenes' pointer columns
_BOX_KEYS = tuple(k.name for k in _BATCH_KEYS if k.extent == "B,R")     # the stacked box labels


def _shape(lead, tail, Cf):
    return lead + tuple(Cf if t == "C" else t for t in tail)


def _alloc_batch(device, B, R, Cf, has_gt, points, instances, entries):
    """The labelled batch's uninitialised output tensors for the given extents (the elastic path passes upper bounds and cuts
    afterwards) -> (data dict in `_BATCH_KEYS` order, the (20,) uint64 pointer array of the C ABI).  Without has_gt the GT
    proposal keys are absent and their pointer slots 0."""
    lead = {"points": (points,), "instances": (instances,), "instances+1": (instances + 1,), "entries": (entries,), "B+1": (B + 1,),
            "B,R": (B, R)}
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
    data = {k.name: new(_shape(lead[k.extent], k.tail, Cf), k.dtype) for k in _BATCH_KEYS if has_gt or not k.gt}
    return data, np.array([data[k.name].data_ptr() if k.name in data else 0 for k in _BATCH_KEYS], np.uint64)


_TABLE_RING = 4
_rings = {}


def _pinned(tag, nbytes, device):
    """A pinned host buffer of at least `nbytes` with its event, handed out round-robin from a ring of `_TABLE_RING` per (tag,
    device, host thread, stream), like the workspace.  The caller records the event behind the asynchronous copy that reads or
    fills the buffer; an entry comes round again only after that copy has run (the wait happens only when the whole ring is
    still in flight: the host may run several batches ahead of the device).  -> (uint8 tensor, event)"""
    key = (tag, device.index, threading.get_ident(), _stream().value or 0)
    ring = _rings.setdefault(key, {"next": 0, "ents": [None] * _TABLE_RING})
    k = ring["next"]
    ring["next"] = (k + 1) % _TABLE_RING
    ent = ring["ents"][k]
    if ent is None or ent[0].numel() < nbytes:
        ent = ring["ents"][k] = (torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8).pin_memory(), torch.cuda.Event())
    elif not ent[1].query():
        ent[1].synchronize()
    return ent


def _store_device(store, device, who):
    """the device of a resident store; a pinned-host store, or a `device` that names another card, is a ValueError"""
    dev = store.points.device
    if dev.type != "cuda":
        raise ValueError("%s: the store is pinned host memory; this path serves the resident store only" % who)
    if device is not None and torch.device(device).type != "cpu" and torch.device(device).index not in (None, dev.index):
        raise ValueError("%s: the store is on %s, not on %s" % (who, dev, device))
    return dev


def _mean_sizes_on(mean_size_arr, dev, who):
    """the (18,3) mean-size table as a float64 tensor on `dev`; nothing is uploaded when it already is one"""
    ms = mean_size_arr if torch.is_tensor(mean_size_arr) and mean_size_arr.device == dev and mean_size_arr.dtype == torch.float64 \
        else _dev_tensor(np.asarray(mean_size_arr, dtype=np.float64), torch.float64, dev)
    if ms.numel() < 54:
        raise ValueError("%s: mean_size_arr has %d values, 18 x 3 expected" % (who, ms.numel()))
    return ms


def collate_scenes(samples, device, mode=4):
    """`sparse_collate_fn`'s stacking (collate.py) over per-scene dicts that are already on the device"""
    data = {k: torch.stack([smp[k] for smp in samples], 0) for k in _BOX_KEYS}
    locs, locs_scaled, feats, sem, ids, info, npt, gt_idx, gt_off = [], [], [], [], [], [], [], [], []
    batch_offsets, instance_offsets = [0], [0]
    total_inst = total_pts = 0
    for i, b in enumerate(samples):
        n = b["locs_scaled"].shape[0]
        locs.append(b["locs"])
        locs_scaled.append(torch.cat([torch.full((n, 1), i, dtype=torch.int64, device=device), b["locs_scaled"].long()], 1))
        feats.append(b["feats"])
        batch_offsets.append(batch_offsets[-1] + n)
        if "gt_proposals_idx" in b:
            gi = b["gt_proposals_idx"].clone()
            gi[:, 0] += total_inst
            gi[:, 1] += total_pts
            gt_idx.append(gi)
            go = b["gt_proposals_offset"]
            gt_off.append(go + gt_off[-1][-1] if gt_off else go)
            if len(gt_off) > 1:
                gt_off[-1] = gt_off[-1][1:]
        ii = b["instance_ids"]
        ids.append(torch.where(ii != -1, ii + total_inst, ii))
        total_inst += b["num_instance"]
        total_pts += n
        sem.append(b["sem_labels"]); info.append(b["instance_info"]); npt.append(b["instance_num_point"])
        instance_offsets.append(instance_offsets[-1] + b["num_instance"])
    data["locs"] = torch.cat(locs, 0)
    data["locs_scaled"] = torch.cat(locs_scaled, 0)
    data["feats"] = torch.cat(feats, 0)
    data["batch_offsets"] = torch.tensor(batch_offsets, dtype=torch.int32, device=device)
    data["sem_labels"] = torch.cat(sem, 0).long()
    data["instance_ids"] = torch.cat(ids, 0).long()
    data["instance_info"] = torch.cat(info, 0)
    data["instance_num_point"] = torch.cat(npt, 0)
    data["instance_offsets"] = torch.tensor(instance_offsets, dtype=torch.int32, device=device)
    if gt_idx:
        data["gt_proposals_idx"] = torch.cat(gt_idx, 0)
        data["gt_proposals_offset"] = torch.cat(gt_off, 0)
    data["voxel_locs"], data["p2v_map"], data["v2p_map"] = pointgroup_ops.voxelization_idx(data["locs_scaled"], len(samples), mode)
    return data


def collate_scenes_device(samples, device, mode=4):
    """`collate_scenes` as ONE launch (csrc/collate.hip, `d3_collate_scenes`): the same keys, dtypes, shapes and bits, from the
    per-scene dicts of `prepare_scene`.  The per-scene pointers and counts go up as one pinned table in one asynchronous copy;
    the voxelisation is `pointgroup_ops.voxelization_idx`, as there.  One batch `collate_scenes` cannot stack has a result here: with
    GT proposal lists, an instance-less scene followed by another leaves that function asking an empty list for its last element
    (IndexError, as in the reference); the kernel shifts each scene's offsets by the proposal entries before it."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device(device.type, torch.cuda.current_device())
    B = len(samples)
    if B < 1:
        raise ValueError("collate_scenes_device: no samples")
    has_gt = "gt_proposals_idx" in samples[0]
    if any(("gt_proposals_idx" in s) != has_gt for s in samples):
        raise ValueError("collate_scenes_device: GT proposal lists on some samples only")
    Cf, R = samples[0]["feats"].shape[1], samples[0]["center_label"].shape[0]
    keep, ptrs, counts = [], np.zeros((B, len(_SCENE_KEYS)), np.uint64), np.zeros((B, 3), np.int32)
    for i, s in enumerate(samples):
        n, K = s["locs"].shape[0], int(s["num_instance"])
        Lp = s["gt_proposals_idx"].shape[0] if has_gt else 0
        lead = {"points": (n,), "instances": (K,), "instances+1": (K + 1,), "entries": (Lp,), "B,R": (R,)}
        for j, k in enumerate(_SCENE_KEYS):
            if k.gt and not has_gt:
                continue
            t, dt, shape = s[k.name], k.scene_dtype, _shape(lead[k.extent], k.scene_tail, Cf)
            if t.dtype != dt or tuple(t.shape) != shape or t.device != device:
                raise ValueError("collate_scenes_device: sample %d %s is %s %s on %s, expected %s %s on %s"
                                 % (i, k.name, t.dtype, tuple(t.shape), t.device, dt, shape, device))
            t = t.contiguous()
            keep.append(t)
            ptrs[i, j] = t.data_ptr()
        counts[i] = (n, K, Lp)
    N, I, Lt = (int(v) for v in counts.sum(0, dtype=np.int64))
    if max(N, I, Lt) >= 2 ** 31:
        _range_error("collate_scenes_device: %d points / %d instances / %d proposal entries" % (N, I, Lt))
    data, out = _alloc_batch(device, B, R, Cf, has_gt, N, I, Lt)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    with _on(device):
        nbytes = int(_lib.lib().d3_collate_table_bytes(B))
        if nbytes == 0:
            _range_error("collate_scenes_device: %d scenes" % B)
        table, copied = _pinned("table", nbytes, device)
        ws = _workspace(nbytes, device, "collate")
        call("collate_scenes", hp(ptrs), hp(counts), B, Cf, R, int(has_gt), hp(out), C.c_void_p(table.data_ptr()), _ptr(ws), nbytes,
             _stream())
        copied.record()
    # `keep` (the contiguous inputs) lives until here; the launch is queued on their stream, which orders any later reuse
    data["voxel_locs"], data["p2v_map"], data["v2p_map"] = pointgroup_ops.voxelization_idx(data["locs_scaled"], B, mode)
    return data


# ------------------------------------------------------------------------------------------------ a batch from the scene store
def fused_applicable(cfg, is_augment, store):
    """Whether `prepare_batch_store` covers this path (a pure host predicate): the store is resident on a device and neither
    elastic distortion nor crop runs, so every scene keeps all its points.  Not covered, and left to `prepare_scene` +
    `collate_scenes_device`: the augmented detector-only mode (its point count is data-dependent), a pinned-host store, and
    noise="host" (which only matters under the elastic; the loader checks it)."""
    return torch.device(store.device).type == "cuda" and not elastic_enabled(cfg, is_augment)


def batch_plan(offsets, table_offsets, scalars, rows):
    """The host half of one batch over an instance index: offsets (S+1) the store's row offsets, table_offsets (S+1) the index
    tables' offsets, scalars (S,5) = id_lo, id_hi, K, Lp, has_unlabelled per scene; rows: the store row of each batch slot (a
    scene may repeat).  -> dict: row0 (B,) int64, slots (B,6) int32 = n, table offset, V, K, Lp, has_unlabelled per slot
    (`d3_batch_prepare`'s two host arrays), and the totals N points, I instances, L proposal entries, V id values."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    offsets, table_offsets, scalars = np.asarray(offsets, np.int64), np.asarray(table_offsets, np.int64), np.asarray(scalars, np.int64)
    n = offsets[rows + 1] - offsets[rows]
    V = np.maximum(scalars[rows, 1], 0) + 1
    slots = np.stack([n, table_offsets[rows], V, scalars[rows, 2], scalars[rows, 3], scalars[rows, 4]], 1)
    return {"row0": np.ascontiguousarray(offsets[rows]), "slots": np.ascontiguousarray(slots.astype(np.int32)),
            "N": int(n.sum()), "I": int(scalars[rows, 2].sum()), "L": int(scalars[rows, 3].sum()), "V": int(V.sum())}


def prepare_batch_store(store, scene_ids, cfg, mean_size_arr, rng=None, is_augment=False, device=None, mode=4, matrices=None):
    """The batch `collate_scenes_device([prepare_scene(store.scene(s), ...) for s in scene_ids])` builds -- the same keys, dtypes,
    shapes and bits -- straight from a resident `dataset.SceneStore` and its `instance_index()`: one table copy and three launches
    (csrc/batch_prep.hip, `d3_batch_prepare`) plus `pointgroup_ops.voxelization_idx`, with no read-back and no per-scene tensor.
    A scene may fill several slots.

    With is_augment one `augment_matrix(rng, ...)` is drawn per slot in slot order -- the per-scene path's draws in its order --
    and nothing otherwise; `matrices` (one 3x3 per slot) replaces the draws for a caller that interleaves them with its own
    (`dataset.PipelineLoader`).  mean_size_arr: (18,3), or a float64 tensor already on the device (nothing is uploaded then).

    Only where `fused_applicable` holds: the elastic / crop path and a pinned-host store raise ValueError."""
    if elastic_enabled(cfg, is_augment):
        raise ValueError("prepare_batch_store: the augmented detector-only path (elastic distortion, crop) is prepare_scene's")
    ix = store.instance_index()                        # a pinned-host store raises ValueError here
    dev = _store_device(store, device, "prepare_batch_store")
    B = len(scene_ids)
    if B < 1:
        raise ValueError("prepare_batch_store: no scenes")
    d = cfg.data
    R, has_gt, Cf = int(d.max_num_instance), bool(d.requires_gt_mask), store.feats.shape[1]
    mats = None
    if is_augment:
        if matrices is None:
            rng = np.random if rng is None else rng
            matrices = [augment_matrix(rng, d.transform) for _ in range(B)]
        mats = np.ascontiguousarray(np.stack([np.asarray(m, np.float64) for m in matrices]).reshape(B, 9))
    plan = batch_plan(store.offsets, ix.table_offsets, ix.scalars, [store.row_of(s) for s in scene_ids])
    N, I, Lt = plan["N"], plan["I"], plan["L"]
    if max(N, I, Lt) >= 2 ** 31:
        _range_error("prepare_batch_store: %d points / %d instances / %d proposal entries" % (N, I, Lt))
    ms = _mean_sizes_on(mean_size_arr, dev, "prepare_batch_store")
    data, out = _alloc_batch(dev, B, R, Cf, has_gt, N, I, Lt)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    with _on(dev):
        L = _lib.lib()
        tbytes, nbytes = int(L.d3_batch_prepare_table_bytes(B)), int(L.d3_batch_prepare_ws_bytes(B, plan["V"]))
        if tbytes == 0 or nbytes == 0:
            _range_error("prepare_batch_store: %d scenes" % B)
        table, copied = _pinned("table", tbytes, dev)
        ws = _workspace(nbytes, dev, "batch_prep")
        call("batch_prepare", _ptr(store.points), _ptr(store.feats), _ptr(store.sem_labels), _ptr(store.instance_ids),
             store.points.shape[0], _ptr(ix.hist), _ptr(ix.rank), _ptr(ix.start), _ptr(ix.sorted), ix.hist.shape[0],
             hp(plan["row0"]), hp(plan["slots"]), hp(mats) if mats is not None else None, B, Cf, R, 0 if is_augment else 1,
             int(has_gt), float(d.scale), _ptr(ms), hp(out), C.c_void_p(table.data_ptr()), _ptr(ws), ws.numel(), _stream())
        copied.record()
    data["voxel_locs"], data["p2v_map"], data["v2p_map"] = pointgroup_ops.voxelization_idx(data["locs_scaled"], B, mode)
    return data


# ------------------------------------------------------------------------------------------------ the elastic / crop batch from the store
READBACK_COLUMNS = ("kept", "K", "Lp", "X1", "Y1", "Z1", "X2", "Y2", "Z2", "crop_iters")


def elastic_applicable(cfg, is_augment, store):
    """Whether `prepare_batch_store_elastic` covers this path (a pure host predicate): the store is resident on a device and the
    elastic distortion and crop run (the augmented detector-only mode) -- the complement of `fused_applicable` on a resident store."""
    return torch.device(store.device).type == "cuda" and elastic_enabled(cfg, is_augment)


def elastic_batch_queue(store, scene_ids, cfg, mean_size_arr, rng=None, device=None, draws=None):
    """The queueing half of `prepare_batch_store_elastic`: the draws, the host bound of the noise grids, one table copy and every
    launch, with no wait for the device.  -> the pending batch `elastic_batch_finish` completes.

    A caller may queue ahead: every pending batch has its own pinned image of the read-back table, from a ring of `_TABLE_RING`
    per (device, host thread, stream).  So at most `_TABLE_RING - 1` batches may be queued and unfinished there when another is
    queued; beyond that the oldest pending batch's image is handed to the new one and that batch must not be finished any more."""
    if not elastic_enabled(cfg, True):
        raise ValueError("prepare_batch_store_elastic: no elastic distortion in this configuration (a language mode): prepare_batch_store's")
    ix = store.instance_index()                        # a pinned-host store raises ValueError here
    dev = _store_device(store, device, "prepare_batch_store_elastic")
    B = len(scene_ids)
    if B < 1:
        raise ValueError("prepare_batch_store_elastic: no scenes")
    d = cfg.data
    scale, R, has_gt, Cf = d.scale, int(d.max_num_instance), bool(d.requires_gt_mask), store.feats.shape[1]
    params = elastic_params(scale)
    grans = [int(g) for g, _ in params]
    if any(g < 1 or g != gf for g, (gf, _) in zip(grans, params)):
        raise ValueError("prepare_batch_store_elastic: data.scale %r gives the elastic granularities %r" % (scale, [g for g, _ in params]))
    crop_scale = d.full_scale[1]
    T = crop_max_iters(crop_scale)
    if draws is None:
        rng = np.random if rng is None else rng
        draws = []
        for _ in range(B):                             # prepare_scene's draws in its order: the matrix, then the noise seed
            m = augment_matrix(rng, d.transform)
            draws.append((m, int(rng.randint(0, 2 ** 31 - 1))))
    if len(draws) != B:
        raise ValueError("prepare_batch_store_elastic: %d draws for %d slots" % (len(draws), B))
    mats = np.ascontiguousarray(np.stack([np.asarray(m, np.float64) for m, _ in draws]).reshape(B, 9))
    seeds = np.ascontiguousarray([int(sd) for _, sd in draws], dtype=np.uint64)
    crop_u = np.ascontiguousarray(np.stack([np.random.RandomState(int(sd)).rand(T, 3) for _, sd in draws]))
    rows = np.asarray([store.row_of(s) for s in scene_ids], np.int64)
    row0 = np.ascontiguousarray(store.offsets[rows])
    n = store.offsets[rows + 1] - row0
    V = np.maximum(ix.scalars[rows, 1], 0) + 1
    absmax = store.absmax()
    bounds = np.stack([np.concatenate([elastic_grid_bound(absmax[r], mats[i].reshape(3, 3), scale, e) for e in (0, 1)])
                       for i, r in enumerate(rows)])
    if bounds.max() >= 2 ** 31:
        _range_error("prepare_batch_store_elastic: noise grid bound %d" % int(bounds.max()))
    slots = np.ascontiguousarray(np.concatenate([n[:, None], V[:, None], bounds], 1).astype(np.int32))
    N, Vt = int(n.sum()), int(V.sum())
    ms = _mean_sizes_on(mean_size_arr, dev, "prepare_batch_store_elastic")
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    with _on(dev):
        L = _lib.lib()
        tbytes = int(L.d3_batch_elastic_table_bytes(B, T))
        nbytes = int(L.d3_batch_elastic_ws_bytes(hp(slots), B, Cf, T)) if tbytes else 0
        if tbytes == 0 or nbytes == 0:                 # refused before anything is allocated or queued
            _range_error("prepare_batch_store_elastic: %d scenes, %d points, noise grid bounds up to %s, %d crop iterations"
                         % (B, N, bounds.max(0).tolist(), T))
        data, out = _alloc_batch(dev, B, R, Cf, has_gt, N, Vt, N)      # the static upper bounds; `elastic_batch_finish` cuts
        readback = torch.empty((B, len(READBACK_COLUMNS)), dtype=torch.int32, device=dev)
        table, copied = _pinned("table", tbytes, dev)
        ws = _workspace(nbytes, dev, "batch_elastic")
        call("batch_elastic", _ptr(store.points), _ptr(store.feats), _ptr(store.sem_labels), _ptr(store.instance_ids),
             store.points.shape[0], hp(row0), hp(slots), hp(mats), hp(seeds), hp(crop_u), B, Cf, R, T, int(has_gt), float(scale),
             grans[0], grans[1], float(params[0][1]), float(params[1][1]), float(crop_scale), int(d.max_num_point), _ptr(ms), hp(out),
             _ptr(readback), C.c_void_p(table.data_ptr()), _ptr(ws), ws.numel(), _stream())
        copied.record()
        image, done = _pinned("readback", readback.numel() * 4, dev)
        host = image[:readback.numel() * 4].view(torch.int32).view(readback.shape)
        host.copy_(readback, non_blocking=True)        # queued behind the launches; `elastic_batch_finish` waits for it
        done.record()
    return {"data": data, "readback": host, "done": done, "bounds": bounds, "B": B, "has_gt": has_gt, "keep": (readback, ms)}


def elastic_batch_finish(pending, mode=4, info=None):
    """The batch's ONE device-to-host read: waits for the read-back table, checks the real noise-grid shapes against the host's
    bound (a wrong bound is an error, never a silent clamp), and cuts the outputs to their real lengths.  info: a dict that
    receives `readback` (B,10) int32 in `READBACK_COLUMNS` order and `bounds` (B,6)."""
    pending["done"].synchronize()
    rb = pending["readback"].numpy().copy()
    if info is not None:
        info.update(readback=rb, bounds=pending["bounds"].copy())
    if (rb[:, 3:9] > pending["bounds"]).any():
        bad = int(np.argmax((rb[:, 3:9] > pending["bounds"]).any(1)))
        raise RuntimeError("prepare_batch_store_elastic: slot %d: real noise grids %s exceed the host bound %s"
                           % (bad, rb[bad, 3:9].tolist(), pending["bounds"][bad].tolist()))
    data, B = pending["data"], pending["B"]
    kept, I, Lt = (int(v) for v in rb[:, :3].sum(0, dtype=np.int64))
    for k in ("locs", "locs_scaled", "feats", "sem_labels", "instance_ids", "instance_info"):
        data[k] = data[k][:kept]
    data["instance_num_point"] = data["instance_num_point"][:I]
    if pending["has_gt"]:
        data["gt_proposals_idx"] = data["gt_proposals_idx"][:Lt]
        data["gt_proposals_offset"] = data["gt_proposals_offset"][:I + 1]
    data["voxel_locs"], data["p2v_map"], data["v2p_map"] = pointgroup_ops.voxelization_idx(data["locs_scaled"], B, mode)
    return data


def prepare_batch_store_elastic(store, scene_ids, cfg, mean_size_arr, rng=None, device=None, mode=4, draws=None, info=None):
    """The batch `collate_scenes_device([prepare_scene(store.scene(s), cfg, msa, rng, is_augment=True, noise="device") for s in
    scene_ids])` builds in the augmented detector-only mode (`elastic_enabled(cfg, True)`: jitter / flip / rotation, two elastic
    distortions, crop to data.max_num_point, `_croppedInstanceIds`; pipeline.py:145-164) -- the same keys, dtypes, shapes and bits
    -- straight from a resident `dataset.SceneStore` (csrc/batch_elastic.hip, `d3_batch_elastic`): one table copy and a number of
    launches that depends neither on the batch size, nor on the scenes' sizes, nor on the crop iterations any slot runs; no
    per-scene tensor; ONE device-to-host read per batch (`READBACK_COLUMNS` per slot) besides the voxelisation's own count
    read-back.  A scene may fill several slots; every slot must have points.

    Draws, per slot in slot order: `augment_matrix(rng, cfg.data.transform)` and `seed = rng.randint(0, 2**31 - 1)` --
    `prepare_scene`'s draws in its order -- and nothing else from `rng`: the crop loop's draws are the rows of
    `np.random.RandomState(seed).rand(crop_max_iters(full_scale[1]), 3)`, one row per iteration, so the caller's stream advances
    the same way whatever the data does (the per-scene path takes one `rng.rand(3)` per crop iteration from the caller's stream
    instead).  Whenever no slot is cropped the batch and the generator's state afterwards equal the per-scene path's outright.
    `draws` (one `(matrix, seed)` per slot) replaces the draws.  mean_size_arr: as for `prepare_batch_store`.

    Only where `elastic_applicable` holds: a configuration without the elastic and a pinned-host store raise ValueError; a noise
    grid bound beyond the library's grid limits, more than 512 slots or a slot without points raise the library's range error,
    all before anything is queued."""
    return elastic_batch_finish(elastic_batch_queue(store, scene_ids, cfg, mean_size_arr, rng, device, draws), mode, info)


# ------------------------------------------------------------------------------------------------ the label-free batch (test split)
_LABEL_FREE_KEYS = ("locs", "locs_scaled", "feats", "batch_offsets", "voxel_locs", "p2v_map", "v2p_map")


def store_extents(store, scale):
    """ONE launch over a resident store (csrc/batch_prep.hip, `d3_store_extents`): (S,3) int64 on the store's device, per scene
    and axis the kernels' order-preserving encoding (`_decode`) of min(fl32(x * fl32(scale))) -- `points.min(0)` of
    pipeline.py:352-380, a constant of the (store, scale) pair since that branch draws nothing and drops no point.
    `SceneStore.extents` caches it."""
    dev, S = _store_device(store, None, "store_extents"), len(store)
    ext = torch.empty((S, 3), dtype=torch.int64, device=dev)
    offsets = np.ascontiguousarray(store.offsets, dtype=np.int64)
    with _on(dev):
        L = _lib.lib()
        tbytes, nbytes = int(L.d3_store_extents_table_bytes(S)), int(L.d3_store_extents_ws_bytes(S))
        if tbytes == 0 or nbytes == 0:
            _range_error("store_extents: %d scenes" % S)
        table, copied = _pinned("table", tbytes, dev)
        ws = _workspace(nbytes, dev, "store_extents")
        call("store_extents", _ptr(store.points), store.points.shape[0], offsets.ctypes.data_as(C.c_void_p), S, float(scale), _ptr(ext),
             C.c_void_p(table.data_ptr()), _ptr(ws), ws.numel(), _stream())
        copied.record()
    return ext


def prepare_points_store(store, scene_ids, cfg, device=None, mode=4):
    """The label-free batch of the reference's test branch (pipeline.py:352-380 per sample, `sparse_collate_fn`'s :937-976 and
    :992) straight from a resident `dataset.SceneStore`: locs (N,3) float32, locs_scaled (N,4) int64, feats (N,C) float32,
    batch_offsets (B+1) int32 and voxel_locs / p2v_map / v2p_map -- no label key.  The arithmetic is the unaugmented labelled
    branch's, so these seven keys equal, bit for bit, those of `collate_scenes_device([prepare_scene(store.scene(s), cfg, ...,
    is_augment=False) for s in scene_ids])`.  One table copy and ONE launch (`d3_points_batch`) plus
    `pointgroup_ops.voxelization_idx`; the per-scene minima come from `store.extents(cfg.data.scale)`, built on the first call.
    The store's labels, if it has any, are ignored; a scene may fill several slots.  A pinned-host store raises ValueError.
    The extents launch covers every scene of the store, so a store that holds a scene without points (a labelled store may) is
    refused by that scene's name on the first call, whether or not the batch names it."""
    dev = _store_device(store, device, "prepare_points_store")
    B = len(scene_ids)
    if B < 1:
        raise ValueError("prepare_points_store: no scenes")
    scale, Cf = cfg.data.scale, store.feats.shape[1]
    ext = store.extents(scale)
    srow = np.ascontiguousarray([store.row_of(s) for s in scene_ids], dtype=np.int32)
    row0 = np.ascontiguousarray(store.offsets[srow], dtype=np.int64)
    n = np.ascontiguousarray(store.offsets[srow + 1] - row0, dtype=np.int32)
    N = int(n.sum(dtype=np.int64))
    if N >= 2 ** 31:
        _range_error("prepare_points_store: %d points" % N)
    f32 = torch.float32
    data = {"locs": torch.empty((N, 3), dtype=f32, device=dev), "locs_scaled": torch.empty((N, 4), dtype=torch.int64, device=dev),
            "feats": torch.empty((N, Cf), dtype=f32, device=dev), "batch_offsets": torch.empty((B + 1,), dtype=torch.int32, device=dev)}
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    with _on(dev):
        L = _lib.lib()
        tbytes, nbytes = int(L.d3_points_batch_table_bytes(B)), int(L.d3_points_batch_ws_bytes(B))
        if tbytes == 0 or nbytes == 0:
            _range_error("prepare_points_store: %d scenes" % B)
        table, copied = _pinned("table", tbytes, dev)
        ws = _workspace(nbytes, dev, "points_batch")
        call("points_batch", _ptr(store.points), _ptr(store.feats), store.points.shape[0], _ptr(ext), len(store), hp(row0), hp(srow), hp(n),
             B, Cf, float(scale), _ptr(data["locs"]), _ptr(data["locs_scaled"]), _ptr(data["feats"]), _ptr(data["batch_offsets"]),
             C.c_void_p(table.data_ptr()), _ptr(ws), ws.numel(), _stream())
        copied.record()
    data["voxel_locs"], data["p2v_map"], data["v2p_map"] = pointgroup_ops.voxelization_idx(data["locs_scaled"], B, mode)
    return data


def prepare_batch(scenes, cfg, mean_size_arr, rng=None, is_augment=True, noise="device", device=None, mode=4):
    """Raw scenes (dicts of `points` (N,3) metres, `feats` (N,C), `sem_labels` (N,) -1 ignored, `instance_ids` (N,) -1 none; numpy
    or device tensors) -> the device batch `collate.sparse_collate_fn` returns for the reference's per-scene sample dicts built
    from the same scenes and draws (point keys, voxelisation maps, GT proposal lists when cfg.data.requires_gt_mask, stacked box
    labels).  Scenes are prepared one after another: each scene's crop draws depend on that scene's device counts and precede
    the next scene's draws, as in the reference's loader.  mean_size_arr: (18,3), scannet_reference_means.npz."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    rng = np.random if rng is None else rng
    samples = [prepare_scene(sc, cfg, mean_size_arr, rng=rng, is_augment=is_augment, noise=noise, device=device) for sc in scenes]
    return collate_scenes(samples, device, mode)
