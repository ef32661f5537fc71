"""The dataset loader: what joins the preparation chain (`scan_export` -> `enet` -> `multiview` -> `scene_prep` / `lang_prep`) to
the fit loop (`trainer.Trainer`), in place of the reference's `PipelineDataset._load` (lib/dataset/pipeline.py:384-413), the three
`init_*_data` functions of scripts/train.py:30-245 and the `DistributedSampler` Lightning installs for them.

  * `SceneStore`: one split's scenes packed into four flat arrays, resident on the device (or pinned on the host); `scene(id)` hands
    `scene_prep.prepare_scene` views of them, so a batch uploads nothing.
  * `PipelineLoader`: a re-iterable source of batches for `Trainer.fit` -- the samples of one rank in `DistributedSampler`'s order,
    in groups of `data.batch_size`, each built by `prepare_scene` per sample, ONE `scene_prep.collate_scenes_device` launch and, with
    descriptions, `lang_prep`'s two launches.  With `fused=True` the scene half of a batch comes straight from the store and its
    `InstanceIndex` instead (`scene_prep.prepare_batch_store`: no read-back, the same bits) wherever that path applies.
  * `PairedLoader`: the joint mode's `[speaker batch, listener batch]` source.
  * `build_loaders`: the sources and the `dataset` namespace of a configuration, from the paths of conf/path.yaml.
  * `build_test_loader`: the `init_data` of benchmark/benchmark_captioning.py / benchmark_grounding.py -- a `SceneStore(labels=False)`
    and a `PipelineLoader(label_free=True)`, whose batches (`scene_prep.prepare_points_store`) carry no label key; `predict.py` runs it.

The per-sample order of random draws is `lang_prep.prepare_pipeline_batch`'s / `scene_prep.prepare_batch`'s; the generators are the
loader's own, seeded from (seed, epoch, rank), never the global ones.
"""
import copy
import ctypes as C
import json
import os
import pickle
import random
import types
import warnings

import numpy as np
import torch

from . import _lib, lang_prep, scene_prep

_FIELDS = ("points", "feats", "sem_labels", "instance_ids")
SYNTHETIC = "SYNTHETIC"


# ------------------------------------------------------------------------------------------------ annotation lists (host only)
def synthetic_entry(scene_id):
    """the description-less entry of scripts/train.py:53-60 / :135-142"""
    return {"scene_id": scene_id, "object_id": SYNTHETIC, "object_name": SYNTHETIC, "ann_id": SYNTHETIC, "description": SYNTHETIC,
            "token": [SYNTHETIC]}


def read_scan_list(path):
    return [s.rstrip() for s in open(path).readlines()]


def scan_list_of(raw):
    """scripts/train.py:109: the sorted scene ids of an annotation list"""
    return sorted(list(set(d["scene_id"] for d in raw)))


def detector_entries(scan_list):
    """`init_detector_data` (scripts/train.py:51-73): one SYNTHETIC entry per scan, in list order"""
    return [synthetic_entry(s) for s in scan_list]


def speaker_val_entries(raw_val):
    """`init_speaker_data` (scripts/train.py:112-118): one entry per validation scene, a copy of raw_val[0] with the scene id swapped"""
    out = []
    for scene_id in scan_list_of(raw_val):
        d = copy.deepcopy(raw_val[0])
        d["scene_id"] = scene_id
        out.append(d)
    return out


def speaker_train_entries(raw_train, all_train_scans, extra_ratio, pyrng):
    """`init_speaker_data` (scripts/train.py:120-150) -> (data_train, scan_list_train): with extra_ratio > 0 the SYNTHETIC fill
    over the scans without annotations (`random.choice` once they run out) and the `random.shuffle` of the whole list, both drawn
    from `pyrng` (a random.Random) where the reference uses the global generator"""
    data = copy.deepcopy(raw_train)
    scans = scan_list_of(raw_train)
    if extra_ratio > 0:
        num_extra = int(len(raw_train) * extra_ratio)
        extra_scans = [s for s in all_train_scans if s not in scans]
        extra = [synthetic_entry(extra_scans[i] if i < len(extra_scans) else pyrng.choice(extra_scans)) for i in range(num_extra)]
        data += extra
        scans = scans + scan_list_of(extra)
        pyrng.shuffle(data)
    return data, scans


def organize(raw_data):
    """`_organize_data` (pipeline.py:567-581): organized[scene_id][object_id] -> the entries, SYNTHETIC ones left out"""
    out = {}
    for d in raw_data:
        if d["object_id"] != SYNTHETIC:
            out.setdefault(d["scene_id"], {}).setdefault(d["object_id"], []).append(d)
    return out


def sampler_indices(n, world=1, rank=0, shuffle=True, seed=0, epoch=0):
    """`list(torch.utils.data.DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=shuffle, seed=seed,
    drop_last=False))` after `set_epoch(epoch)`: randperm under manual_seed(seed + epoch), padded by wrap-around to a multiple of
    `world`, rank r takes r::world"""
    if not 0 <= rank < world:
        raise ValueError("rank %d outside [0, %d)" % (rank, world))
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        idx = torch.randperm(n, generator=g).tolist()
    else:
        idx = list(range(n))
    total = (n + world - 1) // world * world
    pad = total - n
    if pad:
        idx += idx[:pad] if pad <= n else (idx * ((pad + n - 1) // n))[:pad]
    return idx[rank:total:world]


# ------------------------------------------------------------------------------------------------ the scene store
def _host(x, dtype):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x).astype(dtype, copy=False))


def mesh_features(mesh, use_color, use_normal, multiview=None):
    """`_get_coord_and_feat_from_mesh` (pipeline.py:774-802) on an aligned mesh (N, 6 or 9): -> (points (N,3), feats (N,C)) float32;
    colours if use_color, normals if use_normal (the mesh must then have 9 columns, as the reference asserts), then the (N,128)
    multiview rows when `multiview` is not None"""
    mesh = _host(mesh, np.float32)
    cols = []
    if use_color:
        cols.append(mesh[:, 3:6])
    if use_normal:
        if mesh.shape[1] != 9:
            raise ValueError("use_normal needs xyz, rgb and normals: the mesh has %d columns, not 9" % mesh.shape[1])
        cols.append(mesh[:, 6:9])
    if multiview is not None:
        mv = _host(multiview, np.float32)
        if mv.shape != (mesh.shape[0], 128):
            raise ValueError("multiview features are %s, expected %s" % (mv.shape, (mesh.shape[0], 128)))
        cols.append(mv)
    feats = np.concatenate(cols, 1) if cols else np.zeros((mesh.shape[0], 0), np.float32)
    return np.ascontiguousarray(mesh[:, :3]), np.ascontiguousarray(feats)


def scene_instance_tables(ids):
    """One scene's part of the `InstanceIndex` from its instance ids (n,), all >= -1, with V = max(ids.max(), 0) + 1:
    -> (hist (V+1), rank (V+1), start (V+1), order (n)): hist[0] the unlabelled points and hist[v + 1] those with id v; rank / start
    the exclusive scans of presence / count over the id values with the totals K / Lp as last entry; order the stable sort of the
    point indices by rank, unlabelled points behind every instance (`sp_hist_kernel` ... `sp_keys_kernel` and the sort of
    csrc/scene_prep.hip:d3_scene_instances)."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    V = max(int(ids.max()) if len(ids) else -1, 0) + 1
    hist = np.bincount(ids + 1, minlength=V + 1)
    rank = np.concatenate([[0], np.cumsum(hist[1:] > 0)])
    start = np.concatenate([[0], np.cumsum(hist[1:])])
    key = np.where(ids >= 0, rank[np.maximum(ids, 0)], rank[V])
    return hist, rank, start, np.argsort(key, kind="stable").astype(np.int32)


class InstanceIndex:
    """What `scene_prep.prepare_scene` derives per scene and per batch from a scene's `instance_ids` alone (csrc/scene_prep.hip,
    `sp_hist_kernel` ... `sp_totals_kernel`, `sp_keys_kernel` and the stable sort of `d3_scene_instances`), computed ONCE for a
    whole store -- valid wherever a scene keeps all its points, i.e. without the crop of the augmented detector-only path:

      * per scene V = max(id_hi, 0) + 1 and, from `table_offsets[scene]`, V + 1 entries of each flat table: `hist` (hist[0] the
        unlabelled points, hist[v + 1] those with id v), `rank` / `start` (the exclusive scans of presence / count, i.e. the
        instance's place in np.unique order and its first row in the GT proposal list; the extra last entry is K / Lp);
      * `sorted` (one int32 per store point, at the scene's rows): scene-local point indices grouped by instance in np.unique
        order, ascending inside each instance, the unlabelled points last;
      * `scalars` (S,5) on the HOST: id_lo, id_hi, K instances, Lp labelled points, has_unlabelled -- the output shapes of every
        later batch, read here once instead of once per scene and batch.

    The tables are integer functions of the ids, built on the host from one copy of `instance_ids` (a stable argsort is the
    kernels' stable radix sort) and uploaded once; this is a one-off per store.  What `prepare_scene` refuses per scene is
    refused here with the same error and the scene's name: an id below -1, an id above the library's limit, too many points."""

    def __init__(self, store):
        if store.device.type == "cpu":
            raise ValueError("SceneStore.instance_index: the store is pinned host memory; the index serves the resident store only")
        max_points, max_id = C.c_int(0), C.c_int(0)
        _lib.lib().d3_scene_limits(C.byref(max_points), None, C.byref(max_id))
        ids_all = store.instance_ids.cpu().numpy()
        S = len(store)
        self.scalars = np.zeros((S, 5), np.int64)
        self.table_offsets = np.zeros(S + 1, np.int64)
        hist, rank, start = [], [], []
        order = np.empty(ids_all.shape[0], np.int32)
        for i, sid in enumerate(store.scene_ids):
            a, b = int(store.offsets[i]), int(store.offsets[i + 1])
            ids, n = ids_all[a:b].astype(np.int64), b - a
            id_lo, id_hi = (int(ids.min()), int(ids.max())) if n else (-1, -1)
            if id_lo < -1:
                scene_prep._range_error("scene_prep: scene %s: instance id %d < -1" % (sid, id_lo))
            if n > max_points.value or id_hi > max_id.value:
                scene_prep._range_error("scene_prep: scene %s: %d points / instance id %d" % (sid, n, id_hi))
            V = max(id_hi, 0) + 1
            h, r, st, order[a:b] = scene_instance_tables(ids)
            hist.append(h); rank.append(r); start.append(st)
            self.scalars[i] = (id_lo, id_hi, int(r[V]), int(st[V]), int(h[0] > 0))
            self.table_offsets[i + 1] = self.table_offsets[i] + V + 1
        up = lambda parts: torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(store.points.device)
        self.hist, self.rank, self.start = up(hist), up(rank), up(start)
        self.sorted = torch.from_numpy(order).to(store.points.device)

    def bytes(self):
        return sum(t.numel() * t.element_size() for t in (self.hist, self.rank, self.start, self.sorted))


class SceneStore:
    """The scenes of one split as four flat, per-scene-contiguous arrays -- `points` (N,3) float32, `feats` (N,C) float32,
    `sem_labels` (N,) int32, `instance_ids` (N,) int32, N the split's point total -- with the host table `offsets` (S+1) of row
    offsets and `scene_ids`.  Everything is packed on the host and goes up in ONE upload per array.

    `scene(scene_id)` returns the raw-scene dict `scene_prep.prepare_scene` takes as zero-copy row slices of the packed arrays: no
    kernel, no copy, and `prepare_scene` finds them on its device with its dtypes, so its own conversions are no-ops too.
    The views alias the store: writing to one changes the scene for every later batch.  `prepare_scene` does not write to its
    inputs -- every kernel that reads them (`d3_scene_transform`, `d3_scene_emit`) takes them `const` and writes fresh tensors
    (csrc/scene_prep.hip, include/d3hip.h) -- so the loader never needs a copy; a caller who wants to edit a scene clones it first.

    With device="cpu" the arrays are pinned host memory and `scene()` returns non-blocking device copies issued on the caller's
    current stream (for a split whose multiview features someone does not want resident); the batches are the same."""

    def __init__(self, scene_ids, offsets, arrays, device, labels=True):
        self.scene_ids, self.offsets = list(scene_ids), np.asarray(offsets, np.int64)
        self.labels = bool(labels)
        self._row = {s: i for i, s in enumerate(self.scene_ids)}
        if len(self._row) != len(self.scene_ids):
            raise ValueError("SceneStore: a scene id appears twice")
        self.device = torch.device(device)
        for k in _FIELDS:
            t = torch.from_numpy(arrays[k])
            setattr(self, k, t.pin_memory() if self.device.type == "cpu" and torch.cuda.is_available() and t.numel() else t.to(self.device))
        self._index = None
        self._extents = {}
        self._absmax = None

    # --------------------------------------------------------------------------------------------- construction
    @classmethod
    def from_scenes(cls, scenes, cfg=None, device="cuda", multiview=None, labels=True):
        """scenes: {scene_id: scene} in the store's order.  A scene is a raw-scene dict (`points`, `feats`, `sem_labels`,
        `instance_ids`; taken as it is) or what the reference's scene file holds (`aligned_mesh` (N,6|9), `sem_labels`,
        `instance_ids`; a `scan_export.ScanExport` counts), whose feature columns follow cfg.model.use_color / use_normal /
        use_multiview (`mesh_features`).  multiview: {scene_id: (N,128) array or tensor}; a scene missing from it gets the
        reference's zero placeholder (pipeline.py:794-795).  Arrays may be numpy or tensors on any device.

        labels=False is the test split's store (pipeline.py:320-380 never reads the label arrays there, and prepare_scannet.py
        writes placeholders): `sem_labels` / `instance_ids` are not read -- a scene may lack them -- and the store keeps two
        zero-length arrays in their place; a scene without points is refused by name (`points.min(0)` raises in the reference)."""
        packed = {k: [] for k in _FIELDS}
        offsets, width = [0], None
        for sid, sc in scenes.items():
            if hasattr(sc, "to_reference_dict"):
                sc = sc.to_reference_dict()
            if not labels and len(sc["points"] if "points" in sc else sc["aligned_mesh"]) == 0:
                raise ValueError("SceneStore: scene %s has no points" % sid)
            if "points" in sc:
                pts, feats = _host(sc["points"], np.float32), _host(sc["feats"], np.float32)
                feats = feats.reshape(pts.shape[0], -1)
            else:
                if cfg is None:
                    raise ValueError("SceneStore.from_scenes: cfg.model's use_color / use_normal / use_multiview select a mesh's features")
                m, mv = cfg.model, None
                if m.use_multiview:
                    mv = (multiview or {}).get(sid)
                    if mv is None:
                        mv = np.zeros((sc["aligned_mesh"].shape[0], 128), np.float32)
                pts, feats = mesh_features(sc["aligned_mesh"], m.use_color, m.use_normal, mv)
            n = pts.shape[0]
            if not labels:
                if pts.shape != (n, 3) or feats.shape[0] != n:
                    raise ValueError("%s: points %s, feats %s" % (sid, pts.shape, feats.shape))
                sem = ids = np.zeros(0, np.int32)
            else:
                sem, ids = _host(sc["sem_labels"], np.int32).reshape(-1), _host(sc["instance_ids"], np.int32).reshape(-1)
            if labels and (pts.shape != (n, 3) or feats.shape[0] != n or sem.shape != (n,) or ids.shape != (n,)):
                raise ValueError("%s: points %s, feats %s, sem_labels %s, instance_ids %s" % (sid, pts.shape, feats.shape, sem.shape, ids.shape))
            if width is not None and feats.shape[1] != width:
                raise ValueError("%s: %d feature columns, the scenes before have %d" % (sid, feats.shape[1], width))
            width = feats.shape[1]
            for k, a in zip(_FIELDS, (pts, feats, sem, ids)):
                packed[k].append(a)
            offsets.append(offsets[-1] + n)
        if width is None:
            raise ValueError("SceneStore: no scenes")
        return cls(list(scenes), offsets, {k: np.ascontiguousarray(np.concatenate(v, 0)) for k, v in packed.items()}, device, labels)

    @classmethod
    def load(cls, cfg, split, scan_list, device="cuda", multiview=None, labels=True):
        """`_load`'s scene half (pipeline.py:387): torch.load of `<SCANNETV2_PATH.split_data>/<split>/<scene_id><data.file_suffix>`
        per scan of `scan_list`.  multiview: as in `from_scenes`; None with model.use_multiview reads the reference's HDF5 file
        (SCANNETV2_PATH.multiview_features) when `h5py` imports, and otherwise warns and leaves the zero placeholder.
        labels: as in `from_scenes`."""
        root = os.path.join(cfg.SCANNETV2_PATH.split_data, split)
        scenes = {s: torch.load(os.path.join(root, s + cfg.data.file_suffix), weights_only=False) for s in scan_list}
        h5 = None
        if cfg.model.use_multiview and multiview is None:
            try:
                import h5py
            except ImportError:
                warnings.warn("model.use_multiview is set, no multiview= mapping was given and h5py does not import: "
                              "the 128 multiview columns are the zero placeholder")
            else:
                h5 = h5py.File(cfg.SCANNETV2_PATH.multiview_features, "r", libver="latest")
                multiview = {s: h5[s][()] for s in scan_list if s in h5}
        try:
            return cls.from_scenes(scenes, cfg, device, multiview, labels)
        finally:
            if h5 is not None:
                h5.close()

    # --------------------------------------------------------------------------------------------- access
    def __len__(self):
        return len(self.scene_ids)

    def __contains__(self, scene_id):
        return scene_id in self._row

    def num_points(self, scene_id):
        i = self._row[scene_id]
        return int(self.offsets[i + 1] - self.offsets[i])

    def bytes(self):
        """the footprint of the four packed arrays (the two label arrays of a labels=False store are empty)"""
        return sum(getattr(self, k).numel() * getattr(self, k).element_size() for k in _FIELDS)

    def row_of(self, scene_id):
        """the scene's place in `scene_ids` / `offsets`"""
        return self._row[scene_id]

    def instance_index(self):
        """the store's `InstanceIndex`, built on first use and kept (`scene_prep.prepare_batch_store` reads it); a resident store
        only: a pinned-host store raises ValueError, and so does a labels=False store.  The store's arrays must not change
        afterwards."""
        if not self.labels:
            raise ValueError("SceneStore.instance_index: the store was built with labels=False and holds no instance ids")
        if self._index is None:
            self._index = InstanceIndex(self)
        return self._index

    def index_bytes(self):
        """the device footprint of the instance index (4 bytes per point plus the small tables), 0 while it is not built;
        `bytes()` does not count it"""
        return 0 if self._index is None else self._index.bytes()

    def extents(self, scale):
        """the (S,3) device table of `scene_prep.store_extents` for `scale` -- per scene and axis the minimum of fl32(x * scale),
        what the label-free path subtracts (pipeline.py:352-380), in the kernels' order-preserving int64 encoding
        (`scene_prep._decode` reads it) -- built on first use and kept per scale (`scene_prep.prepare_points_store` reads it); a
        resident store only: a pinned-host store raises ValueError.  The store's points must not change afterwards."""
        key = float(scale)
        if key not in self._extents:
            if self.device.type == "cpu":
                raise ValueError("SceneStore.extents: the store is pinned host memory; the table serves the resident store only")
            empty = np.flatnonzero(np.diff(self.offsets) == 0)
            if len(empty):
                raise ValueError("SceneStore.extents: scene %s has no points" % self.scene_ids[int(empty[0])])
            self._extents[key] = scene_prep.store_extents(self, scale)
        return self._extents[key]

    def absmax(self):
        """the (S,3) float64 HOST table of per-scene, per-axis max |xyz| (0 for a scene without points), what
        `scene_prep.elastic_grid_bound` sizes the noise grids from; built on first use (one reduction per scene, one read) and
        kept.  The store's points must not change afterwards."""
        if self._absmax is None:
            zero = torch.zeros(3, dtype=torch.float32, device=self.points.device)
            rows = [self.points[int(a):int(b)].abs().amax(0) if b > a else zero for a, b in zip(self.offsets[:-1], self.offsets[1:])]
            self._absmax = torch.stack(rows).cpu().numpy().astype(np.float64)
        return self._absmax

    def scene(self, scene_id, device=None):
        """the raw-scene dict of `prepare_scene`: views (device store) or non-blocking device copies (pinned store; `device`
        defaults to the current one); `points` and `feats` only from a labels=False store"""
        i = self._row[scene_id]
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        out = {k: getattr(self, k)[a:b] for k in (_FIELDS if self.labels else _FIELDS[:2])}
        if self.device.type == "cpu" and (device is not None or torch.cuda.is_available()):
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            out = {k: v.to(device, non_blocking=True) for k, v in out.items()}
        return out


# ------------------------------------------------------------------------------------------------ the batch source
def _opt(node, key, default):
    """an optional config key of a `config.Cfg` or of a plain namespace"""
    if node is None:
        return default
    return node.get(key, default) if isinstance(node, dict) else getattr(node, key, default)


class PipelineLoader:
    """A re-iterable source of batches over `store` for one rank.

    index: the split's `lang_prep.DescriptionIndex` -- a sample is then one chunk (`index.chunks`, the reference's
    `_get_chunked_data`) -- or None in the pure detector mode, where a sample is one scene of `scene_ids` (default: the store's,
    the SYNTHETIC entries of `init_detector_data`).  mode: the reference dataset's "speaker" / "listener" / "detector", kept
    for the log.  `__iter__` starts a new pass at the loader's current epoch in `sampler_indices`' order, i.e. that of
    `DistributedSampler(shuffle=shuffle, seed=seed, drop_last=False)`, which Lightning installs for the reference under DDP (world=1:
    a seeded shuffle=True), cut into consecutive groups of data.batch_size (the last one short).  `set_epoch(e)` sets the epoch
    of the next pass; every pass without it advances by one.  shuffle defaults to split == "train"; is_augment to False, as
    scripts/train.py builds its datasets.

    A batch is `lang_prep.prepare_pipeline_batch`'s (with an index) or `scene_prep.prepare_batch`'s (without) over
    `store.scene(...)`, stacked by `scene_prep.collate_scenes_device`; draws come from `generators(epoch)`.

    fused=True builds the scene half of every batch with `scene_prep.prepare_batch_store` instead -- straight from the store and its
    instance index, no read-back, no per-scene tensor, the same draws in the same order and the same bits -- wherever
    `fused_active()` holds.  Elsewhere it takes the path above: the augmented detector-only mode (elastic distortion and crop make
    the point count data-dependent), a pinned-host store or one on another device, and noise="host".

    fused_elastic=True (with fused=True) covers the first of these: where `fused_elastic_active()` holds -- is_augment in the
    detector-only configuration, noise="device", the store resident on the loader's device -- a batch is
    `scene_prep.prepare_batch_store_elastic`'s: one read-back per batch instead of four or more per scene.  Its crop draws come from
    a generator seeded per slot, not from the pass's, so a batch equals the per-scene path's whenever no slot is cropped (always,
    at the shipped data.max_num_point) and is a different, equally valid crop otherwise.

    label_free (default: split == "test"; True on another split is the reference's general.task == "test") takes the `else:`
    branch of the reference's `__getitem__` (pipeline.py:320-380): a batch is `scene_prep.prepare_points_store`'s seven keys plus,
    with an index, the description keys of `lang_prep._launch(..., boxes=None)` -- no label key, no draw for the scene, nothing read
    from the store's label arrays (a labels=False store serves).  shuffle then defaults to False; is_augment=True raises
    ValueError; `fused` and `fused_active()` do not bear on it."""

    def __init__(self, cfg, store, index, split, mode, rank=0, world=1, seed=None, shuffle=None, is_augment=False, mean_size_arr=None,
                 noise="device", device=None, scene_ids=None, fused=False, label_free=None, fused_elastic=False):
        self.cfg, self.store, self.index, self.split, self.mode = cfg, store, index, split, mode
        self.rank, self.world = int(rank), int(world)
        self.seed = int(cfg.general.manual_seed if seed is None else seed)
        self.label_free = (split == "test") if label_free is None else bool(label_free)
        if self.label_free and is_augment:
            raise ValueError("PipelineLoader: label_free batches are never augmented (pipeline.py:352-380 draws nothing)")
        self.shuffle = (split == "train" and not self.label_free) if shuffle is None else bool(shuffle)
        self.is_augment, self.noise, self.device = bool(is_augment), noise, device
        self.batch_size, self.voxel_mode = int(cfg.data.batch_size), int(_opt(cfg.data, "mode", 4) or 4)
        self.apply_word_erase = bool(_opt(_opt(cfg, "train", None), "apply_word_erase", True))
        self.mean_size_arr = mean_size_arr
        self.fused, self._mean_size_dev = bool(fused), None
        self.fused_elastic = bool(fused_elastic)
        self.scene_ids = list(store.scene_ids if scene_ids is None else scene_ids) if index is None else None
        self._next_epoch = 0
        self.last_order = None
        missing = sorted({self.sample_scene(i) for i in range(self.num_samples())} - set(store.scene_ids))
        if missing:
            raise ValueError("PipelineLoader: %d scenes are not in the store (%s ...)" % (len(missing), missing[0]))

    def num_samples(self):
        return len(self.index) if self.index is not None else len(self.scene_ids)

    def sample_scene(self, i):
        return self.index.scene_id(i) if self.index is not None else self.scene_ids[i]

    def set_epoch(self, epoch):
        self._next_epoch = int(epoch)

    def order(self, epoch):
        """this rank's sample indices of `epoch`"""
        return sampler_indices(self.num_samples(), self.world, self.rank, self.shuffle, self.seed, epoch)

    def generators(self, epoch):
        """the pass's (numpy RandomState, random.Random), seeded from (seed, epoch, rank)"""
        return (np.random.RandomState([self.seed & 0xFFFFFFFF, int(epoch), self.rank]),
                random.Random("%d/%d/%d" % (self.seed, int(epoch), self.rank)))

    def __len__(self):
        per_rank = (self.num_samples() + self.world - 1) // self.world
        return (per_rank + self.batch_size - 1) // self.batch_size

    def _store_on(self, device=None):
        """whether the store is resident on the loader's device (`device`, else the loader's, else the current one)"""
        dev = self.device if device is None else device
        dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
        return dev.type == "cuda" and dev.index in (None, self.store.points.device.index)

    def fused_active(self, device=None):
        """whether `build` takes `scene_prep.prepare_batch_store` (a host predicate)"""
        return (self.fused and self.noise != "host" and scene_prep.fused_applicable(self.cfg, self.is_augment, self.store)
                and self._store_on(device))

    def fused_elastic_active(self, device=None):
        """whether `build` takes `scene_prep.prepare_batch_store_elastic` (a host predicate): fused and fused_elastic are set,
        the elastic distortion and crop run (is_augment in the detector-only configuration), noise is "device", and the store is
        resident on the loader's device"""
        return (self.fused and self.fused_elastic and self.noise == "device" and not self.label_free
                and scene_prep.elastic_applicable(self.cfg, self.is_augment, self.store) and self._store_on(device))

    def mean_sizes(self):
        """`mean_size_arr` as the float64 tensor on the store's device the store paths take, uploaded once"""
        dev = self.store.points.device
        if self._mean_size_dev is None or self._mean_size_dev.device != dev:
            self._mean_size_dev = scene_prep._mean_sizes_on(self.mean_size_arr, dev, "PipelineLoader")
        return self._mean_size_dev

    def _scene_half(self, rng, dev):
        """The scene-half strategy of `build` -> (draw, batch_of): `draw(scene_id)` runs per sample, right after that sample's
        description draws, and takes the scene's draws from `rng` (None: the path draws nothing); `batch_of(scene_ids, results)`
        turns the per-sample results into the scene batch."""
        cfg, store, mode, P = self.cfg, self.store, self.voxel_mode, scene_prep
        if self.label_free:
            return None, lambda sids, _: P.prepare_points_store(store, sids, cfg, device=dev, mode=mode)
        if self.fused_active(dev):
            draw = (lambda sid: P.augment_matrix(rng, cfg.data.transform)) if self.is_augment else None
            return draw, lambda sids, mats: P.prepare_batch_store(store, sids, cfg, self.mean_sizes(), is_augment=self.is_augment, device=dev,
                                                                  mode=mode, matrices=mats)
        if self.fused_elastic_active(dev):
            draw = lambda sid: (P.augment_matrix(rng, cfg.data.transform), int(rng.randint(0, 2 ** 31 - 1)))
            return draw, lambda sids, draws: P.prepare_batch_store_elastic(store, sids, cfg, self.mean_sizes(), device=dev, mode=mode, draws=draws)
        draw = lambda sid: P.prepare_scene(store.scene(sid), cfg, self.mean_size_arr, rng=rng, is_augment=self.is_augment, noise=self.noise,
                                           device=dev)
        return draw, lambda sids, samples: P.collate_scenes_device(samples, dev, mode)

    def build(self, idxs, rng, pyrng):
        """one batch of the samples `idxs`"""
        index = self.index
        dev = torch.device("cuda", torch.cuda.current_device()) if self.device is None else torch.device(self.device)
        if index is not None:
            dev = lang_prep._device(index, dev)
        draw, batch_of = self._scene_half(rng, dev)
        sids = [self.sample_scene(i) for i in idxs]
        descr, scene = [], None if draw is None else []
        for c, sid in zip(idxs, sids):                     # per sample: the description draws, then the scene's (pipeline.py:91-, :145-)
            if index is not None:
                descr.append(lang_prep.draw_descriptions(index, c, rng, pyrng, self.is_augment, self.apply_word_erase))
            if draw is not None:
                scene.append(draw(sid))
        batch = batch_of(sids, scene)
        if index is not None:
            batch.update(lang_prep._launch(index, descr, idxs, None if self.label_free else batch, dev))
        return batch

    def __iter__(self):
        epoch = self._next_epoch
        self._next_epoch = epoch + 1
        order = self.last_order = self.order(epoch)
        return self._batches(order, *self.generators(epoch))

    def _batches(self, order, rng, pyrng):
        for i in range(0, len(order), self.batch_size):
            yield self.build(order[i:i + self.batch_size], rng, pyrng)


class PairedLoader:
    """The joint mode's training source: `[speaker batch, listener batch]` pairs over the LONGER of the sources, the shorter one
    restarted when it runs out.  This is what Lightning does with a list of training loaders, `CombinedLoader(mode=
    "max_size_cycle")` (its default for `train_dataloaders=[a, b]`, scripts/train.py:360-365): the epoch has max(len) batches and
    a `CycleIterator` re-creates the exhausted loader's iterator.  The restarted pass repeats the epoch's order, as a
    `DistributedSampler` whose epoch Lightning set once per epoch does."""

    def __init__(self, *sources):
        self.sources = list(sources)
        self._epoch = None

    def __len__(self):
        return max(len(s) for s in self.sources)

    def set_epoch(self, epoch):
        self._epoch = int(epoch)
        for s in self.sources:
            if hasattr(s, "set_epoch"):
                s.set_epoch(epoch)

    def __iter__(self):
        epoch = self._epoch
        its = [iter(s) for s in self.sources]
        for _ in range(len(self)):
            pair = []
            for k, s in enumerate(self.sources):
                try:
                    b = next(its[k])
                except StopIteration:
                    if epoch is not None and hasattr(s, "set_epoch"):
                        s.set_epoch(epoch)
                    its[k] = iter(s)
                    b = next(its[k])
                pair.append(b)
            yield pair
        if epoch is not None:
            self._epoch = epoch + 1


# ------------------------------------------------------------------------------------------------ a configuration's sources
def load_vocabulary(cfg, name):
    """`_build_vocabulary` (pipeline.py:433-502) -> (vocabulary, glove (V,300)): the vocabulary json of `<NAME>_PATH.vocabulary`
    (with the special-token entry the reference patches in), the trimmed GloVe table of `glove_numpy`, or -- as the reference --
    built from `glove_pickle` and saved there when that file is missing"""
    paths = cfg["%s_PATH" % name.upper()]
    if not os.path.exists(paths.vocabulary):
        raise FileNotFoundError("no vocabulary at %s (the reference builds it on its first training run)" % paths.vocabulary)
    vocabulary = json.load(open(paths.vocabulary))
    vocabulary.setdefault("special_tokens", {"bos_token": "sos", "eos_token": "eos", "unk_token": "unk", "pad_token": "pad_"})
    if os.path.exists(paths.glove_numpy):
        glove = np.load(paths.glove_numpy)
    else:
        all_glove = pickle.load(open(paths.glove_pickle, "rb"))
        glove = np.zeros((len(vocabulary["word2idx"]), 300))
        for word, idx in vocabulary["word2idx"].items():
            glove[int(idx)] = all_glove[word] if word in all_glove else all_glove["unk"]
        np.save(paths.glove_numpy, glove)
    return vocabulary, glove


def _namespace(index, vocabulary, glove):
    """the `dataset` object PipelineNet reads (train.py:synthetic_dataset's shape)"""
    raw = index.raw_data
    return types.SimpleNamespace(vocabulary=vocabulary, glove=glove, raw_data=raw, organized=organize(raw),
                                 chunked_data=[[raw[n] for n in chunk] for chunk in index.chunks])


def build_loaders(cfg, device, rank=0, world=1, multiview=None, store_device=None, fused=False, augment=False):
    """`init_data` (scripts/train.py:220-245) with its `init_detector_data` / `init_speaker_data` / `init_listener_data` and the
    loader choice of `start_training` (:338-365) -> (training source, validation source(s), dataset, stores):

      mode 0   PipelineLoader over the scans of SCANNETV2_PATH.train_list / val_list, one scene per sample;
      mode 1   the speaker's: <DATASET>_PATH.train_split (plus the data.extra_ratio SYNTHETIC fill and shuffle, under
               random.Random(general.manual_seed)), validation = one entry per validation scene (`speaker_val_entries`);
      mode 2   the listener's: train_split and the full val_split;
      mode 3   PairedLoader(speaker, listener) and the pair of validation sources.

    Training sources shuffle, validation sources do not; both are sharded over `world` ranks (Lightning's DistributedSampler).
    dataset: {"train", "val"} namespaces with vocabulary, glove, chunked_data, organized, raw_data -- the speaker's when there
    is one (scripts/train.py:284), else the listener's, None in mode 0.  stores: {"train", "val"} SceneStores on `store_device`
    (default `device`), one per split, shared by the split's loaders.  fused: every loader's `fused=` (`PipelineLoader`).
    augment: the TRAINING loaders' `is_augment=` (the reference dataset's own switch, which scripts/train.py leaves off); they then
    also get `fused_elastic=fused`.  Validation loaders are never augmented."""
    m = cfg.model
    if m.no_detection:
        raise NotImplementedError("GT-proposal modes 4-6 (no_detection) are not on the hot path")
    if m.no_captioning and m.no_grounding and m.no_detection:
        raise ValueError("invalid mode: detection, captioning and grounding are all off")
    device = torch.device(device)
    store_device = device if store_device is None else torch.device(store_device)
    seed = int(cfg.general.manual_seed)
    means = np.load(os.path.join(cfg.SCANNETV2_PATH.meta_data, "scannet_reference_means.npz"))["arr_0"]
    lists = {}                                             # (role, split) -> (raw_data, scan list)
    if m.no_captioning and m.no_grounding:
        for split, key in (("train", "train_list"), ("val", "val_list")):
            scans = read_scan_list(cfg.SCANNETV2_PATH[key])
            lists[("detector", split)] = (detector_entries(scans), scans)
    else:
        paths = cfg["%s_PATH" % cfg.general.dataset.upper()]
        raw_train, raw_val = json.load(open(paths.train_split)), json.load(open(paths.val_split))
        if not m.no_captioning:
            all_scans = read_scan_list(cfg.SCANNETV2_PATH.train_list) if cfg.data.extra_ratio > 0 else []
            lists[("speaker", "train")] = speaker_train_entries(raw_train, all_scans, cfg.data.extra_ratio, random.Random(seed))
            val = speaker_val_entries(raw_val)
            lists[("speaker", "val")] = (val, scan_list_of(raw_val))
        if not m.no_grounding:
            lists[("listener", "train")] = (copy.deepcopy(raw_train), scan_list_of(raw_train))
            lists[("listener", "val")] = (copy.deepcopy(raw_val), scan_list_of(raw_val))

    stores = {}
    for split in ("train", "val"):
        scans = []
        for (role, sp), (_raw, lst) in lists.items():
            scans += [s for s in lst if sp == split and s not in scans]
        stores[split] = SceneStore.load(cfg, split, scans, store_device, multiview)

    loaders, indexes = {}, {}
    loader = lambda index, split, role, **kw: PipelineLoader(cfg, stores[split], index, split, role, rank, world, seed, mean_size_arr=means,
                                                             device=device, fused=fused, is_augment=bool(augment) and split == "train",
                                                             fused_elastic=bool(augment) and bool(fused) and split == "train", **kw)
    if ("detector", "train") in lists:
        for split in ("train", "val"):
            loaders[("detector", split)] = loader(None, split, "detector", scene_ids=lists[("detector", split)][1])
        return loaders[("detector", "train")], loaders[("detector", "val")], None, stores
    vocabulary, glove = load_vocabulary(cfg, cfg.general.dataset)
    raw2label = lang_prep.raw2label_from_tsv(cfg.SCANNETV2_PATH.combine_file)
    scan2cad = json.load(open(cfg.SCAN2CAD)) if os.path.exists(cfg.SCAN2CAD) else None
    for (role, split), (raw, _lst) in lists.items():
        max_len = cfg.data.max_spk_len if role == "speaker" else cfg.data.max_lis_len
        indexes[(role, split)] = lang_prep.DescriptionIndex(raw, vocabulary, glove, max_len, cfg.data.num_des_per_scene, raw2label,
                                                            scan2cad_rotation=scan2cad, split=split, device=device)
        loaders[(role, split)] = loader(indexes[(role, split)], split, role)
    role = "listener" if m.no_captioning else "speaker"
    dataset = {split: _namespace(indexes[(role, split)], vocabulary, glove) for split in ("train", "val")}
    if m.no_captioning or m.no_grounding:
        return loaders[(role, "train")], loaders[(role, "val")], dataset, stores
    return (PairedLoader(loaders[("speaker", "train")], loaders[("listener", "train")]),
            (loaders[("speaker", "val")], loaders[("listener", "val")]), dataset, stores)


def prediction_entries(raw, split, task):
    """the annotation list of a prediction run -> (entries, scan list).  captioning on the test split: one copy of raw[0] per
    scene (benchmark/benchmark_captioning.py:66-72, `speaker_val_entries`); every other case the full list
    (benchmark_captioning.py:75-81 for the other splits, benchmark/benchmark_grounding.py:62-69)"""
    if task not in ("captioning", "grounding"):
        raise ValueError("task must be 'captioning' or 'grounding', not %r" % (task,))
    entries = speaker_val_entries(raw) if (task == "captioning" and split == "test") else copy.deepcopy(raw)
    return entries, scan_list_of(raw)


def build_test_loader(cfg, device, task, split="test", rank=0, world=1, multiview=None, store_device=None):
    """`init_data` of benchmark/benchmark_captioning.py:49-104 (task="captioning": the speaker's role and max_spk_len) and of
    benchmark/benchmark_grounding.py:45-92 (task="grounding": the listener's role and max_lis_len, no Scan2CAD table), for `split`
    alone -> (loader, dataset, store):

      loader   a label-free `PipelineLoader` over `prediction_entries` of <DATASET>_PATH.<split>_split, unshuffled;
      dataset  {"train": a namespace with vocabulary and glove only, split: the split's `_namespace`} -- what `PipelineNet(cfg,
               dataset)` and the submission's `chunked_data` need; the training split's scenes are not loaded;
      store    `SceneStore.load(cfg, split, scans, labels=False)` on `store_device` (default `device`).

    cfg.data.num_des_per_scene is read as it stands: the scripts' own overrides (8 / 1) are `predict.main`'s to apply."""
    device = torch.device(device)
    store_device = device if store_device is None else torch.device(store_device)
    paths = cfg["%s_PATH" % cfg.general.dataset.upper()]
    raw = json.load(open(paths["%s_split" % split]))
    entries, scans = prediction_entries(raw, split, task)
    store = SceneStore.load(cfg, split, scans, store_device, multiview, labels=False)
    vocabulary, glove = load_vocabulary(cfg, cfg.general.dataset)
    raw2label = lang_prep.raw2label_from_tsv(cfg.SCANNETV2_PATH.combine_file)
    scan2cad = json.load(open(cfg.SCAN2CAD)) if task == "captioning" and os.path.exists(cfg.SCAN2CAD) else None
    role, max_len = ("speaker", cfg.data.max_spk_len) if task == "captioning" else ("listener", cfg.data.max_lis_len)
    index = lang_prep.DescriptionIndex(entries, vocabulary, glove, max_len, cfg.data.num_des_per_scene, raw2label, scan2cad_rotation=scan2cad,
                                       split=split, device=device)
    loader = PipelineLoader(cfg, store, index, split, role, rank, world, int(cfg.general.manual_seed), device=device, label_free=True)
    dataset = {"train": types.SimpleNamespace(vocabulary=vocabulary, glove=glove)}
    dataset[split] = _namespace(index, vocabulary, glove)
    return loader, dataset, store
