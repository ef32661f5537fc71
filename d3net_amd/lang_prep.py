"""Description batches on the device: the description half of the reference's `PipelineDataset.__getitem__`
(lib/dataset/pipeline.py:69-138 language features, :250-264 Scan2CAD rotations, :267-278 grounding targets, :282-318 keys) and
their stacking by `sparse_collate_fn`, from ScanRefer / ReferIt3D annotations in the reference's own dict formats.

`DescriptionIndex` is built once per split.  It restates the reference's `_load` bookkeeping on the host -- `_tranform_des`
(:504-552, token ids only), `_get_chunked_data` / `_chunks` (:583-604), `_get_unique_multiple_lookup` (:626-677), the
`object_cat` lookup (:98-100) -- and keeps on the device the token table (Nd, L) int32, the capped lengths (Nd,), the GloVe table
cast once to float32 (V, D) and the Scan2CAD rotation table.  A step then sends one row index per description and the few erased
positions; the embedding rows are gathered by csrc/lang_prep.hip (`d3_lang_features`), the grounding and rotation targets come
from the stacked box labels (`d3_ref_targets`).  The reference instead keeps an (L, 300) float64 array per description on the
host, deep-copies a chunk of them per scene and ships B*C*L*300 floats per step.

Random draws follow the reference: per real description one `pyrng.random()` when `is_augment` (the reference's `and` chain
draws it even when word erase is off, :108), and on a draw below 0.5 with erase on, one
`rng.choice(list(range(1, lang_len - 2)), int((lang_len - 2) * 0.2), replace=False)` (:554-557).
"""
import ctypes as C
import random

import numpy as np
import torch

from . import _lib, scene_prep
from ._call import _ptr, _stream, call

SCANNET_CLASSES = ("cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture", "counter", "desk", "curtain",
                   "refrigerator", "shower curtain", "toilet", "sink", "bathtub", "others")
_META = ("annotated", "chunk_ids", "object_id", "ann_id", "object_cat", "unique_multiple")


def raw2label_from_tsv(path, class_names=SCANNET_CLASSES):
    """`_get_raw2label` (pipeline.py:606-624): raw category name (column 1 of a scannetv2-labels.combined.tsv-format file) -> index
    of its nyu40class (column 7) among the 18 class names, or the index of "others"."""
    label = {name: i for i, name in enumerate(class_names)}
    lines = [line.rstrip() for line in open(path)][1:]
    out = {}
    for line in lines:
        e = line.split("\t")
        out[e[1]] = label[e[7]] if e[7] in label else label["others"]
    return out


def _object_name(d):
    return " ".join(d["object_name"].split("_"))


class DescriptionIndex:
    """The annotations of one split.  raw_data: list of {scene_id, object_id, object_name, ann_id, token} (object_id "SYNTHETIC" marks
    a description-less scene entry); vocabulary: {"word2idx", "idx2word", "special_tokens"}; glove: (V, D) array indexed by word
    id; raw2label: raw object name -> class (`raw2label_from_tsv`); scan2cad_rotation: {scene_id: {str(instance id): 3x3}} or None.

    Host attributes, all in the reference's iteration orders: `chunks` (list of lists of raw_data indices = `chunked_data`),
    per raw_data entry `row` (-1 SYNTHETIC), `lang_len`, `object_id`, `ann_id`, `object_cat`, `unique_multiple`; `token_ids`
    (Nd, L) and `token_len` (Nd,) are the host copies of the device tables `tokens` / `lens`; `glove` (V, D) float32 on the device.

    Two entries with the same (scene_id, object_id, ann_id) but different tokens raise ValueError: the reference would silently
    give both the later entry's features with each one's own length.  A token id outside [0, V) raises ValueError."""

    def __init__(self, raw_data, vocabulary, glove, max_des_len, num_des_per_scene, raw2label, scan2cad_rotation=None, split="train",
                 device=None):
        self.raw_data, self.vocabulary, self.raw2label = raw_data, vocabulary, raw2label
        self.max_des_len, self.chunk_size, self.split = int(max_des_len), int(num_des_per_scene), split
        self.L = L = self.max_des_len + 2
        w2i = vocabulary["word2idx"]
        glove_host = np.ascontiguousarray(np.asarray(glove), dtype=np.float32)
        self.V, self.D = glove_host.shape
        self.unk = int(w2i["unk"])

        # _tranform_des, ids only
        key_row, rows_tok, rows_len = {}, [], []
        self.row = np.full(len(raw_data), -1, np.int64)
        self.lang_len = np.zeros(len(raw_data), np.int64)
        for n, d in enumerate(raw_data):
            if d["object_id"] == "SYNTHETIC":
                continue
            words = ["sos"] + list(d["token"][:self.max_des_len]) + ["eos"]
            ids = [int(w2i[w if w in w2i else "unk"]) for w in words]
            key = (d["scene_id"], d["object_id"], d["ann_id"])
            if key in key_row:
                if rows_tok[key_row[key]] != ids or rows_len[key_row[key]] != min(len(d["token"]) + 2, L):
                    raise ValueError("two descriptions share scene / object / annotation id %s" % (key,))
            else:
                key_row[key] = len(rows_tok)
                rows_tok.append(ids)
                rows_len.append(min(len(d["token"]) + 2, L))
            self.row[n] = key_row[key]
            self.lang_len[n] = rows_len[key_row[key]]
        self.Nd = len(rows_tok)
        self.token_ids = np.zeros((self.Nd, L), np.int32)
        for r, ids in enumerate(rows_tok):
            self.token_ids[r, :len(ids)] = ids
        self.token_len = np.asarray(rows_len, np.int32).reshape(self.Nd)
        if self.Nd and (self.token_ids.min() < 0 or self.token_ids.max() >= self.V) or not 0 <= self.unk < self.V:
            raise ValueError("a token id lies outside the GloVe table's %d rows" % self.V)

        # _get_chunked_data / _chunks
        by_scene = {}
        for n, d in enumerate(raw_data):
            by_scene.setdefault(d["scene_id"], []).append(n)
        self.chunks = [lst[i:i + self.chunk_size] for lst in by_scene.values() for i in range(0, len(lst), self.chunk_size)]

        # object_cat and _get_unique_multiple_lookup (SYNTHETIC entries count as one more object of class 17, as in the reference)
        cat = np.array([raw2label.get(_object_name(d), 17) for d in raw_data], np.int64)
        scene_labels, seen = {}, set()
        for n, d in enumerate(raw_data):
            scene_labels.setdefault(d["scene_id"], [])
            if (d["scene_id"], d["object_id"]) not in seen:
                seen.add((d["scene_id"], d["object_id"]))
                scene_labels[d["scene_id"]].append(cat[n])
        um = {}
        for n, d in enumerate(raw_data):                   # a later entry with the same key overwrites the flag for all of them
            um[(d["scene_id"], d["object_id"], d["ann_id"])] = 0 if scene_labels[d["scene_id"]].count(cat[n]) == 1 else 1
        self.object_cat = cat
        self.unique_multiple = np.array([um[(d["scene_id"], d["object_id"], d["ann_id"])] for d in raw_data], np.int64)
        synth = self.row < 0
        self.object_id = np.array([-1 if s else int(d["object_id"]) for s, d in zip(synth, raw_data)], np.int64)
        self.ann_id = np.array([-1 if s else int(d["ann_id"]) for s, d in zip(synth, raw_data)], np.int64)

        # Scan2CAD rotations: per scene its instance ids and matrices
        self.rot_scene, off, ids, mats = {}, [0], [], []
        for sid, table in (scan2cad_rotation or {}).items():
            self.rot_scene[sid] = len(off) - 1
            for k, m in table.items():
                ids.append(int(k))
                mats.append(np.asarray(m, dtype=np.float64).reshape(3, 3))
            off.append(len(ids))
        self.rot_off = np.asarray(off, np.int32)
        self.rot_ids = np.asarray(ids, np.int32).reshape(len(ids))
        self.rot_mats = np.asarray(mats, np.float64).reshape(len(ids), 3, 3).astype(np.float32)

        self.device = None
        self._glove_host = glove_host
        if device is not None:
            self.to(device)

    def to(self, device):
        """upload the tables (once)"""
        self.device = torch.device(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.tokens, self.lens, self.glove = up(self.token_ids), up(self.token_len), up(self._glove_host)
        self.rot_off_d, self.rot_ids_d, self.rot_mats_d = up(self.rot_off), up(self.rot_ids), up(self.rot_mats)
        return self

    def __len__(self):
        return len(self.chunks)

    def scene_id(self, chunk_idx):
        return self.raw_data[self.chunks[chunk_idx][0]]["scene_id"]

    def table_bytes(self):
        """(bytes of the token, length and GloVe tables kept here, bytes of the reference's per-description (L, 300) float64
        feature and (L,) float64 id arrays)"""
        return (self.token_ids.nbytes + self.token_len.nbytes + self._glove_host.nbytes, self.Nd * self.L * (self.D + 1) * 8)


def draw_descriptions(index, chunk_idx, rng=None, pyrng=None, is_augment=False, apply_word_erase=True):
    """The host part of one sample (pipeline.py:91-138): the slots' description rows, erased positions and label scalars, with the
    reference's draws.  -> dict: rows (C,) int32, erase (list of C int arrays), lang_len (C,) and the `_META` keys (C,) int64.
    Slots past the chunk's size repeat the last filled slot and take no draws.  Raises ValueError where the reference fails: a
    description picked for erasing (augmented, draw < 0.5, erase on) whose capped length leaves no candidate position, i.e. fewer
    than two tokens after trimming (the reference's empty float index array raises IndexError at :563)."""
    rng = np.random if rng is None else rng
    pyrng = random if pyrng is None else pyrng
    chunk, Cn = index.chunks[chunk_idx], index.chunk_size
    rows = np.full(Cn, -1, np.int32)
    erase = [np.zeros(0, np.int32)] * Cn
    out = {k: np.zeros(Cn, np.int64) for k in _META + ("lang_len",)}
    for i in range(Cn):
        if i >= len(chunk):                                # the last sample repeats (:127-138)
            rows[i], erase[i] = rows[i - 1], erase[i - 1]
            for k in out:
                out[k][i] = out[k][i - 1]
            continue
        n = chunk[i]
        out["chunk_ids"][i] = i
        out["object_id"][i], out["ann_id"][i] = index.object_id[n], index.ann_id[n]
        if index.row[n] < 0:
            out["object_cat"][i] = 17
            continue
        rows[i] = index.row[n]
        ll = int(index.lang_len[n])
        out["annotated"][i], out["lang_len"][i] = 1, ll
        out["object_cat"][i], out["unique_multiple"][i] = index.object_cat[n], index.unique_multiple[n]
        if is_augment and pyrng.random() < 0.5 and apply_word_erase:
            if ll - 2 < 2:
                raise ValueError("word erase on a description of fewer than two tokens (raw_data[%d])" % n)
            erase[i] = np.asarray(rng.choice(list(range(1, ll - 2)), int((ll - 2) * 0.2), replace=False), np.int32).reshape(-1)
    out["rows"], out["erase"] = rows, erase
    return out


def _launch(index, draws, chunk_idxs, boxes, device):
    L_, Cn, B = index.L, index.chunk_size, len(draws)
    lib, st = _lib.lib(), _stream()
    S = B * Cn
    rows = np.ascontiguousarray(np.concatenate([d["rows"] for d in draws]), dtype=np.int32)
    lists = [e for d in draws for e in d["erase"]]
    eptr = np.zeros(S + 1, np.int32)
    eptr[1:] = np.cumsum([len(e) for e in lists])
    epos = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), dtype=np.int32)
    feat = torch.empty((B, Cn, L_, index.D), dtype=torch.float32, device=device)
    ids = torch.empty((B, Cn, L_), dtype=torch.int64, device=device)
    lens = torch.empty((B, Cn), dtype=torch.int64, device=device)
    ws = torch.empty(max(int(lib.d3_lang_features_ws_bytes(S, len(epos))), 1), dtype=torch.uint8, device=device)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    call("lang_features", _ptr(index.tokens), _ptr(index.lens), index.Nd, _ptr(index.glove), index.V, index.D, L_, index.unk,
         hp(rows), hp(eptr), hp(epos), S, _ptr(feat), _ptr(ids), _ptr(lens), _ptr(ws), ws.numel(), st)
    meta = torch.from_numpy(np.stack([np.stack([d[k] for d in draws]) for k in _META])).to(device)
    out = {k: meta[i] for i, k in enumerate(_META)}
    out.update(lang_feat=feat, lang_len=lens, lang_ids=ids,
               id=torch.tensor([int(c) for c in chunk_idxs], dtype=torch.int64, device=device),
               istrain=torch.full((B,), 1 if index.split == "train" else 0, dtype=torch.int64, device=device),
               scene_id=[index.scene_id(c) for c in chunk_idxs])
    if boxes is None:
        return out
    gid, glab, gbox = (boxes[k].contiguous() for k in ("gt_bbox_object_id", "gt_bbox_label", "gt_bbox"))
    R = gid.shape[1]
    if gid.dtype != torch.int64 or glab.dtype != torch.int64 or gbox.dtype != torch.float32 or gbox.shape != (B, R, 8, 3):
        raise ValueError("boxes: gt_bbox_object_id / gt_bbox_label (B,R) int64 and gt_bbox (B,R,8,3) float32 expected")
    scene = np.array([index.rot_scene.get(s, -1) for s in out["scene_id"]], np.int32).reshape(B)
    ref = torch.empty((B, Cn, R), dtype=torch.int64, device=device)
    corner = torch.empty((B, Cn, 8, 3), dtype=torch.float32, device=device)
    rots = torch.empty((B, R, 3, 3), dtype=torch.float32, device=device)
    masks = torch.empty((B, R), dtype=torch.int64, device=device)
    ws2 = torch.empty(max(int(lib.d3_ref_targets_ws_bytes(B)), 1), dtype=torch.uint8, device=device)
    Ns = len(index.rot_off) - 1
    call("ref_targets", _ptr(gid), _ptr(glab), _ptr(gbox), _ptr(out["object_id"]), B, Cn, R,
         _ptr(index.rot_off_d) if Ns else None, _ptr(index.rot_ids_d) if Ns else None,
         _ptr(index.rot_mats_d) if Ns else None, Ns, hp(scene), _ptr(ref), _ptr(corner), _ptr(rots), _ptr(masks),
         _ptr(ws2), ws2.numel(), st)
    out.update(ref_box_label=ref, ref_box_corner_label=corner, scene_object_ids=gid, scene_object_rotations=rots,
               scene_object_rotation_masks=masks)
    index._host_args = (rows, eptr, epos, scene)          # the entry points' host arrays stay referenced until the next batch
    return out


def _device(index, device):
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if index.device != device:
        index.to(device)
    return device


def prepare_descriptions(index, chunk_idxs, boxes=None, rng=None, pyrng=None, is_augment=False, apply_word_erase=True, device=None):
    """The description-half keys of pipeline.py:282-318 for the samples `chunk_idxs` (indices into `index.chunks`), stacked over
    the batch as device tensors with the reference's dtypes: lang_feat (B,C,L,D) float32, lang_len (B,C), lang_ids (B,C,L),
    annotated, chunk_ids, object_id, ann_id, object_cat, unique_multiple (B,C) int64, id, istrain (B,) int64 and the list scene_id.

    boxes: the stacked gt_bbox_object_id, gt_bbox_label (B,R) int64 and gt_bbox (B,R,8,3) float32 of the same scenes
    (`scene_prep.collate_scenes`) -> also ref_box_label (B,C,R) int64, ref_box_corner_label (B,C,8,3) float32, scene_object_ids,
    scene_object_rotations (B,R,3,3) float32 and scene_object_rotation_masks (B,R) int64.  boxes=None is the test-split branch
    (:320-380), which has no targets (and, with the default is_augment=False, no draws).

    rng: numpy RandomState, pyrng: random.Random; None = the global generators, as in the reference's loader.  Draws and the
    ValueError of a too-short description: see `draw_descriptions`."""
    device = _device(index, device)
    draws = [draw_descriptions(index, c, rng, pyrng, is_augment, apply_word_erase) for c in chunk_idxs]
    return _launch(index, draws, chunk_idxs, boxes, device)


def prepare_pipeline_batch(index, chunk_idxs, scenes, cfg, mean_size_arr, rng=None, pyrng=None, is_augment=True, apply_word_erase=True,
                           noise="device", device=None, mode=4):
    """The full training batch of `sparse_collate_fn` over `PipelineDataset.__getitem__` for the samples `chunk_idxs`.  scenes:
    {scene_id: raw scene dict of `scene_prep.prepare_scene`}.  Per sample, in the reference's order: the description draws
    (:91-138), then the scene (`scene_prep.prepare_scene`, :145 on); then one `collate_scenes`, one `d3_lang_features` and one
    `d3_ref_targets` for the whole batch."""
    device = _device(index, device)
    draws, samples = [], []
    for c in chunk_idxs:
        draws.append(draw_descriptions(index, c, rng, pyrng, is_augment, apply_word_erase))
        samples.append(scene_prep.prepare_scene(scenes[index.scene_id(c)], cfg, mean_size_arr, rng=rng, is_augment=is_augment,
                                                noise=noise, device=device))
    batch = scene_prep.collate_scenes(samples, device, mode)
    batch.update(_launch(index, draws, chunk_idxs, batch, device))
    return batch
