#!/usr/bin/env python3
"""Generates tests/golden/lang_prep_golden.npz (and the label fixture lang_prep_labels.tsv next to it) by RUNNING THE REFERENCE's
own description pipeline: PipelineDataset._tranform_des, _get_chunked_data, _get_unique_multiple_lookup, _get_raw2label and
__getitem__ (lib/dataset/pipeline.py) on an instance made without __init__, followed by its sparse_collate_fn, on synthetic
annotations, under random.seed(s) and np.random.seed(s).  The captioning config keeps the elastic distortion and the crop off.  The
modules this path never calls (h5py, MinkowskiEngine(.utils), lib.pointgroup_ops.functions, plyfile, trimesh, matplotlib) are
placeholders; the collate's voxelisation call is a placeholder too and its three outputs are not stored.  Asserts that the
annotations contain the cases (a)-(j) listed at `check_cases`.  Run where the reference is available."""
import copy
import importlib
import json
import os
import random
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SEED = 5
MAX_DES_LEN, CHUNK, R = 6, 4, 128
SA, SB = "scene0000_00", "scene0001_00"

TSV_HEADER = ["id", "raw_category", "category", "count", "nyu40id", "eigen13id", "nyuClass", "nyu40class", "eigen13class"]
TSV_ROWS = [(1, "chair", 5, "chair"), (2, "office chair", 5, "chair"), (3, "table", 7, "table"), (4, "sofa", 6, "sofa"),
            (5, "bed", 4, "bed"), (6, "cabinet", 3, "cabinet"), (7, "trash can", 39, "otherfurniture")]


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _import_reference():
    for name in ("h5py", "plyfile", "trimesh", "matplotlib", "matplotlib.pyplot", "lib.pointgroup_ops", "lib.pointgroup_ops.functions"):
        _stub(name, PlyData=None, PlyElement=None, pointgroup_ops=None)
    _stub("MinkowskiEngine")
    _stub("MinkowskiEngine.utils", batched_coordinates=None)
    try:
        importlib.import_module("tqdm")
    except ImportError:
        _stub("tqdm", tqdm=lambda x, *a, **k: x)
    sys.path.insert(0, REF)
    from lib.dataset import pipeline
    from data.scannet.model_util_scannet import ScannetDatasetConfig
    return pipeline, ScannetDatasetConfig


def ns(**kw):
    return types.SimpleNamespace(**kw)


def make_scene(seed, n=600, n_inst=6, extent=(4.0, 3.0, 2.0), unlabelled=True):
    """a small scene in the manner of gen_scene_prep_golden.make_scene: blob instances, id 3 absent"""
    r = np.random.RandomState(seed)
    pts = (r.rand(n, 3) * np.array(extent)).astype(np.float32)
    ids = np.full(n, -1, np.int64)
    sem = r.randint(0, 20, size=n).astype(np.int64)
    sem[r.rand(n) < 0.05] = -1
    centers = r.rand(n_inst, 3) * np.array(extent) * 0.8 + 0.1 * np.array(extent)
    d = np.linalg.norm(pts[:, None, :] - centers[None], axis=2)
    near = d.argmin(1)
    lab = d.min(1) < (0.7 if unlabelled else 1e9)
    ids[lab] = np.array([k if k < 3 else k + 1 for k in range(n_inst)])[near[lab]]
    feats = r.rand(n, 3).astype(np.float32) * 2 - 1
    return dict(points=pts, feats=feats, sem_labels=sem, instance_ids=ids)


def make_vocabulary(n_words=36):
    words = ["pad_", "unk", "sos", "eos"] + ["w%d" % i for i in range(n_words)]
    return {"word2idx": {w: i for i, w in enumerate(words)}, "idx2word": {str(i): w for i, w in enumerate(words)},
            "special_tokens": {"bos_token": "sos", "eos_token": "eos", "unk_token": "unk", "pad_token": "pad_"}}


def make_raw_data():
    def e(scene, obj, name, ann, toks):
        return {"scene_id": scene, "object_id": str(obj), "object_name": name, "ann_id": str(ann), "token": toks}
    w = lambda *i: ["w%d" % k for k in i]
    return [
        e(SA, 0, "chair", 0, w(1, 2) + ["zzz"] + w(3, 4)),                # (d) a word outside the vocabulary
        e(SA, 1, "office_chair", 0, w(5, 6, 7, 8, 9, 10, 11, 12, 13)),    # (c) longer than max_des_len; (i) second chair
        e(SA, 2, "table", 0, w(14, 15, 16)),                              # (f) three tokens; (i) the only table
        e(SA, 2, "table", 1, w(17, 18, 19, 20, 21, 22)),
        e(SA, 9, "sofa", 0, w(23, 24, 25, 26, 27, 28)),                   # (g) no labelled box has id 9
        e(SA, 4, "lamp_thing", 0, w(29, 30)),                             # (f) two tokens; a name the label file lacks
        e(SB, 0, "bed", 0, w(31, 32, 33, 34, 35, 0)),
        {"scene_id": SB, "object_id": "SYNTHETIC", "object_name": "SYNTHETIC", "ann_id": "SYNTHETIC", "token": ["SYNTHETIC"]},   # (b)
        e(SB, 1, "cabinet", 0, w(1, 3, 5, 7)),
        e(SB, 2, "trash_can", 0, w(2, 4, 6, 8, 10)),
    ]


def make_rotations():
    r = np.random.RandomState(3)
    return {SA: {str(k): np.linalg.qr(r.randn(3, 3))[0].tolist() for k in (0, 2, 77)}}          # (j): SB has no table


def write_tsv(path):
    with open(path, "w") as f:
        f.write("\t".join(TSV_HEADER) + "\n")
        for i, raw, nyu, cls in TSV_ROWS:
            f.write("\t".join([str(i), raw, raw, "1", str(nyu), "0", cls, cls, "Objects"]) + "\n")


def make_dataset(P, DCcls, scenes, raw_data, vocabulary, glove, rotations, meta_dir, is_augment):
    cfg = ns(general=ns(task="train"), train=ns(apply_word_erase=True),
             SCANNETV2_PATH=ns(meta_data=meta_dir, combine_file=os.path.join(meta_dir, "scannetv2-labels.combined.tsv")),
             data=ns(scale=50, full_scale=[128, 512], max_num_point=250000, max_num_instance=R, requires_gt_mask=True,
                     requires_bbox=True, num_des_per_scene=CHUNK, transform=ns(jitter=True, flip=True, rot=True)),
             model=ns(no_detection=False, no_captioning=False, no_grounding=True))
    ds = object.__new__(P.PipelineDataset)
    ds.cfg, ds.split, ds.use_gt, ds.is_augment, ds.scan2cad_rotation, ds.raw_data = cfg, "train", False, is_augment, rotations, raw_data
    ds.DC = DCcls(cfg)
    ds.scale, ds.full_scale, ds.max_num_point, ds.max_des_len = 50, cfg.data.full_scale, cfg.data.max_num_point, MAX_DES_LEN
    ds.use_color, ds.use_multiview, ds.use_normal, ds.requires_bbox = True, False, False, True
    ds.scenes = {sid: {"aligned_mesh": np.concatenate([s["points"], s["feats"]], 1), "instance_ids": s["instance_ids"],
                       "sem_labels": s["sem_labels"]} for sid, s in scenes.items()}
    ds.vocabulary, ds.glove = vocabulary, glove
    ds.lang, ds.lang_ids = ds._tranform_des(MAX_DES_LEN)
    ds.chunk_size = CHUNK
    ds.chunked_data = ds._get_chunked_data(raw_data, CHUNK)
    ds.raw2label = ds._get_raw2label()
    ds.unique_multiple_lookup = ds._get_unique_multiple_lookup()
    return ds


def _peek():
    a, b = random.getstate(), np.random.get_state()
    out = (random.random(), np.random.rand())
    random.setstate(a)
    np.random.set_state(b)
    return out


def run_batch(P, ds, seed):
    random.seed(seed)
    np.random.seed(seed)
    samples, nxt = [], []
    for idx in range(len(ds)):
        samples.append(ds[idx])
        nxt.append(_peek())
    singles = copy.deepcopy(samples)                      # the collate shifts ids in place
    P.pointgroup_ops = ns(voxelization_idx=lambda *a: (np.zeros(0), np.zeros(0), np.zeros(0)))
    batch = P.sparse_collate_fn(samples)
    for k in ("voxel_locs", "p2v_map", "v2p_map"):
        batch.pop(k)
    return batch, singles, np.array(nxt, np.float64)


def check_cases(ds, raw_data, scenes, aug_singles, plain_singles, vocabulary):
    chunks = ds.chunked_data
    assert any(len(c) < CHUNK for c in chunks), "(a) a chunk shorter than C"
    short = [i for i, c in enumerate(chunks) if len(c) < CHUNK][0]
    s = aug_singles[short]
    k = len(chunks[short])
    assert (s["lang_feat"][k:] == s["lang_feat"][k - 1]).all() and (s["object_id"][k:] == s["object_id"][k - 1]).all()
    assert any(d["object_id"] == "SYNTHETIC" for d in raw_data), "(b)"
    real = [d for d in raw_data if d["object_id"] != "SYNTHETIC"]
    assert any(len(d["token"]) > MAX_DES_LEN for d in real), "(c)"
    assert any(t not in vocabulary["word2idx"] for d in real for t in d["token"][:MAX_DES_LEN]), "(d)"
    erased = plain = short_drawn = 0
    for i, c in enumerate(chunks):
        for j, d in enumerate(c):
            if d["object_id"] == "SYNTHETIC":
                continue
            ll = int(aug_singles[i]["lang_len"][j])
            changed = not np.array_equal(aug_singles[i]["lang_feat"][j], plain_singles[i]["lang_feat"][j])
            if int((ll - 2) * 0.2) >= 1:
                erased += changed
                plain += not changed
            else:
                assert not changed
                short_drawn += 2 <= len(d["token"]) <= 4
    assert erased >= 1 and plain >= 1, ("(e)", erased, plain)
    assert short_drawn >= 1, "(f)"
    for i, c in enumerate(chunks):
        ids = set(aug_singles[i]["gt_bbox_object_id"][aug_singles[i]["gt_bbox_label"] == 1].tolist())
        if any(d["object_id"] != "SYNTHETIC" and int(d["object_id"]) not in ids for d in c):
            break
    else:
        raise AssertionError("(g) an object id no labelled box carries")
    assert any((sc["instance_ids"] >= 0).all() for sc in scenes.values()), "(h)"
    nolabel = [i for i, c in enumerate(chunks) if (scenes[c[0]["scene_id"]]["instance_ids"] >= 0).all()]
    assert all(aug_singles[i]["gt_bbox_label"][-1] == 1 for i in nolabel)
    um = np.concatenate([s["unique_multiple"][:len(c)] for s, c in zip(aug_singles, chunks)])
    ann = np.concatenate([s["annotated"][:len(c)] for s, c in zip(aug_singles, chunks)])
    assert (um[ann == 1] == 0).any() and (um[ann == 1] == 1).any(), "(i)"
    masks = [int(s["scene_object_rotation_masks"].sum()) for s in aug_singles]
    assert any(m > 0 for m in masks) and any(c[0]["scene_id"] not in ds.scan2cad_rotation for c in chunks), "(j)"
    sa = [i for i, c in enumerate(chunks) if c[0]["scene_id"] in ds.scan2cad_rotation]
    assert all(0 < masks[i] < int(aug_singles[i]["gt_bbox_label"].sum()) for i in sa), "(j) some, not all, instances"
    for s in aug_singles + plain_singles:                 # no coordinate within 1e-9 of an integer: the truncation is arithmetic-proof
        v = s["locs_scaled"].astype(np.float64)
        v = v[v != 0]
        assert np.abs(v - np.round(v)).min() > 1e-9
    # get_3d_box without a heading and get_3d_box_batch with heading 0 round identically: the corner label IS the matched gt_bbox row
    matched = 0
    for s in aug_singles + plain_singles:
        for j in range(CHUNK):
            for i in np.nonzero(s["ref_box_label"][j])[0]:
                assert s["ref_box_corner_label"][j].tobytes() == s["gt_bbox"][i].tobytes()
                matched += 1
            if not s["ref_box_label"][j].any():
                assert not s["ref_box_corner_label"][j].any()
    assert matched >= 8
    # when the erase fails: an empty candidate list, lang_len - 2 < 2, gives a float index array and an IndexError (:563)
    for ll in (2, 3):
        try:
            ds._tranform_des_with_erase(np.zeros((MAX_DES_LEN + 2, 300)), ll)
            raise AssertionError("lang_len %d was expected to fail" % ll)
        except IndexError:
            pass
    state = np.random.get_state()
    ds._tranform_des_with_erase(np.zeros((MAX_DES_LEN + 2, 300)), 4)          # two tokens: one candidate, nothing to permute, no draw
    assert np.random.get_state()[2] == state[2] and np.array_equal(np.random.get_state()[1], state[1])
    ds._tranform_des_with_erase(np.zeros((MAX_DES_LEN + 2, 300)), 5)          # three tokens: zero erased, but the permutation is drawn
    assert np.random.get_state()[2] != state[2] or not np.array_equal(np.random.get_state()[1], state[1])


def _np(v):
    return v.numpy() if hasattr(v, "numpy") else np.asarray(v)


def main():
    P, DCcls = _import_reference()
    tsv = os.path.join(HERE, "lang_prep_labels.tsv")
    write_tsv(tsv)
    meta_dir = tempfile.mkdtemp()
    shutil.copy(tsv, os.path.join(meta_dir, "scannetv2-labels.combined.tsv"))
    shutil.copy(os.path.join(REF, "data/scannet/meta_data/scannet_reference_means.npz"), meta_dir)
    scenes = {SA: make_scene(21), SB: make_scene(22, unlabelled=False)}
    raw_data, vocabulary, rotations = make_raw_data(), make_vocabulary(), make_rotations()
    glove = np.random.RandomState(7).randn(len(vocabulary["word2idx"]), 300)                 # float64, as np.load of the reference's table
    out = {"glove": glove, "seed": np.int64(SEED), "max_des_len": np.int64(MAX_DES_LEN), "chunk": np.int64(CHUNK)}
    runs = {}
    for name, aug in (("aug", True), ("plain", False)):
        ds = make_dataset(P, DCcls, scenes, raw_data, vocabulary, glove, rotations, meta_dir, aug)
        batch, singles, nxt = run_batch(P, ds, SEED)
        runs[name] = singles
        for k, v in batch.items():
            out["%s/%s" % (name, k)] = np.array(v) if k == "scene_id" else _np(v)
        out["%s/next_draws" % name] = nxt
    check_cases(ds, raw_data, scenes, runs["aug"], runs["plain"], vocabulary)
    out["mean_size_arr"] = ds.DC.mean_size_arr
    out["annotations_json"] = np.array(json.dumps({"raw_data": raw_data, "vocabulary": vocabulary, "scan2cad_rotation": rotations}))
    for sid, s in scenes.items():
        for k, v in s.items():
            out["scene/%s/%s" % (sid, k)] = v
    # the host bookkeeping, flattened in raw_data order / chunk order
    real = [d for d in raw_data if d["object_id"] != "SYNTHETIC"]
    out["token_rows"] = np.stack([ds.lang_ids[d["scene_id"]][d["object_id"]][d["ann_id"]] for d in real]).astype(np.int64)
    out["chunk_sizes"] = np.array([len(c) for c in ds.chunked_data], np.int64)
    out["chunk_entries"] = np.array([raw_data.index(d) for c in ds.chunked_data for d in c], np.int64)
    out["unique_multiple"] = np.array([ds.unique_multiple_lookup[d["scene_id"]][d["object_id"]][d["ann_id"]] for d in raw_data], np.int64)
    out["raw2label_names"] = np.array(sorted(ds.raw2label))
    out["raw2label_values"] = np.array([ds.raw2label[k] for k in sorted(ds.raw2label)], np.int64)
    np.savez_compressed(os.path.join(HERE, "lang_prep_golden.npz"), **out)
    shutil.rmtree(meta_dir)
    print("wrote lang_prep_golden.npz:", os.path.getsize(os.path.join(HERE, "lang_prep_golden.npz")), "bytes;",
          "chunks", out["chunk_sizes"].tolist(), "lang_len", out["aug/lang_len"].tolist())


if __name__ == "__main__":
    main()
