#!/usr/bin/env python3
"""Generates tests/golden/submission_golden.npz by RUNNING THE REFERENCE: its own two leaderboard writers,
`benchmark/benchmark_captioning.py:121-196 predict` and `benchmark/benchmark_grounding.py:110-186 predict`, loaded with importlib and
run on the CPU over canned batches -- a loader that yields empty dicts, a stub model whose `detector.feed` returns the batch's
tensors and whose speaker / listener pass them through -- so the NMS, the decode, the dedupe and json.dump are the reference's.
Run in the build container only (needs /root/reference); the tests never run it.  Inputs are not stored: `caption_case()` and
`grounding_case()` rebuild them.  Stored per case: the records parsed from the reference's file as arrays, the file order of the
scenes and the SHA-256 of the file.

Not in the golden: a scene whose proposal mask is all zero.  The reference asserts `len(pick) > 0` there (lib/det/ap_helper.py:132);
the library writes an empty list for it, which the tests pin against the restatement alone."""
import hashlib
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

SGN = np.array([[1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1], [1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1]], np.float32)
V, EOS = 40, 3
# captioning: (K, T, dataset ids) per batch.  K = 63, 64, 65 (below, at and above a wave), 256 (the full workgroup) and 1; T = 31 and 1
CAP_BATCHES = ((63, 31, (3, 0, 4)), (64, 31, (2, 1)), (65, 31, (5,)), (256, 31, (6, 7)), (1, 1, (8, 9, 10)))
CAP_SCENE_OF_ID = (0, 0, 1, 2, 2, 3, 4, 5, 6, 7, 8, 9)          # ids 3 and 4 name one scene, as do 0 and 1; id 11 never shows up
# grounding: (B, C, K) per batch; N = 5 rows is no multiple of the 4 waves of a workgroup.  The first batch is fed twice.
GROUND_BATCHES = ((2, 4, 63), (5, 1, 1), (1, 4, 64), (2, 4, 65), (5, 1, 257))


def vocabulary():
    words = ["pad_", "unk", "sos", "eos"] + ["w%d" % i for i in range(V - 4)]
    return {"word2idx": {w: i for i, w in enumerate(words)}, "idx2word": {str(i): w for i, w in enumerate(words)},
            "special_tokens": {"bos_token": "sos", "eos_token": "eos", "unk_token": "unk", "pad_token": "pad_"}}


def caption_case(seed=41):
    """-> dict(chunked_data, vocabulary, batches): batches of numpy arrays under the keys the writer reads.
    batch 0 names scene 2 in rows 0 and 2 (ids 3 and 4): row 2 is written, scene 2 stays first in the file; batch 1 names scene 0 again:
    its list is replaced, its place (second) stays; batch 2 is one scene whose 65 proposals are all valid, disjoint and so all kept,
    with the planted captions (eos at position 0, no eos, eos at T - 1 only) and sem ids 0 and 1 (class 17); batch 4 has K = 1, T = 1:
    the eos at position 0 == T - 1, and no eos."""
    rng = np.random.default_rng(seed)
    chunked = [[{"scene_id": "scene%04d_00" % s, "object_id": "0", "ann_id": "0"}] for s in CAP_SCENE_OF_ID]
    batches = []
    for K, T, ids in CAP_BATCHES:
        B = len(ids)
        mask = (rng.random((B, K)) < 0.8).astype(np.float32)
        mask[:, 0] = 1
        room = np.float32(0.35 * K ** (1 / 3) + 0.3)                # crowded: the same-class NMS drops a good part
        c = rng.random((B, K, 3)).astype(np.float32) * room
        s = rng.random((B, K, 3)).astype(np.float32) * np.float32(0.9) + np.float32(0.2)
        if K == 65:                                     # a 5 x 5 x 3 grid of pitch 2 with sizes below 1.1: no two boxes touch
            g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(3), indexing="ij"), -1).reshape(-1, 3)[:K]
            c = np.broadcast_to((2 * g).astype(np.float32), (B, K, 3)).copy()
            mask[:] = 1
        corners = (c[:, :, None] + SGN[None, None] * s[:, :, None] / 2).astype(np.float32)
        sem = rng.integers(0, 7, (B, K)).astype(np.float32)         # few classes (ids 0 and 1 are class 17), so boxes do meet their own class
        scores = ((rng.permutation(B * K) + 1) / np.float32(B * K + 1)).astype(np.float32).reshape(B, K)
        caps = rng.integers(4, V, (B, K, T)).astype(np.int64)
        caps[rng.random((B, K, T)) < 0.06] = EOS
        if K == 65:
            caps[0, 0, 0] = EOS
            caps[0, 1] = np.where(caps[0, 1] == EOS, 5, caps[0, 1])
            caps[0, 2] = np.where(caps[0, 2] == EOS, 6, caps[0, 2]); caps[0, 2, T - 1] = EOS
            sem[0, 3], sem[0, 4], sem[0, 5], sem[0, 6] = 0, 1, 2, 19
        if K == 1:
            caps[0, 0, 0], caps[1, 0, 0], caps[2, 0, 0] = EOS, 7, 8
        batches.append(dict(proposal_bbox_batched=corners, proposal_sem_cls_batched=sem, proposal_scores_batched=scores,
                            proposal_batch_mask=mask, lang_cap=caps, id=np.asarray(ids, np.int64)))
    return dict(chunked_data=chunked, vocabulary=vocabulary(), batches=batches)


def grounding_case(seed=43):
    """-> dict(chunked_data, batches).  6 dataset ids x 4 annotations; chunked_data[1][2] repeats chunked_data[1][0] (a loader pads a
    scene's chunk with repeats).  Planted: batch 0 row 1 a NaN score, row 2 two NaNs (the lower wins), row 3 an exact tie, row 4 its
    maximum at an INVALID slot (chosen all the same), rows 4..7 (id 1) chunk ids 0, 1, 2, 0: rows 6 and 7 repeat row 4's annotation;
    batch 2 a tie across the wave's stride; batch 4 the maximum in the last slot.  Batch 0 comes twice: both copies are written."""
    rng = np.random.default_rng(seed)
    chunked = [[{"scene_id": "scene%04d_00" % i, "object_id": str(3 * j + i), "ann_id": str(j % 3)} for j in range(4)] for i in range(6)]
    chunked[1][2] = dict(chunked[1][0])
    batches = []
    for bi, (B, Cn, K) in enumerate(GROUND_BATCHES):
        N = B * Cn
        mask = (rng.random((B, K)) < 0.6).astype(np.float32)
        c = rng.random((B, K, 3)).astype(np.float32) * np.array([4, 3, 2], np.float32)
        s = rng.random((B, K, 3)).astype(np.float32) * np.float32(0.9) + np.float32(0.2)
        corners = (c[:, :, None] + SGN[None, None] * s[:, :, None] / 2).astype(np.float32)
        ref = rng.standard_normal((N, K)).astype(np.float32)
        cat = rng.integers(0, 18, (B, Cn)).astype(np.int64)
        cat[rng.random((B, Cn)) < 0.3] = 17
        ids = (np.arange(B, dtype=np.int64) + bi) % 6
        chunks = np.tile(np.arange(Cn, dtype=np.int64), (B, 1))
        batches.append(dict(cluster_ref=ref, proposal_bbox_batched=corners, proposal_batch_mask=mask,
                            unique_multiple=rng.integers(0, 2, (B, Cn)).astype(np.int64), object_cat=cat, id=ids, chunk_ids=chunks))
    d = batches[0]                                       # (2, 4, 63), ids 0 and 1
    d["cluster_ref"][1, 62] = np.nan
    d["cluster_ref"][2, 40] = d["cluster_ref"][2, 9] = np.nan
    d["cluster_ref"][3, 20] = d["cluster_ref"][3, 41] = 9.0
    d["proposal_batch_mask"][1, 17] = 0
    d["cluster_ref"][4, 17] = 30.0
    d["chunk_ids"][1] = [0, 1, 2, 0]
    d["object_cat"][0, 0], d["object_cat"][0, 1] = 17, 3
    d["unique_multiple"][0, 0], d["unique_multiple"][0, 1] = 0, 1
    d = batches[2]                                       # (1, 4, 64)
    d["cluster_ref"][0, [0, 63]] = 11.0
    d = batches[4]                                       # (5, 1, 257)
    d["cluster_ref"][2, [70, 134, 198]] = 12.0           # lanes 6, 6, 6: one lane's stride
    d["cluster_ref"][3, 256] = 40.0
    batches.append({k: v.copy() for k, v in batches[0].items()})
    return dict(chunked_data=chunked, batches=batches)


def nms_iou_matrix(corners):
    """pairwise AABB IoU of (K,8,3) corners in float64, as lib/det/nms.py:110-150 forms it"""
    lo, hi = corners.min(1).astype(np.float64), corners.max(1).astype(np.float64)
    d = np.maximum(0, np.minimum(hi[:, None], hi[None]) - np.maximum(lo[:, None], lo[None]))
    inter, vol = d.prod(-1), (hi - lo).prod(-1)
    return inter / (vol[:, None] + vol[None] - inter + 1e-8)


def _load(name, path):
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        os.chdir(cwd)
    return mod


class _Feed:
    """`model.detector`: feed() hands out the next canned batch"""

    def __init__(self, batches):
        self.batches = iter(batches)

    def feed(self, data_dict, epoch=0):
        data_dict.update({k: torch.from_numpy(v.copy()) for k, v in next(self.batches).items()})
        return data_dict


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    for name in ("trimesh", "plyfile", "omegaconf"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = object
    sys.modules["omegaconf"].OmegaConf = object
    stub = types.ModuleType("data.scannet.model_util_scannet")
    stub.extract_pc_in_box3d = None
    stub.ScannetDatasetConfig = type("ScannetDatasetConfig", (), {"num_class": 18, "__init__": lambda self, cfg=None: None})
    for name in ("data", "data.scannet"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["data.scannet.model_util_scannet"] = stub
    ref_cap = _load("ref_benchmark_captioning", os.path.join(REF, "benchmark", "benchmark_captioning.py"))
    ref_ground = _load("ref_benchmark_grounding", os.path.join(REF, "benchmark", "benchmark_grounding.py"))
    ns = types.SimpleNamespace
    passthrough = lambda d, *a, **k: d
    out = {"numpy_version": np.array(np.__version__)}

    # ---- captioning
    case = caption_case()
    for d in case["batches"]:
        for b in range(d["id"].shape[0]):
            valid = d["proposal_batch_mask"][b] == 1
            sc = d["proposal_scores_batched"][b][valid]
            assert len(np.unique(sc)) == len(sc), "equal scores among the valid proposals of a scene: numpy's argsort order is not pinned"
            iou = nms_iou_matrix(d["proposal_bbox_batched"][b][valid])
            assert (np.abs(iou - 0.25) > 1e-6).all(), "an NMS IoU within 1e-6 of 0.25"
    with tempfile.TemporaryDirectory() as root:
        cfg = ns(general=ns(root=root), data=ns(split="test"))
        dataset = ns(chunked_data=case["chunked_data"], vocabulary=case["vocabulary"])
        model = ns(detector=_Feed(case["batches"]), speaker=passthrough, beam_opt={})
        ref_cap.predict(cfg, dataset, [{} for _ in case["batches"]], model)
        raw = open(os.path.join(root, "benchmark_test.nms.json"), "rb").read()
    res = json.loads(raw)
    recs = [r for scene in res.values() for r in scene]
    for r in recs:
        assert sorted(r["sem_prob"]) == [0.0] * 17 + [1.0] and r["obj_prob"][0] == 0.0
    out.update(cap_sha256=np.array(hashlib.sha256(raw).hexdigest()), cap_scenes=np.array(list(res)),
               cap_counts=np.array([len(v) for v in res.values()], np.int64), cap_captions=np.array([r["caption"] for r in recs]),
               cap_box=np.array([r["box"] for r in recs], np.float32).reshape(-1, 8, 3),
               cap_cls=np.array([int(np.argmax(r["sem_prob"])) for r in recs], np.int64),
               cap_score=np.array([r["obj_prob"][1] for r in recs], np.float32))
    assert np.array_equal(out["cap_box"].astype(np.float64).reshape(-1), np.array([r["box"] for r in recs], np.float64).reshape(-1))
    caps = out["cap_captions"].tolist()
    assert "sos eos" in caps and any(c.count(" ") == 32 and c.endswith(" eos") for c in caps) and 17 in out["cap_cls"]
    assert list(res)[:2] == ["scene0002_00", "scene0000_00"] and out["cap_counts"][list(res).index("scene0003_00")] == 65

    # ---- grounding
    case = grounding_case()
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "run"))
        cfg = ns(OUTPUT_PATH=root)
        dataset = ns(chunked_data=case["chunked_data"])
        model = ns(detector=_Feed(case["batches"]), listener=passthrough)
        ref_ground.predict(ns(folder="run"), cfg, dataset, [{} for _ in case["batches"]], model)
        raw = open(os.path.join(root, "run", "pred.json"), "rb").read()
    res = json.loads(raw)
    rows = sum(b["cluster_ref"].shape[0] for b in case["batches"])
    assert len(res) == rows - 4, (len(res), rows)        # two repeats in each copy of batch 0
    out.update(ground_sha256=np.array(hashlib.sha256(raw).hexdigest()),
               ground_names=np.array(["{}-{}-{}".format(r["scene_id"], r["object_id"], r["ann_id"]) for r in res]),
               ground_bbox=np.array([r["bbox"] for r in res], np.float32).reshape(-1, 8, 3),
               ground_unique_multiple=np.array([r["unique_multiple"] for r in res], np.int64),
               ground_others=np.array([r["others"] for r in res], np.int64))
    np.savez_compressed(os.path.join(HERE, "submission_golden.npz"), **out)
    print({k: np.asarray(v).shape for k, v in out.items()})
    print(out["cap_scenes"], out["cap_counts"], out["cap_sha256"], out["ground_sha256"])


if __name__ == "__main__":
    main()
