"""The leaderboard writers' specification, pinned on the CPU: the numpy restatement of csrc/submission.hip's per-row rules
(tests/submission_restate.py) plus the library's host formatter reproduce the records AND the bytes of the files the reference's own
two `predict` functions wrote (tests/golden/submission_golden.npz, made by gen_submission_golden.py: SHA-256 of
benchmark_test.nms.json and of pred.json); CaptionSubmission, GroundingSubmission and PipelineNet.predict_* refuse what they cannot
take before any launch.  Everything here is copies, integers and an arg-max: every comparison is exact."""
import hashlib
import io
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import submission_restate as R  # noqa: E402


def file_sha256(obj):
    buf = io.StringIO()
    json.dump(obj, buf, indent=4)
    return hashlib.sha256(buf.getvalue().encode()).hexdigest()


def host_pick(d):
    """the NMS mask of one batch by the library's host path (numpy, float64: the form tests/test_evaluator.py pins)"""
    from d3net_amd.evaluator import parse_predictions
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}
    parse_predictions(t, device_nms=False)
    return t["pred_mask"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "submission_golden.npz"))


@pytest.fixture(scope="module")
def caption_case():
    from gen_submission_golden import caption_case
    return caption_case()


@pytest.fixture(scope="module")
def grounding_case():
    from gen_submission_golden import grounding_case
    return grounding_case()


def restated_caption_state(case, Kcap=256, Tcap=31):
    from gen_submission_golden import EOS, V
    names, table = R.scene_table(case["chunked_data"])
    state = R.caption_state(len(names), Kcap, Tcap)
    for seq, d in enumerate(case["batches"]):
        R.caption_batch(state, d, host_pick(d), table, V, EOS, seq)
    return names, state


def assert_caption_results_equal_golden(res, g):
    recs = [r for scene in res.values() for r in scene]
    assert list(res) == g["cap_scenes"].tolist() and [len(v) for v in res.values()] == g["cap_counts"].tolist()
    assert [r["caption"] for r in recs] == g["cap_captions"].tolist()
    assert np.array_equal(np.array([r["box"] for r in recs], np.float64), g["cap_box"].astype(np.float64))
    assert [int(np.argmax(r["sem_prob"])) for r in recs] == g["cap_cls"].tolist()
    assert all(len(r["sem_prob"]) == 18 and sorted(r["sem_prob"]) == [0.0] * 17 + [1.0] for r in recs)
    assert [r["obj_prob"] for r in recs] == [[0.0, float(s)] for s in g["cap_score"]]
    assert file_sha256(res) == str(g["cap_sha256"])


def assert_grounding_results_equal_golden(res, g):
    assert ["{}-{}-{}".format(r["scene_id"], r["object_id"], r["ann_id"]) for r in res] == g["ground_names"].tolist()
    assert np.array_equal(np.array([r["bbox"] for r in res], np.float64), g["ground_bbox"].astype(np.float64))
    assert [r["unique_multiple"] for r in res] == g["ground_unique_multiple"].tolist()
    assert [r["others"] for r in res] == g["ground_others"].tolist()
    assert file_sha256(res) == str(g["ground_sha256"])


def test_caption_restatement_reproduces_the_reference_file(golden, caption_case):
    from d3net_amd.submission import format_caption_results
    names, state = restated_caption_state(caption_case)
    assert state["status"][0] == 0
    words = [caption_case["vocabulary"]["idx2word"][str(i)] for i in range(40)]
    res = format_caption_results(state, names, words)
    assert_caption_results_equal_golden(res, golden)
    # the planted rows do what they were planted for
    s2, s0, s3 = names.index("scene0002_00"), names.index("scene0000_00"), names.index("scene0003_00")
    assert state["first_seen"][s2] == 0 and state["first_seen"][s0] == 1            # batch 0, rows 0 and 1
    b0, b1 = caption_case["batches"][:2]
    k0, k1 = int(np.flatnonzero(host_pick(b0)[2])[0]), int(np.flatnonzero(host_pick(b1)[1])[0])
    assert np.array_equal(state["box"][s2, 0], b0["proposal_bbox_batched"][2, k0])       # ... written by row 2, the last of batch 0
    assert np.array_equal(state["box"][s0, 0], b1["proposal_bbox_batched"][1, k1])       # replaced by batch 1
    assert state["count"][s3] == 65 and state["ntok"][s3, :3].tolist() == [1, 31, 31]
    caps = [r["caption"] for r in res["scene0003_00"]]
    assert caps[0] == "sos eos" and caps[1].count(" ") == 32 and caps[2].count(" ") == 31 and caps[1].endswith(" eos")
    assert state["cls"][s3, 3:7].tolist() == [17, 17, 0, 17]
    assert [r["caption"] for k in ("scene0006_00", "scene0007_00") for r in res[k]] == ["sos eos", "sos w3 eos"]
    assert "scene0009_00" not in res                                                # id 11 never came


def test_a_scene_without_valid_proposals_is_an_empty_list(caption_case):
    """outside the golden: the reference asserts on an all-zero mask (lib/det/ap_helper.py:132); here the scene is written, empty"""
    from d3net_amd.submission import format_caption_results
    d = {k: v[:2].copy() for k, v in caption_case["batches"][0].items()}
    d["proposal_batch_mask"][1] = 0
    names, table = R.scene_table(caption_case["chunked_data"])
    pick = host_pick(d)
    assert pick[1].sum() == 0 and pick[0].sum() > 0
    state = R.caption_batch(R.caption_state(len(names), 63, 31), d, pick, table, 40, 3, 0)
    res = format_caption_results(state, names, [caption_case["vocabulary"]["idx2word"][str(i)] for i in range(40)])
    assert list(res) == ["scene0002_00", "scene0000_00"] and res["scene0000_00"] == [] and len(res["scene0002_00"]) == int(pick[0].sum())


def test_status_bits_of_the_restatement(caption_case, grounding_case):
    names, table = R.scene_table(caption_case["chunked_data"])
    base = caption_case["batches"][2]
    pick = host_pick(base)

    def status(**change):
        d = dict(base); d.update(change)
        return int(R.caption_batch(R.caption_state(len(names), 65, 31), d, pick, table, 40, 3, 0)["status"][0])

    caps = base["lang_cap"].copy(); caps[0, 7, 0] = 40
    assert status(lang_cap=caps) == 1
    caps = base["lang_cap"].copy(); caps[0, 0, 1] = 40                             # behind the eos at position 0: never decoded
    assert status(lang_cap=caps) == 0
    sem = base["proposal_sem_cls_batched"].copy(); sem[0, 9] = 20
    assert status(proposal_sem_cls_batched=sem) == 2
    assert status(id=np.array([12], np.int64)) == 4 and status(id=np.array([-1], np.int64)) == 4
    key_of = R.key_table(grounding_case["chunked_data"])
    d = dict(grounding_case["batches"][1]); d["id"] = d["id"].copy(); d["id"][2] = 6
    rec, st = R.ground_batch(d, key_of)
    assert st == 1 and rec["keep"].tolist() == [1, 1, 0, 1, 1]


def test_grounding_restatement_reproduces_the_reference_file(golden, grounding_case):
    from d3net_amd.submission import format_grounding_results
    key_of = R.key_table(grounding_case["chunked_data"])
    rec = R.ground_epoch(grounding_case["batches"], key_of)
    assert rec["status"][0] == 0
    assert_grounding_results_equal_golden(format_grounding_results(rec, grounding_case["chunked_data"]), golden)
    # the planted rows: a NaN, two NaNs, a tie, the maximum at an invalid slot, the repeats (in both copies of batch 0), a stride tie
    assert rec["pred_ref"][1:5].tolist() == [62, 9, 20, 17] and grounding_case["batches"][0]["proposal_batch_mask"][1, 17] == 0
    assert rec["keep"][:8].tolist() == [1, 1, 1, 1, 1, 1, 0, 0] and rec["keep"][-8:].tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
    assert rec["key"][4] == rec["key"][6] == rec["key"][7] and rec["others"][0] == 1 and rec["unique_multiple"][:2].tolist() == [0, 1]
    assert rec["pred_ref"][13] == 0 and rec["pred_ref"][-8 - 5 + 2] == 70 and rec["pred_ref"][-8 - 5 + 3] == 256


def test_bad_input_is_refused_before_any_launch(caption_case, grounding_case, monkeypatch):
    from d3net_amd import _lib, submission as sm

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)
    good = {k: torch.from_numpy(v.copy()) for k, v in caption_case["batches"][0].items()}
    sub = sm.CaptionSubmission(caption_case["chunked_data"], caption_case["vocabulary"])

    def refused(s, match, base, **change):
        d = dict(base)
        d.update(change)
        for k in [k for k, v in change.items() if v is None]:
            del d[k]
        with pytest.raises(ValueError, match=match):
            s.add_batch(d)

    refused(sub, "missing", good, lang_cap=None)
    refused(sub, "missing", good, id=None)
    refused(sub, "must be a tensor", good, id=[3, 0, 4])
    refused(sub, "expected", good, proposal_bbox_batched=good["proposal_bbox_batched"].reshape(3, 63, 24))
    refused(sub, "shape", good, proposal_scores_batched=good["proposal_scores_batched"][:, :-1])
    refused(sub, "shape", good, lang_cap=good["lang_cap"][:, :-1])
    refused(sub, "shape", good, id=good["id"][:2])
    refused(sub, "dtype", good, lang_cap=good["lang_cap"].int())
    refused(sub, "dtype", good, proposal_sem_cls_batched=good["proposal_sem_cls_batched"].long())
    refused(sub, "dtype", good, proposal_bbox_batched=good["proposal_bbox_batched"].double())
    refused(sub, "dtype", good, id=good["id"].float())
    refused(sub, "T = 63", good, lang_cap=torch.zeros((3, 63, 63), dtype=torch.int64))
    big = dict(proposal_bbox_batched=torch.zeros(1, 257, 8, 3), proposal_sem_cls_batched=torch.zeros(1, 257), proposal_scores_batched=torch.zeros(1, 257),
               proposal_batch_mask=torch.zeros(1, 257), lang_cap=torch.zeros((1, 257, 4), dtype=torch.int64), id=torch.zeros(1, dtype=torch.int64))
    refused(sub, "K <= 256", big)
    refused(sub, "no CPU fallback", good)                                       # a well-formed batch in host memory
    with pytest.raises(ValueError, match="no batch"):
        sub.results()
    with pytest.raises(ValueError, match="max_proposals"):
        sm.CaptionSubmission(caption_case["chunked_data"], caption_case["vocabulary"], max_proposals=257)
    with pytest.raises(ValueError, match="max_len"):
        sm.CaptionSubmission(caption_case["chunked_data"], caption_case["vocabulary"], max_len=63)
    small = sm.CaptionSubmission(caption_case["chunked_data"], caption_case["vocabulary"], max_proposals=32, max_len=31)
    refused(small, "K <= 32", good)

    good = {k: torch.from_numpy(v.copy()) for k, v in grounding_case["batches"][0].items()}
    gs = sm.GroundingSubmission(grounding_case["chunked_data"])
    refused(gs, "missing", good, chunk_ids=None)
    refused(gs, "must be a tensor", good, object_cat=grounding_case["batches"][0]["object_cat"])
    refused(gs, "dtype", good, cluster_ref=good["cluster_ref"].double())
    refused(gs, "dtype", good, unique_multiple=good["unique_multiple"].float())
    refused(gs, "shape", good, chunk_ids=good["chunk_ids"].reshape(-1))
    refused(gs, "shape", good, object_cat=good["object_cat"][:, :3])
    refused(gs, "expected", good, proposal_bbox_batched=good["proposal_bbox_batched"].reshape(2, 63, 24))
    refused(gs, "N = B", good, cluster_ref=good["cluster_ref"][:7])
    refused(gs, "1 <= K", good, cluster_ref=torch.zeros(8, 4097), proposal_bbox_batched=torch.zeros(2, 4097, 8, 3))
    refused(gs, "no CPU fallback", good)
    with pytest.raises(ValueError, match="no batch"):
        gs.results()


def _cfg(**model):
    from d3net_amd.config import default_conf
    base = {"model": {"blocks": [1, 2, 3], "num_graph_steps": 2, "num_locals": 10, "use_relation": True, "use_orientation": True,
                      "match_type": "Transformer", "use_lang_classifier": True, "use_bidir": False, "num_bbox_class": 18,
                      "loss_type": "cross_entropy"},
            "data": {"num_des_per_scene": 4, "max_spk_len": 30, "max_lis_len": 126, "min_iou_threshold": 0.25, "num_ori_bins": 6},
            "train": {"use_rl": False, "sample_topn": 1}}
    base["model"].update(model)
    return default_conf(overrides=base)


def test_predict_refuses_other_modes():
    from d3net_amd import synthetic as S
    from d3net_amd.pipeline import PipelineNet
    V = 50
    ds = {"train": types.SimpleNamespace(vocabulary=S.make_vocabulary(V), glove=np.zeros((V, 300), np.float32))}
    net0 = PipelineNet(_cfg(no_captioning=True, no_grounding=True), ds)
    with pytest.raises(NotImplementedError, match=r"modes 1 and 3\), this is mode 0"):
        net0.predict_captioning([])
    with pytest.raises(NotImplementedError, match=r"modes 2 and 3\), this is mode 0"):
        net0.predict_grounding([])
    net2 = PipelineNet(_cfg(no_captioning=True, no_grounding=False), ds).train()
    with pytest.raises(NotImplementedError, match="this is mode 2"):
        net2.predict_captioning([])
    with pytest.raises(ValueError, match="description store"):                 # the right mode, but no chunked_data and no submission
        net2.predict_grounding([])
    assert net2.training                                                        # refused before any work: the flag was not touched
    net1 = PipelineNet(_cfg(no_captioning=False, no_grounding=True), ds)
    with pytest.raises(NotImplementedError, match="this is mode 1"):
        net1.predict_grounding([])


def test_binding_table_entries(built_lib):
    import ctypes as C
    from d3net_amd import _lib
    res, args = _lib.SIGNATURES["d3_caption_submit_batch"]
    assert res is C.c_int and len(args) == 26 and args[13] is C.c_longlong and args[7] is C.c_int
    res, args = _lib.SIGNATURES["d3_ground_submit_batch"]
    assert res is C.c_int and len(args) == 22 and args[12] is C.c_longlong and args[7] is C.c_int
    l = _lib.lib()
    # the range checks come before any launch and before any pointer is looked at: no device needed

    def cap(B, K, T, Kcap=256, Tcap=62, seq=0):
        a = [None] * 26
        a[7:17] = [4, B, K, T, 40, 3, seq, 4, Kcap, Tcap]
        return l.d3_caption_submit_batch(*a)

    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 257, 1), (1, 1, 63), ((1 << 20) + 1, 1, 1)):
        assert cap(*bad) == -2, bad
    assert cap(1, 64, 4, Kcap=63) == -2 and cap(1, 4, 31, Tcap=30) == -2 and cap(1, 1, 1, seq=-1) == -2 and cap(1, 1, 1, seq=1 << 43) == -2
    assert cap(1, 256, 62) == -3 and cap(1 << 20, 1, 1, seq=(1 << 43) - 1) == -3       # in range: D3_ERR_ARG for the null pointers

    def ground(B, Cn, K):
        a = [None] * 22
        a[7:13] = [4, 4, B, Cn, K, 0]
        return l.d3_ground_submit_batch(*a)

    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 4097), (65536, 65536, 8)):
        assert ground(*bad) == -2, bad
    assert ground(1, 1, 4096) == -3
