"""The leaderboard writers on the device (csrc/submission.hip, submission.CaptionSubmission / GroundingSubmission,
PipelineNet.predict_captioning / predict_grounding): both kernels through the C ABI against the plain restatement
(tests/submission_restate.py, pinned to the reference's files on the CPU) field by field, the files `write()` leaves against the
SHA-256 of the reference's, the status bits, no read-back in add_batch, and the two PipelineNet calls against the host chain on a
batch without ground-truth keys.  Copies, integers and an arg-max: every comparison is exact."""
import ctypes as C
import hashlib
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import submission_restate as R  # noqa: E402
from test_submission import assert_caption_results_equal_golden, assert_grounding_results_equal_golden, host_pick  # noqa: E402

V, EOS = 40, 3
R_SGN = np.array([[1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1], [1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1]], np.float32)
CAP_STATE = ("box", "cls", "score", "ntok", "tok", "count", "first_seen", "status")
GROUND_REC = ("bbox", "pred_ref", "unique_multiple", "others", "key", "keep", "ids")
# what a test split's batch does not carry (the teacher switch of the synthetic detector reads sem_labels, instance_info and
# instance_ids in place of the untrained point heads; those three stay)
GT_KEYS = ("center_label", "size_label", "sem_cls_label", "box_label_mask", "instance_num_point", "gt_bbox", "gt_bbox_label",
           "gt_bbox_object_id", "ref_box_label", "ref_box_corner_label", "scene_object_rotations", "scene_object_rotation_masks",
           "annotated", "lang_ids")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "submission_golden.npz"))


@pytest.fixture(scope="module")
def caption_case():
    from gen_submission_golden import caption_case
    case = caption_case()
    case["picks"] = [host_pick(d) for d in case["batches"]]
    return case


@pytest.fixture(scope="module")
def grounding_case():
    from gen_submission_golden import grounding_case
    return grounding_case()


def _to(d, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}


def _sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def _p(t):
    return C.c_void_p(t.data_ptr())


def _caption_state(dev, S, Kcap, Tcap):
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    return dict(box=z((S, Kcap, 8, 3), torch.float32), cls=z((S, Kcap), torch.int32), score=z((S, Kcap), torch.float32),
                ntok=z((S, Kcap), torch.int32), tok=z((S, Kcap, Tcap), torch.int32), count=z((S,), torch.int32),
                first_seen=torch.full((S,), -1, dtype=torch.int64, device=dev), status=z((1,), torch.int32))


def _caption_launch(dev, st, d, pick, table, seq, Kcap, Tcap):
    from d3net_amd import _lib
    t = _to(d, dev)
    pk = torch.from_numpy(np.ascontiguousarray(pick, np.float32)).to(dev)
    B, K, T = t["lang_cap"].shape
    with torch.cuda.device(dev):
        return _lib.lib().d3_caption_submit_batch(
            _p(t["proposal_bbox_batched"]), _p(t["proposal_sem_cls_batched"]), _p(t["proposal_scores_batched"]), _p(pk), _p(t["lang_cap"]),
            _p(t["id"]), _p(table), table.numel(), B, K, T, V, EOS, seq, st["count"].numel(), Kcap, Tcap, _p(st["box"]), _p(st["cls"]),
            _p(st["score"]), _p(st["ntok"]), _p(st["tok"]), _p(st["count"]), _p(st["first_seen"]), _p(st["status"]),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _assert_state_equal(st, want):
    for k in CAP_STATE:
        got = st[k].cpu().numpy()
        assert got.dtype == want[k].dtype and np.array_equal(got, want[k], equal_nan=True), k


def test_caption_kernel_equals_the_restatement(dev, caption_case):
    """the golden batches through the C ABI into one state, then the edge cases: a scene with an all-zero NMS mask (count 0), and
    each status bit"""
    names, table = R.scene_table(caption_case["chunked_data"])
    dtable = torch.from_numpy(table).to(dev)
    st, want = _caption_state(dev, len(names), 256, 31), R.caption_state(len(names), 256, 31)
    for seq, (d, pick) in enumerate(zip(caption_case["batches"], caption_case["picks"])):
        assert _caption_launch(dev, st, d, pick, dtable, seq, 256, 31) == 0
        R.caption_batch(want, d, pick, table, V, EOS, seq)
    _assert_state_equal(st, want)
    assert want["status"][0] == 0 and want["count"].tolist()[:6] == [47, 52, 49, 65, 195, 194]
    # edge cases on the K = 65 scene (all 65 kept) and on two rows of batch 0, in a state with room for exactly K records of T tokens
    base, pick = caption_case["batches"][2], caption_case["picks"][2]

    def both(d, pick, K, seq=5):
        st, want = _caption_state(dev, len(names), K, 31), R.caption_state(len(names), K, 31)
        assert _caption_launch(dev, st, d, pick, dtable, seq, K, 31) == 0
        R.caption_batch(want, d, pick, table, V, EOS, seq)
        _assert_state_equal(st, want)
        return want

    two = {k: v[:2].copy() for k, v in caption_case["batches"][0].items()}
    p2 = caption_case["picks"][0][:2].copy()
    p2[1] = 0
    w = both(two, p2, 63)
    assert w["count"][names.index("scene0000_00")] == 0 and w["first_seen"][names.index("scene0000_00")] == (5 << 20) + 1
    caps = base["lang_cap"].copy(); caps[0, 7, 0] = V
    assert both(dict(base, lang_cap=caps), pick, 65)["status"][0] == 1
    caps = base["lang_cap"].copy(); caps[0, 0, 1] = V; caps[0, 8, 30] = -1          # behind an eos: never decoded; at T - 1 without one: decoded
    assert both(dict(base, lang_cap=caps), pick, 65)["status"][0] == (1 if EOS not in base["lang_cap"][0, 8, :30] else 0)
    sem = base["proposal_sem_cls_batched"].copy(); sem[0, 9] = 20; sem[0, 10] = np.nan
    assert both(dict(base, proposal_sem_cls_batched=sem), pick, 65)["status"][0] == 2
    assert both(dict(base, id=np.array([12], np.int64)), pick, 65)["status"][0] == 4
    assert both(dict(base, id=np.array([11], np.int64)), pick, 65)["status"][0] == 0    # the last id of the table: a scene that had no batch yet


def test_caption_submission_writes_the_reference_file(dev, golden, caption_case, tmp_path):
    from d3net_amd import submission as sm
    from d3net_amd.evaluator import nms_pred_mask_device
    sub = sm.CaptionSubmission(caption_case["chunked_data"], caption_case["vocabulary"], device=dev)
    for d, pick in zip(caption_case["batches"], caption_case["picks"]):
        t = _to(d, dev)
        assert sub.add_batch(t) is None
        assert np.array_equal(nms_pred_mask_device(t).cpu().numpy(), pick)          # the device NMS: the host loop's picks
    assert_caption_results_equal_golden(sub.results(), golden)
    path = str(tmp_path / "benchmark_test.nms.json")
    sub.write(path)
    assert _sha256(path) == str(golden["cap_sha256"])
    sub.reset()
    with pytest.raises(ValueError, match="no batch"):
        sub.results()


def _ground_launch(dev, rec, status, d, key_of, row0):
    from d3net_amd import _lib
    t = _to(d, dev)
    N, K = t["cluster_ref"].shape
    B = t["proposal_bbox_batched"].shape[0]
    with torch.cuda.device(dev):
        return _lib.lib().d3_ground_submit_batch(
            _p(t["cluster_ref"]), _p(t["proposal_bbox_batched"]), _p(t["unique_multiple"]), _p(t["object_cat"]), _p(t["id"]), _p(t["chunk_ids"]),
            _p(key_of), key_of.shape[0], key_of.shape[1], B, N // B, K, row0, _p(rec["bbox"]), _p(rec["pred_ref"]), _p(rec["unique_multiple"]),
            _p(rec["others"]), _p(rec["key"]), _p(rec["keep"]), _p(rec["ids"]), _p(status), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _ground_records(dev, rows):
    z = lambda shape, dt: torch.full((rows,) + shape, -7, dtype=dt, device=dev)
    return dict(bbox=z((8, 3), torch.float32), pred_ref=z((), torch.int32), unique_multiple=z((), torch.int64), others=z((), torch.int32),
                key=z((), torch.int32), keep=z((), torch.int32), ids=z((2,), torch.int64))


def test_grounding_kernel_equals_the_restatement(dev, grounding_case):
    key_of = R.key_table(grounding_case["chunked_data"])
    dkey = torch.from_numpy(key_of).to(dev)
    want = R.ground_epoch(grounding_case["batches"], key_of)
    rows = want["keep"].shape[0]
    rec, status = _ground_records(dev, rows), torch.zeros(1, dtype=torch.int32, device=dev)
    row0 = 0
    for d in grounding_case["batches"]:
        assert _ground_launch(dev, rec, status, d, dkey, row0) == 0
        row0 += d["cluster_ref"].shape[0]
    assert row0 == rows == 38 and int(status.cpu()[0]) == 0
    for k in GROUND_REC:
        got = rec[k].cpu().numpy()
        assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), k
    # quantised scores with many exact ties and NaNs at K = 1, 63, 64, 65, 257 and 4096, C = 1 and 4, chunk ids that repeat within a
    # batch, ids and chunk ids outside the table (status 1, keep 0)
    rng = np.random.default_rng(5)
    for B, Cn, K in ((5, 1, 1), (2, 4, 63), (1, 4, 64), (3, 4, 65), (5, 1, 257), (1, 4, 4096)):
        N = B * Cn
        ref = (rng.integers(-6, 7, (N, K)) / 4).astype(np.float32)
        ref[rng.random((N, K)) < 0.03] = np.nan
        ref[0, rng.integers(K)] = -0.0
        c = rng.random((B, K, 1, 3)).astype(np.float32) * 3
        d = dict(cluster_ref=ref, proposal_bbox_batched=(c + R_SGN * np.float32(0.4)).astype(np.float32),
                 unique_multiple=rng.integers(0, 2, (B, Cn)).astype(np.int64), object_cat=rng.integers(15, 18, (B, Cn)).astype(np.int64),
                 id=rng.integers(0, 7, B).astype(np.int64), chunk_ids=rng.integers(-1, 5, (B, Cn)).astype(np.int64))
        w, st = R.ground_batch(d, key_of)
        rec, status = _ground_records(dev, N + 3), torch.zeros(1, dtype=torch.int32, device=dev)
        assert _ground_launch(dev, rec, status, d, dkey, 3) == 0
        assert int(status.cpu()[0]) == st
        for k in GROUND_REC:
            got = rec[k].cpu().numpy()
            assert np.array_equal(got[3:], w[k]) and (got[:3] == -7).all(), (k, B, Cn, K)


def test_grounding_submission_writes_the_reference_file(dev, golden, grounding_case, tmp_path):
    from d3net_amd import submission as sm
    sub = sm.GroundingSubmission(grounding_case["chunked_data"], device=dev)
    for i, d in enumerate(grounding_case["batches"]):
        t = _to(d, dev)
        if i % 2:                                                            # the shapes and integer types a loader may hand over
            t["unique_multiple"], t["object_cat"], t["id"] = t["unique_multiple"].reshape(-1).int(), t["object_cat"].reshape(-1), t["id"].int()
        assert sub.add_batch(t) is None
    assert_grounding_results_equal_golden(sub.results(), golden)
    path = str(tmp_path / "pred.json")
    sub.write(path)
    assert _sha256(path) == str(golden["ground_sha256"])
    # more rows than the records' first allocation: the storage doubles on the device, the earlier rows stay
    big = sm.GroundingSubmission(grounding_case["chunked_data"], device=dev)
    first = _to(grounding_case["batches"][0], dev)
    for _ in range(130):
        big.add_batch(first)
    res = big.results()
    assert len(res) == 130 * 6 and res[:6] == res[-6:] == sub.results()[:6]


def test_status_bits_make_results_raise(dev, caption_case, grounding_case):
    from d3net_amd import _lib, submission as sm
    base = caption_case["batches"][2]

    def cap(match, **change):
        sub = sm.CaptionSubmission(caption_case["chunked_data"], caption_case["vocabulary"], max_proposals=65, max_len=31, device=dev)
        sub.add_batch(_to(dict(base, **change), dev))
        with pytest.raises(_lib.D3Error, match=match):
            sub.results()

    caps = base["lang_cap"].copy(); caps[0, 7, 0] = V
    cap("vocabulary", lang_cap=caps)
    sem = base["proposal_sem_cls_batched"].copy(); sem[0, 9] = 20
    cap("class", proposal_sem_cls_batched=sem)
    cap("names no scene", id=np.array([12], np.int64))
    gs = sm.GroundingSubmission(grounding_case["chunked_data"], device=dev)
    d = dict(grounding_case["batches"][1]); d["id"] = d["id"].copy(); d["id"][2] = 6
    gs.add_batch(_to(d, dev))
    with pytest.raises(_lib.D3Error, match="no annotation"):
        gs.results()


def test_add_batch_reads_nothing_back(dev, golden, caption_case, grounding_case, monkeypatch):
    from d3net_amd import submission as sm
    cs = sm.CaptionSubmission(caption_case["chunked_data"], caption_case["vocabulary"], device=dev)
    gs = sm.GroundingSubmission(grounding_case["chunked_data"], device=dev)
    cb, gb = [_to(d, dev) for d in caption_case["batches"]], [_to(d, dev) for d in grounding_case["batches"]]

    def refuse(*a, **k):
        raise AssertionError("add_batch read a tensor back")

    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy"):
            m.setattr(torch.Tensor, name, refuse)
        for t in cb:
            assert cs.add_batch(t) is None
        for t in gb:
            assert gs.add_batch(t) is None
    assert_caption_results_equal_golden(cs.results(), golden)
    assert_grounding_results_equal_golden(gs.results(), golden)


def _net(dev, **flags):
    from d3net_amd import synthetic as S
    from d3net_amd.pipeline import PipelineNet
    from test_pipeline_gpu import _cfg
    Vn = 200
    scenes = [S.small_scene(dims=(40, 32, 20), n_boxes=3, seed=s) for s in (3, 4)]
    chunked, organized = S.make_language_corpus(2, chunk=4, vocab=Vn, objects_per_scene=3)
    for chunks in chunked:
        for j, ann in enumerate(chunks):
            ann["ann_id"] = str(j % 3)
    tr = types.SimpleNamespace(vocabulary=S.make_vocabulary(Vn), glove=np.random.default_rng(0).standard_normal((Vn, 300)).astype(np.float32),
                               chunked_data=chunked, organized=organized, raw_data=S.corpus_raw_data(organized))
    cfg = _cfg(**flags)
    net = PipelineNet(cfg, {"train": tr, "val": tr}).to(dev)
    net.detector.teacher = True
    batch = S.add_language(S.make_batch(scenes, dev), dev, chunk=4, vocab=Vn)
    batch["cluster_rand"] = torch.rand(2, 3, generator=torch.Generator().manual_seed(1))
    batch["slot_perms"] = [torch.randperm(cfg.model.max_num_proposal, generator=torch.Generator().manual_seed(2 + b)) for b in range(2)]
    batch["istrain"] = torch.zeros_like(batch["istrain"])
    batch["unique_multiple"] = torch.from_numpy(np.random.default_rng(1).integers(0, 2, (2, 4))).to(dev)
    batch["object_cat"][:, 1] = 17
    bare = {k: v for k, v in batch.items() if k not in GT_KEYS}
    assert "center_label" not in bare and "sem_labels" in bare and cfg.general.task != "test"
    return net, tr, batch, bare


def test_predict_captioning_equals_the_host_chain(dev):
    """detector.feed -> speaker's evaluation decode -> the host NMS mask -> decode_caption, on the batch WITH its ground truth,
    against predict_captioning on the batch without it"""
    from d3net_amd.caption_eval import decode_caption
    from d3net_amd.evaluator import parse_predictions
    net, tr, batch, bare = _net(dev, no_captioning=False, no_grounding=True)
    bare["lang_len"] = batch["lang_len"] = batch["spk_lang_len"]
    net.train()
    sub = net.predict_captioning([bare])
    assert net.training and net.cfg.general.task != "test"
    got = sub.results()
    net.eval()
    with torch.no_grad():
        net._lazy_proposals = False
        d = net.speaker(net.detector.feed(dict(batch), net.current_epoch), use_tf=False, use_rl=False, is_eval=True, beam_opt=net.beam_opt)
    parse_predictions(d, device_nms=False)
    mask, boxes = d["pred_mask"], d["proposal_bbox_batched"].cpu().numpy()
    sem, prob = d["proposal_sem_cls_batched"].cpu().numpy() - 2, d["proposal_scores_batched"].cpu().numpy()
    sem[sem < 0] = 17
    want = {}
    for b in range(2):
        want[tr.chunked_data[b][0]["scene_id"]] = [
            {"caption": decode_caption(d["lang_cap"][b, k].cpu(), tr.vocabulary["idx2word"], tr.vocabulary["special_tokens"]),
             "box": boxes[b, k].tolist(), "sem_prob": np.eye(18, dtype=np.float32)[int(sem[b, k])].tolist(),
             "obj_prob": np.array([0, prob[b, k]], np.float32).tolist()} for k in range(mask.shape[1]) if mask[b, k] == 1]
    print({k: len(v) for k, v in want.items()}, {k: len(v) for k, v in got.items()})
    assert all(len(v) > 0 for v in want.values()) and list(got) == list(want)
    assert got == want


def test_predict_grounding_equals_argmax_and_gathers(dev):
    net, tr, batch, bare = _net(dev, no_captioning=True, no_grounding=False)
    sub = net.eval().predict_grounding([bare, bare])
    assert not net.training and net.cfg.general.task != "test"
    got = sub.results()
    with torch.no_grad():
        net._lazy_proposals = False
        d = net.listener(net.detector.feed(dict(batch), net.current_epoch))
    ref = d["cluster_ref"].cpu()
    assert ref.shape == (8, net.cfg.model.max_num_proposal) and not torch.isnan(ref).any()
    pred = ref.argmax(-1)
    boxes = d["proposal_bbox_batched"].cpu()[torch.arange(8) // 4, pred].numpy()
    um, cat = batch["unique_multiple"].reshape(-1).tolist(), batch["object_cat"].reshape(-1).tolist()
    want, cached = [], []
    for n in range(8):
        ann = tr.chunked_data[n // 4][n % 4]
        query = "{}-{}-{}".format(ann["scene_id"], ann["object_id"], ann["ann_id"])
        if query not in cached:
            cached.append(query)
            want.append({"scene_id": ann["scene_id"], "object_id": ann["object_id"], "ann_id": ann["ann_id"], "bbox": boxes[n].tolist(),
                         "unique_multiple": int(um[n]), "others": int(cat[n] == 17)})
    print(len(want), len(got))
    assert got == want + want                                                  # the batch came twice: both copies are written
