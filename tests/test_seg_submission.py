"""seg_submission.SegmentationSubmission without a GPU: every refusal comes before a launch (host tensors), the host planning --
tile-prefix table, mask chunks, record layout, line width of the cluster ids, the lines of instance/<scene>.txt -- against plain
restatements, `predict.main --task segmentation`'s refusals and the library's entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

from d3net_amd import predict
from d3net_amd import seg_eval as SE
from d3net_amd import seg_submission as SS


def _pred(n0=30, n1=20):
    """a 2-scene predict_instances-shaped dict and its batch, in host memory"""
    members = [np.arange(3, 9), np.arange(n0 + 1, n0 + 7), np.arange(10, 12)]
    idx = np.concatenate([np.stack([np.full(len(m), j), m], 1) for j, m in enumerate(members)]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
    pred = dict(pick=torch.tensor([1, 0, 2]), scores=torch.tensor([0.9, 0.5, 0.25], dtype=torch.float32), proposals_idx=torch.from_numpy(idx),
                proposals_offset=torch.from_numpy(off), semantic_pred=torch.zeros(n0 + n1, dtype=torch.int64))
    return pred, dict(batch_offsets=torch.tensor([0, n0, n0 + n1], dtype=torch.int32))


def test_refusals_come_before_any_launch(tmp_path):
    sub = SS.SegmentationSubmission(str(tmp_path))
    pred, data = _pred()
    names = ["a", "b"]
    with pytest.raises(ValueError, match="no CPU fallback"):
        sub.add_batch(pred, data, names)
    with pytest.raises(ValueError, match="no CPU fallback"):
        SS.SegmentationSubmission(str(tmp_path), device="cpu")
    with pytest.raises(ValueError, match="1 scene names for 2 scenes"):
        sub.add_batch(pred, data, ["a"])
    with pytest.raises(ValueError, match="missing"):
        sub.add_batch({k: v for k, v in pred.items() if k != "scores"}, data, names)
    with pytest.raises(ValueError, match="missing"):
        sub.add_batch(pred, {}, names)
    for key, bad, what in (("scores", pred["scores"].double(), "dtype"), ("pick", pred["pick"].float(), "dtype"),
                           ("semantic_pred", pred["semantic_pred"].float(), "dtype"), ("proposals_idx", pred["proposals_idx"].float(), "dtype"),
                           ("proposals_idx", pred["proposals_idx"].reshape(-1), r"proposals_idx \(L,2\)"),
                           ("proposals_idx", pred["proposals_idx"][:, :1], r"proposals_idx \(L,2\)"),
                           ("proposals_offset", pred["proposals_offset"].reshape(2, 2), r"P \+ 1 entries"),
                           ("proposals_offset", pred["proposals_offset"][:0], r"P \+ 1 entries"),
                           ("scores", pred["scores"][:2], "shape"), ("semantic_pred", pred["semantic_pred"].reshape(-1, 1), "semantic_pred"),
                           ("pick", pred["pick"].reshape(1, -1), "pick")):
        with pytest.raises(ValueError, match=what):
            sub.add_batch(dict(pred, **{key: bad}), data, names)
    with pytest.raises(ValueError, match=r"batch_offsets \(B\+1,\)"):
        sub.add_batch(pred, dict(batch_offsets=torch.tensor([0], dtype=torch.int32)), [])
    with pytest.raises(ValueError, match="dtype"):
        sub.add_batch(pred, dict(batch_offsets=data["batch_offsets"].float()), names)
    with pytest.raises(ValueError, match="must be a tensor"):
        sub.add_batch(pred, dict(batch_offsets=[0, 30, 50]), names)
    assert sub.files() == [] and not os.listdir(tmp_path)
    with pytest.raises(ValueError, match="chunk_bytes"):
        SS.SegmentationSubmission(str(tmp_path), chunk_bytes=0)


def test_too_many_picks_and_totals_are_refused(tmp_path):
    sub = SS.SegmentationSubmission(str(tmp_path))
    # 10 000 picks of one-point proposals, all in scene 0 of two: one more than the %03d names' bound of 9 999
    P, n0 = 10000, 10050
    idx = np.stack([np.arange(P), np.arange(P)], 1).astype(np.int32)
    pred = dict(pick=torch.arange(P), scores=torch.zeros(P), proposals_idx=torch.from_numpy(idx), proposals_offset=torch.arange(P + 1, dtype=torch.int32),
                semantic_pred=torch.zeros(n0 + 5, dtype=torch.int64))
    data = dict(batch_offsets=torch.tensor([0, n0, n0 + 5], dtype=torch.int32))
    with pytest.raises(ValueError, match="10000 picks in one scene, at most 9999"):
        sub.add_batch(pred, data, ["a", "b"])
    # the same picks spread over two scenes stay inside the bound: refused only for where the tensors live
    half = dict(batch_offsets=torch.tensor([0, 5000, n0 + 5], dtype=torch.int32))
    assert SS._picks_per_scene(pred["pick"], pred["proposals_idx"], pred["proposals_offset"], half["batch_offsets"]).tolist() == [5000, 5000]
    with pytest.raises(ValueError, match="no CPU fallback"):
        sub.add_batch(pred, half, ["a", "b"])
    # totals outside int32: N * (bytes per line) of a text, checked from the shapes alone
    big = torch.zeros(1, dtype=torch.int64).expand(SS.INT32_MAX // 3 + 1)
    with pytest.raises(ValueError, match="outside int32"):
        sub.add_batch(dict(pred, semantic_pred=big), data, ["a", "b"])
    gt = dict(sem_labels=torch.zeros(1, dtype=torch.int64).expand(SS.INT32_MAX // SS.GT_WIDTH + 1), batch_offsets=data["batch_offsets"])
    gt["instance_ids"] = gt["sem_labels"]
    with pytest.raises(ValueError, match="outside int32"):
        sub.add_gt(gt, ["a", "b"])


def test_gt_refusals(tmp_path):
    sub = SS.SegmentationSubmission(str(tmp_path))
    gt = dict(sem_labels=torch.zeros(50, dtype=torch.int64), instance_ids=torch.full((50,), -1), batch_offsets=torch.tensor([0, 30, 50], dtype=torch.int32))
    with pytest.raises(ValueError, match="no CPU fallback"):
        sub.add_gt(gt, ["a", "b"])
    with pytest.raises(ValueError, match="3 scene names for 2 scenes"):
        sub.add_gt(gt, ["a", "b", "c"])
    with pytest.raises(ValueError, match="missing"):
        sub.add_gt({k: v for k, v in gt.items() if k != "instance_ids"}, ["a", "b"])
    with pytest.raises(ValueError, match="shape"):
        sub.add_gt(dict(gt, instance_ids=gt["instance_ids"][:49]), ["a", "b"])
    with pytest.raises(ValueError, match="dtype"):
        sub.add_gt(dict(gt, sem_labels=gt["sem_labels"].float()), ["a", "b"])
    assert not os.listdir(tmp_path)


def test_tile_prefix_table():
    T = SS.TILE_LINES
    for sizes in ([1], [64, 65], [T - 1, T, T + 1], [2500, 0, 2049], [0, 0, 3 * T], [0]):
        bo = np.concatenate([[0], np.cumsum(sizes)])
        want, tiles = [0], 0
        for n in sizes:                                    # plain restatement: tiles of T lines, the last one short
            tiles += len(range(0, n, T))
            want.append(tiles)
        got = SS.plan_tiles(bo)
        assert got.dtype == np.int64 and got.tolist() == want, sizes
    assert SS.plan_tiles([0, 10, 30], tile=8).tolist() == [0, 2, 5]
    assert SS.plan_tiles(torch.tensor([5, 5, 6]).numpy()).tolist() == [0, 0, 1]


def test_mask_chunks_hold_whole_proposals():
    for count, npts, room in ((50, 185000, 64 << 20), (7, 2500, 4096), (3, 300, 4096), (11, 2049, 4096), (101, 1, 4096), (5, 10, 1), (1, 1, 2),
                              (0, 100, 4096), (4, 0, 4096)):
        chunks = SS.plan_chunks(count, npts, room)
        want, c = [], 0
        while c < count and npts > 0:                      # plain restatement: as many whole files as fit, at least one
            m = 1
            while c + m < count and (m + 1) * 2 * npts <= room:
                m += 1
            want.append((c, m))
            c += m
        assert chunks == want, (count, npts, room)
        assert sum(m for _, m in chunks) == (count if npts else 0)
        assert all(m == 1 or 2 * npts * m <= room for _, m in chunks)
    assert SS.plan_chunks(7, 2500, 4096) == [(c, 1) for c in range(7)]          # a proposal larger than the chunk still goes, alone
    assert SS.plan_chunks(50, 185000, 64 << 20) == [(0, 50)]


def test_widths_layout_and_instance_lines():
    assert SS.SEM_WIDTH == 3 and SS.GT_WIDTH == 12
    assert [SS.cluster_id_width(n) for n in (0, 1, 10, 11, 100, 101, 1000, 1001, 9999)] == [3, 3, 3, 3, 3, 4, 4, 5, 5]
    for n in (1, 10, 11, 100, 101, 1000, 9999):            # room for "-1\n" and for the largest id, n - 1
        assert SS.cluster_id_width(n) == max(len("-1\n"), len("%d\n" % (n - 1)))
    lay = SS.record_layout(3, 7, 1000, (3, 4))
    assert lay["status"] == 0 and lay["counts"] == 8 and lay["table"] == 20 and lay["lens0"] == 160 and lay["lens1"] == 184 and lay["head"] == 208
    assert lay["text0"] == 208 and lay["text1"] == 3216 and lay["total"] == 7216
    for B, n, N, widths in ((1, 0, 0, (3, 3)), (2, 3, 77, (3, 4)), (5, 101, 12345, (12,))):
        lay = SS.record_layout(B, n, N, widths)
        spans = [(lay["status"], 8), (lay["counts"], 4 * B), (lay["table"], 20 * n)] + [(lay["lens%d" % k], 8 * B) for k in range(len(widths))] + \
                [(lay["text%d" % k], N * w) for k, w in enumerate(widths)]
        assert all(a + la <= b for (a, la), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= lay["total"]
        assert all(lay["lens%d" % k] % 8 == 0 and lay["text%d" % k] % 16 == 0 for k in range(len(widths))) and lay["total"] % 16 == 0
    scores = np.array([0.91234, 0.5, 0.123449, 0.99995, 1e-5, 1.0], np.float32)
    rows = np.zeros((6, 5), np.int32)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 4] = 0, np.arange(6), [3, 39, 1, 12, 24, 5], scores.view(np.int32)
    want = "".join("predicted_masks/%s_%03d.txt %d %.4f\n" % ("scene0000_00", c, cls, float(s)) for c, cls, s in zip(range(6), rows[:, 2], scores))
    assert SS.instance_lines("scene0000_00", rows) == want
    # (the float32 nearest 0.99995 lies below it: 0.99994999...)
    assert want.splitlines()[3].endswith(" 12 0.9999") and want.splitlines()[5].endswith(" 5 1.0000") and want.splitlines()[4].endswith(" 24 0.0000") and want.splitlines()[2].endswith(" 1 0.1234")
    assert SS.instance_lines("s", rows[:0]) == ""


def test_predict_segmentation_refusals(monkeypatch, tmp_path):
    argv = ["--task", "segmentation", "--root", str(tmp_path)]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="segmentation needs the detector"):
        predict.main(argv, overrides={"model": {"no_detection": True}})
    with pytest.raises(SystemExit, match="no checkpoint at .*model.ckpt"):
        predict.main(argv)
    (tmp_path / "model.ckpt").write_bytes(b"")
    with pytest.raises(SystemExit, match="needs a GPU"):
        predict.main(argv)
    with pytest.raises(SystemExit, match="needs a GPU"):                      # a joint configuration has a detector as well
        predict.main(["-c", "pointgroup_captioning.yaml"] + argv)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single-process"):
        predict.main(argv)
    cfg = predict.task_conf("pointgroup.yaml", "segmentation")
    plain = predict.task_conf("pointgroup.yaml", "segmentation", {"data": {"num_des_per_scene": 5}})
    assert cfg.cluster.prepare_epochs == -1 and plain.data.num_des_per_scene == 5 and cfg.model.no_captioning and cfg.model.no_grounding
    assert predict.task_conf("pointgroup_captioning.yaml", "captioning").data.num_des_per_scene == 8
    with pytest.raises(ValueError, match="captioning"):                        # build_test_loader keeps refusing other task names
        from d3net_amd.dataset import prediction_entries
        prediction_entries([], "test", "segmentation")


def test_model_hooks_refuse_without_names_or_detector():
    from d3net_amd.pipeline import PipelineNet
    from d3net_amd.pointgroup import PointGroup
    net = PipelineNet.__new__(PipelineNet)
    net.no_detection = True
    with pytest.raises(NotImplementedError, match="no_detection"):
        PipelineNet.predict_segmentation(net, [], None)
    assert PointGroup.predict_segmentation.__doc__ and "scene_names" in PointGroup.predict_segmentation.__doc__


def test_abi_entries(built_lib):
    from d3net_amd import _lib
    names = {"d3_seg_submit_limits", "d3_seg_cluster_table", "d3_seg_cluster_ids", "d3_seg_int_lines_ws_bytes", "d3_seg_int_lines",
             "d3_seg_mask_lines"}
    assert names <= set(_lib.SIGNATURES)
    so = ctypes.CDLL(built_lib)
    assert all(hasattr(so, n) for n in names)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "d3hip.h")).read()
    assert all(n + "(" in header for n in names) and "model/pointgroup.py:603-625" in header
    assert SS._limits() == (SS.TILE_LINES, SS.MAX_WIDTH, SS.MAX_SCENES, SS.TABLE_COLS) == (1024, 12, 4096, 5)
    l = _lib.lib()
    assert l.d3_seg_int_lines_ws_bytes(3, 1) == 512 and l.d3_seg_int_lines_ws_bytes(181, 2) == 2 * 1536
    assert l.d3_seg_int_lines_ws_bytes(-1, 1) == 0 and l.d3_seg_int_lines_ws_bytes(1, 3) == 0
    # range and argument checks return before anything is launched (no GPU is touched here)
    null = ctypes.c_void_p(0)
    assert l.d3_seg_int_lines(null, null, 0, 13, null, null, null, null, 0, 0, null, null, 10, null, null, 1, 1, null, null, 0, null) == -2
    assert l.d3_seg_int_lines(null, null, 0, 3, null, null, null, null, 0, 0, null, null, 10, null, null, 1, 3, null, null, 0, null) == -2
    assert l.d3_seg_int_lines(null, null, 0, 3, null, null, null, null, 0, 0, null, null, 10, null, null, 1, 1, null, null, 0, null) == -3
    assert l.d3_seg_mask_lines(null, null, 1, null, 0, null, 0, 0, 0, 0, 0, 1, null, 0, null) == -2
    assert l.d3_seg_cluster_table(null, 0, null, 0, null, 0, null, null, 0, null, 4097, null, 20, null, null, null, null) == -2
    assert SE.SEM_CLASS_IDX[-1] == 39 and len(SE.SEM_CLASS_IDX) == 20
