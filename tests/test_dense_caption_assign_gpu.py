"""csrc/assign.hip on the GPU: the batched assignment solver against scipy (exact pairs, ties included), the in-kernel GIoU cost
bit for bit against the float32 restatement (tests/lsap_restate.py), and assign_dense_caption's device path against its host
path."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import lsap_restate as L  # noqa: E402

pytestmark = pytest.mark.gpu

SGN = np.array([[1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1], [1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1]], np.float32)
LSAP_SHAPES = [(5, 3, [3, 2, 0]), (4, 7, [7, 4, 5]), (70, 9, [9, 9, 1]), (130, 66, [66, 65, 64]), (256, 128, [128, 128, 127])]
BOX_KINDS = ("random", "integer_grid", "duplicated_proposals", "zero_padded_proposals", "identical_gt")


def _lsap_device(dev, cost, ncols):
    """raw d3_lsap_batched -> (rc, per_col (B,C), status (B)) as numpy"""
    from d3net_amd import _lib
    cost_t = torch.from_numpy(np.ascontiguousarray(cost, np.float32)).to(dev)
    B, R, Cc = cost_t.shape
    nc = torch.tensor(list(ncols), dtype=torch.int32, device=dev)
    per_col = torch.full((B, Cc), -7, dtype=torch.int32, device=dev)
    status = torch.full((B,), -7, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = _lib.lib().d3_lsap_batched(p(cost_t), p(nc), B, R, Cc, p(per_col), p(status), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, per_col.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("family", L.FAMILIES)
@pytest.mark.parametrize("shape", LSAP_SHAPES, ids=lambda s: "%dx%d" % (s[0], s[1]))
def test_lsap_batched_matches_scipy(dev, shape, family):
    R, Cc, ncols = shape
    rng = np.random.default_rng(1000 * R + Cc + L.FAMILIES.index(family))
    cost = np.stack([L.matrix_family(rng, family, R, Cc) for _ in ncols])
    rc, per_col, status = _lsap_device(dev, cost, ncols)
    assert rc == 0 and (status == 0).all(), (rc, status)
    assert np.array_equal(per_col, L.per_col_from_scipy(cost, ncols))


def test_lsap_batched_machol_wien_and_limits(dev):
    cost = np.stack([L.machol_wien(24, 24)] * 2)
    rc, per_col, status = _lsap_device(dev, cost, [24, 17])
    assert rc == 0 and (status == 0).all()
    assert np.array_equal(per_col, L.per_col_from_scipy(cost, [24, 17]))
    rc, per_col, _ = _lsap_device(dev, np.zeros((1, 257, 4), np.float32), [4])
    assert rc == -2 and (per_col == -7).all()          # D3_ERR_RANGE before any launch
    rc, _, _ = _lsap_device(dev, np.zeros((1, 4, 257), np.float32), [4])
    assert rc == -2
    # a non-finite entry in a valid column: status 1 and a zero row; in a padded column it is never read
    cost = np.ones((2, 6, 5), np.float32)
    cost[0, 2, 1] = np.nan
    cost[1, 2, 4] = np.inf
    rc, per_col, status = _lsap_device(dev, cost, [5, 4])
    assert rc == 0 and status.tolist() == [1, 0] and (per_col[0] == 0).all()
    assert np.array_equal(per_col[1], L.per_col_from_scipy(cost, [0, 4])[1])


def box_set(kind, K, G, seed=0, B=2):
    """-> pred (B,K,8,3), gt (B,G,8,3) float32 corners, nactual (B) int64; the GT boxes have positive extent"""
    rng = np.random.default_rng(seed)
    room = np.array([4, 3, 2], np.float32)
    if kind == "integer_grid":
        gc, gs = rng.integers(0, 4, (B, G, 3)).astype(np.float32), rng.integers(1, 3, (B, G, 3)).astype(np.float32) * 2
        pc, ps = rng.integers(0, 4, (B, K, 3)).astype(np.float32), rng.integers(1, 3, (B, K, 3)).astype(np.float32) * 2
    else:
        gc, gs = rng.random((B, G, 3)).astype(np.float32) * room, rng.random((B, G, 3)).astype(np.float32) * 0.9 + 0.3
        pc, ps = rng.random((B, K, 3)).astype(np.float32) * room, rng.random((B, K, 3)).astype(np.float32) * 0.9 + 0.3
        m = min(K, G)                                   # some proposals are jittered GT boxes, in shuffled slots
        for b in range(B):
            slots = rng.permutation(K)[:m]
            pc[b, slots] = gc[b, :m] + rng.normal(0, 0.1, (m, 3)).astype(np.float32)
            ps[b, slots] = gs[b, :m] * rng.uniform(0.8, 1.25, (m, 3)).astype(np.float32)
    gt = gc[:, :, None] + SGN[None, None] * gs[:, :, None] / 2
    pred = pc[:, :, None] + SGN[None, None] * ps[:, :, None] / 2
    nactual = np.array([G, max(G - 2, 1)][:B], np.int64)
    if kind == "duplicated_proposals":                  # PointGroup's two clusterings: every other proposal a copy of its neighbour
        h = K // 2
        pred[:, 1:2 * h:2] = pred[:, 0:2 * h:2]
    elif kind == "zero_padded_proposals":               # fewer real proposals than GT boxes: zero slots must be assigned
        valid = max(1, min(K, int(nactual.min())) // 2)
        pred[:, valid:] = 0
    elif kind == "identical_gt":
        gt[:, 1] = gt[:, 0]
    return pred.astype(np.float32), gt.astype(np.float32), nactual


@pytest.mark.parametrize("kind", BOX_KINDS)
@pytest.mark.parametrize("KG", [(12, 7), (128, 128)], ids=lambda s: "%dx%d" % s)
def test_dense_caption_assign_cost_bits_and_pairs(dev, KG, kind):
    from d3net_amd import caption_eval as ce
    K, G = KG
    pred, gt, nactual = box_set(kind, K, G, seed=K + BOX_KINDS.index(kind))
    per_gt, cost = ce.assign_boxes_device(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), torch.from_numpy(nactual).to(dev),
                                          return_cost=True)
    assert per_gt.dtype == torch.int64 and per_gt.is_cuda and tuple(per_gt.shape) == (pred.shape[0], G)
    cost, per_gt = cost.cpu().numpy(), per_gt.cpu().numpy()
    for b in range(pred.shape[0]):
        n = int(nactual[b])
        assert np.array_equal(cost[b, :, :n], L.giou_cost(pred[b], gt[b, :n])), (kind, b)
    assert np.array_equal(per_gt, L.per_col_from_scipy(cost, nactual))
    # without cost_out the same pairs
    again = ce.assign_boxes_device(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), torch.from_numpy(nactual).to(dev))
    assert np.array_equal(again.cpu().numpy(), per_gt)


def _caption_case(pred, gt, nactual, seed=5, L_cap=12):
    words = ["pad_", "unk", "sos", "eos"] + ["w%d" % i for i in range(56)]
    vocab = {"idx2word": {str(i): w for i, w in enumerate(words)},
             "special_tokens": {"bos_token": "sos", "eos_token": "eos", "unk_token": "unk", "pad_token": "pad_"}}
    rng = np.random.default_rng(seed)
    B, K, G = pred.shape[0], pred.shape[1], gt.shape[1]
    caps = rng.integers(4, 60, (B, K, L_cap)).astype(np.int64)
    caps[rng.random(caps.shape) < 0.1] = 3
    masks = (np.arange(G)[None] < nactual[:, None]).astype(np.float32)
    ids = np.stack([rng.permutation(300)[:G] for _ in range(B)]).astype(np.int64)
    return dict(pred_captions=caps, pred_boxes=pred, gt_boxes=gt, gt_box_ids=ids, gt_box_masks=masks,
                scene_list=["scene%04d_00" % b for b in range(B)], vocab=vocab)


def _candidates(dev, inp, **kw):
    from d3net_amd import caption_eval as ce
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items() if isinstance(v, np.ndarray)}
    return ce.assign_dense_caption(t["pred_captions"], t["pred_boxes"], t["gt_boxes"], t["gt_box_ids"], t["gt_box_masks"],
                                   inp["scene_list"], inp["vocab"]["idx2word"], inp["vocab"]["special_tokens"], **kw)


@pytest.mark.parametrize("strategy", ["giou", "center"])
@pytest.mark.parametrize("inputs", ["golden", "random"])
def test_assign_dense_caption_device_equals_host(dev, inputs, strategy):
    if inputs == "golden":
        from gen_caption_eval_golden import caption_inputs
        inp = caption_inputs()
    else:
        inp = _caption_case(*box_set("random", 128, 128, seed=128))
    host = _candidates(dev, inp, strategy=strategy, device_assign=False)
    device = _candidates(dev, inp, strategy=strategy, device_assign=True)
    assert sorted(host) == sorted(device) and len(host) > 0
    for k in host:
        assert host[k]["caption"] == device[k]["caption"], k
        assert host[k]["iou"] == device[k]["iou"], k
        assert host[k]["box"] == device[k]["box"], k


def test_zero_enclosing_volume_raises_on_both_paths(dev):
    pred, gt, nactual = box_set("random", 12, 7, seed=3)
    pred[0, 5] = 0                                     # a zero proposal against a zero GT box: enclosing == 0 -> inf * 0
    gt[0, 2] = 0
    inp = _caption_case(pred, gt, nactual)
    for device_assign in (False, True):
        with pytest.raises(ValueError):
            _candidates(dev, inp, device_assign=device_assign)
    # the same pair in a padded column is never read
    gt2 = gt.copy()
    gt2[0, 2], gt2[0, 6] = gt[0, 6], 0
    inp2 = _caption_case(pred, gt2, np.array([6, 5], np.int64))
    host, device = _candidates(dev, inp2, device_assign=False), _candidates(dev, inp2, device_assign=True)
    assert sorted(host) == sorted(device) and all(host[k]["iou"] == device[k]["iou"] for k in host)
    from d3net_amd import caption_eval as ce
    with pytest.raises(ValueError):
        ce.assign_boxes_device(torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(nactual))   # boxes on the host


def test_default_takes_the_kernel_within_its_limits(dev, monkeypatch):
    """device_assign=None: the kernel for GPU boxes with K, G <= 256 (DESIGN.md 3.6 has the measurement), else the host path"""
    from d3net_amd import caption_eval as ce
    calls, real = [], ce._assign_launch
    monkeypatch.setattr(ce, "_assign_launch", lambda *a: calls.append(a[3]) or real(*a))
    inp = _caption_case(*box_set("random", 12, 7, seed=9))
    by_default = _candidates(dev, inp)
    assert calls == ["giou"]
    assert by_default == _candidates(dev, inp, device_assign=False) and calls == ["giou"]
    big = _caption_case(*box_set("random", 257, 7, seed=9))
    assert len(_candidates(dev, big)) == int(big["gt_box_masks"].sum()) and calls == ["giou"]      # beyond the limit: host path
    with pytest.raises(ValueError):
        _candidates(dev, big, device_assign=True)
