"""The host side of the fused batch preparation, without a GPU: `scene_prep.fused_applicable` over its four combinations and
`scene_prep.batch_plan` (the per-slot table and totals `d3_batch_prepare` takes) against a plain restatement, and the table of the
batch's 20 output tensors with its allocator (`scene_prep._BATCH_KEYS`, `_alloc_batch`) against a literal one."""
import types

import numpy as np
import pytest
import torch

from d3net_amd import dataset as D
from d3net_amd import scene_prep as SP
from d3net_amd.config import default_conf


def _cfg(detector_only):
    return default_conf(overrides={"model": {"no_captioning": True, "no_grounding": detector_only}})


@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("detector_only", [True, False])
def test_fused_applicable(resident, detector_only):
    store = types.SimpleNamespace(device=torch.device("cuda", 0) if resident else torch.device("cpu"))
    cfg = _cfg(detector_only)
    assert SP.elastic_enabled(cfg, True) == detector_only and not SP.elastic_enabled(cfg, False)
    assert SP.fused_applicable(cfg, True, store) == (resident and not detector_only)     # elastic on or off
    assert SP.fused_applicable(cfg, False, store) == resident                            # no augmentation: never elastic


def test_batch_plan_against_a_restatement():
    r = np.random.RandomState(0)
    S = 6
    n = np.array([5, 0, 1200, 1, 77, 300])
    offsets = np.concatenate([[0], np.cumsum(n)])
    id_hi = np.array([3, -1, 40, 0, -1, 65535])
    V = np.maximum(id_hi, 0) + 1
    table_offsets = np.concatenate([[0], np.cumsum(V + 1)])
    K = np.array([2, 0, 30, 1, 0, 9])
    Lp = np.array([4, 0, 1100, 1, 0, 300])
    scalars = np.stack([np.full(S, -1), id_hi, K, Lp, r.randint(0, 2, S)], 1)
    rows = [2, 5, 2, 1, 0, 4]                                # a scene twice, an empty one, one without labels
    plan = SP.batch_plan(offsets, table_offsets, scalars, rows)
    assert plan["row0"].dtype == np.int64 and plan["slots"].dtype == np.int32 and plan["slots"].shape == (6, 6)
    assert plan["row0"].flags["C_CONTIGUOUS"] and plan["slots"].flags["C_CONTIGUOUS"]
    N = I = L = Vt = 0
    for slot, s in enumerate(rows):
        assert plan["row0"][slot] == offsets[s]
        assert list(plan["slots"][slot]) == [n[s], table_offsets[s], V[s], K[s], Lp[s], scalars[s, 4]]
        N, I, L, Vt = N + n[s], I + K[s], L + Lp[s], Vt + V[s]
    assert (plan["N"], plan["I"], plan["L"], plan["V"]) == (N, I, L, Vt)


@pytest.mark.parametrize("ids", [[-1] * 7, [0], [3, 3, -1, 0, 3, 0, 5, -1], [2, 1, 0, 1, 2], []])
def test_scene_instance_tables_against_np_unique(ids):
    ids = np.asarray(ids, np.int64)
    hist, rank, start, order = D.scene_instance_tables(ids)
    V = max(int(ids.max()) if len(ids) else -1, 0) + 1
    assert len(hist) == len(rank) == len(start) == V + 1 and order.dtype == np.int32
    uniq = [v for v in np.unique(ids) if v >= 0]
    assert rank[V] == len(uniq) and start[V] == (ids >= 0).sum() and hist[0] == (ids < 0).sum()
    lists = [np.nonzero(ids == v)[0] for v in uniq] + [np.nonzero(ids < 0)[0]]
    assert np.array_equal(order, np.concatenate(lists).astype(np.int32) if len(ids) else np.zeros(0, np.int32))
    for k, v in enumerate(uniq):                             # np.unique order, ascending point index inside an instance
        assert rank[v] == k and hist[v + 1] == len(lists[k]) and start[v] == sum(len(l) for l in lists[:k])


# the batch's 20 outputs as they stood written out in every batch builder, restated literally: key, batch dtype, trailing shape
# (C the feature columns), leading extent, in the C ABI's order (BpOut, csrc/scene_prep.h)
_F32, _I32, _I64 = torch.float32, torch.int32, torch.int64
_OUTPUTS = [("locs", _F32, (3,), "points"), ("locs_scaled", _I64, (4,), "points"), ("feats", _F32, ("C",), "points"),
            ("sem_labels", _I64, (), "points"), ("instance_ids", _I64, (), "points"), ("instance_info", _F32, (12,), "points"),
            ("instance_num_point", _I32, (), "instances"), ("gt_proposals_idx", _I32, (2,), "entries"),
            ("gt_proposals_offset", _I32, (), "instances+1"), ("batch_offsets", _I32, (), "B+1"), ("instance_offsets", _I32, (), "B+1"),
            ("center_label", _F32, (3,), "B,R"), ("sem_cls_label", _I64, (), "B,R"), ("heading_class_label", _I64, (), "B,R"),
            ("heading_residual_label", _F32, (), "B,R"), ("size_class_label", _I64, (), "B,R"), ("size_residual_label", _F32, (3,), "B,R"),
            ("gt_bbox_object_id", _I64, (), "B,R"), ("gt_bbox_label", _I64, (), "B,R"), ("gt_bbox", _F32, (8, 3), "B,R")]
_PER_SCENE = {"locs_scaled": (_F32, (3,)), "sem_labels": (_I32, ()), "instance_ids": (_I32, ())}    # where a prepare_scene sample differs
_GT = ("gt_proposals_idx", "gt_proposals_offset")


def test_batch_key_table_against_a_restatement():
    assert len(_OUTPUTS) == 20
    assert [(k.name, k.dtype, k.tail, k.extent) for k in SP._BATCH_KEYS] == _OUTPUTS
    for k in SP._BATCH_KEYS:
        assert (k.scene_dtype, k.scene_tail) == _PER_SCENE.get(k.name, (k.dtype, k.tail)), k.name
        assert k.gt == (k.name in _GT), k.name
    assert [k.name for k in SP._BATCH_KEYS if k.dtype == _I64 and k.scene_dtype != _I64] == ["locs_scaled", "sem_labels", "instance_ids"]
    assert list(SP._BOX_KEYS) == [o[0] for o in _OUTPUTS[11:]]
    assert [k.name for k in SP._SCENE_KEYS] == [o[0] for o in _OUTPUTS[:9] + _OUTPUTS[11:]]        # d3_collate_scenes' 18 pointer columns


@pytest.mark.parametrize("has_gt", [True, False])
def test_batch_allocator_against_the_restatement(has_gt):
    B, R, Cf, N, I, Lt = 3, 5, 7, 11, 4, 9                   # six different extents: no shape can pass by coincidence
    lead = {"points": (N,), "instances": (I,), "instances+1": (I + 1,), "entries": (Lt,), "B+1": (B + 1,), "B,R": (B, R)}
    data, out = SP._alloc_batch(torch.device("cpu"), B, R, Cf, has_gt, N, I, Lt)
    want = [o for o in _OUTPUTS if has_gt or o[0] not in _GT]
    assert list(data) == [o[0] for o in want]
    for name, dt, tail, extent in want:
        assert data[name].dtype == dt and tuple(data[name].shape) == lead[extent] + tuple(Cf if t == "C" else t for t in tail), name
        assert data[name].is_contiguous() and data[name].device.type == "cpu"
    assert out.dtype == np.uint64 and out.shape == (20,)
    for slot, o in enumerate(_OUTPUTS):
        assert int(out[slot]) == (data[o[0]].data_ptr() if o[0] in data else 0), o[0]
    assert (int(out[7]) == 0 and int(out[8]) == 0) == (not has_gt)
    assert len({int(p) for p in out if p}) == len(want)      # every tensor its own storage
