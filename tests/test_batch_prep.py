"""The host side of the fused batch preparation, without a GPU: `scene_prep.fused_applicable` over its four combinations and
`scene_prep.batch_plan` (the per-slot table and totals `d3_batch_prepare` takes) against a plain restatement."""
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
