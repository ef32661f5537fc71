"""The specification of csrc/assign.hip, pinned on the CPU: the restated solver (tests/lsap_restate.py) returns scipy's rows
and columns exactly, ties included, and the restated float32 GIoU cost agrees with caption_eval.generalized_box3d_iou."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import lsap_restate as L  # noqa: E402


def _same_as_scipy(m):
    r0, c0 = linear_sum_assignment(m)
    r1, c1 = L.lsap(m)
    assert np.array_equal(r0, r1) and np.array_equal(c0, c1), (m.shape, r0, c0, r1, c1)


@pytest.mark.parametrize("family", L.FAMILIES)
def test_restated_solver_matches_scipy_exactly(family):
    rng = np.random.default_rng(L.FAMILIES.index(family) + 1)
    shapes = [(1, 1), (1, 5), (5, 1), (2, 2), (7, 7), (24, 24), (40, 24), (24, 40), (40, 1), (13, 14), (14, 13)]
    shapes += [(int(rng.integers(1, 41)), int(rng.integers(1, 25))) for _ in range(40)]
    for R, C in shapes:
        m = L.matrix_family(rng, family, R, C)
        _same_as_scipy(m)            # nr > nc (mostly), nr == nc, nr < nc all occur in `shapes`
        _same_as_scipy(m.T.copy())   # and the other orientation


@pytest.mark.parametrize("shape", [(24, 24), (24, 17), (17, 24)])
def test_restated_solver_machol_wien(shape):
    _same_as_scipy(L.machol_wien(*shape))


def test_restated_solver_rejects_what_scipy_rejects():
    for bad in (np.nan, np.inf, -np.inf):
        m = np.ones((3, 4), np.float32)
        m[1, 2] = bad
        with pytest.raises(ValueError):
            L.lsap(m)
    for bad in (np.nan, -np.inf):
        m = np.ones((3, 4), np.float32)
        m[1, 2] = bad
        with pytest.raises(ValueError):
            linear_sum_assignment(m)


def test_restated_giou_matches_caption_eval():
    from gen_caption_eval_golden import caption_inputs
    from d3net_amd import caption_eval as ce
    inp = caption_inputs()
    pred, gt = inp["pred_boxes"], inp["gt_boxes"]
    ref = ce.generalized_box3d_iou(torch.from_numpy(pred), torch.from_numpy(gt)).numpy()
    for b in range(pred.shape[0]):
        n = int(inp["gt_box_masks"][b].sum())
        got = L.giou_cost(pred[b], gt[b, :n])
        assert got.dtype == np.float32 and got.shape == (pred.shape[1], n)
        assert np.allclose(-got, ref[b, :, :n], rtol=1e-5, atol=1e-6)
    # a degenerate pair (all corners at one point: enclosing == 0) is inf * 0 = NaN on both sides
    z = np.zeros((1, 8, 3), np.float32)
    assert np.isnan(L.giou_cost(z, z)).all()
    assert torch.isnan(ce.generalized_box3d_iou(torch.zeros(1, 1, 8, 3), torch.zeros(1, 1, 8, 3))).all()
