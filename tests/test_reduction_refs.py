"""tests/reduction_refs.py against torch's own float64 CPU ops and autograd (1e-12 relative), the conventions torch does
not define (all-ignored -> 0, M = 1, |pt| = 0), and the properties of the shared inputs that the GPU tests rely on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import reduction_refs as R

RTOL = 1e-12


def close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    scale = max(float(np.abs(b).max()) if b.size else 0.0, 1e-300)
    assert float(np.abs(a - b).max() if b.size else 0.0) <= RTOL * scale, what


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


@pytest.mark.parametrize("M,C,relu", [(4, 3, 1), (37, 5, 0), (300, 16, 1)])
def test_batchnorm(M, C, relu):
    # (M = 2 leaves of dx only the cancellation residue of two equal terms: no relative bound applies to it)
    rng = np.random.default_rng(M)
    x = (1.5 + 2 * rng.standard_normal((M, C))).astype(np.float32)
    gamma, beta = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    rm, rv = rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    dy = rng.standard_normal((M, C)).astype(np.float32)
    mom, eps = np.float32(0.1), np.float32(1e-4)
    xt, gt, bt = t64(x).requires_grad_(True), t64(gamma).requires_grad_(True), t64(beta).requires_grad_(True)
    trm, trv = t64(rm), t64(rv)
    y = Fn.batch_norm(xt, trm, trv, gt, bt, True, float(mom), float(eps))
    if relu:
        y = torch.relu(y)
    y.backward(t64(dy))
    mean, var, nrm, nrv = R.bn_stats(x, rm, rv, mom)
    close(mean, t64(x).mean(0), "mean")
    close(var, t64(x).var(0, unbiased=False), "var")
    close(nrm, trm, "running_mean")
    close(nrv, trv, "running_var")
    close(R.bn_relu_fwd(x, mean, var, gamma, beta, eps, relu), y.detach(), "y")
    dx, dgamma, dbeta = R.bn_relu_bwd(x, dy, mean, var, gamma, beta, eps, relu)
    close(dx, xt.grad, "dx")
    close(dgamma, gt.grad, "dgamma")
    close(dbeta, bt.grad, "dbeta")


def test_batchnorm_one_row():
    """M = 1 (torch refuses it in training): var 0, running variance updated with factor 1, y = beta, dx = 0"""
    x = np.array([[3.0, -2.0]], np.float32)
    rm, rv = np.array([1.0, 2.0], np.float32), np.array([4.0, 8.0], np.float32)
    mean, var, nrm, nrv = R.bn_stats(x, rm, rv, 0.25)
    assert np.array_equal(mean, [3.0, -2.0]) and np.array_equal(var, [0.0, 0.0])
    assert np.array_equal(nrm, [1.5, 1.0]) and np.array_equal(nrv, [3.0, 6.0])
    g, b = np.array([2.0, 3.0], np.float32), np.array([0.5, -0.5], np.float32)
    assert np.array_equal(R.bn_relu_fwd(x, mean, var, g, b, 1e-4, 1), [[0.5, 0.0]])
    dx, dgamma, dbeta = R.bn_relu_bwd(x, np.array([[1.0, 1.0]], np.float32), mean, var, g, b, 1e-4, 1)
    assert np.array_equal(dx, [[0.0, 0.0]]) and np.array_equal(dgamma, [0.0, 0.0]) and np.array_equal(dbeta, [1.0, 0.0])


def test_bn_inputs_keep_the_relu_mask_unambiguous():
    """dy is zeroed where |y| < 1e-3; that must stay under 1 % of the elements, over all the shapes the GPU test uses
    together and in every shape with at least 1000 elements"""
    banded = total = 0
    for M, C, shift, relu in R.bn_cases():
        case = R.bn_case(M, C, shift, 1000 * C + M)
        n = int(case["band"].sum())
        assert np.all(case["dy"][case["band"]] == 0)
        if M * C >= 1000:
            assert n < 0.01 * M * C, (M, C, n)
        banded, total = banded + n, total + M * C
    assert banded < 0.01 * total
    assert set(R.bn_case(4097, 16, 0, 1)["fam"]) == set(range(len(R.BN_FAMILIES)))


@pytest.mark.parametrize("N,C,ignore", [(50, 7, -1), (64, 20, -100), (33, 5, 3), (9, 1, -1)])
def test_cross_entropy(N, C, ignore):
    z, label = R.ce_case(N, C, "some", ignore, N)
    loss, count, grad = R.cross_entropy(z, label, ignore)
    lab = torch.from_numpy(np.where((label < 0) | (label >= C), ignore, label))
    zt = t64(z).requires_grad_(True)
    Fn.cross_entropy(zt, lab, ignore_index=ignore, reduction="sum").backward()
    assert count == int(((lab != ignore)).sum()) and 0 < count < N
    close(loss, Fn.cross_entropy(t64(z), lab, ignore_index=ignore), "loss")
    close(grad, zt.grad, "grad")
    assert np.all(grad[np.asarray(lab) == ignore] == 0)


def test_cross_entropy_all_ignored():
    z, label = R.ce_case(40, 7, "all", -1, 3)
    loss, count, grad = R.cross_entropy(z, label, -1)
    assert loss == 0.0 and count == 0 and not grad.any()
    z, label = R.ce_case(40, 7, "none", 3, 3)
    assert R.cross_entropy(z, label, 3)[1] == 40 and not (label == 3).any()


def test_tall_wgrad():
    rng = np.random.default_rng(0)
    x, dy = rng.standard_normal((70, 17)).astype(np.float32), rng.standard_normal((70, 3)).astype(np.float32)
    dW, db = R.tall_wgrad(x, dy)
    close(dW, t64(dy).t() @ t64(x), "dW")
    close(db, t64(dy).sum(0), "db")


def _offset_torch(pt, coords, info, ids, ignore):
    """the offset part of PointGroup.loss, written with torch ops"""
    gt = info[:, 0:3] - coords
    valid = (ids != ignore).to(pt.dtype)
    dist = (pt - gt).abs().sum(-1)
    gt_n = gt / (torch.norm(gt, p=2, dim=1).unsqueeze(-1) + 1e-8)
    pt_n = pt / (torch.norm(pt, p=2, dim=1).unsqueeze(-1) + 1e-8)
    direction = -(gt_n * pt_n).sum(-1)
    return (dist * valid).sum(), (direction * valid).sum(), valid.sum()


@pytest.mark.parametrize("ldi", [3, 12])
def test_offset_loss(ldi):
    pt, coords, info, ids, kind = R.offset_case(400, ldi, 0, ldi)
    out, g1, g2 = R.offset_loss(pt, coords, info, ids, -100)
    p = t64(pt).requires_grad_(True)
    a, b, c = _offset_torch(p, t64(coords), t64(info), torch.from_numpy(ids), -100)
    ga, = torch.autograd.grad(a, p, retain_graph=True)
    gb, = torch.autograd.grad(b, p)
    close(out, torch.stack([a / (c + 1e-6), b / (c + 1e-6), c]).detach(), "out")
    close(g1, ga, "g1")
    close(g2, gb, "g2")          # includes the |pt| = 0 rows: torch's norm has a zero subgradient there too
    rows = np.nonzero((kind == 1) & (ids != -100))[0]
    gt = info[:, :3].astype(np.float64) - coords
    close(g2[rows], -gt[rows] / (np.linalg.norm(gt[rows], axis=1, keepdims=True) + 1e-8) / 1e-8, "g2 at pt = 0")
    out0, g10, g20 = R.offset_loss(pt, coords, info, np.full(400, -100), -100)
    assert not out0.any() and not g10.any() and not g20.any()


def test_offset_inputs_are_exact():
    """info - coords has no rounding in fp32, pt = gt rows give sign 0, the other rows stay 1e-3 away per component"""
    pt, coords, info, ids, kind = R.offset_case(5000, 12, 3, 7)
    gt32 = info[:, :3] - coords
    assert gt32.dtype == np.float32 and np.array_equal(gt32.astype(np.float64), info[:, :3].astype(np.float64) - coords)
    assert np.all(pt[kind == 0] == gt32[kind == 0]) and not pt[kind == 1].any() and not gt32[kind == 2].any()
    rest = kind > 2
    assert np.abs(pt[rest].astype(np.float64) - gt32[rest]).min() >= 1e-3
    assert set(kind) == set(range(8)) and (ids == -100).any() and (ids != -100).any()


@pytest.mark.parametrize("P,nInst", [(1, 1), (45, 7), (300, 64)])
def test_score_loss(P, nInst):
    scores, ious, kind = R.score_case(P, nInst, P)
    loss, gt_iou, dscore, term = R.score_loss(scores, ious, R.SCORE_FG, R.SCORE_BG)
    m = t64(ious).max(1)[0]
    k, b = 1 / (R.SCORE_FG - R.SCORE_BG), R.SCORE_BG / (R.SCORE_BG - R.SCORE_FG)
    target = torch.where(m > R.SCORE_FG, torch.ones_like(m), torch.where(m < R.SCORE_BG, torch.zeros_like(m), m * k + b))
    x = t64(scores).requires_grad_(True)
    terms = Fn.binary_cross_entropy_with_logits(x, target, reduction="none")
    terms.mean().backward()
    assert np.array_equal(gt_iou, m.numpy())
    close(term, terms.detach(), "terms")
    close(loss, terms.mean().detach(), "loss")
    close(dscore, x.grad, "dscore")
    if P >= 45:
        assert np.all(gt_iou[kind == 0] == R.SCORE_FG) and np.all(gt_iou[kind == 1] == R.SCORE_BG)
        assert np.all(target.numpy()[kind == 0] == 1.0) and np.all(target.numpy()[kind == 1] == 0.0)
        assert scores.max() == 100.0 and scores.min() == -100.0


@pytest.mark.parametrize("N,S,V", [(5, 7, 33), (1, 3, 2), (24, 25, 300)])
def test_masked_xe(N, S, V):
    pred, target, good, ties = R.xe_case(N, S, V, V)
    loss, acc, dpred, term, hit, denom = R.masked_xe(pred, target, good, S)
    sel = torch.from_numpy(good.astype(bool))
    p = t64(pred).requires_grad_(True)
    tg = torch.from_numpy(target)[:, :S][sel].reshape(-1)
    lt = Fn.cross_entropy(p[sel].reshape(-1, V), tg, ignore_index=0)
    lt.backward()
    am = p.detach()[sel].reshape(-1, V).argmax(-1)
    mask = tg != 0
    assert denom == int(mask.sum()) > 0
    close(loss, lt.detach(), "loss")
    close(acc, (am[mask] == tg[mask]).sum().double() / mask.sum().double(), "acc")
    close(dpred, p.grad, "dpred")
    for row, want in ties:
        assert hit[row] == want and term[row] > 0
    zero_rows = np.nonzero(np.where(good.astype(bool)[:, None], target[:, :S], 0).reshape(-1) == 0)[0]
    assert zero_rows.size and not dpred.reshape(N * S, V)[zero_rows].any()


def test_masked_xe_no_good_box():
    pred, target, good, _ = R.xe_case(4, 5, 9, 0, good_none=True)
    loss, acc, dpred, term, hit, denom = R.masked_xe(pred, target, good, 5)
    assert denom == 1.0 and loss == 0.0 and acc == 0.0 and not dpred.any()
