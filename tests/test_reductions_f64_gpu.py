"""The streaming reductions outside the convolutions against float64 (tests/reduction_refs.py), at the shapes where their
kernels change path: d3net_amd/csrc/bn.hip and the reduction parts of d3net_amd/csrc/heads.hip, called through the C entry
points so that no wrapper threshold decides which kernel runs.

Every call gets a workspace of exactly the queried size filled with NaN bit patterns, and writes into the middle of NaN
tensors with 64 guard elements on each side: the guards must stay NaN and no output may be NaN.

Bound.  Counts, gt_iou, g1, zero rows and the accuracy hits equal the reference.  Every other output, per group:
    err = max|kernel - ref|,  lib = max|L - ref|,  err <= 4 * lib + 4 * 2^-24 * max|ref|
with L = torch's fp32 op on the device for the same inputs (F.batch_norm + autograd, F.cross_entropy, dy.t() @ x,
BCE-with-logits, the reference expressions of the offset and caption losses).  4: two correct fp32 implementations that add in
different orders; the floor: a library that happens to be exact.  Where torch defines no result (one-row BatchNorm, a mean
over no rows) or returns NaN, lib = 0.  A group is the whole output, except where one call mixes inputs of different
conditioning on purpose, since a maximum over the whole output would hide all but the worst of them: the channels of one
BatchNorm input family (checked next to the whole output, not instead of it), and the |pt| = 0 rows of the offset gradient
(magnitude 1e8) against the other rows.  Within a BatchNorm family the floor of mean, running_mean, y and dx takes the
magnitude of the operands of their last difference instead of |ref| (test_batchnorm says why); the whole-output check keeps
|ref|.

Measured on an MI355X (every test prints its figures), max err / max lib over all cases; the largest err / bound of any
single figure is 0.67 (cross-entropy gradient, C = 64), 0.61 in BatchNorm:

    BatchNorm         mean             var              running_var      y                dx               dgamma           dbeta
    mean 0.5 std 2    1e-07 / 1e-07    5e-07 / 8e-07    3e-07 / 2e-07    8e-07 / 8e-07    1e-05 / 1e-05    2e-05 / 7e-05    1e-05 / 4e-05
    mean 0 std 1e-3   6e-11 / 6e-11    6e-14 / 2e-13    1e-07 / 1e-07    7e-08 / 7e-08    8e-05 / 8e-05    2e-06 / 4e-06    3e-05 / 3e-05
    mean 30 std 1     1e-06 / 6e-06    6e-08 / 3e-06    1e-07 / 3e-07    1e-05 / 1e-05    7e-05 / 7e-05    3e-04 / 2e-03    1e-05 / 3e-05
    mean -300 std 1   2e-05 / 4e-05    1e-07 / 2e-05    1e-07 / 4e-06    7e-04 / 7e-04    4e-02 / 4e-02    4e-03 / 7e-03    1e-05 / 3e-05
    mean 1000 std 0.1 3e-05 / 1e-04    9e-10 / 7e-06    1e-07 / 5e-07    4e-03 / 4e-03    1e-01 / 2e+01    9e-02 / 5e-01    1e-05 / 2e+00
    constant          0e+00 / 1e-06    0e+00 / 0e+00    9e-08 / 9e-08    0e+00 / 1e-04    6e-05 / 6e-05    0e+00 / 8e-03    6e-06 / 3e-05
    one 1e4 outlier   2e-04 / 2e-04    1e+00 / 3e+00    6e-01 / 8e-01    2e-05 / 7e-05    3e-08 / 4e-08    1e-05 / 1e-04    9e-06 / 8e-05
    outlier in row 0  2e-04 / 2e-04    1e+00 / 3e+00    5e-01 / 7e-01    2e-05 / 3e-05    2e-08 / 2e-08    4e-05 / 2e-05    3e-05 / 3e-05
    whole output      2e-04 / 2e-04    1e+00 / 3e+00    6e-01 / 8e-01    4e-03 / 4e-03    1e-01 / 2e+01    9e-02 / 5e-01    3e-05 / 2e+00
  (the large dx / dgamma / dbeta figures are the two-row cases, where 1 / sqrt(var + eps) reaches 100)

    cross-entropy   loss 2e-05 / 2e-05        grad 6e-07 / 2e-07
    tall wgrad      dW   3e-04 / 9e-03        db   1e-03 / 2e-03
    offset loss     norm 8e-07 / 8e-07        dir  4e-08 / 2e-08     g2 6e-06 / 6e-06, at |pt| = 0: 2e+01 / 2e+01 of 1e8
    score loss      loss 1e-06 / 3e-06        terms 5e-07 / 5e-07    dscore 2e-08 / 3e-08
    caption XE      loss 8e-07 / 8e-07        acc  2e-08 / 2e-08     dpred 4e-08 / 4e-08

What these tests met first, measured the same way (seven families then).  d3_bn_stats with fp32 sums of the raw values (var =
E[x^2] - mean^2): 50 of 56 test_batchnorm cases failed -- var err 1e-04 / 2e-02 / 2e-01 and y err 6e-03 / 2e+00 / 4e+01 at
mean 30 / -300 / 1000, a constant column with a variance up to 7e-06 and a single row with up to 3e-02 instead of 0, dx and
dgamma following; mean, the guards and the bf16 identity passed.  With fp32 sums of x - x[0] all passed; the sums are fp64
since, which an outlier in the pivot row needs, and so are the backward's (dbeta of 130 terms of both signs missed by 11 %,
6.6e-07 against lib 5.7e-08, once the eighth family moved the inputs).  The score loss missed at P >= 1023 (serial fp32 sum:
err up to 1.9e-06 against lib 3e-08), the caption loss at 600 rows of 3004 words (3.0e-06 against a bound of 2.95e-06), the
cross-entropy loss at C = 7 (3.1e-06 against lib 2e-07: (m + log se) - z rounded at the 1e4 of the logits).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import reduction_refs as R

pytestmark = pytest.mark.gpu

GUARD = 64
ERR_ARG = -3
FLOOR = 4.0 * 2.0 ** -24


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _L():
    from d3net_amd import _lib
    return _lib.lib()


class Out:
    """an output buffer: the middle of a NaN tensor"""

    def __init__(self, shape, dev, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.big = torch.full((self.n + 2 * GUARD,), float("nan"), dtype=dtype, device=dev)
        self.t = self.big[GUARD:GUARD + self.n].view(shape)

    def get(self, what):
        big = self.big.float().cpu().numpy()
        assert np.isnan(big[:GUARD]).all() and np.isnan(big[GUARD + self.n:]).all(), "%s: guard overwritten" % what
        v = big[GUARD:GUARD + self.n].reshape(tuple(self.t.shape))
        assert not np.isnan(v).any(), "%s: %d elements NaN (unwritten?)" % (what, int(np.isnan(v).sum()))
        return v.astype(np.float64)


def workspace(nbytes, dev):
    """exactly nbytes, every byte 0xFF: NaN read as fp32 or as fp64"""
    return torch.full((int(nbytes),), 255, dtype=torch.uint8, device=dev)


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bounded(what, kernel, ref, lib, groups=None, scale=None):
    """the bound of the module docstring; groups: {name: index or mask selecting the group's elements}; scale: per element,
    the magnitude of the operands of the output's last difference, where that is the scale of its fp32 rounding"""
    kernel, ref = np.asarray(kernel, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    lib = None if lib is None else np.asarray(lib, dtype=np.float64)
    assert kernel.shape == ref.shape, what
    scale = np.abs(ref) if scale is None else np.maximum(np.abs(ref), np.broadcast_to(np.asarray(scale, dtype=np.float64), ref.shape))
    bad = []
    for name, sel in (groups or {"": Ellipsis}).items():
        k, r = kernel[sel], ref[sel]
        if r.size == 0:
            continue
        err = float(np.abs(k - r).max())
        libe = 0.0 if lib is None else float(np.nan_to_num(np.abs(lib[sel] - r), nan=0.0, posinf=0.0).max())
        bound = 4.0 * libe + FLOOR * float(scale[sel].max())
        print("F64 %s%s err=%.3e lib=%.3e bound=%.3e scale=%.3e" % (what, " [%s]" % name if name else "", err, libe, bound,
                                                                   float(scale[sel].max())))
        if not err <= bound:
            bad.append("%s [%s]: err %.3e > bound %.3e (lib %.3e)" % (what, name, err, bound, libe))
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------------ BatchNorm
@pytest.mark.parametrize("M,Cc,shift,relu", list(R.bn_cases()))
def test_batchnorm(dev, M, Cc, shift, relu):
    L = _L()
    case = R.bn_case(M, Cc, shift, 1000 * Cc + M)
    fam = case["fam"]
    groups = {R.BN_FAMILIES[f]: np.nonzero(fam == f)[0] for f in sorted(set(fam))}
    cols = {k: (slice(None), v) for k, v in groups.items()}
    eps, mom = R.BN_EPS, 0.1
    assert case["band"].mean() < 0.01 or M * Cc < 1000
    x, dy = dv(case["x"], dev), dv(case["dy"], dev)
    gamma, beta = dv(case["gamma"], dev), dv(case["beta"], dev)

    # float64
    mean_r, var_r, rm_r, rv_r = R.bn_stats(case["x"], case["rm"], case["rv"], mom)
    y_r = R.bn_relu_fwd(case["x"], mean_r, var_r, case["gamma"], case["beta"], eps, relu)
    dx_r, dg_r, db_r = R.bn_relu_bwd(case["x"], case["dy"], mean_r, var_r, case["gamma"], case["beta"], eps, relu)

    # library, fp32 on the device (it refuses one row)
    lib = dict.fromkeys(("mean", "var", "rm", "rv", "y", "dx", "dg", "db"))
    if M > 1:
        xl, gl, bl = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        rml, rvl = dv(case["rm"], dev), dv(case["rv"], dev)
        yl = Fn.batch_norm(xl, rml, rvl, gl, bl, True, mom, eps)
        yl = torch.relu(yl) if relu else yl
        yl.backward(dy)
        lib = dict(mean=x.mean(0), var=x.var(0, unbiased=False), rm=rml, rv=rvl, y=yl.detach(), dx=xl.grad, dg=gl.grad, db=bl.grad)
        lib = {k: v.double().cpu().numpy() for k, v in lib.items()}

    # kernels
    ws = workspace(L.d3_bn_ws_bytes(Cc), dev)
    mean, var, rm, rv = (Out((Cc,), dev) for _ in range(4))
    rm.t.copy_(dv(case["rm"], dev)); rv.t.copy_(dv(case["rv"], dev))
    assert L.d3_bn_stats(_ptr(x), M, Cc, _ptr(mean.t), _ptr(var.t), _ptr(rm.t), _ptr(rv.t), mom, _ptr(ws), ws.numel(), _stream()) == 0
    y = Out((M, Cc), dev)
    assert L.d3_bn_relu_fwd(_ptr(x), _ptr(mean.t), _ptr(var.t), _ptr(gamma), _ptr(beta), _ptr(y.t), M, Cc, eps, relu, _stream()) == 0
    ws2 = workspace(L.d3_bn_ws_bytes(Cc), dev)
    dx, dg, db = Out((M, Cc), dev), Out((Cc,), dev), Out((Cc,), dev)
    assert L.d3_bn_relu_bwd(_ptr(x), _ptr(dy), _ptr(mean.t), _ptr(var.t), _ptr(gamma), _ptr(beta), _ptr(dx.t), _ptr(dg.t), _ptr(db.t),
                            M, Cc, eps, relu, _ptr(ws2), ws2.numel(), _stream()) == 0
    ybf = None
    if Cc % 4 == 0:
        ybf = Out((M, Cc), dev, torch.bfloat16)
        assert L.d3_bn_relu_fwd_bf16(_ptr(x), _ptr(mean.t), _ptr(var.t), _ptr(gamma), _ptr(beta), _ptr(ybf.t), M, Cc, eps, relu,
                                     _stream()) == 0
    torch.cuda.synchronize()

    var_k = var.get("var")
    assert (var_k >= 0).all()
    tag = "bn C=%d M=%d relu=%d " % (Cc, M, relu)
    # Per family, four outputs end in a difference whose operands set the fp32 rounding, not the result: the mean of data that
    # straddle zero, gamma * xhat + beta, and dx = gamma * inv * (g - mean g - xhat * mean(g xhat)), which cancels to nothing
    # at two rows or at a lone unmasked outlier.  Their floor takes the operands' magnitude; the other outputs keep |ref|.
    xa = np.abs(case["x"].astype(np.float64))
    inv = 1.0 / np.sqrt(var_r + eps)
    xh = (case["x"] - mean_r) * inv
    ga = case["gamma"].astype(np.float64)
    g = case["dy"].astype(np.float64) * ((xh * ga + case["beta"] > 0) if relu else 1.0)
    s_mean = xa.max(0)
    s_rm = (1 - mom) * np.abs(case["rm"]) + mom * s_mean
    s_y = np.abs(ga * xh) + np.abs(case["beta"])
    s_dx = np.abs(ga * inv) * (np.abs(g) + np.abs(g.mean(0)) + np.abs(xh * (g * xh).mean(0)))
    failures = []
    for name, k, r, l, g_, sc in (("mean", mean.get("mean"), mean_r, lib["mean"], groups, s_mean),
                                  ("var", var_k, var_r, lib["var"], groups, None),
                                  ("running_mean", rm.get("rm"), rm_r, lib["rm"], groups, s_rm),
                                  ("running_var", rv.get("rv"), rv_r, lib["rv"], groups, None),
                                  ("y", y.get("y"), y_r, lib["y"], cols, s_y), ("dx", dx.get("dx"), dx_r, lib["dx"], cols, s_dx),
                                  ("dgamma", dg.get("dgamma"), dg_r, lib["dg"], groups, None),
                                  ("dbeta", db.get("dbeta"), db_r, lib["db"], groups, None)):
        for grp, scl in ((g_, sc), (None, None)):        # per family; then the whole output with the plain floor
            try:
                bounded(tag + name, k, r, l, grp, scl)
            except AssertionError as e:
                failures.append(str(e))
    assert np.isfinite(y.get("y")).all()
    if ybf is not None:
        ybf.get("y bf16")
        assert torch.equal(ybf.t.view(torch.int16), y.t.to(torch.bfloat16).view(torch.int16)), "bf16 forward: not RNE of the fp32 forward"
    assert not failures, "\n".join(failures)


def test_batchnorm_refuses_bad_channel_counts(dev):
    L = _L()
    x = torch.zeros(4, 260, device=dev)
    v = torch.ones(260, device=dev)
    for Cc in (0, 257):
        ws = workspace(L.d3_bn_ws_bytes(max(Cc, 1)), dev)
        assert L.d3_bn_stats(_ptr(x), 4, Cc, _ptr(v), _ptr(v), None, None, 0.1, _ptr(ws), ws.numel(), _stream()) == ERR_ARG
        assert L.d3_bn_relu_bwd(_ptr(x), _ptr(x), _ptr(v), _ptr(v), _ptr(v), _ptr(v), _ptr(x), _ptr(v), _ptr(v), 4, Cc, 1e-4, 1,
                                _ptr(ws), ws.numel(), _stream()) == ERR_ARG
    y = torch.zeros(4, 3, dtype=torch.bfloat16, device=dev)
    assert L.d3_bn_relu_fwd_bf16(_ptr(x), _ptr(v), _ptr(v), _ptr(v), _ptr(v), _ptr(y), 4, 3, 1e-4, 1, _stream()) == ERR_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ cross-entropy
def _ce_run(dev, N, Cc, mode, ignore, seed):
    L = _L()
    z, label = R.ce_case(N, Cc, mode, ignore, seed)
    loss_r, count_r, grad_r = R.cross_entropy(z, label, ignore)
    zd, ld = dv(z, dev), dv(label, dev)
    # the library asserts on labels outside [0, C): hand it the ignore index for those
    ll = dv(np.where((label < 0) | (label >= Cc), ignore, label), dev)
    zl = zd.clone().requires_grad_(True)
    Fn.cross_entropy(zl, ll, ignore_index=ignore, reduction="sum").backward()
    loss_l = float(Fn.cross_entropy(zd, ll, ignore_index=ignore)) if count_r else None
    ws = workspace(L.d3_cross_entropy_ws_bytes(), dev)
    grad, out = Out((N, Cc), dev), Out((2,), dev)
    assert L.d3_cross_entropy(_ptr(zd), _ptr(ld), _ptr(grad.t), _ptr(out.t), N, Cc, ignore, _ptr(ws), ws.numel(), _stream()) == 0
    torch.cuda.synchronize()
    o, g = out.get("out"), grad.get("grad")
    tag = "ce C=%d N=%d %s ignore=%d " % (Cc, N, mode, ignore)
    assert o[1] == count_r, tag + "count"
    counted = (label != ignore) & (label >= 0) & (label < Cc)
    assert not g[~counted].any(), tag + "gradient of an ignored row"
    if count_r == 0:
        assert o[0] == 0.0
    bounded(tag + "loss", o[:1], [loss_r], None if loss_l is None else [loss_l])
    bounded(tag + "grad", g, grad_r, zl.grad.double().cpu().numpy())


@pytest.mark.parametrize("N", [1, 255, 256, 257])
@pytest.mark.parametrize("Cc", [1, 2, 7, 20, 31, 32, 33, 64])
def test_cross_entropy(dev, N, Cc):
    """C <= 32: the LDS kernel, above: one thread per row"""
    seed = 0
    for mode in ("none", "some", "all"):
        for ignore in (-1, -100, 3):
            seed += 1
            _ce_run(dev, N, Cc, mode, ignore, 100 * N + seed)


@pytest.mark.parametrize("Cc", [2, 33])
def test_cross_entropy_second_sweep(dev, Cc):
    """1024 * 256 + 300 rows: every workgroup's first tile, then a second sweep with a ragged last tile"""
    _ce_run(dev, 262144 + 300, Cc, "some", -100, Cc)


def test_cross_entropy_refuses_bad_class_counts(dev):
    L = _L()
    z = torch.zeros(4, 65, device=dev)
    lab = torch.zeros(4, dtype=torch.int64, device=dev)
    ws = workspace(L.d3_cross_entropy_ws_bytes(), dev)
    out = torch.zeros(2, device=dev)
    for Cc in (0, 65):
        assert L.d3_cross_entropy(_ptr(z), _ptr(lab), _ptr(z), _ptr(out), 4, Cc, -1, _ptr(ws), ws.numel(), _stream()) == ERR_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ tall weight gradient
TW_N = (1, 63, 64, 65, 32767, 32768, 32769, 40000)
TW_O = (1, 3, 16, 17, 20, 32)


@pytest.fixture(scope="module")
def tall_inputs():
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((40000, 32)) * rng.uniform(0.5, 2, 32)).astype(np.float32)
    dy = (rng.standard_normal((40000, 32)) + 0.5).astype(np.float32)
    return x, dy


@pytest.mark.parametrize("I", [1, 15, 16, 17, 31, 32])
def test_tall_wgrad(dev, tall_inputs, I):
    """I <= 31: the MFMA kernel (the bias gradient is its column I), I = 32: the scalar kernel; N around one 64-row tile and
    around 512 * 64, where the grid stops growing; db = NULL once per kernel"""
    L = _L()
    failures = []
    for O in TW_O:
        for N in TW_N:
            x, dy = np.ascontiguousarray(tall_inputs[0][:N, :I]), np.ascontiguousarray(tall_inputs[1][:N, :O])
            dW_r, db_r = R.tall_wgrad(x, dy)
            xd, dyd = dv(x, dev), dv(dy, dev)
            with_db = not (O == 17 and N == 65)
            ws = workspace(L.d3_tall_wgrad_ws_bytes(I, O), dev)
            dW, db = Out((O, I), dev), Out((O,), dev)
            assert L.d3_tall_wgrad(_ptr(xd), _ptr(dyd), _ptr(dW.t), _ptr(db.t) if with_db else None, N, I, O, _ptr(ws), ws.numel(),
                                   _stream()) == 0
            torch.cuda.synchronize()
            tag = "tall_wgrad I=%d O=%d N=%d " % (I, O, N)
            try:
                bounded(tag + "dW", dW.get("dW"), dW_r, (dyd.t() @ xd).double().cpu().numpy())
                if with_db:
                    bounded(tag + "db", db.get("db"), db_r, dyd.sum(0).double().cpu().numpy())
                else:
                    assert torch.isnan(db.big).all(), tag + "db = NULL was written"
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "\n".join(failures)


def test_tall_wgrad_refuses_wide_layers(dev):
    L = _L()
    a = torch.zeros(8, 33, device=dev)
    ws = workspace(L.d3_tall_wgrad_ws_bytes(33, 33), dev)
    w = torch.zeros(33, 33, device=dev)
    assert L.d3_tall_wgrad(_ptr(a), _ptr(a), _ptr(w), None, 8, 33, 16, _ptr(ws), ws.numel(), _stream()) == ERR_ARG
    assert L.d3_tall_wgrad(_ptr(a), _ptr(a), _ptr(w), None, 8, 16, 33, _ptr(ws), ws.numel(), _stream()) == ERR_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ offset loss
def _offset_lib(pt, coords, info, ids, ignore):
    """the offset part of PointGroup.loss in torch fp32: the two losses, the valid count and the two unscaled gradients"""
    p = pt.clone().requires_grad_(True)
    gt = info[:, 0:3] - coords
    valid = (ids != ignore).float()
    dist = (p - gt).abs().sum(-1)
    gt_n = gt / (torch.norm(gt, p=2, dim=1).unsqueeze(-1) + 1e-8)
    pt_n = p / (torch.norm(p, p=2, dim=1).unsqueeze(-1) + 1e-8)
    direction = -(gt_n * pt_n).sum(-1)
    a, b, c = (dist * valid).sum(), (direction * valid).sum(), valid.sum()
    g2, = torch.autograd.grad(b, p)
    return torch.stack([a / (c + 1e-6), b / (c + 1e-6), c]).detach(), g2


@pytest.mark.parametrize("all_ignored", [False, True])
@pytest.mark.parametrize("ldi", [3, 12])
@pytest.mark.parametrize("N", [1, 257, 262144 + 300])
def test_offset_loss(dev, N, ldi, all_ignored):
    L = _L()
    ignore = -100
    # one row: pt = 0, gt = 0, a plain row in turn (alone, a pt = gt row has a direction gradient of zero up to the cancellation
    # of two terms of magnitude 1 / |pt|: no scale to bound it against; the larger N hold such rows among the others)
    for shift in (range(1, 4) if N == 1 else (0,)):
        pt, coords, info, ids, kind = R.offset_case(N, ldi, shift, N + ldi, all_ignored, ignore)
        if N == 1 and not all_ignored:
            ids[:] = 5
        out_r, g1_r, g2_r = R.offset_loss(pt, coords, info, ids, ignore)
        ptd, cd, infd, idd = dv(pt, dev), dv(coords, dev), dv(info, dev), dv(ids, dev)
        out_l, g2_l = _offset_lib(ptd, cd, infd, idd, ignore)
        ws = workspace(L.d3_offset_loss_ws_bytes(), dev)
        g1, g2, out = Out((N, 3), dev), Out((N, 3), dev), Out((3,), dev)
        assert L.d3_offset_loss(_ptr(ptd), _ptr(cd), _ptr(infd), ldi, _ptr(idd), ignore, _ptr(g1.t), _ptr(g2.t), _ptr(out.t), N,
                                _ptr(ws), ws.numel(), _stream()) == 0
        torch.cuda.synchronize()
        o = out.get("out")
        tag = "offset N=%d ldi=%d ignored=%d shift=%d " % (N, ldi, all_ignored, shift)
        assert np.array_equal(g1.get("g1"), g1_r), tag + "g1"
        assert o[2] == out_r[2], tag + "valid count"
        if all_ignored:
            assert not o.any() and not g2.get("g2").any()
        out_l = out_l.double().cpu().numpy()
        bounded(tag + "norm loss", o[:1], out_r[:1], out_l[:1])
        bounded(tag + "dir loss", o[1:2], out_r[1:2], out_l[1:2])
        bounded(tag + "g2", g2.get("g2"), g2_r, g2_l.double().cpu().numpy(), {"pt = 0": kind == 1, "other rows": kind != 1})


# ------------------------------------------------------------------------------------------------ score loss
@pytest.mark.parametrize("nInst", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("P", [1, 3, 4, 5, 1023, 1024, 1025, 2500])
def test_score_loss(dev, P, nInst):
    """P around one workgroup of four proposals and around the 1024-term passes of the sum; nInst around one wave"""
    L = _L()
    fg, bg = R.SCORE_FG, R.SCORE_BG
    scores, ious, _ = R.score_case(P, nInst, P + nInst)
    loss_r, gt_r, ds_r, term_r = R.score_loss(scores, ious, fg, bg)
    sd, iod = dv(scores, dev), dv(ious, dev)
    sl = sd.clone().requires_grad_(True)
    m = iod.max(1)[0]
    target = torch.where(m > fg, torch.ones_like(m), torch.where(m < bg, torch.zeros_like(m), m * (1 / (fg - bg)) + bg / (bg - fg)))
    terms_l = Fn.binary_cross_entropy_with_logits(sl, target, reduction="none")
    terms_l.mean().backward()
    gt, ds, out = Out((P,), dev), Out((P,), dev), Out((1 + P,), dev)
    assert L.d3_score_loss(_ptr(sd), _ptr(iod), P, nInst, fg, bg, _ptr(gt.t), _ptr(ds.t), _ptr(out.t), _stream()) == 0
    torch.cuda.synchronize()
    o = out.get("out")
    tag = "score P=%d nInst=%d " % (P, nInst)
    assert np.array_equal(gt.get("gt_iou"), gt_r), tag + "gt_iou"
    failures = []
    for name, k, r, l in (("loss", o[:1], [loss_r], [float(terms_l.detach().mean())]), ("terms", o[1:], term_r, terms_l.detach().double().cpu().numpy()),
                          ("dscore", ds.get("dscore"), ds_r, sl.grad.double().cpu().numpy())):
        try:
            bounded(tag + name, k, r, l)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


def test_score_loss_refuses_no_proposals(dev):
    L = _L()
    a = torch.zeros(8, device=dev)
    assert L.d3_score_loss(_ptr(a), _ptr(a), 0, 4, 0.75, 0.25, _ptr(a), _ptr(a), _ptr(a), _stream()) == ERR_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ caption cross-entropy
@pytest.mark.parametrize("N,S", [(1, 1), (15, 17), (1, 257), (257, 1), (24, 25)])
@pytest.mark.parametrize("V", [2, 255, 256, 257, 3004])
def test_masked_xe(dev, V, N, S):
    """V around one 256-thread pass over a row; N * S = 1, 255, 257, 600 rows: 1, 1, 2 and 3 terms per thread of the final sum;
    the target matrix is wider than S; then the same call with no good box"""
    L = _L()
    for good_none in (False, True):
        pred, target, good, ties = R.xe_case(N, S, V, V + N, good_none)
        loss_r, acc_r, dp_r, term_r, hit_r, denom_r = R.masked_xe(pred, target, good, S)
        pd, td, gd = dv(pred, dev), dv(target, dev), dv(good, dev)
        assert td.stride(0) == S + 3
        # library: compute_cap_loss's expression, fp32
        loss_l = acc_l = None
        dp_l = torch.zeros_like(pd)
        sel = gd.bool()
        tsel = td[:, :S][sel].reshape(-1)
        if int((tsel != 0).sum()) > 0:
            pl = pd.clone().requires_grad_(True)
            lt = Fn.cross_entropy(pl[sel].reshape(-1, V), tsel, ignore_index=0)
            lt.backward()
            am = pd[sel].reshape(-1, V).argmax(-1)
            mask = tsel != 0
            loss_l, acc_l, dp_l = [float(lt)], [float((am[mask] == tsel[mask]).sum().float() / mask.sum().float())], pl.grad
        nws = int(L.d3_masked_xe_ws_bytes(N, S))
        ws = workspace(nws, dev)
        dp, out = Out((N, S, V), dev), Out((2,), dev)
        assert L.d3_masked_xe(_ptr(pd), _ptr(td), td.stride(0), _ptr(gd), N, S, V, _ptr(dp.t), _ptr(out.t), _ptr(ws), nws, _stream()) == 0
        torch.cuda.synchronize()
        rowterm = ws.view(torch.float32).cpu().numpy().astype(np.float64)
        o, g = out.get("out"), dp.get("dpred")
        tag = "masked_xe V=%d N=%d S=%d none=%d " % (V, N, S, good_none)
        assert np.array_equal(rowterm[1:2 * N * S:2], hit_r), tag + "hits"
        assert rowterm[2 * N * S] == denom_r, tag + "denom"
        for row, want in ties:
            assert rowterm[2 * row + 1] == want, tag + "tie"
        assert not g.reshape(N * S, V)[term_r == 0].any(), tag + "gradient of an uncounted row"
        if good_none:
            assert denom_r == 1.0 and o[0] == 0.0 and o[1] == 0.0
        bounded(tag + "loss", o[:1], [loss_r], loss_l)
        bounded(tag + "acc", o[1:], [acc_r], acc_l)
        bounded(tag + "dpred", g, dp_r, dp_l.double().cpu().numpy())
